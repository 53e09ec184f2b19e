// The speaker-verification test on the device (GE2E/train_speech_embedder.py:112-322 around the embedder), gfx950: the trial scores of
// get_centroids + get_cossim (ssv_sv_trial_scores), the threshold sweep that ends in EER and spoof rate (ssv_sv_eer_sweep) and the
// accept rate at a given threshold over a stack of score matrices (ssv_sv_accept_rate).  Latency-class: 20 x 80 x 20 dot products of
// 256 and 50 x 32000 comparisons at the configuration's shape -- what counts is that a batch is three launches and no host traffic.
// Every float sum runs in a fixed order that does not depend on the grid, every count is an integer: the same inputs give the same bits.
#include "ssv_common.h"

#define SE_THREADS 256
#define SE_WAVES (SE_THREADS / 64)
#define SE_LDS_FLOATS 15360         // 60 KiB of centroid tile + speaker sum; a tile of TJ speakers takes (TJ + 1) * D + TJ floats
#define SE_EPS 1e-8f                // torch.nn.functional.cosine_similarity clamps each norm there

// ---- the values both forms of the kernel read: staged in LDS, or recomputed from global memory with the SAME operations -------------
// centroid element: the enrolment embeddings added in e order, then one division (enr.mean(1))
__device__ __forceinline__ float se_centroid(const float* __restrict__ enr, long j, int E, int D, int d) {
  const float* p = enr + (j * E) * (long)D + d;
  float s = p[0];
  for (int e = 1; e < E; ++e) s += p[(long)e * D];
  return s / (float)E;
}
// element of the speaker's verification sum: the V rows in use added in v order
__device__ __forceinline__ float se_versum(const float* __restrict__ ver, long i, int V, int ver_stride, int D, int d) {
  const float* p = ver + (i * ver_stride) * (long)D + d;
  float s = p[0];
  for (int v = 1; v < V; ++v) s += p[(long)v * D];
  return s;
}

// Workgroup (speaker i, tile of TJ centroids j0 ...).  Stage: the tile's centroids, their clamped norms and -- when i's own column lies in
// the tile -- the sum of i's verification rows.  Then one wave per verification row v: the lanes split d (lane, lane + 64, ...), every
// dot product is a chain of fmaf per lane and the 64 partial sums meet in ssv_wave_sum's butterfly, so a score's bits depend on D alone,
// not on TJ, the grid or the wave that computed it.  STAGED = false (one centroid does not fit the LDS budget): TJ = 1 and every staged
// value is recomputed where it is used, by the same functions.
template <bool STAGED>
__global__ __launch_bounds__(SE_THREADS) void sv_trial_scores_kernel(const float* __restrict__ enr, const float* __restrict__ ver, float* __restrict__ sim,
                                                                     float* __restrict__ cent_out, int N, int E, int V, int ver_stride, int D, int TJ, int tiles) {
  extern __shared__ float lds[];
  const int i = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * TJ, nj = min(TJ, N - j0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool own_here = i >= j0 && i < j0 + nj;
  float* cs = lds;                                   // [TJ][D] centroids
  float* ss = lds + (STAGED ? (long)TJ * D : 0);     // [D] sum of speaker i's verification rows
  float* cn = ss + (STAGED ? D : 0);                 // [TJ] clamped centroid norms
  if (STAGED) {
    for (long e = threadIdx.x; e < (long)nj * D; e += SE_THREADS) {
      const int jj = (int)(e / D), d = (int)(e - (long)jj * D);
      const float c = se_centroid(enr, j0 + jj, E, D, d);
      cs[e] = c;
      if (cent_out && i == 0) cent_out[(long)(j0 + jj) * D + d] = c;
    }
    if (own_here)
      for (int d = threadIdx.x; d < D; d += SE_THREADS) ss[d] = se_versum(ver, i, V, ver_stride, D, d);
    __syncthreads();
  } else if (cent_out && i == 0) {
    for (int d = threadIdx.x; d < D; d += SE_THREADS) cent_out[(long)j0 * D + d] = se_centroid(enr, j0, E, D, d);
  }
  for (int jj = wave; jj < nj; jj += SE_WAVES) {
    float a = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float c = STAGED ? cs[(long)jj * D + d] : se_centroid(enr, j0 + jj, E, D, d);
      a = fmaf(c, c, a);
    }
    a = fmaxf(sqrtf(ssv_wave_sum(a)), SE_EPS);
    if (lane == 0) cn[jj] = a;
  }
  __syncthreads();
  const float others = (float)(V - 1);
  for (int v = wave; v < V; v += SE_WAVES) {
    const float* x = ver + ((long)i * ver_stride + v) * (long)D;
    float* out = sim + (((long)i * V + v) * N + j0);
    float a = 0.f;
    for (int d = lane; d < D; d += 64) a = fmaf(x[d], x[d], a);
    const float xn = fmaxf(sqrtf(ssv_wave_sum(a)), SE_EPS);
    for (int jj = 0; jj < nj; ++jj) {
      float dot = 0.f, sc;
      if (j0 + jj == i) {
        // own column: the mean of the speaker's OTHER rows (utils.py:42-43)
        float ln = 0.f;
        for (int d = lane; d < D; d += 64) {
          const float s = STAGED ? ss[d] : se_versum(ver, i, V, ver_stride, D, d);
          const float l = (s - x[d]) / others;
          dot = fmaf(x[d], l, dot);
          ln = fmaf(l, l, ln);
        }
        sc = ssv_wave_sum(dot) / (xn * fmaxf(sqrtf(ssv_wave_sum(ln)), SE_EPS));
      } else {
        for (int d = lane; d < D; d += 64) dot = fmaf(x[d], STAGED ? cs[(long)jj * D + d] : se_centroid(enr, j0 + jj, E, D, d), dot);
        sc = ssv_wave_sum(dot) / (xn * cn[jj]);
      }
      if (lane == 0) out[jj] = sc + 1e-6f;
    }
  }
}

extern "C" int ssv_sv_trial_scores(const float* enr, const float* ver, float* sim, float* cent, int N, int E, int V, int ver_stride, int D,
                                   ssv_stream_t stream) {
  SSV_CHECK(enr && ver && sim, SSV_BAD_SHAPE, "sv_trial_scores: null pointer (enr, ver and sim are required)");
  SSV_CHECK(N >= 2 && V >= 2 && E >= 1 && D >= 1 && V <= ver_stride, SSV_BAD_SHAPE,
            "sv_trial_scores: need N >= 2 speakers, V >= 2 verification rows (the own column leaves one out), E >= 1, D >= 1 and V <= ver_stride; "
            "got N=%d E=%d V=%d ver_stride=%d D=%d", N, E, V, ver_stride, D);
  // (TJ + 1) * D + TJ floats per tile; no centroid fits: the unstaged form, one centroid per workgroup
  const bool staged = 2L * D + 1 <= SE_LDS_FLOATS;
  const int TJ = staged ? (int)min((long)N, (SE_LDS_FLOATS - D) / ((long)D + 1)) : 1;
  const int tiles = ssv_cdiv(N, TJ);
  SSV_CHECK((long)N * tiles <= 0x7fffffffL, SSV_UNSUPPORTED, "sv_trial_scores: N=%d x %d centroid tiles exceed the grid", N, tiles);
  if (staged) {
    const size_t lds = ((size_t)(TJ + 1) * D + TJ) * sizeof(float);
    hipLaunchKernelGGL(sv_trial_scores_kernel<true>, dim3(N * tiles), dim3(SE_THREADS), lds, (hipStream_t)stream, enr, ver, sim, cent, N, E, V, ver_stride, D,
                       TJ, tiles);
  } else {
    hipLaunchKernelGGL(sv_trial_scores_kernel<false>, dim3(N * tiles), dim3(SE_THREADS), sizeof(float), (hipStream_t)stream, enr, ver, sim, cent, N, E, V,
                       ver_stride, D, TJ, tiles);
  }
  return ssv_check_launch("sv_trial_scores");
}

// ---- the threshold sweep ------------------------------------------------------------------------------------------------------------
// Pass 1, workgroup = threshold t: counts[t] = accepted trials (sim > thr[t], strict) over (the whole matrix, the own-speaker column, its
// first `head` rows, its last `tail` rows).  Thread k takes elements k, k + 256, ...; the 256 integer counts meet in LDS.
__global__ __launch_bounds__(SE_THREADS) void sv_sweep_counts_kernel(const float* __restrict__ sim, const float* __restrict__ thr, int* __restrict__ counts,
                                                                     int N, int V, int head, int tail) {
  __shared__ int red[4][SE_THREADS];
  const float th = thr[blockIdx.x];
  const long total = (long)N * V * N;
  int c[4] = {0, 0, 0, 0};
  for (long e = threadIdx.x; e < total; e += SE_THREADS) {
    if (!(sim[e] > th)) continue;
    const int j = (int)(e % N), v = (int)((e / N) % V), i = (int)(e / ((long)N * V));
    c[0] += 1;
    if (i == j) {
      c[1] += 1;
      c[2] += v < head;
      c[3] += v >= V - tail;
    }
  }
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = c[k];
  __syncthreads();
  for (int s = SE_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 4) counts[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// Pass 2, one thread: FAR, FRR and |FAR - FRR| per threshold in float64, operation for operation as the host sweep has them; the first
// minimum (strict <, from 1.0) wins; its row goes to slot *step_dev % hist_len and the counter moves on.
__global__ void sv_sweep_finish_kernel(const int* __restrict__ counts, int nthr, int N, int spoof, double den, double pos, double hden, double hpos,
                                       double* __restrict__ hist, int hist_len, int* __restrict__ step_dev) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double n = (double)N;
  double cur = 1.0, far_b = 0.0, frr_b = 0.0;
  int best = 0;
  for (int t = 0; t < nthr; ++t) {
    const double tot = (double)counts[4 * t], own = (double)counts[4 * t + 1];
    const double fa = (tot - own) / (n - 1.0) / den / n;
    const double fr = (n * pos - own) / den / n;
    const double d = fabs(fa - fr);
    if (t == 0) { far_b = fa; frr_b = fr; }
    if (cur > d) { cur = d; best = t; far_b = fa; frr_b = fr; }
  }
  const int s = step_dev[0];
  double* row = hist + (long)(s % hist_len) * 6;
  row[0] = (far_b + frr_b) / 2;
  row[1] = (double)best;
  row[2] = far_b;
  row[3] = frr_b;
  row[4] = spoof ? (n * hpos - (double)counts[4 * best + 2]) / hden / n : 0.0;
  row[5] = spoof ? (double)counts[4 * best + 3] / hden / n : 0.0;
  step_dev[0] = s + 1;
}

extern "C" int ssv_sv_eer_sweep(const float* sim, int N, int V, const float* thr, int nthr, int head, int tail, double den, double pos, double hden,
                                double hpos, int* counts, double* hist, int hist_len, int* step_dev, ssv_stream_t stream) {
  SSV_CHECK(sim && thr && counts && hist && step_dev, SSV_BAD_SHAPE, "sv_eer_sweep: null pointer (sim, thr, counts, hist and step_dev are required)");
  SSV_CHECK(N >= 2 && V >= 1 && nthr >= 1 && hist_len >= 1, SSV_BAD_SHAPE, "sv_eer_sweep: need N >= 2, V >= 1, nthr >= 1 and hist_len >= 1; got N=%d V=%d nthr=%d hist_len=%d",
            N, V, nthr, hist_len);
  SSV_CHECK(head >= 0 && tail >= 0 && head <= V && tail <= V, SSV_BAD_SHAPE, "sv_eer_sweep: head=%d and tail=%d must lie in [0, V=%d]", head, tail, V);
  SSV_CHECK((long)N * V * N <= 0x7fffffffL, SSV_UNSUPPORTED, "sv_eer_sweep: %ld trials do not fit the int32 counts", (long)N * V * N);
  hipLaunchKernelGGL(sv_sweep_counts_kernel, dim3(nthr), dim3(SE_THREADS), 0, (hipStream_t)stream, sim, thr, counts, N, V, head, tail);
  SSV_TRY(ssv_check_launch("sv_sweep_counts"));
  hipLaunchKernelGGL(sv_sweep_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)counts, nthr, N, (head | tail) != 0 ? 1 : 0, den, pos, hden,
                     hpos, hist, hist_len, step_dev);
  return ssv_check_launch("sv_sweep_finish");
}

// ---- accept rate at one threshold over a stack of matrices ----------------------------------------------------------------------------
// Workgroup = matrix: the own-speaker trials of the last `tail` rows above thres (strict, in float32), as a float32 fraction computed as
// the host computes it: count / float(tail) / N, each quotient rounded once.
__global__ __launch_bounds__(SE_THREADS) void sv_accept_rate_kernel(const float* __restrict__ stack, int N, int V, int tail, float thres, float* __restrict__ rates) {
  __shared__ int red[SE_THREADS];
  const float* sim = stack + (long)blockIdx.x * N * V * N;
  int c = 0;
  for (int e = threadIdx.x; e < N * tail; e += SE_THREADS) {
    const int i = e / tail, v = V - tail + (e - i * tail);
    c += sim[((long)i * V + v) * N + i] > thres;
  }
  red[threadIdx.x] = c;
  __syncthreads();
  for (int s = SE_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) rates[blockIdx.x] = (float)red[0] / (float)tail / (float)N;
}

extern "C" int ssv_sv_accept_rate(const float* sim_stack, int nmat, int N, int V, int tail, float thres, float* rates, ssv_stream_t stream) {
  SSV_CHECK(sim_stack && rates, SSV_BAD_SHAPE, "sv_accept_rate: null pointer (sim_stack and rates are required)");
  SSV_CHECK(nmat >= 1 && N >= 1 && V >= 1 && tail >= 1 && tail <= V, SSV_BAD_SHAPE, "sv_accept_rate: need nmat >= 1, N >= 1 and 1 <= tail <= V; got nmat=%d N=%d V=%d tail=%d",
            nmat, N, V, tail);
  SSV_CHECK((long)N * tail <= 0x7fffffffL && (long)N * tail < (1L << 24), SSV_UNSUPPORTED, "sv_accept_rate: %ld trials per matrix are not exact in float32", (long)N * tail);
  hipLaunchKernelGGL(sv_accept_rate_kernel, dim3(nmat), dim3(SE_THREADS), 0, (hipStream_t)stream, sim_stack, N, V, tail, thres, rates);
  return ssv_check_launch("sv_accept_rate");
}
