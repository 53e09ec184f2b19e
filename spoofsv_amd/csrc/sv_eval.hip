// The speaker-verification test on the device (GE2E/train_speech_embedder.py:112-322 around the embedder), gfx950: the trial scores of
// get_centroids + get_cossim (ssv_sv_trial_scores), the threshold sweep that ends in EER and spoof rate (ssv_sv_eer_sweep) and the
// accept rate at a given threshold over a stack of score matrices (ssv_sv_accept_rate); and the counting of curve.py's two sweeps and of
// kaldi_ivectors/ivector_spoofrate.py, thousands of thresholds in one pass (ssv_sv_score_curve, ssv_score_list_curve_*).  Latency-class: 20 x 80 x 20 dot products of
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

// ---- spoof-rate / FRR curves: thousands of thresholds in one pass --------------------------------------------------------------------
// The sweep above gives every threshold a workgroup that reads the whole matrix: right for 50 thresholds, 5,000 passes for curve.py's.
// Here a workgroup owns a TILE of SC_TILE sorted thresholds, staged in LDS, and walks its matrix (or score list) once.  Per score x:
// p = the number of tile thresholds strictly below x (a lower-bound search; sorted thresholds make x > thr[t] the same as t < p, with
// duplicates too; every comparison of a NaN is false, so a NaN gives 0), then an integer atomicAdd on bin p of an LDS histogram of
// (SC_TILE + 1) bins x 4 classes.  The two ends never reach the LDS: p = 0 (x above no threshold of the tile) adds to no count, and a
// score above the whole tile -- the common case: a tile spans 0.0256 of curve.py's range -- is counted in registers and the wave's sum
// goes to the top bin once at the end, so a crowd of scores in one bin costs no serialised atomics.  (Scores crowding ONE bin inside the
// tile do serialise, 64 lanes on an address at worst: 125 walk steps of 4 atomics at the configuration's shape, microseconds.)  A suffix
// sum over the bins then gives the tile's rows of counts: a score above the tile is in every row, one below it in none, so tiles need
// nothing from each other -- no global atomics, no second launch, no arrival order; integer sums: the same bits on every run.
// SC_TILE = 256 = the workgroup: thread t owns threshold t in the scan and the store.  The LDS is 2 KiB of thresholds (as doubles) and
// 4 KiB of bins, no limit on occupancy; what the tile sets is the number of passes over the data, ceil(nthr / 256) = 20 for 5,000
// thresholds, against the workgroups there are to fill the device with (20 per matrix), and the 8 steps of a search.
#define SC_TILE 256

__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// STACK: scores = blockIdx.y-th matrix (N, V, N) of n = N * V * N trials, classes (whole matrix, own column, its first `head` rows, its
// last `tail` rows), NC = 4 columns of counts.  Otherwise a list of n items with class codes cls[e] (>= NC: counted nowhere), NC columns.
template <typename T, bool STACK>
__global__ __launch_bounds__(SC_TILE) void score_curve_kernel(const T* __restrict__ scores, const unsigned char* __restrict__ cls, long n, int N, int V, int head,
                                                              int tail, int NC, const T* __restrict__ thr, int nthr, int* __restrict__ counts) {
  __shared__ T th[SC_TILE];
  __shared__ int4 hist[SC_TILE + 1];
  const int tid = threadIdx.x, t0 = blockIdx.x * SC_TILE, nt = min(SC_TILE, nthr - t0);
  if (tid < nt) th[tid] = thr[t0 + tid];
  hist[tid] = make_int4(0, 0, 0, 0);
  if (tid == 0) hist[SC_TILE] = make_int4(0, 0, 0, 0);
  __syncthreads();
  const T lo_t = th[0], hi_t = th[nt - 1];
  const T* __restrict__ s = scores + (STACK ? (long)blockIdx.y * n : 0L);
  int* bins = (int*)hist;
  int top[4] = {0, 0, 0, 0};
  for (long e = tid; e < n; e += SC_TILE) {
    const T x = s[e];
    if (!(x > lo_t)) continue;                       // above no threshold of the tile (a NaN, -inf): in none of its counts
    unsigned mask;
    if (STACK) {
      const unsigned u = (unsigned)e, r = u / (unsigned)N;
      const int j = (int)(u - r * (unsigned)N), i = (int)(r / (unsigned)V), v = (int)(r - (unsigned)i * (unsigned)V);
      const unsigned own = i == j;
      mask = 1u | own << 1 | (own & (unsigned)(v < head)) << 2 | (own & (unsigned)(v >= V - tail)) << 3;
    } else {
      const unsigned c = cls[e];
      mask = c < (unsigned)NC ? 1u << c : 0u;
    }
    if (x > hi_t) {                                  // above the whole tile: the top bin, kept in registers
#pragma unroll
      for (int k = 0; k < 4; ++k) top[k] += (int)(mask >> k & 1u);
      continue;
    }
    int lo = 1, hi = nt - 1;                         // th[0] < x and not th[nt - 1] < x: p lies in [1, nt - 1]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (th[mid] < x) lo = mid + 1; else hi = mid;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (mask >> k & 1u) atomicAdd(&bins[lo * 4 + k], 1);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int w = sc_wave_sum(top[k]);
    if ((tid & 63) == 0 && w) atomicAdd(&bins[nt * 4 + k], w);
  }
  __syncthreads();
  // counts[t] = bins t + 1 ... SC_TILE summed (the bins past nt hold zeros): thread t starts from bin t + 1, eight doubling steps
  int4 a = hist[tid + 1];
  for (int d = 1; d < SC_TILE; d <<= 1) {
    int4 b = make_int4(0, 0, 0, 0);
    if (tid + d < SC_TILE) b = hist[tid + 1 + d];
    __syncthreads();
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    hist[tid + 1] = a;
    __syncthreads();
  }
  if (tid < nt) {
    int* out = counts + ((STACK ? (long)blockIdx.y * nthr : 0L) + t0 + tid) * NC;
    const int r[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < NC) out[k] = r[k];
  }
}

extern "C" int ssv_sv_curve_tile(void) { return SC_TILE; }

extern "C" int ssv_sv_score_curve(const float* sim_stack, int nmat, int N, int V, int head, int tail, const float* thr, int nthr, int* counts,
                                  ssv_stream_t stream) {
  SSV_CHECK(sim_stack && thr && counts, SSV_BAD_SHAPE, "sv_score_curve: null pointer (sim_stack, thr and counts are required)");
  SSV_CHECK(nmat >= 1 && N >= 1 && V >= 1 && nthr >= 1, SSV_BAD_SHAPE, "sv_score_curve: need nmat >= 1, N >= 1, V >= 1 and nthr >= 1; got nmat=%d N=%d V=%d nthr=%d",
            nmat, N, V, nthr);
  SSV_CHECK(head >= 0 && tail >= 0 && head <= V && tail <= V, SSV_BAD_SHAPE, "sv_score_curve: head=%d and tail=%d must lie in [0, V=%d]", head, tail, V);
  SSV_CHECK((long)N * V * N <= 0x7fffffffL, SSV_UNSUPPORTED, "sv_score_curve: %ld trials per matrix do not fit the int32 counts", (long)N * V * N);
  SSV_CHECK(nmat <= 65535, SSV_UNSUPPORTED, "sv_score_curve: nmat=%d matrices exceed the grid (65535 per call)", nmat);
  hipLaunchKernelGGL((score_curve_kernel<float, true>), dim3(ssv_cdiv(nthr, SC_TILE), nmat), dim3(SC_TILE), 0, (hipStream_t)stream, sim_stack,
                     (const unsigned char*)nullptr, (long)N * V * N, N, V, head, tail, 4, thr, nthr, counts);
  return ssv_check_launch("sv_score_curve");
}

template <typename T>
static int score_list_curve(const char* what, const T* scores, const unsigned char* cls, long n, int nclass, const T* thr, int nthr, int* counts,
                            ssv_stream_t stream) {
  SSV_CHECK(scores && cls && thr && counts, SSV_BAD_SHAPE, "%s: null pointer (scores, cls, thr and counts are required)", what);
  SSV_CHECK(n >= 1 && nthr >= 1 && nclass >= 1 && nclass <= 4, SSV_BAD_SHAPE, "%s: need n >= 1, nthr >= 1 and 1 <= nclass <= 4; got n=%ld nthr=%d nclass=%d", what, n,
            nthr, nclass);
  SSV_CHECK(n <= 0x7fffffffL, SSV_UNSUPPORTED, "%s: %ld items do not fit the int32 counts", what, n);
  hipLaunchKernelGGL((score_curve_kernel<T, false>), dim3(ssv_cdiv(nthr, SC_TILE)), dim3(SC_TILE), 0, (hipStream_t)stream, scores, cls, n, 1, 1, 0, 0, nclass, thr,
                     nthr, counts);
  return ssv_check_launch(what);
}

extern "C" int ssv_score_list_curve_f32(const float* scores, const unsigned char* cls, long n, int nclass, const float* thr, int nthr, int* counts,
                                        ssv_stream_t stream) {
  return score_list_curve<float>("score_list_curve_f32", scores, cls, n, nclass, thr, nthr, counts, stream);
}
extern "C" int ssv_score_list_curve_f64(const double* scores, const unsigned char* cls, long n, int nclass, const double* thr, int nthr, int* counts,
                                        ssv_stream_t stream) {
  return score_list_curve<double>("score_list_curve_f64", scores, cls, n, nclass, thr, nthr, counts, stream);
}
