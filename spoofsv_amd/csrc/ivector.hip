// The front half of the i-vector system on the device (the reference's kaldi_ivectors/run.sh up to the diagonal UBM; the algorithms are
// stated in include/ssv_hip.h, Kaldi itself is not reproduced), gfx950: cepstral features from the compact log-mel frames (DCT, deltas,
// sliding mean subtraction), per-frame Gaussian selection and posteriors of a diagonal-covariance GMM, the sufficient statistics
// sum_f gamma_fc [1, x, x^2] per segment, their float64 reduction and the M-step.
// The two GEMM-shaped kernels -- the log-likelihoods (F x 2D)(2D x C) and the statistics Gamma^T [1, X, X^2] -- run on
// v_mfma_f32_16x16x4_f32 whatever ssv_set_precision says: the quadratic form cancels (x^2 (-1/2 sigma^-2) against x mu sigma^-2), which a
// 16-bit split does not survive without scale lists, and K = 2D <= 256, so the fp32 rate is not what limits them.
// No float atomics anywhere; every sum runs in an order fixed by the shapes alone: the same inputs give the same bits.
// This file holds the kernels and their launchers, which know the tiles and refuse a shape beyond them (-2) before anything is launched;
// api_ivector.hip holds the C-ABI entries and the argument checks (-1).
#include <string.h>
#include "tv_triangle.h"          // tv_wg_sum, TV_LDS_MAX, tv_lds_limit_set; the limits and launchers (ivec_chain.h)

#define IV_FT 64                    // features: frames per workgroup of the delta pass
#define IV_MAX_W 8                  // largest delta window (the halo is 2 w frames on each side)
#define IV_MAX_CC 128               // most static coefficients (LDS: (IV_FT + 4 IV_MAX_W) x IV_MAX_CC floats = 48 KiB)
#define IV_CMN_RUN 64               // mean subtraction: consecutive frames one thread slides over
#define ST_TG 64                    // statistics: Gaussians per workgroup (16 per wave)
#define ST_TF 64                    // frames per step of the walk over a segment
#define ST_GS (ST_TF + 4)           // row stride of the Gaussian x frame tile (16-byte rows, b128 reads 4 banks apart per row)
#define ST_MAXB 17                  // value blocks of 16: 1 + 2 * 128 = 257 columns at most (the kernel is instantiated for 4, 12 and 17)
struct IvecDelta { float c1[2 * IV_MAX_W + 1]; float c2[4 * IV_MAX_W + 1]; };

// utterance / segment of a compact frame index: the LAST u in [0, U) with off[u] <= g, provided g < off[u + 1] (empty utterances are
// skipped: their two offsets are equal).  Returns false when g lies in no utterance.  The bounds come back clamped to [0, G]; the search
// ends whatever the table holds.
__device__ __forceinline__ bool iv_find_utt(const long* __restrict__ off, int U, long g, long G, long& a, long& b) {
  int lo = 0, hi = U + 1;                 // p = number of entries of off[0 .. U] that are <= g
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid + 1; else hi = mid;
  }
  if (lo == 0 || lo == U + 1) return false;
  a = min(max(off[lo - 1], 0L), G);
  b = min(max(off[lo], 0L), G);
  return g >= a && g < b;
}

// ---- features, pass 1: statics and deltas ------------------------------------------------------------------------------------------
// Workgroup = IV_FT consecutive compact frames (utterances may meet inside a tile).  The statics s = dct . mel of the tile and of a halo of
// order * w frames on each side are staged in LDS (one fmaf chain over the mel bins per element); the deltas then read them at frame
// indices clamped to the frame's own utterance -- |offset| <= order * w, so a clamped index never leaves the halo.  v = [s, d, dd] goes
// to the workspace; the mean subtraction is pass 2.
template <bool DCT>
__global__ __launch_bounds__(256) void ivec_delta_kernel(const float* __restrict__ mel, const long* __restrict__ utt_off, const float* __restrict__ dct,
                                                         float* __restrict__ v, long G, int M, int U, int Cc, int order, int w, const IvecDelta co) {
  extern __shared__ float st[];           // [IV_FT + 2 H][Cc]
  __shared__ long ua[IV_FT], ub[IV_FT];   // the utterance of every frame of the tile (ub = -1: none)
  const int tid = threadIdx.x, H = order * w, nst = IV_FT + 2 * H;
  const long g0 = (long)blockIdx.x * IV_FT, base = g0 - H;
  for (int e = tid; e < nst * Cc; e += 256) {
    const int r = e / Cc, c = e - r * Cc;
    const long g = base + r;
    float val = 0.f;
    if (g >= 0 && g < G) {
      const float* row = mel + g * M;
      if (DCT) {
        const float* d = dct + (long)c * M;
        for (int m = 0; m < M; ++m) val = fmaf(d[m], row[m], val);
      } else {
        val = row[c];
      }
    }
    st[e] = val;
  }
  if (tid < IV_FT) {
    long a = 0, b = -1;
    const long g = g0 + tid;
    if (g < G && !iv_find_utt(utt_off, U, g, G, a, b)) b = -1;
    ua[tid] = a;
    ub[tid] = b;
  }
  __syncthreads();
  const int cols = Cc * (order + 1);
  const long s_lo = max(base, 0L), s_hi = min(base + nst, G) - 1;       // the staged frames that exist
  for (int e = tid; e < IV_FT * Cc; e += 256) {
    const int r = e / Cc, c = e - r * Cc;
    const long g = g0 + r, a = ua[r], b = ub[r];
    if (g >= G || b < 0) continue;
    float* o = v + g * cols;
    o[c] = st[(r + H) * Cc + c];
    if (order >= 1) {
      float d1 = 0.f;
      for (int j = -w; j <= w; ++j) {
        const long q = min(max(min(max(g + j, a), b - 1), s_lo), s_hi);
        d1 = fmaf(co.c1[j + w], st[(int)(q - base) * Cc + c], d1);
      }
      o[Cc + c] = d1;
    }
    if (order >= 2) {
      float d2 = 0.f;
      for (int j = -2 * w; j <= 2 * w; ++j) {
        const long q = min(max(min(max(g + j, a), b - 1), s_lo), s_hi);
        d2 = fmaf(co.c2[j + 2 * w], st[(int)(q - base) * Cc + c], d2);
      }
      o[2 * Cc + c] = d2;
    }
  }
}

// ---- features, pass 2: centred sliding mean subtraction ------------------------------------------------------------------------------
// Thread = (column, run of IV_CMN_RUN frames).  The window [lo, hi) of a frame moves forward only inside an utterance, so the thread keeps
// its sum in DOUBLE and slides it: the entering rows added, the leaving ones subtracted, started afresh at every utterance.  The error of
// a double slide over a run is far below that of adding <= W float32 terms directly; nothing is a prefix sum over the utterance.
__global__ __launch_bounds__(256) void ivec_cmn_kernel(const float* __restrict__ v, const long* __restrict__ utt_off, float* __restrict__ out, long G, int U,
                                                       int cols, int W) {
  const int col = blockIdx.y * 64 + threadIdx.x;
  if (col >= cols) return;
  const long f0 = ((long)blockIdx.x * 4 + threadIdx.y) * IV_CMN_RUN, f1 = min(f0 + IV_CMN_RUN, G);
  long a = 0, b = -1, cl = 0, ch = 0;
  double sum = 0.0;
  for (long g = f0; g < f1; ++g) {
    if (!(g >= a && g < b)) {
      if (!iv_find_utt(utt_off, U, g, G, a, b)) { b = -1; continue; }
      sum = 0.0;
      cl = ch = -1;
    }
    const long T = b - a, t = g - a;
    long lo = t - W / 2, hi = lo + W;
    if (lo < 0) { lo = 0; hi = min(T, (long)W); }
    if (hi > T) { hi = T; lo = max(0L, T - W); }
    const long glo = a + lo, ghi = a + hi;
    if (cl < 0) cl = ch = glo;
    while (ch < ghi) { sum += (double)v[ch * cols + col]; ++ch; }
    while (cl < glo) { sum -= (double)v[cl * cols + col]; ++cl; }
    out[g * cols + col] = (float)((double)v[g * cols + col] - sum / (double)(hi - lo));
  }
}

int ivec_launch_features(const float* mel, const long* utt_off, const float* dct, float* out, float* v, long G, int M, int U, int Cc, int order, int w, int W,
                         hipStream_t st) {
  SSV_CHECK(Cc <= IV_MAX_CC && (order == 0 || w <= IV_MAX_W), SSV_UNSUPPORTED, "ivec_features: %d static coefficients (at most %d) or delta window %d (at most %d)",
            Cc, IV_MAX_CC, w, IV_MAX_W);
  SSV_CHECK((G + IV_FT - 1) / IV_FT <= 0x7fffffffL, SSV_UNSUPPORTED, "ivec_features: %ld frames exceed the grid", G);
  if (order == 0) w = 0;
  // first order: c_j = j / (2 sum_{i = 1..w} i^2); second order: c (*) c, as add-deltas builds it; each rounded once from double
  IvecDelta co;
  memset(&co, 0, sizeof(co));
  double c1[2 * IV_MAX_W + 1] = {0.0}, c2[4 * IV_MAX_W + 1] = {0.0}, den = 0.0;
  for (int i = 1; i <= w; ++i) den += 2.0 * i * i;
  for (int j = -w; j <= w && w > 0; ++j) c1[j + w] = (double)j / den;
  for (int i = 0; i <= 2 * w && w > 0; ++i)
    for (int j = 0; j <= 2 * w; ++j) c2[i + j] += c1[i] * c1[j];
  for (int j = 0; j <= 2 * w; ++j) co.c1[j] = (float)c1[j];
  for (int j = 0; j <= 4 * w; ++j) co.c2[j] = (float)c2[j];
  const size_t lds = (size_t)(IV_FT + 2 * order * w) * Cc * sizeof(float);
  const dim3 grid(ssv_cdiv(G, IV_FT));
  if (dct) hipLaunchKernelGGL(ivec_delta_kernel<true>, grid, dim3(256), lds, st, mel, utt_off, dct, v, G, M, U, Cc, order, w, co);
  else hipLaunchKernelGGL(ivec_delta_kernel<false>, grid, dim3(256), lds, st, mel, utt_off, dct, v, G, M, U, Cc, order, w, co);
  SSV_TRY(ssv_check_launch("ivec_delta"));
  const int cols = Cc * (order + 1);
  hipLaunchKernelGGL(ivec_cmn_kernel, dim3(ssv_cdiv(G, 4 * IV_CMN_RUN), ssv_cdiv(cols, 64)), dim3(64, 4), 0, st, (const float*)v, utt_off, out, G, U, cols, W);
  return ssv_check_launch("ivec_cmn");
}

// ---- Gaussian selection and posteriors -----------------------------------------------------------------------------------------------
// Workgroup = 16 RB frames x ALL C Gaussians.  L = [X | X^2] [A | B]^T + g on the fp32 MFMA: the frames' [x, x^2] rows are staged in LDS
// (each half padded to DP = D rounded up to 8, so K = 2 DP is a multiple of 16), the parameter planes stream from memory in fragment
// order -- lane (column c = lane & 15, quarter q = lane >> 4) loads the 4 floats k = 16 ch + 4 q .. + 3 of row c, and MFMA step s of the
// chunk takes k = 16 ch + 4 q + s on both operands: a permutation of K, the same for every element, so a 16-byte load feeds four steps.
// The accumulators start from g.  Wave w of 16 takes the column blocks 2 w, 2 w + 1, 2 w + 32, ...; each B fragment feeds RB row blocks.
// The tile's L stays in LDS (row stride C16 + 4: the four row groups of an accumulator land 16 banks apart); then wave w finishes frames
// w, w + 16, ...: nsel rounds of (lane-local arg max over its strided elements, butterfly over the wave with the smaller index winning a
// tie, the owner marks its element), soft max over the selected in a fixed butterfly order, pruning, renormalisation.
#define GS_THREADS 1024             // selection: 16 waves, four per SIMD -- the LDS tile allows one workgroup a CU, so the waves that hide the
#define GS_WAVES (GS_THREADS / 64)  // parameter planes' load latency and share the frames of the finish must come from inside it
template <int CTRL> __device__ __forceinline__ int gs_dpp_int(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ void gs_argmax_step(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

template <int RB>
__global__ __launch_bounds__(GS_THREADS) void gmm_gselect_kernel(const float* __restrict__ X, const float* __restrict__ PA, const float* __restrict__ PB,
                                                          const float* __restrict__ gc, int* __restrict__ idx, float* __restrict__ post,
                                                          float* __restrict__ loglik, long F, int D, int C, int nsel, float min_post, int DP, int LS) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TF = 16 * RB;
  const int XS = 2 * DP + 4;
  float* Ls = lds;                        // [TF][LS]
  float* Xs = lds + TF * LS;              // [TF][XS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cq = lane & 15;
  const long f0 = (long)blockIdx.x * TF;
  for (int e = tid; e < TF * DP; e += GS_THREADS) {
    const int r = e / DP, d = e - r * DP;
    const long f = f0 + r;
    const float x = (f < F && d < D) ? X[f * D + d] : 0.f;
    Xs[r * XS + d] = x;
    Xs[r * XS + DP + d] = x * x;
  }
  __syncthreads();
  const int ncb = (C + 15) >> 4, nch = DP >> 3;      // column blocks; K chunks of 16 (2 DP / 16)
  const bool vec = (D & 3) == 0;
  for (int cb = wave * 2; cb < ncb; cb += 2 * GS_WAVES) {
    int cc[2];
    bool cok[2];
    f32x4 acc[RB][2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int c = (cb + nb) * 16 + cq;
      cok[nb] = c < C;
      cc[nb] = min(c, C - 1);
      const float gv = cok[nb] ? gc[cc[nb]] : 0.f;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) acc[rb][nb] = (f32x4){gv, gv, gv, gv};
    }
    auto load_b = [&](int ch, float (&b)[2][4]) {
      const int k = ch * 16 + 4 * kq;
      const float* __restrict__ P = k < DP ? PA : PB;
      const int d = k < DP ? k : k - DP;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float* row = P + (long)cc[nb] * D;
        if (vec) {
          // D % 4 == 0: d + 3 < D whenever d < D, and the planes' rows are 16-byte aligned (api_ivector.hip checks the bases)
          const float4 q = d < D ? *reinterpret_cast<const float4*>(row + d) : make_float4(0.f, 0.f, 0.f, 0.f);
          b[nb][0] = q.x; b[nb][1] = q.y; b[nb][2] = q.z; b[nb][3] = q.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) b[nb][i] = d + i < D ? row[d + i] : 0.f;
        }
      }
    };
    float bcur[2][4], bnext[2][4];
    load_b(0, bcur);
    for (int ch = 0; ch < nch; ++ch) {
      if (ch + 1 < nch) load_b(ch + 1, bnext);
      float4 a[RB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) a[rb] = *reinterpret_cast<const float4*>(Xs + (rb * 16 + cq) * XS + ch * 16 + 4 * kq);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const float av = s == 0 ? a[rb].x : s == 1 ? a[rb].y : s == 2 ? a[rb].z : a[rb].w;
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bcur[nb][s], acc[rb][nb], 0, 0, 0);
        }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int i = 0; i < 4; ++i) bcur[nb][i] = bnext[nb][i];
    }
    // C/D layout: column = lane & 15 (the Gaussian), row = (lane >> 4) * 4 + r (the frame)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      if (!cok[nb]) continue;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ls[(rb * 16 + kq * 4 + r) * LS + cc[nb]] = acc[rb][nb][r];
    }
  }
  __syncthreads();
  const float NEG = -__builtin_huge_valf();
  for (int r = wave; r < TF; r += GS_WAVES) {
    const long f = f0 + r;
    if (f >= F) break;
    float* row = Ls + r * LS;
    float myv = NEG;
    int myi = 0;
    for (int j = 0; j < nsel; ++j) {
      float bv = NEG;
      int bi = 0x7fffffff;
      for (int i = lane; i < C; i += 64) {
        const float x = row[i];
        if (x > bv) { bv = x; bi = i; }
      }
      // arg max over the wave, the smaller index winning a tie: inside a row of 16 lanes on the VALU (DPP; after a step both lanes of a
      // pair agree, so the mirrors serve as the xor 4 and xor 8 steps), then across the four rows
      gs_argmax_step(bv, bi, ssv_dpp_mov<0xB1>(bv), gs_dpp_int<0xB1>(bi));
      gs_argmax_step(bv, bi, ssv_dpp_mov<0x4E>(bv), gs_dpp_int<0x4E>(bi));
      gs_argmax_step(bv, bi, ssv_dpp_mov<0x141>(bv), gs_dpp_int<0x141>(bi));
      gs_argmax_step(bv, bi, ssv_dpp_mov<0x140>(bv), gs_dpp_int<0x140>(bi));
      gs_argmax_step(bv, bi, __shfl_xor(bv, 16), __shfl_xor(bi, 16));
      gs_argmax_step(bv, bi, __shfl_xor(bv, 32), __shfl_xor(bi, 32));
      if (bi == 0x7fffffff) bi = j;       // nothing left above -inf (a row of NaNs): an index inside [0, C), never a stray one
      else if ((bi & 63) == lane) row[bi] = NEG;
      if (lane == j) { myv = bv; myi = bi; }
    }
    const float mx = __shfl(myv, 0);
    const float e = lane < nsel ? expf(myv - mx) : 0.f;
    const float s = ssv_wave_sum(e);
    float p = e / s;
    if (min_post > 0.f) {
      if (lane != 0 && p < min_post) p = 0.f;     // lane 0 holds the largest: never pruned
      p = p / ssv_wave_sum(p);
    }
    if (lane < nsel) {
      idx[f * nsel + lane] = myi;
      post[f * nsel + lane] = p;
    }
    if (lane == 0) loglik[f] = mx + logf(s);
  }
}

// ---- sufficient statistics -----------------------------------------------------------------------------------------------------------
// Workgroup = (segment s, tile of ST_TG Gaussians); slab[s][c][:] = sum over the segment's frames of gamma_fc [1, x_f, x_f^2] as the
// product Gamma^T V with K = frames, on the fp32 MFMA.  The segment is walked in tiles of ST_TF frames: V = [1, x, x^2] is staged, the
// Gamma tile zeroed, and the sparse posteriors whose Gaussian lies in the tile are deposited -- thread f owns frame f's column and adds
// its entries in list order, so a repeated index sums, in a fixed order, and nothing races.  Wave w multiplies the Gaussians
// 16 w .. 16 w + 15 against every value block.  A step's product is an fp32 chain over its ST_TF frames starting from zero; the steps are
// added in DOUBLE registers and the slab entry is that sum rounded once -- the second-order sums feed var = S / N - mu^2, which cancels,
// and an fp32 chain over a 2048-frame run costs the M-step a digit that the double walk keeps.  The K order inside a step is permuted as
// in gmm_gselect_kernel; it depends on the segment's length alone.
template <int MAXB>                       // value blocks of 16 the instantiation has registers for (nvb <= MAXB)
__global__ __launch_bounds__(256, 2) void gmm_stats_kernel(const float* __restrict__ X, const int* __restrict__ idx, const float* __restrict__ post,
                                                        const long* __restrict__ seg_off, float* __restrict__ slab, long F, int D, int C, int nsel,
                                                        int order, int gtiles, int NV, int nvb, int VS) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Gs = lds;                        // [ST_TG][ST_GS]: Gaussian x frame
  float* Vs = lds + ST_TG * ST_GS;        // [ST_TF][VS]: frame x value
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cq = lane & 15;
  const long s = blockIdx.x / gtiles;
  const int c0 = (int)(blockIdx.x % gtiles) * ST_TG;
  long a = min(max(seg_off[s], 0L), F), b = min(max(seg_off[s + 1], 0L), F);
  if (b < a) b = a;
  double sum[MAXB][4];
#pragma unroll
  for (int cb = 0; cb < MAXB; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[cb][r] = 0.0;
  const int nv16 = nvb * 16;
  for (long t0 = a; t0 < b; t0 += ST_TF) {
    __syncthreads();                      // the previous tile's MFMAs have read Gs and Vs
    for (int e = tid; e < ST_TG * ST_GS; e += 256) Gs[e] = 0.f;
    for (int e = tid; e < ST_TF * nv16; e += 256) {
      const int r = e / nv16, v = e - r * nv16;
      const long f = t0 + r;
      float val = 0.f;
      if (f < b && v < NV) {
        if (v == 0) val = 1.f;
        else if (v <= D) val = X[f * D + (v - 1)];
        else { const float x = X[f * D + (v - 1 - D)]; val = x * x; }
      }
      Vs[r * VS + v] = val;
    }
    __syncthreads();
    if (tid < ST_TF && t0 + tid < b) {
      const int* ip = idx + (t0 + tid) * nsel;
      const float* pp = post + (t0 + tid) * nsel;
      for (int j = 0; j < nsel; ++j) {
        const int i = ip[j], li = i - c0;
        if (i >= 0 && i < C && li >= 0 && li < ST_TG) Gs[li * ST_GS + tid] += pp[j];
      }
    }
    __syncthreads();
    f32x4 acc[MAXB];
#pragma unroll
    for (int cb = 0; cb < MAXB; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < ST_TF / 16; ++ch) {
      const float4 av = *reinterpret_cast<const float4*>(Gs + (wave * 16 + cq) * ST_GS + ch * 16 + 4 * kq);
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const float ag = s4 == 0 ? av.x : s4 == 1 ? av.y : s4 == 2 ? av.z : av.w;
        const float* vrow = Vs + (ch * 16 + 4 * kq + s4) * VS + cq;
#pragma unroll
        for (int cb = 0; cb < MAXB; ++cb)
          if (cb < nvb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag, vrow[cb * 16], acc[cb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int cb = 0; cb < MAXB; ++cb)
      if (cb < nvb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[cb][r] += (double)acc[cb][r];
      }
  }
  // C/D layout: column = lane & 15 (the value), row = (lane >> 4) * 4 + r (the Gaussian)
#pragma unroll
  for (int cb = 0; cb < MAXB; ++cb) {
    const int v = cb * 16 + cq;
    if (cb >= nvb || v >= NV) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + wave * 16 + kq * 4 + r;
      if (c < C) slab[(s * C + c) * NV + v] = (float)sum[cb][r];
    }
  }
}

// out[e] = sum over s of slab[s][e], added in ascending s, in double
__global__ __launch_bounds__(256) void gmm_reduce_kernel(const float* __restrict__ slab, double* __restrict__ out, int S, long n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += (double)slab[(long)s * n + e];
  out[e] = acc;
}

// ---- M-step ----------------------------------------------------------------------------------------------------------------------------
// Workgroup = Gaussian c, all in double.  stats != null: the M-step from (C, 1 + 2 D) statistics (every workgroup adds the C occupancies
// and the C floored weights itself, by the same tree: the same bits everywhere); stats == null: the planes of the given w, mu, var.
__global__ __launch_bounds__(256) void gmm_update_kernel(const double* __restrict__ stats, const double* __restrict__ w_in, double* __restrict__ w_out,
                                                         double* __restrict__ mu, double* __restrict__ var, float* __restrict__ PA, float* __restrict__ PB,
                                                         float* __restrict__ gc, int C, int D, double var_floor, double min_count, double min_weight) {
  __shared__ double sm[256];
  const int c = blockIdx.x, tid = threadIdx.x, NV = 1 + 2 * D;
  double wc;
  bool starved = false;
  if (stats) {
    double part = 0.0;
    for (int i = tid; i < C; i += 256) part += stats[(long)i * NV];
    const double ntot = tv_wg_sum(part, sm);
    part = 0.0;
    for (int i = tid; i < C; i += 256) {
      const double n = stats[(long)i * NV], wi = n / ntot;
      part += (n < min_count || !(n > 0.0)) ? fmax(wi, min_weight) : wi;
    }
    const double wtot = tv_wg_sum(part, sm);
    const double n = stats[(long)c * NV];
    starved = n < min_count || !(n > 0.0);
    wc = (starved ? fmax(n / ntot, min_weight) : n / ntot) / wtot;
    if (tid == 0) w_out[c] = wc;
  } else {
    wc = w_in[c];
  }
  double part = 0.0;
  for (int d = tid; d < D; d += 256) {
    double m = mu[(long)c * D + d], v = var[(long)c * D + d];
    if (stats && !starved) {
      const double n = stats[(long)c * NV];
      m = stats[(long)c * NV + 1 + d] / n;
      v = fmax(stats[(long)c * NV + 1 + D + d] / n - m * m, var_floor);
      mu[(long)c * D + d] = m;
      var[(long)c * D + d] = v;
    }
    PA[(long)c * D + d] = (float)(m / v);
    PB[(long)c * D + d] = (float)(-0.5 / v);
    part += log(6.283185307179586476925 * v) + m * m / v;
  }
  const double q = tv_wg_sum(part, sm);
  if (tid == 0) gc[c] = (float)(log(wc) - 0.5 * q);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
int ivec_gselect_tile(int D, int C, size_t* lds_bytes) {
  if (D < 1 || C < 1 || D > IVEC_MAX_D || C > IVEC_MAX_C) return 0;
  const int DP = (D + 7) & ~7, LS = ((C + 15) & ~15) + 4, XS = 2 * DP + 4;
  for (int tf = 32; tf >= 16; tf >>= 1) {
    const size_t need = (size_t)tf * (LS + XS) * sizeof(float);
    if (need <= TV_LDS_MAX) {
      if (lds_bytes) *lds_bytes = need;
      return tf;
    }
  }
  return 0;
}

static int iv_lds_limit() {               // the kernels below take more than 64 KB of dynamic LDS: say so once per device
  static std::atomic<int> done[64];
  const void* ks[5] = {(const void*)gmm_gselect_kernel<1>, (const void*)gmm_gselect_kernel<2>, (const void*)gmm_stats_kernel<4>,
                       (const void*)gmm_stats_kernel<12>, (const void*)gmm_stats_kernel<ST_MAXB>};
  return tv_lds_limit_set(done, ks, 5, "ivector");
}

int ivec_launch_gselect(const float* X, const float* A, const float* B, const float* g, int* idx, float* post, float* loglik, long F, int D, int C, int nsel,
                        float min_post, hipStream_t st) {
  size_t lds = 0;
  const int tf = ivec_gselect_tile(D, C, &lds);
  SSV_CHECK(tf > 0 && nsel <= IVEC_MAX_NSEL, SSV_UNSUPPORTED, "gmm_diag_gselect: D=%d (at most %d), C=%d (at most %d) or nsel=%d (at most %d) beyond the tiles", D, IVEC_MAX_D,
            C, IVEC_MAX_C, nsel, IVEC_MAX_NSEL);
  SSV_CHECK((F + tf - 1) / tf <= 0x7fffffffL, SSV_UNSUPPORTED, "gmm_diag_gselect: %ld frames exceed the grid", F);
  SSV_TRY(iv_lds_limit());
  const int DP = (D + 7) & ~7, LS = ((C + 15) & ~15) + 4;
  const dim3 grid(ssv_cdiv(F, tf));
  if (tf == 32) hipLaunchKernelGGL(gmm_gselect_kernel<2>, grid, dim3(GS_THREADS), lds, st, X, A, B, g, idx, post, loglik, F, D, C, nsel, min_post, DP, LS);
  else hipLaunchKernelGGL(gmm_gselect_kernel<1>, grid, dim3(GS_THREADS), lds, st, X, A, B, g, idx, post, loglik, F, D, C, nsel, min_post, DP, LS);
  return ssv_check_launch("gmm_diag_gselect");
}

int ivec_launch_stats(const float* X, const int* idx, const float* post, const long* seg_off, float* slab, long F, int D, int C, int nsel, int S, int order,
                      hipStream_t st) {
  SSV_CHECK(D <= IVEC_MAX_D && C <= IVEC_MAX_C && nsel <= IVEC_MAX_NSEL, SSV_UNSUPPORTED, "gmm_diag_stats: D=%d (at most %d), C=%d (at most %d) or nsel=%d (at most %d) beyond the tiles",
            D, IVEC_MAX_D, C, IVEC_MAX_C, nsel, IVEC_MAX_NSEL);
  const int NV = 1 + order * D, nvb = (NV + 15) >> 4, VS = nvb * 16 + 4, gtiles = ssv_cdiv(C, ST_TG);
  SSV_CHECK((long)S * gtiles <= 0x7fffffffL, SSV_UNSUPPORTED, "gmm_diag_stats: %d segments x %d Gaussian tiles exceed the grid", S, gtiles);
  const size_t lds = ((size_t)ST_TG * ST_GS + (size_t)ST_TF * VS) * sizeof(float);
  SSV_TRY(iv_lds_limit());
  const dim3 grid((unsigned)((long)S * gtiles));
#define IV_STATS(MAXB_) hipLaunchKernelGGL(gmm_stats_kernel<MAXB_>, grid, dim3(256), lds, st, X, idx, post, seg_off, slab, F, D, C, nsel, order, gtiles, NV, nvb, VS)
  if (nvb <= 4) IV_STATS(4);
  else if (nvb <= 12) IV_STATS(12);      // (an instantiation for 8 spills: hipcc hoists every LDS read of the step there)
  else IV_STATS(ST_MAXB);
#undef IV_STATS
  return ssv_check_launch("gmm_diag_stats");
}

int ivec_launch_reduce(const float* slab, double* out, int S, long n, hipStream_t st) {
  hipLaunchKernelGGL(gmm_reduce_kernel, dim3(ssv_cdiv(n, 256)), dim3(256), 0, st, slab, out, S, n);
  return ssv_check_launch("gmm_stats_reduce");
}

int ivec_launch_update(const double* stats, const double* w_in, double* w_out, double* mu, double* var, float* A, float* B, float* g, int C, int D,
                       double var_floor, double min_count, double min_weight, hipStream_t st) {
  hipLaunchKernelGGL(gmm_update_kernel, dim3(C), dim3(256), 0, st, stats, w_in, w_out, mu, var, A, B, g, C, D, var_floor, min_count, min_weight);
  return ssv_check_launch("gmm_diag_update");
}
