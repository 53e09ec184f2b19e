// The full-covariance UBM on the device (include/ssv_hip.h, "I-vector groundwork: full-covariance UBM"), gfx950: the whitening planes of a
// mixture (Cholesky, triangular inverse and W^T W of the packed float64 triangle in LDS, tv_triangle.h), the Gaussian-major selection
// lists (a stable counting sort of the slots f * nsel + j by their Gaussian), the log-likelihoods and posteriors over the selected pairs,
// the centred second-order statistics over each Gaussian's list, the M-step and the extractor's planes G = Sigma^-1 T, Pk = T^T G.
// The two hot kernels walk a Gaussian's list in tiles of FGMM_TILE pairs: the pairs' frame rows are gathered into LDS and centred on the
// Gaussian's float32 mean (one subtraction, before any product), and the products run on v_mfma_f32_16x16x4_f32 whatever
// ssv_set_precision says -- K is D (likelihoods) or 64 pairs (statistics), so the fp32 rate is not what limits them (ivector.hip).  What
// a workgroup stages once -- Wt_c, 14 KB at D = 60 -- serves all pairs of its run: that sharing is the point of the Gaussian-major order.
// No float atomics anywhere (the counting sort adds INTEGERS in LDS, and no position depends on them arriving in any order); every sum
// runs in an order fixed by the shapes and the selection lists alone: the same inputs give the same bits.
// This file holds the kernels and their launchers; api_fgmm.hip holds the C-ABI entries and the argument checks.
#include "tv_triangle.h"          // the packed triangle, tv_wg_sum, tv_lds_limit_set; the limits, FGMM_TILE, FGMM_SL and the launchers (ivec_chain.h)

#define FG_SB 32                    // extractor planes: columns of T one workgroup owns

// ---- planes and M-step -----------------------------------------------------------------------------------------------------------------
// tri = packed Sigma -> its Cholesky factor in place; logdet = log|Sigma| from the pivots.  False at a pivot that is not positive or, with
// floor > 0, when some L_ii^2 < floor (the conditional variance of dimension i given those before it).  Every thread reads the same
// values from LDS, so the whole workgroup takes the same branch.
__device__ inline bool fg_factor(double* tri, double* col, int D, double floor, double& logdet) {
  if (!tv_cholesky(tri, col, nullptr, D)) return false;
  double ld = 0.0;
  bool ok = true;
  for (int i = 0; i < D; ++i) {
    const double l = tri[tv_tri(i, i)];
    ld += log(l);
    if (l * l < floor) ok = false;
  }
  logdet = 2.0 * ld;
  return ok;
}

// tri = the factor L -> W = L^-1 (written to Wt_c as float32, exact zeros above the diagonal), then W^T W = Sigma^-1 (written to icov_c)
__device__ inline void fg_whiten(double* tri, double* col, double* part, float* __restrict__ Wt_c, double* __restrict__ icov_c, int D) {
  const int tid = threadIdx.x, Pd = D * (D + 1) / 2;
  tv_trtri(tri, col, D);
  for (int e = tid; e < D * D; e += 256) {
    const int i = e / D, j = e - i * D;
    Wt_c[e] = j <= i ? (float)tri[tv_tri(i, j)] : 0.f;
  }
  __syncthreads();
  tv_lauum(tri, col, part, D);
  for (int e = tid; e < Pd; e += 256) icov_c[e] = tri[e];
}

__device__ __forceinline__ double fg_new_cov(const double* __restrict__ S2, double n, const double* dl, int i, int j) {
  return fma(-dl[i], dl[j], S2[tv_tri(i, j)] / n);
}

// Workgroup = Gaussian c, all in double, the packed triangle in LDS.  stats == null: the planes of the given w, mu, cov (g complete).
// stats != null: the M-step's mean and covariance with the kept rule, the planes of the result, and in w[c] the part of g that does not
// depend on the weights, -1/2 (D log 2 pi + log|Sigma_c|): fgmm_weights_kernel, which needs every Gaussian's kept flag, finishes w and g.
__global__ __launch_bounds__(256) void fgmm_planes_kernel(const double* __restrict__ stats, double* __restrict__ w, double* __restrict__ mu,
                                                          double* __restrict__ cov, float* __restrict__ Wt, float* __restrict__ muf, float* __restrict__ g,
                                                          double* __restrict__ icov, int* __restrict__ kept, int D, double var_floor, double min_count) {
  extern __shared__ __attribute__((aligned(16))) double fg_lds[];
  const int c = blockIdx.x, tid = threadIdx.x, Pd = D * (D + 1) / 2, NV = 1 + D + Pd;
  double* tri = fg_lds;                   // [Pd]
  double* col = tri + Pd;                 // [D]
  double* dl = col + D;                   // [D]
  double* part = dl + D;                  // [256]
  double* mu_c = mu + (long)c * D;
  double* cov_c = cov + (long)c * Pd;
  float* Wt_c = Wt + (long)c * D * D;
  double* icov_c = icov + (long)c * Pd;
  double logdet = 0.0;
  bool keep = true, ok = false;
  if (stats) {
    const double* sc = stats + (long)c * NV;
    const double n = sc[0];
    keep = n < min_count || !(n > 0.0);
    if (!keep) {
      for (int d = tid; d < D; d += 256) dl[d] = sc[1 + d] / n;
      __syncthreads();
      for (int i = 0; i < D; ++i)
        for (int j = tid; j <= i; j += 256) tri[tv_tri(i, j)] = fg_new_cov(sc + 1 + D, n, dl, i, j);
      __syncthreads();
      ok = fg_factor(tri, col, D, var_floor, logdet);
      __syncthreads();
      if (ok) {
        for (int i = 0; i < D; ++i)
          for (int j = tid; j <= i; j += 256) cov_c[tv_tri(i, j)] = fg_new_cov(sc + 1 + D, n, dl, i, j);
        for (int d = tid; d < D; d += 256) mu_c[d] = mu_c[d] + dl[d];
      } else {
        keep = true;
      }
    }
    if (tid == 0) kept[c] = keep ? 1 : 0;
  }
  if (keep) {                             // the Gaussian's own covariance: nothing of mu, cov is written
    for (int e = tid; e < Pd; e += 256) tri[e] = cov_c[e];
    __syncthreads();
    ok = fg_factor(tri, col, D, -1.0, logdet);
    __syncthreads();
  }
  if (!ok) {                              // not positive definite: NaN planes for this Gaussian, nothing else is touched
    const float qn = __builtin_nanf("");
    for (int e = tid; e < D * D; e += 256) Wt_c[e] = qn;
    for (int e = tid; e < Pd; e += 256) icov_c[e] = (double)qn;
    for (int d = tid; d < D; d += 256) muf[(long)c * D + d] = qn;
    if (tid == 0) {
      if (stats) w[c] = (double)qn;
      else g[c] = qn;
    }
    return;
  }
  fg_whiten(tri, col, part, Wt_c, icov_c, D);
  for (int d = tid; d < D; d += 256) muf[(long)c * D + d] = (float)mu_c[d];      // (each thread reads back what it wrote itself)
  if (tid == 0) {
    const double gp = -0.5 * ((double)D * 1.8378770664093454835606594728112 + logdet);
    if (stats) w[c] = gp;
    else g[c] = (float)(log(w[c]) + gp);
  }
}

// One workgroup: w_c = N_c / sum N, a kept Gaussian taking max(w_c, min_weight), renormalised to sum 1 (ssv_gmm_diag_update's rule with
// "starved" read as "kept"); g_c = log w_c + what fgmm_planes_kernel left in w[c], rounded once.
__global__ __launch_bounds__(256) void fgmm_weights_kernel(const double* __restrict__ stats, const int* __restrict__ kept, double* __restrict__ w,
                                                           float* __restrict__ g, int C, int NV, double min_weight) {
  __shared__ double sm[256];
  const int tid = threadIdx.x;
  double p = 0.0;
  for (int i = tid; i < C; i += 256) p += stats[(long)i * NV];
  const double ntot = tv_wg_sum(p, sm);
  p = 0.0;
  for (int i = tid; i < C; i += 256) {
    const double wi = stats[(long)i * NV] / ntot;
    p += kept[i] ? fmax(wi, min_weight) : wi;
  }
  const double wtot = tv_wg_sum(p, sm);
  for (int i = tid; i < C; i += 256) {
    const double wi = stats[(long)i * NV] / ntot, wc = (kept[i] ? fmax(wi, min_weight) : wi) / wtot, gp = w[i];
    w[i] = wc;
    g[i] = (float)(log(wc) + gp);
  }
}

// ---- the Gaussian-major selection lists ----------------------------------------------------------------------------------------------
// A stable counting sort of the n = F nsel slots by idx[slot], in three steps over blocks of FGMM_SL slots:
//   count:   counts[b][c] = slots of block b whose idx is c (integer adds in LDS);
//   prefix:  per c, counts[b][c] <- the slots of c in the blocks before b, and the list's length; one wave then scans the lengths to start;
//   scatter: ONE wave per block walks its slots in ascending order, 64 at a time; a lane's position is start[c] + counts[b][c] + the slots
//            of c the block has placed so far + the lanes below it that hold the same c (found by ballots over the 11 bits of c).
// Nothing in a position depends on the order in which workgroups or lanes ran.
__global__ __launch_bounds__(256) void fgmm_count_kernel(const int* __restrict__ idx, int* __restrict__ counts, long n, int C) {
  __shared__ int cnt[IVEC_MAX_C];
  const int tid = threadIdx.x;
  const long s0 = (long)blockIdx.x * FGMM_SL, s1 = min(s0 + FGMM_SL, n);
  for (int c = tid; c < C; c += 256) cnt[c] = 0;
  __syncthreads();
  for (long s = s0 + tid; s < s1; s += 256) {
    const int i = idx[s];
    if (i >= 0 && i < C) atomicAdd(&cnt[i], 1);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) counts[(long)blockIdx.x * C + c] = cnt[c];
}

__global__ __launch_bounds__(64) void fgmm_prefix_kernel(int* __restrict__ counts, int* __restrict__ start, int nb, int C) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  int run = 0;
  for (int b = 0; b < nb; ++b) {
    const int t = counts[(long)b * C + c];
    counts[(long)b * C + c] = run;
    run += t;
  }
  start[c + 1] = run;
}

__global__ __launch_bounds__(64) void fgmm_scan_kernel(int* __restrict__ start, int C) {      // start[1 ..] holds the lengths; one wave
  __shared__ int base[64];
  const int lane = threadIdx.x, chunk = (C + 63) / 64, c0 = min(lane * chunk, C), c1 = min(c0 + chunk, C);
  int s = 0;
  for (int c = c0; c < c1; ++c) s += start[c + 1];
  base[lane] = s;
  __syncthreads();
  if (lane == 0) {
    int run = 0;
    for (int l = 0; l < 64; ++l) { const int t = base[l]; base[l] = run; run += t; }
    start[0] = 0;
  }
  __syncthreads();
  int run = base[lane];
  for (int c = c0; c < c1; ++c) { run += start[c + 1]; start[c + 1] = run; }
}

__global__ __launch_bounds__(64) void fgmm_scatter_kernel(const int* __restrict__ idx, const int* __restrict__ counts, const int* __restrict__ start,
                                                          int* __restrict__ pairs, long n, int C) {
  __shared__ int cnt[IVEC_MAX_C];
  const int lane = threadIdx.x;
  const long s0 = (long)blockIdx.x * FGMM_SL, s1 = min(s0 + FGMM_SL, n);
  for (int c = lane; c < C; c += 64) cnt[c] = start[c] + counts[(long)blockIdx.x * C + c];
  __syncthreads();
  for (long sb = s0; sb < s1; sb += 64) {
    const long s = sb + lane;
    int c = s < s1 ? idx[s] : -1;
    const bool valid = c >= 0 && c < C;
    if (!valid) c = 0;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 11; ++bit) {
      const bool on = (c >> bit) & 1;
      const unsigned long long m = __ballot(on);
      peers &= on ? m : ~m;
    }
    const int below = __popcll(peers & ((1ull << lane) - 1ull)), all = __popcll(peers);
    int at = 0;
    if (valid) {
      at = cnt[c] + below;
      if (at >= 0 && at < n) pairs[at] = (int)s;
    }
    __syncthreads();
    if (valid && below == all - 1) cnt[c] = at + 1;      // the highest lane of the group moves the list's cursor
    __syncthreads();
  }
}

// ---- log-likelihoods over the selected pairs ---------------------------------------------------------------------------------------------
// the run [t0, t1) of tiles that workgroup r of nrun owns in a list of len pairs: it follows from len and nrun alone
__device__ __forceinline__ void fg_run(int len, int r, int nrun, int& t0, int& t1) {
  const int nt = (len + FGMM_TILE - 1) / FGMM_TILE, per = (nt + nrun - 1) / nrun;
  t0 = min(r * per, nt);
  t1 = min(t0 + per, nt);
}

// The tile's slots and frames into LDS, then the frames' rows gathered and centred: Xs[r][d] = X[f_r][d] - muf_c[d], one float32
// subtraction; rows beyond the list and columns d >= D are zero.  Ends with the barrier after which Xs may be read.
__device__ __forceinline__ void fg_gather(const float* __restrict__ X, const int* __restrict__ pairs, const float* mus, int* sl, int* fr, float* Xs, long p0,
                                          long pend, long n, long F, int D, int nsel, int DP, int XS) {
  const int tid = threadIdx.x;
  if (tid < FGMM_TILE) {
    int slot = p0 + tid < pend ? pairs[p0 + tid] : -1;
    if (slot < 0 || slot >= n) slot = -1;
    sl[tid] = slot;
    fr[tid] = slot < 0 ? -1 : slot / nsel;
  }
  __syncthreads();
  for (int e = tid; e < FGMM_TILE * DP; e += 256) {
    const int r = e / DP, d = e - r * DP, f = fr[r];
    Xs[r * XS + d] = (f >= 0 && f < F && d < D) ? X[(long)f * D + d] - mus[d] : 0.f;
  }
  __syncthreads();
}

// Workgroup = (Gaussian c, run r of its list).  Wt_c is staged once (row i = dimension i of z, zero beyond D); per tile of 64 pairs wave w
// takes the rows 16 w .. 16 w + 15: Z = Xc Wt_c^T on the fp32 MFMA, column block ib over the K chunks ch <= ib only (W is lower triangular:
// what is left out is exact zeros), the K order inside a chunk permuted as in gmm_gselect_kernel so that a 16-byte LDS read feeds four
// steps.  Each lane squares and adds its elements over the column blocks, the 16 lanes of a row group add up (DPP), and
// L[slot] = g_c - 1/2 |z|^2.  A row's value depends on its own frame, c and D alone.
__global__ __launch_bounds__(256) void fgmm_like_kernel(const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ muf,
                                                        const float* __restrict__ g, const int* __restrict__ start, const int* __restrict__ pairs,
                                                        float* __restrict__ L, long F, int D, int nsel, int nrun, int DP) {
  extern __shared__ __attribute__((aligned(16))) float lds[];      // all of the kernel's LDS is dynamic: the raised limit counts static LDS on top
  const int XS = DP + 4;
  float* Ws = lds;                        // [DP][XS]
  float* Xs = lds + DP * XS;              // [FGMM_TILE][XS]
  int* sl = reinterpret_cast<int*>(Xs + FGMM_TILE * XS);      // [FGMM_TILE]
  int* fr = sl + FGMM_TILE;               // [FGMM_TILE]
  float* mus = reinterpret_cast<float*>(fr + FGMM_TILE);      // [IVEC_MAX_D]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cq = lane & 15;
  const int c = blockIdx.x / nrun, r = blockIdx.x - c * nrun;
  const long n = F * nsel;
  const long a = min(max((long)start[c], 0L), n), b = min(max((long)start[c + 1], a), n);
  int t0, t1;
  fg_run((int)(b - a), r, nrun, t0, t1);
  if (t0 >= t1) return;
  const float* Wc = Wt + (long)c * D * D;
  for (int e = tid; e < DP * DP; e += 256) {
    const int i = e / DP, j = e - i * DP;
    Ws[i * XS + j] = (i < D && j < D) ? Wc[i * D + j] : 0.f;
  }
  if (tid < D) mus[tid] = muf[(long)c * D + tid];
  const float gc = g[c];
  const int nib = DP >> 4;
  for (int t = t0; t < t1; ++t) {
    __syncthreads();                      // the tile before has been read (first tile: mus is written)
    fg_gather(X, pairs, mus, sl, fr, Xs, a + (long)t * FGMM_TILE, b, n, F, D, nsel, DP, XS);
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ib = 0; ib < nib; ++ib) {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      for (int ch = 0; ch <= ib; ++ch) {
        const float4 av = *reinterpret_cast<const float4*>(Xs + (wave * 16 + cq) * XS + ch * 16 + 4 * kq);
        const float4 bv = *reinterpret_cast<const float4*>(Ws + (ib * 16 + cq) * XS + ch * 16 + 4 * kq);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
      }
      // C/D layout: column = lane & 15 (the dimension of z), row = (lane >> 4) * 4 + r (the pair)
#pragma unroll
      for (int q = 0; q < 4; ++q) sq[q] = fmaf(acc[q], acc[q], sq[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float s = ssv_row16_sum(sq[q]);
      const int slot = sl[wave * 16 + kq * 4 + q];
      if (cq == 0 && slot >= 0) L[slot] = gc - 0.5f * s;
    }
  }
}

// Thread = frame: over its nsel slots in idx's order, the log-sum-exp and the soft max of L over the slots whose idx lies in [0, C), the
// entries below min_post set to 0 (never the first largest) and the rest renormalised.  A slot outside has posterior 0 and takes no part;
// a frame without a slot inside has posteriors 0 and loglik -inf.  The values are recomputed pass by pass (no per-thread array).
__global__ __launch_bounds__(256) void fgmm_finish_kernel(const float* __restrict__ L, const int* __restrict__ idx, float* __restrict__ post,
                                                          float* __restrict__ loglik, long F, int C, int nsel, float min_post) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const float* Lf = L + f * nsel;
  const int* ip = idx + f * nsel;
  float* pf = post + f * nsel;
  const float NEG = -__builtin_huge_valf();
  float mx = NEG;
  int jm = -1;
  for (int j = 0; j < nsel; ++j) {
    const int i = ip[j];
    if (i < 0 || i >= C) continue;
    const float v = Lf[j];
    if (jm < 0 || v > mx) { mx = v; jm = j; }
  }
  if (jm < 0) {
    for (int j = 0; j < nsel; ++j) pf[j] = 0.f;
    loglik[f] = NEG;
    return;
  }
  float s = 0.f;
  for (int j = 0; j < nsel; ++j) {
    const int i = ip[j];
    if (i >= 0 && i < C) s += expf(Lf[j] - mx);
  }
  float s2 = 0.f;
  for (int j = 0; j < nsel; ++j) {
    const int i = ip[j];
    float p = (i >= 0 && i < C) ? expf(Lf[j] - mx) / s : 0.f;
    if (min_post > 0.f && j != jm && p < min_post) p = 0.f;
    s2 += p;
  }
  for (int j = 0; j < nsel; ++j) {
    const int i = ip[j];
    float p = (i >= 0 && i < C) ? expf(Lf[j] - mx) / s : 0.f;
    if (min_post > 0.f) {
      if (j != jm && p < min_post) p = 0.f;
      p = p / s2;
    }
    pf[j] = p;
  }
  loglik[f] = mx + logf(s);
}

// ---- centred statistics over the lists ---------------------------------------------------------------------------------------------------
// Workgroup = (Gaussian c, run r of its list); slab[r][c] = [N, S1 (D), S2 (Pd)] of the run, centred on muf_c.  Per tile of 64 pairs the
// rows are gathered and centred as above and gamma = post[slot] (a pruned pair is MULTIPLIED by its zero, not skipped); S2's 16 x 16
// blocks on and below the diagonal are dealt to the four waves (block t = rb (rb + 1) / 2 + cb to wave t % 4) and computed as
// (gamma Xc)^T Xc on the fp32 MFMA with K = the tile's 64 pairs in list order; S1 (thread d) and N (thread 255) are fp32 chains over the
// same 64 pairs.  Every tile's fp32 result is added to DOUBLE registers along the list (gmm_stats_kernel's reason: the M-step's
// Sigma = S2 / N - delta delta^T needs the digits), and the slab entry is that sum rounded once.  An empty run writes exact zeros.
template <int NBW>                        // blocks per wave the instantiation has registers for
__global__ __launch_bounds__(256) void fgmm_stats_kernel(const float* __restrict__ X, const float* __restrict__ muf, const float* __restrict__ post,
                                                         const int* __restrict__ start, const int* __restrict__ pairs, float* __restrict__ slab, long F, int D,
                                                         int C, int nsel, int nrun, int DP) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int sl[FGMM_TILE], fr[FGMM_TILE];
  __shared__ float mus[IVEC_MAX_D], gam[FGMM_TILE];
  const int XS = DP + 4;
  float* Xs = lds;                        // [FGMM_TILE][XS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cq = lane & 15;
  const int c = blockIdx.x / nrun, r = blockIdx.x - c * nrun;
  const long n = F * nsel;
  const long a = min(max((long)start[c], 0L), n), b = min(max((long)start[c + 1], a), n);
  int t0, t1;
  fg_run((int)(b - a), r, nrun, t0, t1);
  if (tid < D) mus[tid] = muf[(long)c * D + tid];
  const int nb = DP >> 4, nblk = nb * (nb + 1) / 2;
  int rbk[NBW], cbk[NBW];
#pragma unroll
  for (int i = 0; i < NBW; ++i) {
    const int t = wave + 4 * i;
    int rb = 0;
    while ((rb + 1) * (rb + 2) / 2 <= t) ++rb;
    rbk[i] = rb;
    cbk[i] = t - rb * (rb + 1) / 2;
  }
  double sum[NBW][4];
#pragma unroll
  for (int i = 0; i < NBW; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) sum[i][q] = 0.0;
  double s1 = 0.0;
  for (int t = t0; t < t1; ++t) {
    __syncthreads();
    fg_gather(X, pairs, mus, sl, fr, Xs, a + (long)t * FGMM_TILE, b, n, F, D, nsel, DP, XS);
    if (tid < FGMM_TILE) gam[tid] = sl[tid] >= 0 ? post[sl[tid]] : 0.f;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NBW; ++i) {
      if (wave + 4 * i >= nblk) continue;
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* ar = Xs + rbk[i] * 16 + cq;
      const float* br = Xs + cbk[i] * 16 + cq;
#pragma unroll 4
      for (int ks = 0; ks < FGMM_TILE / 4; ++ks) {
        const int k = 4 * ks + kq;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(gam[k] * ar[k * XS], br[k * XS], acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) sum[i][q] += (double)acc[q];
    }
    if (tid < D) {
      float s = 0.f;
      for (int p = 0; p < FGMM_TILE; ++p) s = fmaf(gam[p], Xs[p * XS + tid], s);
      s1 += (double)s;
    } else if (tid == 255) {
      float s = 0.f;
      for (int p = 0; p < FGMM_TILE; ++p) s += gam[p];
      s1 += (double)s;
    }
  }
  const int NV = 1 + D + D * (D + 1) / 2;
  float* out = slab + ((long)r * C + c) * NV;
  if (tid < D) out[1 + tid] = (float)s1;
  else if (tid == 255) out[0] = (float)s1;
  // C/D layout: column = lane & 15 (dimension j), row = (lane >> 4) * 4 + q (dimension i)
#pragma unroll
  for (int i = 0; i < NBW; ++i) {
    if (wave + 4 * i >= nblk) continue;
    const int j = cbk[i] * 16 + cq;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ii = rbk[i] * 16 + kq * 4 + q;
      if (ii < D && j <= ii) out[1 + D + ii * (ii + 1) / 2 + j] = (float)sum[i][q];
    }
  }
}

// ---- the extractor's planes under full covariances ---------------------------------------------------------------------------------------
// Workgroup = (Gaussian c, FG_SB columns s of T_c).  G_c[:, s] = Sigma_c^-1 T_c[:, s] in double (ascending d), kept in LDS and written
// rounded once; then Pk_c (r, s) = sum_d T_c[d][r] G_c[d][s] for every r >= s, in double, rounded once: the layout of ssv_ivec_tv_planes.
__global__ __launch_bounds__(256) void fgmm_tv_planes_kernel(const double* __restrict__ T, const double* __restrict__ icov, float* __restrict__ G,
                                                             float* __restrict__ Pk, int D, int R) {
  __shared__ double Gb[IVEC_MAX_D * FG_SB];
  const int c = blockIdx.x, s0 = blockIdx.y * FG_SB, ns = min(FG_SB, R - s0), tid = threadIdx.x;
  const long Pd = (long)D * (D + 1) / 2, P = (long)R * (R + 1) / 2;
  const double* Tc = T + (long)c * D * R;
  const double* ic = icov + c * Pd;
  for (int e = tid; e < D * FG_SB; e += 256) {
    const int d = e / FG_SB, s = e - d * FG_SB;
    double v = 0.0;
    if (s < ns) {
      for (int d2 = 0; d2 < D; ++d2) v += ic[d2 <= d ? tv_tri(d, d2) : tv_tri(d2, d)] * Tc[d2 * R + s0 + s];
      G[((long)c * D + d) * R + s0 + s] = (float)v;
    }
    Gb[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < R * FG_SB; e += 256) {
    const int rr = e / FG_SB, s = e - rr * FG_SB;
    if (s >= ns || rr < s0 + s) continue;
    double v = 0.0;
    for (int d = 0; d < D; ++d) v += Tc[d * R + rr] * Gb[d * FG_SB + s];
    Pk[c * P + tv_tri(rr, s0 + s)] = (float)v;
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
static int fg_lds_limit() {               // the kernels below may take more than 64 KB of dynamic LDS: say so once per device
  static std::atomic<int> done[64];
  const void* ks[2] = {(const void*)fgmm_planes_kernel, (const void*)fgmm_like_kernel};
  return tv_lds_limit_set(done, ks, 2, "fgmm");
}

static int fg_launch_planes(const double* stats, double* w, double* mu, double* cov, float* Wt, float* muf, float* g, double* icov, int* kept, int C, int D,
                            double var_floor, double min_count, hipStream_t st) {
  SSV_TRY(fg_lds_limit());
  const size_t lds = ((size_t)D * (D + 1) / 2 + 2 * (size_t)D + 256) * sizeof(double);
  hipLaunchKernelGGL(fgmm_planes_kernel, dim3(C), dim3(256), lds, st, stats, w, mu, cov, Wt, muf, g, icov, kept, D, var_floor, min_count);
  return ssv_check_launch("fgmm_planes");
}

int fgmm_launch_planes(const double* w, const double* mu, const double* cov, float* Wt, float* muf, float* g, double* icov, int C, int D, hipStream_t st) {
  return fg_launch_planes(nullptr, (double*)w, (double*)mu, (double*)cov, Wt, muf, g, icov, nullptr, C, D, 0.0, 0.0, st);
}

int fgmm_launch_update(const double* stats, double* w, double* mu, double* cov, float* Wt, float* muf, float* g, double* icov, int* kept, int C, int D,
                       double var_floor, double min_count, double min_weight, hipStream_t st) {
  SSV_TRY(fg_launch_planes(stats, w, mu, cov, Wt, muf, g, icov, kept, C, D, var_floor, min_count, st));
  hipLaunchKernelGGL(fgmm_weights_kernel, dim3(1), dim3(256), 0, st, stats, (const int*)kept, w, g, C, 1 + D + D * (D + 1) / 2, min_weight);
  return ssv_check_launch("fgmm_weights");
}

int fgmm_launch_group(const int* idx, int* start, int* pairs, int* counts, long n, int C, hipStream_t st) {
  const int nb = ssv_cdiv(n, FGMM_SL);
  hipLaunchKernelGGL(fgmm_count_kernel, dim3(nb), dim3(256), 0, st, idx, counts, n, C);
  SSV_TRY(ssv_check_launch("fgmm_count"));
  hipLaunchKernelGGL(fgmm_prefix_kernel, dim3(ssv_cdiv(C, 64)), dim3(64), 0, st, counts, start, nb, C);
  SSV_TRY(ssv_check_launch("fgmm_prefix"));
  hipLaunchKernelGGL(fgmm_scan_kernel, dim3(1), dim3(64), 0, st, start, C);
  SSV_TRY(ssv_check_launch("fgmm_scan"));
  hipLaunchKernelGGL(fgmm_scatter_kernel, dim3(nb), dim3(64), 0, st, idx, (const int*)counts, (const int*)start, pairs, n, C);
  return ssv_check_launch("fgmm_scatter");
}

int fgmm_launch_post(const float* X, const float* Wt, const float* muf, const float* g, const int* idx, const int* start, const int* pairs, float* post,
                     float* loglik, float* L, long F, int D, int C, int nsel, int nrun, float min_post, hipStream_t st) {
  SSV_TRY(fg_lds_limit());
  const int DP = (D + 15) & ~15;
  const size_t lds = ((size_t)(DP + FGMM_TILE) * (DP + 4) + 2 * FGMM_TILE + IVEC_MAX_D) * sizeof(float);
  hipLaunchKernelGGL(fgmm_like_kernel, dim3(C * nrun), dim3(256), lds, st, X, Wt, muf, g, start, pairs, L, F, D, nsel, nrun, DP);
  SSV_TRY(ssv_check_launch("fgmm_like"));
  hipLaunchKernelGGL(fgmm_finish_kernel, dim3(ssv_cdiv(F, 256)), dim3(256), 0, st, (const float*)L, idx, post, loglik, F, C, nsel, min_post);
  return ssv_check_launch("fgmm_finish");
}

int fgmm_launch_stats(const float* X, const float* muf, const float* post, const int* start, const int* pairs, float* slab, long F, int D, int C, int nsel,
                      int nrun, hipStream_t st) {
  const int DP = (D + 15) & ~15, nb = DP >> 4, nblk = nb * (nb + 1) / 2, nbw = (nblk + 3) / 4;
  const size_t lds = (size_t)FGMM_TILE * (DP + 4) * sizeof(float);
  const dim3 grid(C * nrun);
#define FG_STATS(NBW_) hipLaunchKernelGGL(fgmm_stats_kernel<NBW_>, grid, dim3(256), lds, st, X, muf, post, start, pairs, slab, F, D, C, nsel, nrun, DP)
  if (nbw <= 1) FG_STATS(1);
  else if (nbw <= 3) FG_STATS(3);
  else FG_STATS(9);
#undef FG_STATS
  return ssv_check_launch("fgmm_stats");
}

int fgmm_launch_tv_planes(const double* T, const double* icov, float* G, float* Pk, int C, int D, int R, hipStream_t st) {
  hipLaunchKernelGGL(fgmm_tv_planes_kernel, dim3(C, ssv_cdiv(R, FG_SB)), dim3(256), 0, st, T, icov, G, Pk, D, R);
  return ssv_check_launch("ivec_tv_planes_full");
}
