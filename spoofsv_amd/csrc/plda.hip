// The back end of the i-vector system on the device (include/ssv_hip.h, "I-vector back end: PLDA"), gfx950: class statistics of
// length-normalised vectors, the float64 pieces of two-covariance PLDA's EM (inverses of packed triangles in LDS by the extractor's
// three functions, the per-speaker posterior means, the weighted outer-product sums, the update and the objective), the transform's row
// kernels, the speaker planes, and the score product [t^2, t] H^T + k on the exact-fp32 tile of exact_product.h.
// The model is OURS, stated at the entries; Kaldi's ivector-compute-plda and ivector-plda-scoring are not reproduced.
// Arithmetic is independent of ssv_set_precision.  No float atomics; the order of every sum follows from the shapes alone.
// This file holds the kernels and their launchers (-2 for a shape beyond them); api_plda.hip holds the entries and the checks (-1).
#include "tv_triangle.h"          // the packed triangle, tv_wave_sum, tv_lds_limit_set; IVEC_MAX_R and the launchers (ivec_chain.h)
#include "exact_product.h"        // xp_tile, XpKFast, xp_grid

#define PL_THREADS 256
#define PL_INV_THREADS 512          // the inverse: 8 waves (the triangle allows one workgroup a CU)
#define PL_CHUNK 256                // class statistics: rows whose factors wait in LDS at a time
#define PL_SY_TILE 16               // wsyrk: a workgroup owns 16 x 16 elements of the output, a thread one
#define PL_SY_ROWS 64               // wsyrk: rows of V staged per step

// sum over R <= IVEC_MAX_R of a per-element value held three to a lane (elements lane, lane + 64, lane + 128), then the butterfly
__device__ __forceinline__ double pl_row_ss(const float* __restrict__ row, int R, int lane) {
  double ss = 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double v = lane + 64 * q < R ? (double)row[lane + 64 * q] : 0.0;
    ss += v * v;
  }
  return tv_wave_sum(ss);
}

// ---- class statistics --------------------------------------------------------------------------------------------------------------------
// Workgroup = speaker k, rows [a, b) of X (clamped to [0, n]; a descending pair is empty).  Rows pass in chunks of PL_CHUNK: a wave per row
// takes the row's factor f = sqrt(R / |x|^2) in double (0 for a zero row; 1 without length normalisation), then thread d adds x f over the
// chunk's rows in ascending order, in double.  The mean leaves as float64; the second walk writes d = x f - m, rounded once to float32; the
// model row is m sqrt(R) / |m|, rounded once.  A speaker without rows writes zeros to its model row and touches nothing else.
__global__ __launch_bounds__(PL_THREADS) void plda_class_stats_kernel(const float* __restrict__ X, const long* __restrict__ spk_off, float* __restrict__ Xd,
                                                                     double* __restrict__ means, float* __restrict__ model, long n, int R, int length_norm) {
  __shared__ double fac[PL_CHUNK];
  __shared__ double mrow[PL_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long k = blockIdx.x;
  long a = min(max(spk_off[k], 0L), n), b = min(max(spk_off[k + 1], 0L), n);
  if (b <= a) {                           // (uniform: every thread read the same pair)
    if (model && tid < R) model[k * R + tid] = 0.f;
    return;
  }
  double m = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    for (long c0 = a; c0 < b; c0 += PL_CHUNK) {
      const int rows = (int)min((long)PL_CHUNK, b - c0);
      __syncthreads();                    // the chunk before has been read
      for (int i = wave; i < rows; i += PL_THREADS / 64) {
        double f = 1.0;
        if (length_norm) {
          const double ss = pl_row_ss(X + (c0 + i) * R, R, lane);
          f = ss > 0.0 ? sqrt((double)R / ss) : 0.0;
        }
        if (lane == 0) fac[i] = f;
      }
      __syncthreads();
      if (tid < R) {
        if (pass == 0) {
          for (int i = 0; i < rows; ++i) m += (double)X[(c0 + i) * R + tid] * fac[i];
        } else if (Xd) {
          for (int i = 0; i < rows; ++i) Xd[(c0 + i) * R + tid] = (float)((double)X[(c0 + i) * R + tid] * fac[i] - m);
        }
      }
    }
    if (pass == 0) {
      m /= (double)(b - a);
      if (means && tid < R) means[k * R + tid] = m;
      if (!Xd) break;
    }
  }
  if (!model) return;
  __syncthreads();
  mrow[tid] = tid < R ? m * m : 0.0;
  __syncthreads();
  if (wave == 0) {
    double ss = mrow[lane] + mrow[lane + 64] + mrow[lane + 128];
    ss = tv_wave_sum(ss);
    if (lane == 0) fac[0] = ss > 0.0 ? sqrt((double)R / ss) : 0.0;
  }
  __syncthreads();
  if (tid < R) model[k * R + tid] = (float)(m * fac[0]);
}

// mu = the mean of the means of the speakers that have rows, unweighted, in ascending speaker order (one workgroup, thread d)
__global__ __launch_bounds__(PL_THREADS) void plda_mu_kernel(const double* __restrict__ means, const long* __restrict__ spk_off, double* __restrict__ mu, long n,
                                                            int S, int R) {
  const int d = threadIdx.x;
  if (d >= R) return;
  double s = 0.0;
  long cnt = 0;
  for (int k = 0; k < S; ++k) {
    const long a = min(max(spk_off[k], 0L), n), b = min(max(spk_off[k + 1], 0L), n);
    if (b > a) {
      s += means[(long)k * R + d];
      ++cnt;
    }
  }
  mu[d] = cnt > 0 ? s / (double)cnt : 0.0;
}

// ---- the mixed inverse ---------------------------------------------------------------------------------------------------------------------
// Workgroup = matrix j: tri = a + coef_j b_j, b_j = b + j b_stride (a == null: coef_j b_j; coef == null: coef_j = 1) in LDS, then Cholesky,
// trtri, lauum in place.
// logdet_j = log|a + coef_j b_j| = 2 sum log C_ii.  A pivot that is not positive: NaN in out_j and logdet_j, nothing else.
__global__ __launch_bounds__(PL_INV_THREADS) void plda_mixed_inverse_kernel(const double* __restrict__ a, const double* __restrict__ b, long b_stride, const double* __restrict__ coef,
                                                                           double* __restrict__ out, double* __restrict__ logdet, int R, int P) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* tri = lds_d;                    // [P]
  double* col = tri + P;                  // [R]
  double* part = col + R;                 // [PL_INV_THREADS / 256][256]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long j = blockIdx.x;
  const double cj = coef ? coef[j] : 1.0;
  const double* bj = b + j * b_stride;
  for (int p = tid; p < P; p += PL_INV_THREADS) tri[p] = a ? a[p] + cj * bj[p] : cj * bj[p];
  __syncthreads();
  double* oj = out + j * P;
  if (!tv_cholesky(tri, col, nullptr, R)) {
    const double qnan = (double)__builtin_nanf("");
    for (int p = tid; p < P; p += PL_INV_THREADS) oj[p] = qnan;
    if (logdet && tid == 0) logdet[j] = qnan;
    return;
  }
  if (logdet && wave == 0) {
    double ld = 0.0;
    for (int i = lane; i < R; i += 64) ld += log(tri[tv_tri(i, i)]);
    ld = tv_wave_sum(ld);
    if (lane == 0) logdet[j] = 2.0 * ld;
  }
  __syncthreads();
  tv_trtri(tri, col, R);
  tv_lauum(tri, col, part, R);
  for (int p = tid; p < P; p += PL_INV_THREADS) oj[p] = tri[p];
}

// ---- EM: the speakers ------------------------------------------------------------------------------------------------------------------------
// y_i = sum_k M[i][k] v[k] of a packed symmetric M in global memory, in ascending k, for thread i < R (v in LDS)
__device__ __forceinline__ double pl_symv(const double* __restrict__ M, const double* v, int i, int R) {
  double s = 0.0;
  const double* row = M + tv_tri(i, 0);
  for (int k = 0; k <= i; ++k) s += row[k] * v[k];
  for (int k = i + 1; k < R; ++k) s += M[tv_tri(k, i)] * v[k];
  return s;
}

// Workgroup = speaker k with n = cnt[k] rows and the matrix Mx[cls[k]] = (B^-1 + n W^-1)^-1:  c = m_k - mu,  t = W^-1 c,  w = n Mx t,
// r = c - w,  quad = n t . r  ( = c^T (B + W / n)^-1 c, by the matrix inversion lemma).  n = 0: w = r = 0 and quad = 0.
__global__ __launch_bounds__(PL_THREADS) void plda_em_classes_kernel(const double* __restrict__ means, const double* __restrict__ mu, const int* __restrict__ cnt,
                                                                    const int* __restrict__ cls, const double* __restrict__ Mx, const double* __restrict__ Winv,
                                                                    double* __restrict__ w, double* __restrict__ r, double* __restrict__ quad, int R, int P, int J) {
  __shared__ double v[PL_THREADS];
  __shared__ double tr[PL_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long k = blockIdx.x;
  const int nk = cnt[k], j = cls[k];
  if (nk <= 0 || j < 0 || j >= J) {       // (uniform)
    if (tid < R) w[k * R + tid] = r[k * R + tid] = 0.0;
    if (tid == 0) quad[k] = 0.0;
    return;
  }
  const double c = tid < R ? means[k * R + tid] - mu[tid] : 0.0;
  v[tid] = c;
  __syncthreads();
  const double t = tid < R ? pl_symv(Winv, v, tid, R) : 0.0;
  __syncthreads();
  v[tid] = t;
  __syncthreads();
  const double wk = tid < R ? (double)nk * pl_symv(Mx + (long)j * P, v, tid, R) : 0.0;
  const double rk = c - wk;
  if (tid < R) {
    w[k * R + tid] = wk;
    r[k * R + tid] = rk;
  }
  tr[tid] = t * rk;
  __syncthreads();
  if (wave == 0) {
    double s = tr[lane] + tr[lane + 64] + tr[lane + 128];
    s = tv_wave_sum(s);
    if (lane == 0) quad[k] = (double)nk * s;
  }
}

// ---- EM: the weighted outer-product sum ----------------------------------------------------------------------------------------------------
// acc (R, R) += V^T diag(c) V, V (S, R) float64 (c == null: ones).  A thread owns one element and adds its rows in ascending order.
__global__ __launch_bounds__(PL_SY_TILE * PL_SY_TILE) void plda_wsyrk_kernel(const double* __restrict__ V, const double* __restrict__ c, double* __restrict__ acc, long S,
                                                                            int R) {
  __shared__ double Vi[PL_SY_ROWS][PL_SY_TILE + 1], Vj[PL_SY_ROWS][PL_SY_TILE + 1];
  const int tid = threadIdx.x, ti = tid / PL_SY_TILE, tj = tid % PL_SY_TILE;
  const int i0 = blockIdx.y * PL_SY_TILE, j0 = blockIdx.x * PL_SY_TILE;
  double s = 0.0;
  for (long k0 = 0; k0 < S; k0 += PL_SY_ROWS) {
    __syncthreads();
    for (int e = tid; e < PL_SY_ROWS * PL_SY_TILE; e += PL_SY_TILE * PL_SY_TILE) {
      const int kk = e / PL_SY_TILE, d = e % PL_SY_TILE;
      const long k = k0 + kk;
      const double ck = k < S ? (c ? c[k] : 1.0) : 0.0;
      Vi[kk][d] = (k < S && i0 + d < R) ? ck * V[k * R + i0 + d] : 0.0;
      Vj[kk][d] = (k < S && j0 + d < R) ? V[k * R + j0 + d] : 0.0;
    }
    __syncthreads();
    const int rows = (int)min((long)PL_SY_ROWS, S - k0);
    for (int kk = 0; kk < rows; ++kk) s += Vi[kk][ti] * Vj[kk][tj];
  }
  if (i0 + ti < R && j0 + tj < R) acc[(long)(i0 + ti) * R + j0 + tj] += s;
}

// ---- EM: the update and the objective --------------------------------------------------------------------------------------------------
// B (P) = (sum_j nspk_j Mx_j + WW) / Sn,  W (P) = (Sigma + sum_j nrow_j Mx_j + RR) / N, packed; the classes added in ascending j.
__global__ __launch_bounds__(PL_THREADS) void plda_em_update_kernel(const double* __restrict__ Mx, const double* __restrict__ nspk, const double* __restrict__ nrow,
                                                                   const double* __restrict__ WW, const double* __restrict__ RR, const double* __restrict__ Sigma,
                                                                   double* __restrict__ W, double* __restrict__ B, int J, int R, int P, double Sn, double N) {
  const int i = blockIdx.x;
  for (int jj = threadIdx.x; jj <= i; jj += PL_THREADS) {
    const int p = tv_tri(i, jj);
    double sb = 0.0, sw = 0.0;
    for (int j = 0; j < J; ++j) {
      const double m = Mx[(long)j * P + p];
      sb += nspk[j] * m;
      sw += nrow[j] * m;
    }
    const long e = (long)i * R + jj;
    B[p] = (sb + WW[e]) / Sn;
    W[p] = (Sigma[e] + sw + RR[e]) / N;
  }
}

// the sum of 256 per-thread partial values: wave 0 adds four to a lane in ascending order, then the butterfly; every thread of wave 0 gets it
// (not tv_wg_sum: that one's halving tree adds in another order, and these sums keep theirs)
__device__ __forceinline__ double pl_block_sum(double* part, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  part[tid] = v;
  __syncthreads();
  double s = 0.0;
  if (tid < 64) {
    s = part[tid] + part[tid + 64] + part[tid + 128] + part[tid + 192];
    s = tv_wave_sum(s);
  }
  return s;
}

// obj = (1/N) { -1/2 [(N - Sn) log|W| + tr(W^-1 Sigma)] - 1/2 sum_k [log|B + W / n_k| + quad_k] }, with
// log|B + W / n| = log|W| - R log n + log|B| + log|B^-1 + n W^-1| (ldMx of the speaker's class).  One workgroup.
__global__ __launch_bounds__(PL_THREADS) void plda_objective_kernel(const double* __restrict__ Winv, const double* __restrict__ Sigma, const double* __restrict__ ldW,
                                                                   const double* __restrict__ ldB, const double* __restrict__ ldMx, const int* __restrict__ cnt,
                                                                   const int* __restrict__ cls, const double* __restrict__ quad, double* __restrict__ obj, int J,
                                                                   int S, int R, double Sn, double N) {
  __shared__ double part[PL_THREADS];
  const int tid = threadIdx.x;
  double tr = 0.0;
  for (int i = 0; i < R; ++i)
    for (int j = tid; j <= i; j += PL_THREADS) tr += Winv[tv_tri(i, j)] * Sigma[(long)i * R + j] * (i == j ? 1.0 : 2.0);
  tr = pl_block_sum(part, tr);
  const double lw = ldW[0], lb = ldB[0];
  double sk = 0.0;
  for (int k = tid; k < S; k += PL_THREADS) {
    const int nk = cnt[k], j = cls[k];
    if (nk > 0 && j >= 0 && j < J) sk += (lw - (double)R * log((double)nk) + lb + ldMx[j]) + quad[k];
  }
  sk = pl_block_sum(part, sk);
  if (tid == 0) obj[0] = (-0.5 * ((N - Sn) * lw + tr) - 0.5 * sk) / N;
}

// ---- the transform's row kernels -------------------------------------------------------------------------------------------------------
// Xc = x f - mu, one float32 fused multiply-add per element: f = sqrt(R / |x|^2) taken in double and rounded once (0 for a zero row; 1
// without length normalisation), mu rounded once.  A wave per row.
__global__ __launch_bounds__(PL_THREADS) void plda_centre_kernel(const float* __restrict__ X, const double* __restrict__ mu, float* __restrict__ Xc, long n, int R,
                                                                int length_norm) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * (PL_THREADS / 64) + (threadIdx.x >> 6);
  if (e >= n) return;
  float f = 1.f;
  if (length_norm) {
    const double ss = pl_row_ss(X + e * R, R, lane);
    f = ss > 0.0 ? (float)sqrt((double)R / ss) : 0.f;
  }
  for (int d = lane; d < R; d += 64) Xc[e * R + d] = fmaf(X[e * R + d], f, -(float)mu[d]);
}

// u <- u sqrt(R / sum_d u_d^2 / (psi_d + 1 / n)), the sum and the factor in double, each element rounded once; the factor is 1 where the sum
// is 0.  n = nex[row] (nex == null: nex_all), at least 1.  A wave per row, in place.
__global__ __launch_bounds__(PL_THREADS) void plda_scale_kernel(float* __restrict__ U, const double* __restrict__ psi, const int* __restrict__ nex, int nex_all, long n,
                                                               int R) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * (PL_THREADS / 64) + (threadIdx.x >> 6);
  if (e >= n) return;
  const int ne = max(nex ? nex[e] : nex_all, 1);
  const double inv_n = 1.0 / (double)ne;
  double u[3], s = 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int d = lane + 64 * q;
    u[q] = d < R ? (double)U[e * R + d] : 0.0;
    if (d < R) s += u[q] * u[q] / (psi[d] + inv_n);
  }
  s = tv_wave_sum(s);
  const double f = s > 0.0 ? sqrt((double)R / s) : 1.0;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (lane + 64 * q < R) U[e * R + lane + 64 * q] = (float)(u[q] * f);
}

// ---- the speaker planes ------------------------------------------------------------------------------------------------------------------
// Workgroup = speaker s with n enrolment rows and the transformed model y:  c = n psi / (n psi + 1),  v = 1 + psi / (n psi + 1),  a = 1 / v,
// H_s = [-1/2 (a - 1 / (psi + 1)), a c y] rounded once,  k_s = -1/2 sum a c^2 y^2 - 1/2 sum (log v - log(psi + 1)) in double.  n = 0: zeros.
__global__ __launch_bounds__(PL_THREADS) void plda_speaker_planes_kernel(const float* __restrict__ y, const int* __restrict__ nspk, const double* __restrict__ psi,
                                                                        float* __restrict__ H, double* __restrict__ kout, int R) {
  __shared__ double part[PL_THREADS];
  const int tid = threadIdx.x;
  const long s = blockIdx.x;
  const int n = nspk[s];
  if (n <= 0) {                           // (uniform)
    if (tid < R) H[s * 2 * R + tid] = H[s * 2 * R + R + tid] = 0.f;
    if (tid == 0) kout[s] = 0.0;
    return;
  }
  double term = 0.0;
  if (tid < R) {
    const double ps = psi[tid], den = (double)n * ps + 1.0, c = (double)n * ps / den, v = 1.0 + ps / den, a = 1.0 / v, yy = (double)y[s * R + tid];
    H[s * 2 * R + tid] = (float)(-0.5 * (a - 1.0 / (ps + 1.0)));
    H[s * 2 * R + R + tid] = (float)(a * c * yy);
    term = -0.5 * a * c * c * yy * yy - 0.5 * (log(v) - log(ps + 1.0));
  }
  term = pl_block_sum(part, term);
  if (tid == 0) kout[s] = term;
}

// ---- the score ---------------------------------------------------------------------------------------------------------------------------
// scores (E, S) float32 = [t^2, t] H^T + k on the tile of exact_product.h, which states the order of the sums (K = 2 R): T (E, R),
// H (S, 2 R) float32 row-major, k (S) float64.  Element kk of the left operand is t[kk]^2 for kk < R (one float32 product, made as the eval
// tile is fetched) and t[kk - R] beyond, so the (E, 2 R) array is never written; both operands are K-contiguous in memory.  k is added in
// double and the result rounded once.  Workgroup = one tile of the scores: every element has one owner.
__global__ __launch_bounds__(256) void plda_score_kernel(const float* __restrict__ T, const float* __restrict__ H, const double* __restrict__ kv,
                                                         float* __restrict__ scores, long E, long S, int R) {
  const long m0 = (long)blockIdx.y * XP_TILE, n0 = (long)blockIdx.x * XP_TILE;
  const int K = 2 * R;
  auto load_a = [&](long kl, int r) {
    const int k = (int)kl;
    float a = 0.f;
    if (k < K && m0 + r < E) {
      a = T[(m0 + r) * R + (k < R ? k : k - R)];
      if (k < R) a = a * a;
    }
    return a;
  };
  auto load_b = [&](long kl, int c) {
    const int k = (int)kl;
    return (k < K && n0 + c < S) ? H[(n0 + c) * K + k] : 0.f;
  };
  auto store = [&](int r, int c, double v) {
    const long row = m0 + r, col = n0 + c;
    if (row < E && col < S) scores[row * S + col] = (float)(v + kv[col]);
  };
  xp_tile<XpKFast, XpKFast>(K, load_a, load_b, store);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
static int plda_lds_limit() {             // the inverse takes more than 64 KB of dynamic LDS: say so once per device
  static std::atomic<int> done[64];
  const void* ks[1] = {(const void*)plda_mixed_inverse_kernel};
  return tv_lds_limit_set(done, ks, 1, "plda");
}

static int plda_rank_ok(const char* what, int R) {
  SSV_CHECK(R <= IVEC_MAX_R, SSV_UNSUPPORTED, "%s: R=%d (at most %d) beyond the kernels", what, R, IVEC_MAX_R);
  return 0;
}

int plda_launch_class_stats(const float* X, const long* spk_off, float* Xd, double* means, double* mu, float* model, long n, int S, int R, int length_norm,
                            hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_class_stats", R));
  hipLaunchKernelGGL(plda_class_stats_kernel, dim3(S), dim3(PL_THREADS), 0, st, X, spk_off, Xd, means, model, n, R, length_norm);
  SSV_TRY(ssv_check_launch("plda_class_stats"));
  if (!mu) return 0;
  hipLaunchKernelGGL(plda_mu_kernel, dim3(1), dim3(PL_THREADS), 0, st, (const double*)means, spk_off, mu, n, S, R);
  return ssv_check_launch("plda_class_stats (mu)");
}

int plda_launch_mixed_inverse(const double* a, const double* b, long b_stride, const double* coef, double* out, double* logdet, int J, int R, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_mixed_inverse", R));
  SSV_TRY(plda_lds_limit());
  const int P = R * (R + 1) / 2;
  const size_t lds = ((size_t)P + R + PL_INV_THREADS) * sizeof(double);
  hipLaunchKernelGGL(plda_mixed_inverse_kernel, dim3(J), dim3(PL_INV_THREADS), lds, st, a, b, b_stride, coef, out, logdet, R, P);
  return ssv_check_launch("plda_mixed_inverse");
}

int plda_launch_em_classes(const double* means, const double* mu, const int* cnt, const int* cls, const double* Mx, const double* Winv, double* w, double* r,
                           double* quad, int S, int R, int J, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_em_classes", R));
  hipLaunchKernelGGL(plda_em_classes_kernel, dim3(S), dim3(PL_THREADS), 0, st, means, mu, cnt, cls, Mx, Winv, w, r, quad, R, R * (R + 1) / 2, J);
  return ssv_check_launch("plda_em_classes");
}

int plda_launch_wsyrk(const double* V, const double* c, double* acc, long S, int R, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_wsyrk_f64", R));
  const int g = ssv_cdiv(R, PL_SY_TILE);
  hipLaunchKernelGGL(plda_wsyrk_kernel, dim3(g, g), dim3(PL_SY_TILE * PL_SY_TILE), 0, st, V, c, acc, S, R);
  return ssv_check_launch("plda_wsyrk_f64");
}

int plda_launch_em_update(const double* Mx, const double* ldMx, const double* nspk, const double* nrow, const double* WW, const double* RR, const double* Sigma,
                          const double* Winv, const double* ldW, const double* ldB, const int* cnt, const int* cls, const double* quad, double* W, double* B,
                          double* obj, int J, int S, int R, double Sn, double N, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_em_update", R));
  if (obj) {                              // first: it reads nothing the update writes, and W, B may be what Winv was taken from
    hipLaunchKernelGGL(plda_objective_kernel, dim3(1), dim3(PL_THREADS), 0, st, Winv, Sigma, ldW, ldB, ldMx, cnt, cls, quad, obj, J, S, R, Sn, N);
    SSV_TRY(ssv_check_launch("plda_em_update (objective)"));
  }
  if (W) {
    hipLaunchKernelGGL(plda_em_update_kernel, dim3(R), dim3(PL_THREADS), 0, st, Mx, nspk, nrow, WW, RR, Sigma, W, B, J, R, R * (R + 1) / 2, Sn, N);
    SSV_TRY(ssv_check_launch("plda_em_update"));
  }
  return 0;
}

static int plda_row_grid(const char* what, long n, unsigned* grid) {
  const long g = (n + PL_THREADS / 64 - 1) / (PL_THREADS / 64);
  SSV_CHECK(g <= 0x7fffffffL, SSV_UNSUPPORTED, "%s: %ld rows exceed the grid", what, n);
  *grid = (unsigned)g;
  return 0;
}

int plda_launch_centre(const float* X, const double* mu, float* Xc, long n, int R, int length_norm, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_transform", R));
  unsigned g;
  SSV_TRY(plda_row_grid("plda_transform", n, &g));
  hipLaunchKernelGGL(plda_centre_kernel, dim3(g), dim3(PL_THREADS), 0, st, X, mu, Xc, n, R, length_norm);
  return ssv_check_launch("plda_transform (centre)");
}

int plda_launch_scale(float* U, const double* psi, const int* nex, int nex_all, long n, int R, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_transform", R));
  unsigned g;
  SSV_TRY(plda_row_grid("plda_transform", n, &g));
  hipLaunchKernelGGL(plda_scale_kernel, dim3(g), dim3(PL_THREADS), 0, st, U, psi, nex, nex_all, n, R);
  return ssv_check_launch("plda_transform (scale)");
}

int plda_launch_speaker_planes(const float* y, const int* nspk, const double* psi, float* H, double* k, int S, int R, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_speaker_planes", R));
  hipLaunchKernelGGL(plda_speaker_planes_kernel, dim3(S), dim3(PL_THREADS), 0, st, y, nspk, psi, H, k, R);
  return ssv_check_launch("plda_speaker_planes");
}

int plda_launch_score(const float* T, const float* H, const double* k, float* scores, long E, long S, int R, hipStream_t st) {
  SSV_TRY(plda_rank_ok("plda_score", R));
  dim3 grid;
  SSV_TRY(xp_grid("plda_score", E, S, &grid));
  hipLaunchKernelGGL(plda_score_kernel, grid, dim3(256), 0, st, T, H, k, scores, E, S, R);
  return ssv_check_launch("plda_score");
}
