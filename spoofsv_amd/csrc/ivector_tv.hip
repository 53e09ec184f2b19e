// The middle of the i-vector system on the device (include/ssv_hip.h, "I-vector extractor"), gfx950: the planes of a total-variability
// matrix, the exact-fp32 product family (the tile of exact_product.h) that builds every utterance's posterior precision and linear term (and, transposed, the
// M-step's accumulators), the per-utterance E-step and the per-Gaussian M-step -- both a Cholesky factorisation, inverse and solve of a
// packed lower triangle held in LDS, in double -- the centring of the first-order statistics, and cosine trial scoring.
// The model is OURS, stated at the entries; Kaldi's ivector-extractor-* binaries are not reproduced.
// Arithmetic is independent of ssv_set_precision.  No float atomics; the order of every sum follows from the shapes alone.
// This file holds the kernels and their launchers (-2 for a shape beyond them); api_ivector.hip holds the entries and the checks (-1).
#include <type_traits>
#include "tv_triangle.h"          // tv_tri, tv_wave_sum, tv_cholesky, tv_trtri, tv_lauum, TV_LDS_MAX, tv_lds_limit_set; the limits and launchers (ivec_chain.h)
#include "exact_product.h"        // xp_tile, its maps and constants, xp_grid

#define TV_ES_THREADS 1024          // E-step: 16 waves, four per SIMD -- the triangle allows one workgroup a CU, so its waves are the occupancy
#define TV_UP_THREADS 512           // M-step: 8 waves (a right-hand side per wave; the waves' solution rows share the LDS left by the triangle)
#define TV_COS_THREADS 256

// ---- planes ------------------------------------------------------------------------------------------------------------------------------
// Workgroup = Gaussian c.  G_c = diag(1 / var_c) T_c and the packed lower triangle of Pk_c = T_c^T G_c, summed over d in double in
// ascending d and rounded once.
__global__ __launch_bounds__(256) void tv_planes_kernel(const double* __restrict__ T, const double* __restrict__ var, float* __restrict__ G,
                                                        float* __restrict__ Pk, int D, int R, int P) {
  __shared__ double iv[IVEC_MAX_D];
  const int c = blockIdx.x, tid = threadIdx.x;
  const double* Tc = T + (long)c * D * R;
  const double* vc = var + (long)c * D;
  for (int d = tid; d < D; d += 256) iv[d] = 1.0 / vc[d];
  for (int e = tid; e < D * R; e += 256) G[(long)c * D * R + e] = (float)(Tc[e] / vc[e / R]);
  __syncthreads();
  for (int i = 0; i < R; ++i)
    for (int j = tid; j <= i; j += 256) {
      double s = 0.0;
      for (int d = 0; d < D; ++d) s += Tc[d * R + i] * Tc[d * R + j] * iv[d];
      Pk[(long)c * P + tv_tri(i, j)] = (float)s;
    }
}

// ---- centring ------------------------------------------------------------------------------------------------------------------------------
// Ft = F - N mu: one fused multiply-add per element in float32 (mu rounded once from double).  Ft may be F itself.
__global__ __launch_bounds__(256) void tv_centre_kernel(const float* __restrict__ N, const float* F, const double* __restrict__ mu, float* Ft, long n, int CD, int D) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long u = e / CD;
  const int cd = (int)(e - u * CD);
  Ft[e] = fmaf(-N[u * (CD / D) + cd / D], (float)mu[cd], F[e]);
}

// ---- the product family ------------------------------------------------------------------------------------------------------------------
// out (m, n) = A B on the tile of exact_product.h, which states the order of the sums; B (K, n) row-major.  TR = false: A (m, K) row-major,
// out float32, rounded once; TR = true: A (K, m) row-major (the product is A^T B) and the result is ADDED to float64 accumulators.
// Workgroup = one tile of the output: every element has one owner.
template <bool TR>
__global__ __launch_bounds__(256) void tv_product_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out,
                                                         double* __restrict__ acc_out, long m, long n, long K) {
  const long m0 = (long)blockIdx.y * XP_TILE, n0 = (long)blockIdx.x * XP_TILE;
  auto load_a = [&](long k, int r) { return (k < K && m0 + r < m) ? (TR ? A[k * m + m0 + r] : A[(m0 + r) * K + k]) : 0.f; };
  auto load_b = [&](long k, int c) { return (k < K && n0 + c < n) ? B[k * n + n0 + c] : 0.f; };
  auto store = [&](int r, int c, double v) {
    const long row = m0 + r, col = n0 + c;
    if (row < m && col < n) {
      if (TR) acc_out[row * n + col] += v;
      else out[row * n + col] = (float)v;
    }
  };
  xp_tile<typename std::conditional<TR, XpRowFast, XpKFast>::type, XpRowFast>(K, load_a, load_b, store);
}

// ---- E-step ------------------------------------------------------------------------------------------------------------------------------
// Workgroup = utterance u.  L = I + unpack(Lp_u) in double; C = chol(L) with y = C^-1 b on the way; w from the back substitution
// C^T w = y (row j of C is contiguous: y[k] -= C[j][k] w[j]); obj = -1/2 log|L| + 1/2 b.w; with M != null the inverse by trtri + lauum and
// M = L^-1 + w w^T.  A pivot that is not positive (it cannot be for N >= 0: L >= I) gives NaN in this utterance's outputs and nothing else.
__global__ __launch_bounds__(TV_ES_THREADS) void tv_estep_kernel(const float* __restrict__ Lp, const float* __restrict__ b, float* __restrict__ w,
                                                                  float* __restrict__ M, double* __restrict__ obj, int R, int P) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* tri = lds_d;                    // [P]
  double* col = tri + P;                  // [R]
  double* y = col + R;                    // [R]
  double* bv = y + R;                     // [R]
  double* part = bv + R;                  // [TV_ES_THREADS / 256][256]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long u = blockIdx.x;
  for (int p = tid; p < P; p += TV_ES_THREADS) tri[p] = (double)Lp[u * P + p];
  for (int i = tid; i < R; i += TV_ES_THREADS) y[i] = bv[i] = (double)b[u * R + i];
  __syncthreads();
  for (int i = tid; i < R; i += TV_ES_THREADS) tri[tv_tri(i, i)] += 1.0;
  __syncthreads();
  const float qnan = __builtin_nanf("");
  if (!tv_cholesky(tri, col, y, R)) {
    for (int i = tid; i < R; i += TV_ES_THREADS) w[u * R + i] = qnan;
    if (M)
      for (int p = tid; p < P; p += TV_ES_THREADS) M[u * P + p] = qnan;
    if (tid == 0) obj[u] = (double)qnan;
    return;
  }
  for (int j = R - 1; j >= 0; --j) {      // col <- w
    const double wj = y[j] / tri[tv_tri(j, j)];      // (y[j] is final: step j writes y[k], k < j, only)
    const double* row = tri + tv_tri(j, 0);
    for (int k = tid; k < j; k += TV_ES_THREADS) y[k] -= row[k] * wj;
    if (tid == 0) col[j] = wj;
    __syncthreads();
  }
  for (int i = tid; i < R; i += TV_ES_THREADS) w[u * R + i] = (float)col[i];
  if (wave == 0) {
    double ld = 0.0, bw = 0.0;
    for (int i = lane; i < R; i += 64) {
      ld += log(tri[tv_tri(i, i)]);
      bw += bv[i] * col[i];
    }
    ld = tv_wave_sum(ld);
    bw = tv_wave_sum(bw);
    if (lane == 0) obj[u] = -ld + 0.5 * bw;       // log|L| = 2 sum log C_ii
  }
  if (!M) return;
  __syncthreads();
  for (int i = tid; i < R; i += TV_ES_THREADS) y[i] = col[i];      // w moves to y: the inverse uses col
  tv_trtri(tri, col, R);
  tv_lauum(tri, col, part, R);
  for (int i = wave; i < R; i += TV_ES_THREADS / 64) {
    const double wi = y[i];
    for (int j = lane; j <= i; j += 64) M[u * P + tv_tri(i, j)] = (float)(tri[tv_tri(i, j)] + wi * y[j]);
  }
}

// ---- M-step ------------------------------------------------------------------------------------------------------------------------------
// Workgroup = Gaussian c.  A_c is inverted in LDS by the same three functions; the D right-hand sides (the rows of Cm_c) then stream past
// it, a wave per row: x = A_c^-1 cm_d, lane i taking the elements i, i + 64, i + 128 of the symmetric product.  With J the waves' rows wait
// in LDS (where lauum kept its partial sums) and leave as x J.  A Gaussian with Nc < min_count (or not > 0) returns before it writes.
__global__ __launch_bounds__(TV_UP_THREADS) void tv_update_kernel(const double* __restrict__ A, const double* __restrict__ Cm, const double* __restrict__ Nc,
                                                                   const double* __restrict__ J, double* __restrict__ T, int D, int R, int P, double min_count) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double* tri = lds_d;                    // [P]
  double* col = tri + P;                  // [R]
  double* part = col + R;                 // [TV_UP_THREADS / 256][256], later the waves' rows [TV_UP_THREADS / 64][R]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.x;
  const double nc = Nc[c];
  if (nc < min_count || !(nc > 0.0)) return;
  for (int p = tid; p < P; p += TV_UP_THREADS) tri[p] = A[(long)c * P + p];
  __syncthreads();
  double* Tc = T + (long)c * D * R;
  if (!tv_cholesky(tri, col, nullptr, R)) {
    for (int e = tid; e < D * R; e += TV_UP_THREADS) Tc[e] = (double)__builtin_nanf("");
    return;
  }
  tv_trtri(tri, col, R);
  tv_lauum(tri, col, part, R);
  double* xs = part + wave * R;
  for (int d0 = 0; d0 < D; d0 += TV_UP_THREADS / 64) {
    const int d = d0 + wave;
    double x[3] = {0.0, 0.0, 0.0};
    if (d < D) {
      const double* cm = Cm + ((long)c * D + d) * R;
      for (int k = 0; k < R; ++k) {
        const double v = cm[k];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int i = lane + 64 * q;
          if (i < R) x[q] += tri[i >= k ? tv_tri(i, k) : tv_tri(k, i)] * v;
        }
      }
    }
    if (!J) {
      if (d < D)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (lane + 64 * q < R) Tc[d * R + lane + 64 * q] = x[q];
      continue;
    }
    __syncthreads();                      // the rows of the round before have been read
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (lane + 64 * q < R) xs[lane + 64 * q] = x[q];
    __syncthreads();
    if (d < D)
      for (int r = lane; r < R; r += 64) {
        double s = 0.0;
        for (int i = 0; i < R; ++i) s += xs[i] * J[(long)i * R + r];
        Tc[d * R + r] = s;
      }
  }
}

// ---- cosine trials -----------------------------------------------------------------------------------------------------------------------
// Every workgroup builds all S speaker models in LDS -- per speaker (a wave each) the mean of its length-normalised enrolment vectors
// [spk_off[s], spk_off[s+1]) in ascending order, normalised again, float32 -- then scores its share of the eval vectors, a wave per vector:
// the vector normalised in double, its dot product with every model in double, rounded once.  A vector of norm 0 (or a speaker without
// enrolment) normalises to zero and scores 0.
__global__ __launch_bounds__(TV_COS_THREADS) void tv_cosine_kernel(const float* __restrict__ enroll, const long* __restrict__ spk_off, const float* __restrict__ evalv,
                                                                    float* __restrict__ scores, long n_enroll, int S, long E, int R) {
  extern __shared__ __attribute__((aligned(16))) float models[];      // [S][R]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int s = wave; s < S; s += TV_COS_THREADS / 64) {
    long a = min(max(spk_off[s], 0L), n_enroll), b = min(max(spk_off[s + 1], 0L), n_enroll);
    if (b < a) b = a;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long e = a; e < b; ++e) {
      double v[3], ss = 0.0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        v[q] = lane + 64 * q < R ? (double)enroll[e * R + lane + 64 * q] : 0.0;
        ss += v[q] * v[q];
      }
      ss = tv_wave_sum(ss);
      const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[q] += v[q] * inv;
    }
    double ss = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      acc[q] = b > a ? acc[q] / (double)(b - a) : 0.0;
      ss += acc[q] * acc[q];
    }
    ss = tv_wave_sum(ss);
    const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (lane + 64 * q < R) models[s * R + lane + 64 * q] = (float)(acc[q] * inv);
  }
  __syncthreads();
  for (long e = (long)blockIdx.x * (TV_COS_THREADS / 64) + wave; e < E; e += (long)gridDim.x * (TV_COS_THREADS / 64)) {
    double v[3], ss = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      v[q] = lane + 64 * q < R ? (double)evalv[e * R + lane + 64 * q] : 0.0;
      ss += v[q] * v[q];
    }
    ss = tv_wave_sum(ss);
    const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
    for (int s = 0; s < S; ++s) {
      double dot = 0.0;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (lane + 64 * q < R) dot += v[q] * inv * (double)models[s * R + lane + 64 * q];
      dot = tv_wave_sum(dot);
      if (lane == 0) scores[e * S + s] = (float)dot;
    }
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
static int tv_lds_limit() {               // the kernels below take more than 64 KB of dynamic LDS: say so once per device
  static std::atomic<int> done[64];
  const void* ks[3] = {(const void*)tv_estep_kernel, (const void*)tv_update_kernel, (const void*)tv_cosine_kernel};
  return tv_lds_limit_set(done, ks, 3, "ivector_tv");
}

static int tv_shape_ok(const char* what, int C, int D, int R) {
  SSV_CHECK(R <= IVEC_MAX_R && C <= IVEC_MAX_C && D <= IVEC_MAX_D, SSV_UNSUPPORTED, "%s: R=%d (at most %d), C=%d (at most %d) or D=%d (at most %d) beyond the kernels", what, R,
            IVEC_MAX_R, C, IVEC_MAX_C, D, IVEC_MAX_D);
  return 0;
}

int tv_launch_planes(const double* T, const double* var, float* G, float* Pk, int C, int D, int R, hipStream_t st) {
  SSV_TRY(tv_shape_ok("ivec_tv_planes", C, D, R));
  hipLaunchKernelGGL(tv_planes_kernel, dim3(C), dim3(256), 0, st, T, var, G, Pk, D, R, R * (R + 1) / 2);
  return ssv_check_launch("ivec_tv_planes");
}

int tv_launch_centre(const float* N, const float* F, const double* mu, float* Ft, long U, int C, int D, hipStream_t st) {
  SSV_TRY(tv_shape_ok("ivec_centre_stats", C, D, 1));
  const long n = U * C * D;
  SSV_CHECK((n + 255) / 256 <= 0x7fffffffL, SSV_UNSUPPORTED, "ivec_centre_stats: %ld elements exceed the grid", n);
  hipLaunchKernelGGL(tv_centre_kernel, dim3(ssv_cdiv(n, 256)), dim3(256), 0, st, N, F, mu, Ft, n, C * D, D);
  return ssv_check_launch("ivec_centre_stats");
}

int tv_launch_product(const float* A, const float* B, float* out, long m, long n, long K, hipStream_t st) {
  dim3 grid;
  SSV_TRY(xp_grid("ivec_product", m, n, &grid));
  hipLaunchKernelGGL(tv_product_kernel<false>, grid, dim3(256), 0, st, A, B, out, (double*)nullptr, m, n, K);
  return ssv_check_launch("ivec_product");
}

int tv_launch_product_tn(const float* A, const float* B, double* acc, long U, long m, long n, hipStream_t st) {
  dim3 grid;
  SSV_TRY(xp_grid("ivec_product_tn", m, n, &grid));
  hipLaunchKernelGGL(tv_product_kernel<true>, grid, dim3(256), 0, st, A, B, (float*)nullptr, acc, m, n, U);
  return ssv_check_launch("ivec_product_tn");
}

int tv_launch_estep(const float* Lp, const float* b, float* w, float* M, double* obj, long U, int R, hipStream_t st) {
  SSV_TRY(tv_shape_ok("ivec_estep", 1, 1, R));
  SSV_CHECK(U <= 0x7fffffffL, SSV_UNSUPPORTED, "ivec_estep: %ld utterances exceed the grid", U);
  SSV_TRY(tv_lds_limit());
  const int P = R * (R + 1) / 2;
  const size_t lds = ((size_t)P + 3 * R + TV_ES_THREADS) * sizeof(double);
  hipLaunchKernelGGL(tv_estep_kernel, dim3((unsigned)U), dim3(TV_ES_THREADS), lds, st, Lp, b, w, M, obj, R, P);
  return ssv_check_launch("ivec_estep");
}

int tv_launch_update(const double* A, const double* Cm, const double* Nc, const double* J, double* T, int C, int D, int R, double min_count, hipStream_t st) {
  SSV_TRY(tv_shape_ok("ivec_tv_update", C, D, R));
  SSV_TRY(tv_lds_limit());
  const int P = R * (R + 1) / 2;
  const size_t shared = TV_UP_THREADS > (TV_UP_THREADS / 64) * R ? TV_UP_THREADS : (size_t)(TV_UP_THREADS / 64) * R;
  const size_t lds = ((size_t)P + R + shared) * sizeof(double);
  hipLaunchKernelGGL(tv_update_kernel, dim3(C), dim3(TV_UP_THREADS), lds, st, A, Cm, Nc, J, T, D, R, P, min_count);
  return ssv_check_launch("ivec_tv_update");
}

int tv_launch_cosine(const float* enroll, const long* spk_off, const float* evalv, float* scores, long n_enroll, int S, long E, int R, hipStream_t st) {
  SSV_TRY(tv_shape_ok("ivec_cosine_trials", 1, 1, R));
  const size_t lds = (size_t)S * R * sizeof(float);
  SSV_CHECK(lds <= 128 * 1024, SSV_UNSUPPORTED, "ivec_cosine_trials: %d speaker models of rank %d take %zu bytes of LDS (at most 131072)", S, R, lds);
  SSV_TRY(tv_lds_limit());
  const long per = TV_COS_THREADS / 64, want = (E + per - 1) / per;
  hipLaunchKernelGGL(tv_cosine_kernel, dim3((unsigned)(want < 256 ? want : 256)), dim3(TV_COS_THREADS), lds, st, enroll, spk_off, evalv, scores, n_enroll, S, E, R);
  return ssv_check_launch("ivec_cosine_trials");
}
