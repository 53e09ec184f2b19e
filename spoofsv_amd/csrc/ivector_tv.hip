// The middle of the i-vector system on the device (include/ssv_hip.h, "I-vector extractor"), gfx950: the planes of a total-variability
// matrix, the exact-fp32 product family that builds every utterance's posterior precision and linear term (and, transposed, the
// M-step's accumulators), the per-utterance E-step and the per-Gaussian M-step -- both a Cholesky factorisation, inverse and solve of a
// packed lower triangle held in LDS, in double -- the centring of the first-order statistics, and cosine trial scoring.
// The model is OURS, stated at the entries; Kaldi's ivector-extractor-* binaries are not reproduced.
// Arithmetic is independent of ssv_set_precision.  No float atomics; the order of every sum follows from the shapes alone.
// This file holds the kernels and their launchers (-2 for a shape beyond them); api_ivector.hip holds the entries and the checks (-1).
#include "tv_triangle.h"          // tv_tri, tv_wave_sum, tv_cholesky, tv_trtri, tv_lauum, TV_MAX_R, TV_LDS_MAX, tv_lds_limit_set

#define TV_MAX_C 2048
#define TV_MAX_D 128
#define TV_TILE 64                  // products: a workgroup owns a 64 x 64 tile of the output, a wave a 32 x 32 quarter of it
#define TV_KS 32                    // K elements staged per step
#define TV_LS (TV_TILE + 1)         // row stride of a staged step (k-major): the transposing store of the plain form hits 32 banks
#define TV_RUN 256                  // K elements of one fp32 chain; the runs are added in double (ssv_ivec_product_run)
#define TV_ES_THREADS 1024          // E-step: 16 waves, four per SIMD -- the triangle allows one workgroup a CU, so its waves are the occupancy
#define TV_UP_THREADS 512           // M-step: 8 waves (a right-hand side per wave; the waves' solution rows share the LDS left by the triangle)
#define TV_COS_THREADS 256

#pragma GCC visibility push(hidden)      // the launchers: called by api_ivector.hip (which repeats these lines), not exported
int tv_launch_planes(const double* T, const double* var, float* G, float* Pk, int C, int D, int R, hipStream_t st);
int tv_launch_centre(const float* N, const float* F, const double* mu, float* Ft, long U, int C, int D, hipStream_t st);
int tv_launch_product(const float* A, const float* B, float* out, long m, long n, long K, hipStream_t st);
int tv_launch_product_tn(const float* A, const float* B, double* acc, long U, long m, long n, hipStream_t st);
int tv_launch_estep(const float* Lp, const float* b, float* w, float* M, double* obj, long U, int R, hipStream_t st);
int tv_launch_update(const double* A, const double* Cm, const double* Nc, const double* J, double* T, int C, int D, int R, double min_count, hipStream_t st);
int tv_launch_cosine(const float* enroll, const long* spk_off, const float* evalv, float* scores, long n_enroll, int S, long E, int R, hipStream_t st);
#pragma GCC visibility pop


// ---- planes ------------------------------------------------------------------------------------------------------------------------------
// Workgroup = Gaussian c.  G_c = diag(1 / var_c) T_c and the packed lower triangle of Pk_c = T_c^T G_c, summed over d in double in
// ascending d and rounded once.
__global__ __launch_bounds__(256) void tv_planes_kernel(const double* __restrict__ T, const double* __restrict__ var, float* __restrict__ G,
                                                        float* __restrict__ Pk, int D, int R, int P) {
  __shared__ double iv[TV_MAX_D];
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
// out (m, n) = A B on v_mfma_f32_16x16x4_f32, B (K, n) row-major; TR = false: A (m, K) row-major, out float32, rounded once;
// TR = true: A (K, m) row-major (the product is A^T B) and the result is ADDED to float64 accumulators.  Workgroup = one 64 x 64 tile of
// the output (every element has one owner), wave = a 32 x 32 quarter.  K is walked in steps of TV_KS staged k-major in LDS (zeros
// beyond an edge); the step after the one being multiplied waits in registers.  An fp32 chain runs over TV_RUN elements of K from zero
// accumulators and is then added to DOUBLE registers.  The order of an element's sum depends on K alone: a row of the output does
// not depend on the rows that share its launch.
template <bool TR>
__global__ __launch_bounds__(256) void tv_product_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out,
                                                         double* __restrict__ acc_out, long m, long n, long K) {
  __shared__ float As[TV_KS * TV_LS], Bs[TV_KS * TV_LS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cq = lane & 15;
  const long m0 = (long)blockIdx.y * TV_TILE, n0 = (long)blockIdx.x * TV_TILE;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  float ra[8], rb[8];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (TR) {
        const long k = k0 + (tid >> 6) + 4 * i, r = m0 + (tid & 63);
        ra[i] = (k < K && r < m) ? A[k * m + r] : 0.f;
      } else {
        const long k = k0 + (tid & 31), r = m0 + (tid >> 5) + 8 * i;
        ra[i] = (k < K && r < m) ? A[r * K + k] : 0.f;
      }
      const long k = k0 + (tid >> 6) + 4 * i, c = n0 + (tid & 63);
      rb[i] = (k < K && c < n) ? B[k * n + c] : 0.f;
    }
  };
  double sum[2][2][4];
  f32x4 acc[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      acc[bi][bj] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[bi][bj][r] = 0.0;
    }
  const long nst = (K + TV_KS - 1) / TV_KS;
  fetch(0);
  for (long s = 0; s < nst; ++s) {
    __syncthreads();                      // the previous step's MFMAs have read As and Bs
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (TR) As[((tid >> 6) + 4 * i) * TV_LS + (tid & 63)] = ra[i];
      else As[(tid & 31) * TV_LS + (tid >> 5) + 8 * i] = ra[i];
      Bs[((tid >> 6) + 4 * i) * TV_LS + (tid & 63)] = rb[i];
    }
    __syncthreads();
    if (s + 1 < nst) fetch((s + 1) * TV_KS);
#pragma unroll
    for (int q = 0; q < TV_KS / 4; ++q) {
      const int kk = (q * 4 + kq) * TV_LS;
      const float a0 = As[kk + wm + cq], a1 = As[kk + wm + 16 + cq], b0 = Bs[kk + wn + cq], b1 = Bs[kk + wn + 16 + cq];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if ((s + 1) % (TV_RUN / TV_KS) == 0 || s + 1 == nst) {
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sum[bi][bj][r] += (double)acc[bi][bj][r];
          acc[bi][bj] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
  }
  // C/D layout: column = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = m0 + wm + bi * 16 + kq * 4 + r, col = n0 + wn + bj * 16 + cq;
        if (row < m && col < n) {
          if (TR) acc_out[row * n + col] += sum[bi][bj][r];
          else out[row * n + col] = (float)sum[bi][bj][r];
        }
      }
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
  SSV_CHECK(R <= TV_MAX_R && C <= TV_MAX_C && D <= TV_MAX_D, SSV_UNSUPPORTED, "%s: R=%d (at most %d), C=%d (at most %d) or D=%d (at most %d) beyond the kernels", what, R,
            TV_MAX_R, C, TV_MAX_C, D, TV_MAX_D);
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

static int tv_product_grid(const char* what, long m, long n, dim3* grid) {
  const long gx = (n + TV_TILE - 1) / TV_TILE, gy = (m + TV_TILE - 1) / TV_TILE;
  SSV_CHECK(gx <= 0x7fffffffL && gy <= 65535, SSV_UNSUPPORTED, "%s: %ld x %ld tiles exceed the grid (2^31 - 1 x 65535)", what, gx, gy);
  *grid = dim3((unsigned)gx, (unsigned)gy);
  return 0;
}

int tv_launch_product(const float* A, const float* B, float* out, long m, long n, long K, hipStream_t st) {
  dim3 grid;
  SSV_TRY(tv_product_grid("ivec_product", m, n, &grid));
  hipLaunchKernelGGL(tv_product_kernel<false>, grid, dim3(256), 0, st, A, B, out, (double*)nullptr, m, n, K);
  return ssv_check_launch("ivec_product");
}

int tv_launch_product_tn(const float* A, const float* B, double* acc, long U, long m, long n, hipStream_t st) {
  dim3 grid;
  SSV_TRY(tv_product_grid("ivec_product_tn", m, n, &grid));
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
