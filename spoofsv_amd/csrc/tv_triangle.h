// The packed float64 triangle in LDS: Cholesky, triangular inverse and W^T W of a symmetric positive definite matrix, shared by the
// i-vector extractor (ivector_tv.hip), the PLDA back end (plda.hip) and the full-covariance UBM (fgmm.hip), with the wave sum, the
// workgroup sum and the dynamic-LDS limit that the chain's kernel files need (ivector.hip takes the last two).
#pragma once
#include <atomic>
#include "ivec_chain.h"             // IVEC_MAX_R: the largest triangle

#define TV_LDS_MAX (160 * 1024)     // LDS of a CU: one workgroup may take all of it

__device__ __forceinline__ int tv_tri(int i, int j) { return i * (i + 1) / 2 + j; }       // packed lower triangle, row-major, j <= i
__device__ __forceinline__ double tv_wave_sum(double v) {      // every lane gets the sum over the 64 lanes; the butterfly's shape is fixed
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// sum of a per-thread double over the 256 threads of a workgroup (sm: 256 doubles of LDS), every thread gets it; the tree's shape is fixed
__device__ __forceinline__ double tv_wg_sum(double v, double* sm) {
  __syncthreads();
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  return sm[0];
}

// ---- the packed triangle in LDS --------------------------------------------------------------------------------------------------------
// All three work in place on tri, the packed lower triangle of a symmetric positive definite matrix in double, with any number of whole
// waves; every thread of the workgroup calls them, and every branch on the data is taken by all of them alike (the value is read from LDS
// by every thread), so a bad pivot ends the call for the whole workgroup at once: nothing waits at a barrier the others have left.
//
// Cholesky, right-looking: column j is scaled by the root of its pivot and copied to col, then rows i > j subtract col[i] col[k] from
// their entries k in (j, i] -- a wave per row, the lanes along the row, which is contiguous.  y, when given, is solved along the way:
// y <- C^-1 y (the forward substitution needs column j exactly when col holds it).  Returns false at a pivot that is not positive.
__device__ inline bool tv_cholesky(double* tri, double* col, double* y, int R) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  for (int j = 0; j < R; ++j) {
    const double d = tri[tv_tri(j, j)];
    if (!(d > 0.0)) return false;
    const double s = sqrt(d);
    __syncthreads();                      // every thread has read the pivot (and, from the step before, col)
    for (int k = j + tid; k < R; k += nt) {
      const double v = k == j ? s : tri[tv_tri(k, j)] / s;
      tri[tv_tri(k, j)] = v;
      col[k] = v;
    }
    if (y && tid == 0) y[j] = y[j] / s;
    __syncthreads();
    for (int i = j + 1 + wave; i < R; i += nw) {
      const double ci = col[i];
      double* row = tri + tv_tri(i, 0);
      for (int k = j + 1 + lane; k <= i; k += 64) row[k] -= ci * col[k];
    }
    if (y)
      for (int i = j + 1 + tid; i < R; i += nt) y[i] -= col[i] * y[j];
    __syncthreads();
  }
  return true;
}

// The inverse of the lower triangular factor, in place (LAPACK's trtri, unblocked, from the last column to the first): with the columns
// beyond j done, column j becomes -W[j+1:, j+1:] C[j+1:, j] / C[j][j] -- the old column copied to col, then a wave per row i, the lanes along
// k in (j, i], a butterfly sum.
__device__ inline void tv_trtri(double* tri, double* col, int R) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  for (int j = R - 1; j >= 0; --j) {
    const double dj = 1.0 / tri[tv_tri(j, j)];
    __syncthreads();
    for (int k = j + 1 + tid; k < R; k += nt) col[k] = tri[tv_tri(k, j)];
    if (tid == 0) tri[tv_tri(j, j)] = dj;
    __syncthreads();
    for (int i = j + 1 + wave; i < R; i += nw) {
      const double* row = tri + tv_tri(i, 0);
      double s = 0.0;
      for (int k = j + 1 + lane; k <= i; k += 64) s += row[k] * col[k];
      s = tv_wave_sum(s);
      if (lane == 0) tri[tv_tri(i, j)] = -s * dj;
    }
  }
  __syncthreads();
}

// W^T W of the lower triangular W, in place (LAPACK's lauum, unblocked, from the first row to the last): row i of the result is
// sum_{m >= i} W[m][i] W[m][k], k <= i, and needs only rows m >= i of W.  Column i is copied to col; thread (g, k) of nt / 256 groups adds
// the rows m = i + g, i + g + groups, ... for its k (the lanes along a row); the groups' partial sums meet in part, added in ascending g.
__device__ inline void tv_lauum(double* tri, double* col, double* part /* [nt / 256][256] */, int R) {
  const int tid = threadIdx.x, nt = blockDim.x, k = tid & 255, g = tid >> 8, ng = nt >> 8;
  for (int i = 0; i < R; ++i) {
    for (int mm = i + tid; mm < R; mm += nt) col[mm] = tri[tv_tri(mm, i)];
    __syncthreads();
    if (k <= i) {
      double s = 0.0;
      for (int mm = i + g; mm < R; mm += ng) s += col[mm] * tri[tv_tri(mm, k)];
      part[g * 256 + k] = s;
    }
    __syncthreads();
    if (g == 0 && k <= i) {
      double s = part[k];
      for (int q = 1; q < ng; ++q) s += part[q * 256 + k];
      tri[tv_tri(i, k)] = s;              // (row i is read by no later step: they take rows m > i and columns of them)
    }
  }
  __syncthreads();
}

// Kernels that take more than 64 KB of dynamic LDS say so once per device: done is the caller's table of 64 flags, ks its kernels.
static inline int tv_lds_limit_set(std::atomic<int>* done, const void* const* ks, int nk, const char* who) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return ssv_fail(-(int)e, "%s: hipGetDevice: %s", who, hipGetErrorString(e));
  if (dev >= 0 && dev < 64 && done[dev].load(std::memory_order_acquire)) return 0;
  for (int i = 0; i < nk; ++i) {
    e = hipFuncSetAttribute(ks[i], hipFuncAttributeMaxDynamicSharedMemorySize, TV_LDS_MAX);
    if (e != hipSuccess) return ssv_fail(-(int)e, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", who, hipGetErrorString(e));
  }
  if (dev >= 0 && dev < 64) done[dev].store(1, std::memory_order_release);
  return 0;
}
