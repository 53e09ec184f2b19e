// The exact-fp32 product tile of the i-vector chain on v_mfma_f32_16x16x4_f32, once: tv_product_kernel<false / true> (ivector_tv.hip) and
// plda_score_kernel (plda.hip) are this tile with their own operand loaders and their own store.
#pragma once
#include "ssv_common.h"

#define XP_TILE 64                  // a workgroup owns a 64 x 64 tile of the output, a wave a 32 x 32 quarter of it (ssv_ivec_product_tile)
#define XP_KS 32                    // K elements staged per step
#define XP_LS (XP_TILE + 1)         // row stride of a staged step (k-major): the transposing store of the k-fastest map hits 32 banks
#define XP_RUN 256                  // K elements of one fp32 chain; the runs are added in double (ssv_ivec_product_run)

// Which (k, row) of a 32 x 64 step thread tid of 256 holds in register i of 8: the map that walks the operand's memory along its rows.
struct XpKFast {                    // K-contiguous operand
  static __device__ __forceinline__ int k(int tid, int i) { return tid & 31; }
  static __device__ __forceinline__ int row(int tid, int i) { return (tid >> 5) + 8 * i; }
};
struct XpRowFast {                  // row-contiguous operand (K, rows)
  static __device__ __forceinline__ int k(int tid, int i) { return (tid >> 6) + 4 * i; }
  static __device__ __forceinline__ int row(int tid, int i) { return tid & 63; }
};

// One 64 x 64 tile of A B^T over K, called by every thread of a 256-thread workgroup.  load_a / load_b (k, row in tile) -> float give an
// operand element, 0 beyond an edge; store (row in tile, column in tile, double) takes a finished element (it checks the edges itself).
// K is walked in steps of XP_KS staged k-major in LDS; the step after the one being multiplied waits in registers.  A wave multiplies its
// quarter as 2 x 2 blocks of 16 x 16, element k of a step in MFMA q = k / 4.  An fp32 chain runs over XP_RUN elements of K from zero
// accumulators and is then added to DOUBLE registers.  The order of an element's sum depends on K alone: a row of the output does not
// depend on the rows that share its launch, nor on which of the kernels computes it.
template <class MapA, class MapB, class LoadA, class LoadB, class Store>
__device__ __forceinline__ void xp_tile(long K, LoadA load_a, LoadB load_b, Store store) {
  __shared__ float As[XP_KS * XP_LS], Bs[XP_KS * XP_LS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cq = lane & 15;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  float ra[8], rb[8];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ra[i] = load_a(k0 + MapA::k(tid, i), MapA::row(tid, i));
      rb[i] = load_b(k0 + MapB::k(tid, i), MapB::row(tid, i));
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
  const long nst = (K + XP_KS - 1) / XP_KS;
  fetch(0);
  for (long s = 0; s < nst; ++s) {
    __syncthreads();                      // the previous step's MFMAs have read As and Bs
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      As[MapA::k(tid, i) * XP_LS + MapA::row(tid, i)] = ra[i];
      Bs[MapB::k(tid, i) * XP_LS + MapB::row(tid, i)] = rb[i];
    }
    __syncthreads();
    if (s + 1 < nst) fetch((s + 1) * XP_KS);
#pragma unroll
    for (int q = 0; q < XP_KS / 4; ++q) {
      const int kk = (q * 4 + kq) * XP_LS;
      const float a0 = As[kk + wm + cq], a1 = As[kk + wm + 16 + cq], b0 = Bs[kk + wn + cq], b1 = Bs[kk + wn + 16 + cq];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if ((s + 1) % (XP_RUN / XP_KS) == 0 || s + 1 == nst) {
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
      for (int r = 0; r < 4; ++r) store(wm + bi * 16 + kq * 4 + r, wn + bj * 16 + cq, sum[bi][bj][r]);
}

// the launch grid of an (m, n) output: tiles of n along x, of m along y
static inline int xp_grid(const char* what, long m, long n, dim3* grid) {
  const long gx = (n + XP_TILE - 1) / XP_TILE, gy = (m + XP_TILE - 1) / XP_TILE;
  SSV_CHECK(gx <= 0x7fffffffL && gy <= 65535, SSV_UNSUPPORTED, "%s: %ld x %ld tiles exceed the grid (2^31 - 1 x 65535)", what, gx, gy);
  *grid = dim3((unsigned)gx, (unsigned)gy);
  return 0;
}
