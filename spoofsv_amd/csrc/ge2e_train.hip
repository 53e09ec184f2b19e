// GE2E training on a corpus held on the device (GE2E/train_speech_embedder.py:63-86 around the embedder), gfx950: the batch assembly
// of GE2E/data_load.py:77-85 for a whole batch (ssv_tisv_batch_gather) and gradient clipping + SGD for every parameter in two launches
// (ssv_clip_sgd_multi).  Both are bandwidth-class: 5.8 MB of batch at 300 utterances of 40 x 120, 48 MB x 2.5 of weights and gradients
// at 12 M parameters.  All sums run in a fixed order (no atomics, no arrival order): the same inputs give the same bits.
#include "ssv_common.h"

#define GT_THREADS 256
#define GT_TILE 64                  // mel rows and frames of one workgroup's tile: one 256-byte run per mel row and wave load
#define GT_LD (GT_TILE + 1)         // LDS row stride in floats: odd, so the transposed ds_read_b32 (32 banks) meets every bank once per 32 lanes

// ---- out[b][t][f] = corpus[rows[b]][f][t] -------------------------------------------------------------------------------------------
// Workgroup (b * nft + frame tile, mel tile): reads min(64, frames - t0) consecutive frames of each of its mel rows (lane = frame),
// writes for every frame its mel bins (lane = mel bin fastest: with nmels <= 64 the whole tile is ONE run of nt * nmels floats of
// out).  A row outside the corpus is not dereferenced: the utterance becomes NaN (the host validates the table it drew; this keeps a
// wrong one from reading out of bounds, and visible).
__global__ __launch_bounds__(GT_THREADS) void tisv_batch_gather_kernel(const float* __restrict__ corpus, long U_total, const int* __restrict__ rows,
                                                                       float* __restrict__ out, int nmels, int frames, int nft) {
  __shared__ float tile[GT_TILE * GT_LD];
  const int b = blockIdx.x / nft, t0 = (blockIdx.x % nft) * GT_TILE, f0 = blockIdx.y * GT_TILE;
  const int nt = min(GT_TILE, frames - t0), nf = min(GT_TILE, nmels - f0);
  const long row = rows[b];
  const bool ok = row >= 0 && row < U_total;
  const float* src = corpus + ((ok ? row : 0) * nmels + f0) * (long)frames + t0;
  for (int e = threadIdx.x; e < nf * GT_TILE; e += GT_THREADS) {
    const int f = e / GT_TILE, t = e % GT_TILE;
    if (t < nt) tile[f * GT_LD + t] = ok ? src[(long)f * frames + t] : __builtin_nanf("");
  }
  __syncthreads();
  float* dst = out + ((long)b * frames + t0) * nmels + f0;
  for (int e = threadIdx.x; e < nt * nf; e += GT_THREADS) {
    const int t = e / nf, f = e - t * nf;
    dst[(long)t * nmels + f] = tile[f * GT_LD + t];
  }
}

extern "C" int ssv_tisv_batch_gather(const float* corpus, long U_total, const int* rows, float* out, int Bn, int nmels, int frames,
                                     ssv_stream_t stream) {
  SSV_CHECK(corpus && rows && out && U_total > 0 && Bn > 0 && nmels > 0 && frames > 0, SSV_BAD_SHAPE,
            "tisv_batch_gather: null pointer or empty problem (U_total=%ld Bn=%d nmels=%d frames=%d)", U_total, Bn, nmels, frames);
  const int nft = ssv_cdiv(frames, GT_TILE), nmt = ssv_cdiv(nmels, GT_TILE);
  SSV_CHECK((long)Bn * nft <= 0x7fffffffL && nmt <= 65535, SSV_UNSUPPORTED, "tisv_batch_gather: Bn=%d x %d frame tiles or %d mel tiles exceed the grid", Bn, nft, nmt);
  hipLaunchKernelGGL(tisv_batch_gather_kernel, dim3(Bn * nft, nmt), dim3(GT_THREADS), 0, (hipStream_t)stream, corpus, U_total, rows, out, nmels, frames, nft);
  return ssv_check_launch("tisv_batch_gather");
}

// ---- clip_grad_norm_ per group + SGD ----------------------------------------------------------------------------------------------
#define CS_THREADS 256
typedef float cs_f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) cs_f4 cs_gf4;        // pointers come from the chunk table, i.e. from memory: spelled out as global (ssv_global)
struct ClipNorms { float max_norm[SSV_CLIP_SGD_MAX_GROUPS]; };

// Pass 1: partial[piece] = sum g^2 in double.  Thread i adds its elements i, i + 256, ... in that order (four at a time where the
// gradient pointer is 16-byte aligned), then the 256 sums meet in a fixed tree.  (double)g * g is exact, so fused or not is the same.
__global__ __launch_bounds__(CS_THREADS) void clip_sgd_sumsq_kernel(const ssv_clip_sgd_chunk* __restrict__ chunks, double* __restrict__ partial) {
  __shared__ double red[CS_THREADS];
  const ssv_clip_sgd_chunk ch = chunks[blockIdx.x];
  const float* g = ssv_global(ch.g);
  double acc = 0.0;
  long i0 = 0;
  if (((uintptr_t)ch.g & 15) == 0) {
    const cs_gf4* g4 = (const cs_gf4*)ch.g;
    const long n4 = ch.n >> 2;
    for (long i = threadIdx.x; i < n4; i += CS_THREADS) {
      const cs_f4 v = g4[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)v[k] * (double)v[k];
    }
    i0 = n4 > 0 ? n4 << 2 : 0;
  }
  for (long i = i0 + threadIdx.x; i < ch.n; i += CS_THREADS) acc += (double)g[i] * (double)g[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = CS_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// Pass 2.  Workgroups [0, ngroups) write norms[group] (workgroup 0 also the loss history slot and the counter); workgroup
// ngroups + j updates piece j.  Every workgroup adds the partials of ITS group in piece order -- 256 at a time staged in LDS (a piece
// of another group contributes +0.0, which changes no sum of squares), every thread then adding the staged values in index order
// (broadcast reads) -- so all workgroups of a group hold the same bits of S without exchanging anything.  Under a thousand doubles
// from L2 at 12 M parameters in 16 K-element pieces.
__global__ __launch_bounds__(CS_THREADS) void clip_sgd_apply_kernel(const ssv_clip_sgd_chunk* __restrict__ chunks, int nchunks, int ngroups, ClipNorms mn,
                                                                    float lr, const double* __restrict__ partial, float* __restrict__ norms,
                                                                    const float* __restrict__ loss, float* __restrict__ loss_hist, int hist_len,
                                                                    int* __restrict__ step_dev) {
  __shared__ double stage[CS_THREADS];
  const bool writer = (int)blockIdx.x < ngroups;
  ssv_clip_sgd_chunk ch = {nullptr, nullptr, 0, 0, 0};
  int group = blockIdx.x;
  if (!writer) {
    ch = chunks[blockIdx.x - ngroups];
    group = ch.group;
    if (group < 0 || group >= ngroups || ch.n < 1) return;          // (block-uniform) a piece without a group is left alone
  }
  double S = 0.0;
  for (int base = 0; base < nchunks; base += CS_THREADS) {
    const int j = base + threadIdx.x;
    stage[threadIdx.x] = (j < nchunks && chunks[j].group == group) ? partial[j] : 0.0;
    __syncthreads();
    const int m = min(CS_THREADS, nchunks - base);
    for (int k = 0; k < m; ++k) S += stage[k];
    __syncthreads();
  }
  const double total = sqrt(S);
  if (writer) {
    if (threadIdx.x == 0) {
      norms[group] = (float)total;
      if (blockIdx.x == 0 && step_dev) {
        const int s = step_dev[0];
        if (loss && loss_hist && hist_len > 0) loss_hist[((s % hist_len) + hist_len) % hist_len] = loss[0];
        step_dev[0] = s + 1;
      }
    }
    return;
  }
  float max_norm = 0.f;
#pragma unroll
  for (int k = 0; k < SSV_CLIP_SGD_MAX_GROUPS; ++k) max_norm = (k == group) ? mn.max_norm[k] : max_norm;
  double cd = (double)max_norm / (total + 1e-6);
  cd = cd > 1.0 ? 1.0 : cd;                                         // torch.clamp(max=1.0): a NaN stays a NaN
  const float step = __fmul_rn(lr, (float)cd);
  float* p = ssv_global(ch.p);
  const float* g = ssv_global(ch.g);
  long i0 = 0;
  if ((((uintptr_t)ch.p | (uintptr_t)ch.g) & 15) == 0) {
    cs_gf4* p4 = (cs_gf4*)ch.p;
    const cs_gf4* g4 = (const cs_gf4*)ch.g;
    const long n4 = ch.n >> 2;
    for (long i = threadIdx.x; i < n4; i += CS_THREADS) {
      cs_f4 pv = p4[i];
      const cs_f4 gv = g4[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) pv[k] = __fsub_rn(pv[k], __fmul_rn(step, gv[k]));
      p4[i] = pv;
    }
    i0 = n4 << 2;
  }
  for (long i = i0 + threadIdx.x; i < ch.n; i += CS_THREADS) p[i] = __fsub_rn(p[i], __fmul_rn(step, g[i]));
}

extern "C" long ssv_clip_sgd_workspace(int nchunks) { return nchunks > 0 ? (long)nchunks * (long)sizeof(double) : 0; }

extern "C" int ssv_clip_sgd_multi(const ssv_clip_sgd_chunk* chunks, int nchunks, const float* max_norm, int ngroups, float lr, float* norms,
                                  const float* loss, float* loss_hist, int hist_len, int* step_dev, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(chunks && max_norm && norms && nchunks > 0 && ngroups > 0 && ngroups <= SSV_CLIP_SGD_MAX_GROUPS, SSV_BAD_SHAPE,
            "clip_sgd_multi: null pointer, nchunks=%d or ngroups=%d (1..%d)", nchunks, ngroups, SSV_CLIP_SGD_MAX_GROUPS);
  SSV_CHECK(!loss_hist || (loss && step_dev && hist_len > 0), SSV_BAD_SHAPE, "clip_sgd_multi: a loss history needs loss, step_dev and hist_len=%d > 0", hist_len);
  SSV_CHECK(ws && ws_bytes >= (size_t)ssv_clip_sgd_workspace(nchunks), SSV_BAD_SHAPE, "clip_sgd_multi: workspace of %zu bytes, need %ld", ws_bytes, ssv_clip_sgd_workspace(nchunks));
  ClipNorms mn = {};
  for (int k = 0; k < ngroups; ++k) mn.max_norm[k] = max_norm[k];
  hipLaunchKernelGGL(clip_sgd_sumsq_kernel, dim3(nchunks), dim3(CS_THREADS), 0, (hipStream_t)stream, chunks, (double*)ws);
  SSV_TRY(ssv_check_launch("clip_sgd_sumsq"));
  hipLaunchKernelGGL(clip_sgd_apply_kernel, dim3(ngroups + nchunks), dim3(CS_THREADS), 0, (hipStream_t)stream, chunks, nchunks, ngroups, mn, lr,
                     (const double*)ws, norms, loss, loss_hist, hist_len, step_dev);
  return ssv_check_launch("clip_sgd_apply");
}
