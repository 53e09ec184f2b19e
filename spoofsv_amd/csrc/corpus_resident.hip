// Text2Mel / SSRN training from a spectrogram corpus held on the device (data/dataset.py:83-173, the items; :187-258, the collate
// functions), gfx950: a batch is gathered from ragged arenas into the collated layout -- zero padding to a common width -- in one launch
// per tensor.  Bandwidth-class: an SSRN batch of 32 items is ~60 MB read and ~85 MB written.  Plain copies, no atomics: the same inputs
// give the same bits.
#include "ssv_common.h"

#define CG_THREADS 256
#define CG_ROWS (CG_THREADS / 64)   // one wave per output row: its alignment case and its length are wave-uniform

// ---- out[b][f][t] = t < len[r] ? arena[off[r] + f * len[r] + t] : 0,  r = rows[b] -----------------------------------------------------
// Workgroup (b, group of CG_ROWS rows); lane = t fastest, so a wave reads one run of the item's row and writes one run of the output's.
// When the row starts on a 16-byte boundary on both sides every lane moves four floats per access (1 KiB per wave instruction), else one.
// The last, partial quad of an aligned row is read float by float: nothing past the item's own row is touched.  An item that is not in
// the corpus (a row index outside [0, n_items), a negative length, a block that leaves the arena) is never dereferenced: the whole
// (F, width) item becomes NaN, as tisv_batch_gather_kernel has it.
__global__ __launch_bounds__(CG_THREADS) void corpus_gather_kernel(const float* __restrict__ arena, long arena_n, const long* __restrict__ off,
                                                                   const int* __restrict__ len, int n_items, const int* __restrict__ rows,
                                                                   float* __restrict__ out, int F, int width, long out_bs, int groups) {
  const int b = blockIdx.x / groups, f = (blockIdx.x % groups) * CG_ROWS + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= F) return;
  float* dst = out + (long)b * out_bs + (long)f * width;
  const int r = rows[b];
  bool ok = r >= 0 && r < n_items;
  long o = 0;
  int n = 0;
  if (ok) {
    o = off[r];
    n = len[r];
    ok = n >= 0 && o >= 0 && o <= arena_n && (long)F * n <= arena_n - o;
  }
  if (!ok) {
    for (int t = lane; t < width; t += 64) dst[t] = __builtin_nanf("");
    return;
  }
  const float* src = arena + o + (long)f * n;
  const int m = min(n, width);                                   // a longer item is clipped
  int t0 = 0;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int wq = width & ~3;
    for (int t = lane * 4; t < wq; t += 256) {
      f32x4 v;
      if (t + 4 <= m) {
        v = *(const f32x4*)(src + t);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = t + k < m ? src[t + k] : 0.f;
      }
      *(f32x4*)(dst + t) = v;
    }
    t0 = wq;
  }
  for (int t = t0 + lane; t < width; t += 64) dst[t] = t < m ? src[t] : 0.f;
}

// ---- out[b][0][t] = t < len[r] ? (int64) arena[off[r] + t] : 0 ------------------------------------------------------------------------
// Text ids: a few hundred bytes per item.  Workgroup (b, 256 positions).  An item outside the corpus becomes -1 everywhere (no id is
// negative; an embedding lookup with it fails loudly).
__global__ __launch_bounds__(CG_THREADS) void corpus_gather_ids_kernel(const int* __restrict__ arena, long arena_n, const long* __restrict__ off,
                                                                       const int* __restrict__ len, int n_items, const int* __restrict__ rows,
                                                                       long* __restrict__ out, int width, int tiles) {
  const int b = blockIdx.x / tiles, t = (blockIdx.x % tiles) * CG_THREADS + (int)threadIdx.x;
  if (t >= width) return;
  const int r = rows[b];
  bool ok = r >= 0 && r < n_items;
  long o = 0;
  int n = 0;
  if (ok) {
    o = off[r];
    n = len[r];
    ok = n >= 0 && o >= 0 && o <= arena_n && n <= arena_n - o;
  }
  out[(long)b * width + t] = !ok ? -1L : (t < n ? (long)arena[o + t] : 0L);
}

// ---- arena[off[i] + f * len[i] + t] = src[b][f][t] for t < len[i],  i = item0 + b: the inverse of corpus_gather_kernel --------------
// The same decomposition: workgroup (b, group of CG_ROWS rows), one wave per row, lane = t fastest; 16-byte accesses when the row starts
// on a 16-byte boundary on both sides, the last partial quad and every other row float by float, so nothing past the item's own row is
// written.  An item that does not fit -- len < 0, len > width (the batch does not hold all of it), a block that leaves the arena -- is
// left alone: no word of the arena changes for it.
__global__ __launch_bounds__(CG_THREADS) void corpus_scatter_kernel(const float* __restrict__ src, long src_bs, float* __restrict__ arena, long arena_n,
                                                                    const long* __restrict__ off, const int* __restrict__ len, int item0, int F,
                                                                    int width, int groups) {
  const int b = blockIdx.x / groups, f = (blockIdx.x % groups) * CG_ROWS + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= F) return;
  const long o = off[item0 + b];
  const int n = len[item0 + b];
  if (n < 0 || n > width || o < 0 || o > arena_n || (long)F * n > arena_n - o) return;
  const float* from = src + (long)b * src_bs + (long)f * width;
  float* dst = arena + o + (long)f * n;
  int t0 = 0;
  if ((((uintptr_t)from | (uintptr_t)dst) & 15) == 0) {
    const int nq = n & ~3;
    for (int t = lane * 4; t < nq; t += 256) *(f32x4*)(dst + t) = *(const f32x4*)(from + t);
    t0 = nq;
  }
  for (int t = t0 + lane; t < n; t += 64) dst[t] = from[t];
}

extern "C" int ssv_corpus_gather(const float* arena, long arena_n, const long* off, const int* len, int n_items, const int* rows, long n_rows,
                                 long row0, float* out, int B, int F, int width, long out_bs, ssv_stream_t stream) {
  SSV_CHECK(arena && off && len && rows && out && arena_n > 0 && n_items > 0 && B > 0 && F > 0 && width > 0, SSV_BAD_SHAPE,
            "corpus_gather: null pointer or empty problem (arena_n=%ld n_items=%d B=%d F=%d width=%d)", arena_n, n_items, B, F, width);
  SSV_CHECK(row0 >= 0 && n_rows > 0 && row0 <= n_rows - B, SSV_BAD_SHAPE, "corpus_gather: rows [%ld, %ld + %d) leave the table of %ld", row0, row0, B, n_rows);
  SSV_CHECK(out_bs >= (long)F * width, SSV_BAD_SHAPE, "corpus_gather: batch stride %ld below F * width = %ld", out_bs, (long)F * width);
  const int groups = ssv_cdiv(F, CG_ROWS);
  SSV_CHECK((long)B * groups <= 0x7fffffffL, SSV_UNSUPPORTED, "corpus_gather: B=%d x %d row groups exceed the grid", B, groups);
  hipLaunchKernelGGL(corpus_gather_kernel, dim3(B * groups), dim3(CG_THREADS), 0, (hipStream_t)stream, arena, arena_n, off, len, n_items, rows + row0, out,
                     F, width, out_bs, groups);
  return ssv_check_launch("corpus_gather");
}

extern "C" int ssv_corpus_gather_ids(const int* arena, long arena_n, const long* off, const int* len, int n_items, const int* rows, long n_rows,
                                     long row0, long* out, int B, int width, ssv_stream_t stream) {
  SSV_CHECK(arena && off && len && rows && out && arena_n > 0 && n_items > 0 && B > 0 && width > 0, SSV_BAD_SHAPE,
            "corpus_gather_ids: null pointer or empty problem (arena_n=%ld n_items=%d B=%d width=%d)", arena_n, n_items, B, width);
  SSV_CHECK(row0 >= 0 && n_rows > 0 && row0 <= n_rows - B, SSV_BAD_SHAPE, "corpus_gather_ids: rows [%ld, %ld + %d) leave the table of %ld", row0, row0, B, n_rows);
  const int tiles = ssv_cdiv(width, CG_THREADS);
  SSV_CHECK((long)B * tiles <= 0x7fffffffL, SSV_UNSUPPORTED, "corpus_gather_ids: B=%d x %d tiles exceed the grid", B, tiles);
  hipLaunchKernelGGL(corpus_gather_ids_kernel, dim3(B * tiles), dim3(CG_THREADS), 0, (hipStream_t)stream, arena, arena_n, off, len, n_items, rows + row0, out,
                     width, tiles);
  return ssv_check_launch("corpus_gather_ids");
}

extern "C" int ssv_corpus_scatter(const float* src, long src_bs, int B, int F, int width, float* arena, long arena_n, const long* off, const int* len,
                                  int n_items, int item0, ssv_stream_t stream) {
  SSV_CHECK(src && arena && off && len && arena_n > 0 && n_items > 0 && B > 0 && F > 0 && width > 0, SSV_BAD_SHAPE,
            "corpus_scatter: null pointer or empty problem (arena_n=%ld n_items=%d B=%d F=%d width=%d)", arena_n, n_items, B, F, width);
  SSV_CHECK(item0 >= 0 && item0 <= n_items - B, SSV_BAD_SHAPE, "corpus_scatter: items [%d, %d + %d) leave the table of %d", item0, item0, B, n_items);
  SSV_CHECK(src_bs >= (long)F * width, SSV_BAD_SHAPE, "corpus_scatter: batch stride %ld below F * width = %ld", src_bs, (long)F * width);
  const int groups = ssv_cdiv(F, CG_ROWS);
  SSV_CHECK((long)B * groups <= 0x7fffffffL, SSV_UNSUPPORTED, "corpus_scatter: B=%d x %d row groups exceed the grid", B, groups);
  hipLaunchKernelGGL(corpus_scatter_kernel, dim3(B * groups), dim3(CG_THREADS), 0, (hipStream_t)stream, src, src_bs, arena, arena_n, off, len, item0, F,
                     width, groups);
  return ssv_check_launch("corpus_scatter");
}
