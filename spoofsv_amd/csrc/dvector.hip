// Whole-utterance d-vector extraction (GE2E/dvector_create.py:38-73), gfx950: every centred STFT frame of a table of voiced spans,
// the 24-frame windows of the log-mel frames, and the partition means of the window embeddings.  The DFT and the log-mel step between
// ssv_span_frames and ssv_gather_windows are ssv_conv1d_fwd (k = 1) and ssv_power_mel_log, as in sv_frontend.hip; the embedder is
// ssv_lstm_fwd_cached + ssv_proj_l2norm_fwd.  The host plans (spoofsv_amd/dvector.py: plan) and ships three int tables; a kernel
// checks every table entry it reads against the buffers' sizes and skips what does not fit, so a wrong table cannot write out of
// bounds.  All sums run in a fixed order (no atomics).
#include "ssv_common.h"
#include "frame_stage.h"

#define DV_THREADS 256
#define DV_TILE 64                 // frames of one workgroup's tile: one 256-byte run per sample row and wave store
#define DV_SPAN_MAX 12288          // floats of a tile's staged sample range, (DV_TILE - 1) * hop + n_fft; 10,592 at hop 160, n_fft 512
#define DV_SKEW_SHIFT 5            // ssv_skew's shift: conflict-free at hop = 160 = 5 * 32
#define DV_LDS_FLOATS (DV_SPAN_MAX + DV_SPAN_MAX / 32 + 1)      // 50,692 bytes: three workgroups per CU

// ---- librosa.stft's framing (dvector_create.py:43) of every span, all frames ---------------------------------------------------------
// tiles (n_tiles, 6) int: row, span start, span end, first frame f0 of the tile in its span, its first compact frame index g0, frame
// count cnt <= DV_TILE.  Compact frame g of this call (g = g0 + t - g_base, 0 <= g < n_frames) is column g % Tc of item g / Tc:
// fr[g / Tc][i][g % Tc] = reflect_pad(seg, N / 2)[(f0 + t) * hop + i], seg = y[row][start:end].  A workgroup stages the samples its
// tile reads once in LDS and writes each of the N sample rows as one run of cnt floats (frame_stage.h).  Workgroup n_tiles zeroes the
// pad columns of the last item.
__global__ __launch_bounds__(DV_THREADS) void span_frames_kernel(const float* __restrict__ y, const int* __restrict__ tiles,
                                                                 float* __restrict__ fr, int B, int n_max, int n_tiles, int N, int hop,
                                                                 int Tc, int R, int g_base, int n_frames) {
  __shared__ float sm[DV_LDS_FLOATS];
  if ((int)blockIdx.x >= n_tiles) {                         // pad columns [n_frames, R * Tc): all in item R - 1 (checked on the host)
    const int pad = R * Tc - n_frames;
    float* last = fr + (long)(R - 1) * N * Tc + (Tc - pad);
    for (int e = threadIdx.x; e < N * pad; e += DV_THREADS) last[(long)(e / pad) * Tc + e % pad] = 0.f;
    return;
  }
  const int* tl = tiles + 6 * (long)blockIdx.x;
  const int row = tl[0], start = tl[1], end = tl[2], f0 = tl[3], g0 = tl[4], cnt = tl[5];
  const int len = end - start;
  // a tile that does not fit the buffers or the single reflection is skipped (block-uniform)
  if (row < 0 || row >= B || start < 0 || end > n_max || len <= N / 2 || f0 < 0 || cnt < 1 || cnt > DV_TILE ||
      (long)(f0 + cnt - 1) * hop > (long)len)
    return;
  frame_stage_load<false, DV_THREADS>(sm, y + (long)row * n_max + start, len, f0 * hop - N / 2, (cnt - 1) * hop + N, DV_SKEW_SHIFT, 0.f);   // count <= DV_SPAN_MAX, checked on the host
  __syncthreads();
  const int wave = threadIdx.x >> 6, t = threadIdx.x & 63;
  const long g = (long)g0 + t - g_base;
  if (t >= cnt || g < 0 || g >= n_frames) return;
  frame_stage_store(sm, fr + (g / Tc) * (long)N * Tc + g % Tc, Tc, t * hop, wave, DV_THREADS / 64, N, DV_SKEW_SHIFT);
}

// ---- S[:, j:j + 24] for j = 0, 12, ... (dvector_create.py:48-52) as rows of the frames-major log-mel array -----------------------------
// out[w] (window, nmels) = mel[g0[w] : g0[w] + window]: one contiguous run of window * nmels floats, copied 16 bytes at a time when
// nmels % 4 == 0 (V = 4), float by float otherwise.  A window whose g0 does not fit the array is written as zeros.
template <int V>
__global__ __launch_bounds__(DV_THREADS) void gather_windows_kernel(const float* __restrict__ mel, const int* __restrict__ g0,
                                                                    float* __restrict__ out, int G, long total, int per, int window,
                                                                    int nmels) {
  const long idx = (long)blockIdx.x * DV_THREADS + threadIdx.x;
  if (idx >= total) return;
  const long w = idx / per;
  const int k = (int)(idx % per);
  const int g = g0[w];
  const bool ok = g >= 0 && (long)g + window <= (long)G;
  if (V == 4) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok) v = *reinterpret_cast<const f32x4*>(mel + (long)g * nmels + 4 * k);
    *reinterpret_cast<f32x4*>(out + (w * per + k) * 4) = v;
  } else {
    out[w * per + k] = ok ? mel[(long)g * nmels + k] : 0.f;
  }
}

// ---- np.average(embeddings[start:end], axis=0) (dvector_create.py:70-72) ----------------------------------------------------------------
// One wave per partition p; lane l owns columns l, l + 64, ...: the rows offs[p] .. offs[p + 1] - 1 are added in ascending order in
// fp32, then divided by their count -- the result depends on nothing but the data.  normalize: the row is divided by its L2 norm (the
// squares are summed per lane in column order, then over the wave by the fixed butterfly of ssv_wave_sum).  An empty partition is zeros.
__global__ __launch_bounds__(64) void segment_mean_kernel(const float* __restrict__ e, const int* __restrict__ offs, float* __restrict__ out,
                                                          int Nw, int D, int normalize) {
  const int p = blockIdx.x, lane = threadIdx.x;
  int a = offs[p], b = offs[p + 1];
  a = a < 0 ? 0 : (a > Nw ? Nw : a);
  b = b < a ? a : (b > Nw ? Nw : b);
  const float n = (float)(b > a ? b - a : 1);
  float* o = out + (long)p * D;
  float sq = 0.f;
  for (int d = lane; d < D; d += 64) {
    float acc = 0.f;
    for (int r = a; r < b; ++r) acc += e[(long)r * D + d];
    acc /= n;
    o[d] = acc;
    sq = fmaf(acc, acc, sq);
  }
  if (!normalize) return;
  sq = ssv_wave_sum(sq);
  if (!(sq > 0.f)) return;
  const float s = 1.f / sqrtf(sq);
  for (int d = lane; d < D; d += 64) o[d] *= s;             // this lane's own stores
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------
extern "C" int ssv_span_frames(const float* y, const int* tiles, float* fr, int B, int n_max, int n_tiles, int n_fft, int hop, int window,
                               int Tc, int R, int g_base, int n_frames, ssv_stream_t stream) {
  SSV_CHECK(y && tiles && fr && B > 0 && n_max > 0 && n_tiles > 0 && n_fft >= 2 && n_fft % 2 == 0 && hop > 0 && hop <= n_fft && window > 0 &&
            Tc > 0 && R > 0 && g_base >= 0 && n_frames > 0, SSV_BAD_SHAPE,
            "span_frames: bad argument B=%d n_max=%d n_tiles=%d n_fft=%d hop=%d window=%d Tc=%d R=%d g_base=%d n_frames=%d", B, n_max, n_tiles, n_fft,
            hop, window, Tc, R, g_base, n_frames);
  SSV_CHECK((long)window * hop > n_fft / 2, SSV_BAD_SHAPE,
            "span_frames: window*hop=%ld must exceed n_fft/2=%d (a framed span is reflected once per end)", (long)window * hop, n_fft / 2);
  SSV_CHECK((long)(R - 1) * Tc < (long)n_frames && (long)n_frames <= (long)R * Tc && (long)Tc * n_fft < (1L << 31) &&
            (long)R * Tc * n_fft < (1L << 40), SSV_BAD_SHAPE,
            "span_frames: n_frames=%d does not end in the last of R=%d items of Tc=%d columns", n_frames, R, Tc);
  SSV_CHECK((long)(DV_TILE - 1) * hop + n_fft <= DV_SPAN_MAX, SSV_UNSUPPORTED,
            "span_frames: a tile of %d frames at hop=%d n_fft=%d reads %ld samples (LDS tile: %d)", DV_TILE, hop, n_fft,
            (long)(DV_TILE - 1) * hop + n_fft, DV_SPAN_MAX);
  const int pad = (long)R * Tc > (long)n_frames ? 1 : 0;
  hipLaunchKernelGGL(span_frames_kernel, dim3(n_tiles + pad), dim3(DV_THREADS), 0, (hipStream_t)stream, y, tiles, fr, B, n_max, n_tiles, n_fft, hop,
                     Tc, R, g_base, n_frames);
  return ssv_check_launch("span_frames");
}

extern "C" int ssv_gather_windows(const float* mel, const int* g0, float* out, int G, int Nw, int window, int nmels, ssv_stream_t stream) {
  SSV_CHECK(mel && g0 && out && mel != out && G > 0 && Nw > 0 && window > 0 && nmels > 0, SSV_BAD_SHAPE,
            "gather_windows: bad argument G=%d Nw=%d window=%d nmels=%d", G, Nw, window, nmels);
  const bool vec = nmels % 4 == 0 && ((uintptr_t)mel | (uintptr_t)out) % 16 == 0;
  const int per = vec ? window * (nmels / 4) : window * nmels;
  const long total = (long)Nw * per;
  SSV_CHECK(total < (1L << 38), SSV_BAD_SHAPE, "gather_windows: %d windows of %d x %d are too many for one launch", Nw, window, nmels);
  const dim3 grid((unsigned)((total + DV_THREADS - 1) / DV_THREADS));
  if (vec) hipLaunchKernelGGL(gather_windows_kernel<4>, grid, dim3(DV_THREADS), 0, (hipStream_t)stream, mel, g0, out, G, total, per, window, nmels);
  else hipLaunchKernelGGL(gather_windows_kernel<1>, grid, dim3(DV_THREADS), 0, (hipStream_t)stream, mel, g0, out, G, total, per, window, nmels);
  return ssv_check_launch("gather_windows");
}

extern "C" int ssv_segment_mean(const float* e, const int* offs, float* out, int Nw, int P, int D, int normalize, ssv_stream_t stream) {
  SSV_CHECK(e && offs && out && e != out && Nw > 0 && P > 0 && D > 0, SSV_BAD_SHAPE, "segment_mean: bad argument Nw=%d P=%d D=%d", Nw, P, D);
  hipLaunchKernelGGL(segment_mean_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, e, offs, out, Nw, D, normalize);
  return ssv_check_launch("segment_mean");
}
