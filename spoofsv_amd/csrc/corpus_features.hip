// Corpus spectrogram extraction for ragged batches (data/dataset.py:94-118), gfx950: the trimmed segment of every row -> pre-emphasis ->
// centred STFT frames, and after the DFT / magnitude / mel product (ssv_conv1d_fwd with k = 1, ssv_complex_abs, as in vocoder.hip) the
// normalisation, the time reduction and the zero padding of the collated batch in one pass.  Waveforms are (B, n_max) float32 rows with
// DEVICE (start, end) bounds each (ssv_trim_bounds); nothing below reads a length on the host and every shape is static.
#include "ssv_common.h"
#include "frame_stage.h"

#define CF_THREADS 256
#define CF_LDS_FLOATS 12800        // 51,200 bytes: three workgroups per CU

// ---- librosa.effects.trim's segment, np.append(x[0], x[1:] - a * x[:-1]) and librosa.stft's framing (data/dataset.py:95-97) ----------
// fr[b][i][t] = reflect_pad(p, N / 2)[t * hop + i] for t < T_b = 1 + len / hop, p the pre-emphasised seg = y[b][start:end] (p[0] =
// seg[0]: the sample before `start` is not read), zeros for t >= T_b; a segment of len <= N / 2 has nothing to reflect from and gets
// T_b = 0.  A workgroup owns `tile` frames of one row: it stages the pre-emphasised samples they read once in LDS, skewed by sh = ctz(hop),
// and writes each of the N sample rows as one run of `tile` floats (frame_stage.h).
__global__ __launch_bounds__(CF_THREADS) void preemph_frames_ragged_kernel(const float* __restrict__ y, const int* __restrict__ bounds,
                                                                           float* __restrict__ fr, int* __restrict__ n_frames, int n_max, int N,
                                                                           int hop, int T_max, int tile, int tshift, int sh, float a) {
  __shared__ float sm[CF_LDS_FLOATS];
  const int b = blockIdx.y, t0 = blockIdx.x * tile;
  int start = bounds[2 * b], end = bounds[2 * b + 1];
  ssv_clamp_span(start, end, n_max);
  const int len = end - start;
  int Tb = len > N / 2 ? 1 + len / hop : 0;
  if (Tb > T_max) Tb = T_max;                             // T_max >= 1 + n_max / hop (checked on the host): never taken
  if (blockIdx.x == 0 && threadIdx.x == 0) n_frames[b] = Tb;
  int cnt = Tb - t0;                                      // live frames of this tile (block-uniform)
  cnt = cnt < 0 ? 0 : (cnt > tile ? tile : cnt);
  if (cnt > 0) {
    // ssv_skew(count - 1, sh) < CF_LDS_FLOATS, checked on the host
    frame_stage_load<true, CF_THREADS>(sm, y + (long)b * n_max + start, len, t0 * hop - N / 2, (cnt - 1) * hop + N, sh, a);
    __syncthreads();
  }
  const int t = threadIdx.x & (tile - 1), col = t0 + t;
  if (col >= T_max) return;
  float* dst = fr + (long)b * N * T_max + col;
  const int rows = CF_THREADS >> tshift;
  if (t < cnt) frame_stage_store(sm, dst, T_max, t * hop, threadIdx.x >> tshift, rows, N, sh);
  else for (int i = threadIdx.x >> tshift; i < N; i += rows) dst[(long)i * T_max] = 0.f;
}

// ---- normalisation, time reduction and collate padding (data/dataset.py:101-118, :215-224) ------------------------------------------
// Row blockIdx.y of item b: a linear row (< F) keeps its first r * rt_b columns, a mel row columns 0, r, 2r, ... (rt_b of them),
// rt_b = T_b / r; everything after is zero, as collate_pad_* pads.  Default: (x / max_b)^p with the row's own maximum (ssv_rowmax over the
// padded view: pad frames are zero and magnitudes non-negative); a maximum of 0 gives zeros.  LOG_FEATURE: the clip of ssv_log_norm.
__global__ __launch_bounds__(CF_THREADS) void corpus_normalize_pack_kernel(const float* __restrict__ lin, const float* __restrict__ mel,
                                                                           const float* __restrict__ max_lin, const float* __restrict__ max_mel,
                                                                           const int* __restrict__ n_frames, float* __restrict__ mel_out,
                                                                           float* __restrict__ lin_out, int* __restrict__ rt_out, int F, int M,
                                                                           int T_max, int RT_max, int r, int log_feature, float p, float ref_db,
                                                                           float max_db) {
  const int b = blockIdx.z, row = blockIdx.y, c = blockIdx.x * CF_THREADS + threadIdx.x;
  int Tb = n_frames[b];
  Tb = Tb < 0 ? 0 : (Tb > T_max ? T_max : Tb);
  int rt = Tb / r;
  if (rt > RT_max) rt = RT_max;
  if (blockIdx.x == 0 && row == 0 && threadIdx.x == 0) rt_out[b] = rt;
  const bool is_lin = row < F;
  const int W = is_lin ? r * RT_max : RT_max;
  if (c >= W) return;
  float v = 0.f;
  if (c < (is_lin ? r * rt : rt)) {                       // source column c (linear) or c * r (mel) < r * rt <= T_b <= T_max
    const float x = is_lin ? lin[((long)b * F + row) * T_max + c] : mel[((long)b * M + (row - F)) * T_max + (long)c * r];
    if (log_feature) {
      v = fminf(fmaxf((20.f * log10f(fmaxf(1e-5f, x)) - ref_db + max_db) / max_db, 1e-8f), 1.f);
    } else {
      const float mx = is_lin ? max_lin[b] : max_mel[b];
      if (mx > 0.f) {
        v = fmaxf(x, 0.f) / mx;
        if (p != 1.f) v = powf(v, p);
      }
    }
  }
  if (is_lin) lin_out[((long)b * F + row) * W + c] = v;
  else mel_out[((long)b * M + (row - F)) * W + c] = v;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------
// the widest tile of frames (64, 32 or 16) whose staged range fits the LDS image; 0 when none does
static int cf_tile(int n_fft, int hop, int sh) {
  for (int tile = 64; tile >= 16; tile >>= 1) {
    const long count = (long)(tile - 1) * hop + n_fft;
    if (count + (sh < 31 ? count >> sh : 0) + 1 <= CF_LDS_FLOATS) return tile;
  }
  return 0;
}

extern "C" int ssv_preemph_frames_ragged(const float* y, const int* bounds, float* fr, int* n_frames, int B, int n_max, int n_fft, int hop,
                                         int T_max, float preemph, ssv_stream_t stream) {
  SSV_CHECK(y && bounds && fr && n_frames && y != fr && B > 0 && B <= 65535 && n_max > 0 && n_fft >= 2 && n_fft % 2 == 0 && hop > 0 &&
            hop <= n_fft && T_max > 0, SSV_BAD_SHAPE, "preemph_frames_ragged: bad argument B=%d n_max=%d n_fft=%d hop=%d T_max=%d", B, n_max,
            n_fft, hop, T_max);
  SSV_CHECK((long)T_max >= 1 + (long)n_max / hop && (long)n_fft * T_max < (1L << 31) && (long)B * n_fft * T_max < (1L << 40), SSV_BAD_SHAPE,
            "preemph_frames_ragged: T_max=%d must hold the 1 + n_max / hop = %ld frames of a full row (n_max=%d hop=%d n_fft=%d)", T_max,
            1 + (long)n_max / hop, n_max, hop, n_fft);
  const int sh = hop % 2 ? 31 : __builtin_ctz((unsigned)hop);
  const int tile = cf_tile(n_fft, hop, sh);
  SSV_CHECK(tile > 0, SSV_UNSUPPORTED, "preemph_frames_ragged: a tile of 16 frames at hop=%d n_fft=%d reads %ld samples (LDS tile: %d)", hop, n_fft,
            15L * hop + n_fft, CF_LDS_FLOATS);
  hipLaunchKernelGGL(preemph_frames_ragged_kernel, dim3(ssv_cdiv(T_max, tile), B), dim3(CF_THREADS), 0, (hipStream_t)stream, y, bounds, fr, n_frames,
                     n_max, n_fft, hop, T_max, tile, __builtin_ctz((unsigned)tile), sh, preemph);
  return ssv_check_launch("preemph_frames_ragged");
}

extern "C" int ssv_corpus_normalize_pack(const float* lin, const float* mel, const float* max_lin, const float* max_mel, const int* n_frames,
                                         float* mel_out, float* lin_out, int* rt, int B, int F, int M, int T_max, int RT_max, int r,
                                         int log_feature, float power, float ref_db, float max_db, ssv_stream_t stream) {
  SSV_CHECK(lin && mel && n_frames && mel_out && lin_out && rt && lin != lin_out && mel != mel_out && B > 0 && B <= 65535 && F > 0 && M > 0 &&
            (long)F + M <= 65535 && T_max > 0 && RT_max > 0 && r > 0, SSV_BAD_SHAPE,
            "corpus_normalize_pack: bad argument B=%d F=%d M=%d T_max=%d RT_max=%d r=%d", B, F, M, T_max, RT_max, r);
  SSV_CHECK((long)r * RT_max <= (long)T_max && (long)B * F * T_max < (1L << 40), SSV_BAD_SHAPE,
            "corpus_normalize_pack: r * RT_max = %ld columns do not fit T_max=%d", (long)r * RT_max, T_max);
  SSV_CHECK(log_feature ? max_db > 0.f : (max_lin && max_mel && power > 0.f), SSV_BAD_SHAPE,
            "corpus_normalize_pack: %s", log_feature ? "LOG_FEATURE needs max_db > 0" : "the default normalisation needs both maxima and power > 0");
  hipLaunchKernelGGL(corpus_normalize_pack_kernel, dim3(ssv_cdiv((long)r * RT_max, CF_THREADS), F + M, B), dim3(CF_THREADS), 0, (hipStream_t)stream,
                     lin, mel, max_lin, max_mel, n_frames, mel_out, lin_out, rt, F, M, T_max, RT_max, r, log_feature, power, ref_db, max_db);
  return ssv_check_launch("corpus_normalize_pack");
}
