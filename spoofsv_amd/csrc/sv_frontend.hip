// Speaker-verification front end (GE2E/data_preprocess.py:15-93), gfx950: waveform -> resampled -> trimmed -> the first and last
// tisv_frame STFT frames -> power -> mel -> log10, for ragged batches whose live lengths stay on the device.  The DFT itself is the
// 1x1 convolution of api.hip (ssv_conv1d_fwd) with a windowed Fourier basis; everything here is gather / reduce work around it.
//
// Waveforms are (B, n_max) float32 rows with a DEVICE int length each; nothing below reads a length on the host, every shape is
// static, so the whole chain replays from a captured graph.  All sums run in a fixed order (no atomics).
#include "ssv_common.h"
#include "frame_stage.h"

#define SVF_THREADS 256
#define SVF_SPAN_MAX 8192         // floats of one workgroup's staged input span (resampler)
#define SVF_TRIM_FRAMES_MAX 8192  // frames of one row (trim)

__device__ __forceinline__ float svf_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ---- resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') as librosa.load calls it (data_preprocess.py:45) ------------------
// Output sample t sits at input time t * down / up: n = floor, phase p = (t * down) mod up.  bank[p][j] is the weight of
// x[n - left + j] (resampy's table interpolation and its min(1, ratio) stretch folded in on the host, float64 -> float32); x is zero
// outside [0, n_in).  A workgroup stages the span its 256 outputs read in LDS; one fp32 dot product per output, j ascending.
// resampy computes int(n * ratio) samples, librosa.resample's fix_length pads to ceil(n * ratio): both in double, as they do.
__global__ __launch_bounds__(SVF_THREADS) void resample_sinc_kernel(const float* __restrict__ x, const int* __restrict__ n_in,
                                                                    const float* __restrict__ bank, float* __restrict__ y,
                                                                    int* __restrict__ n_out, int n_max, int m_max, int up, int down,
                                                                    int taps, int left, double ratio) {
  __shared__ float span[SVF_SPAN_MAX];
  const int b = blockIdx.y;
  int n = n_in[b];
  n = n < 0 ? 0 : (n > n_max ? n_max : n);
  const double pos = (double)n * ratio;
  int n_res = (int)pos, n_fix = (int)ceil(pos);
  if (n_fix > m_max) n_fix = m_max;
  if (n_res > n_fix) n_res = n_fix;
  const long t0 = (long)blockIdx.x * SVF_THREADS;
  if (blockIdx.x == 0 && threadIdx.x == 0) n_out[b] = n_fix;
  float* yb = y + (long)b * m_max;
  const long t = t0 + threadIdx.x;
  if (t0 >= n_res) {                                   // nothing live in this tile: zeros (block-uniform branch)
    if (t < m_max) yb[t] = 0.f;
    return;
  }
  const float* xb = x + (long)b * n_max;
  if (taps == 0) {                                     // equal rates: librosa.resample returns its input
    if (t < m_max) yb[t] = t < n ? xb[t] : 0.f;
    return;
  }
  long t_last = t0 + SVF_THREADS - 1;
  if (t_last > n_res - 1) t_last = n_res - 1;
  const long lo = t0 * down / up - left;
  const int len = (int)(t_last * down / up - left + taps - lo);       // <= SVF_SPAN_MAX, checked on the host
  for (int i = threadIdx.x; i < len; i += SVF_THREADS) {
    const long j = lo + i;
    span[i] = (j >= 0 && j < n) ? xb[j] : 0.f;
  }
  __syncthreads();
  if (t >= m_max) return;
  float acc = 0.f;
  if (t < n_res) {
    const long q = t * down;
    const int p = (int)(q % up);
    const float* s = span + (q / up - left - lo);
    const float* w = bank + (long)p * taps;
    for (int j = 0; j < taps; ++j) acc = fmaf(w[j], s[j], acc);
  }
  yb[t] = acc;
}

// ---- librosa.effects.trim(y, top_db) of librosa 0.7.0 (data_preprocess.py:46; host form: vocoder.trim_silence) -----------------------
// One workgroup per row.  Frame f covers padded samples [f * hop, f * hop + FL) of the row reflect-padded by FL / 2 (zero-padded when
// the row is no longer than FL / 2); a wave sums one frame's squares in fp32 (lane partial sums in sample order, then the wave tree).
// dB against the loudest frame and the threshold compare run in double on the <= n / hop + 1 frame energies.

// The energy stage of trim and split, one arithmetic for both: mse[f] for f < nf = 1 + n / hop (<= SVF_TRIM_FRAMES_MAX, checked on the
// host against n_max) and, returned, the dB of the loudest frame.  redf: SVF_THREADS floats; ends on a barrier.
__device__ __forceinline__ double svf_frame_energies(const float* __restrict__ yb, int n, int nf, int FL, int hop, float* mse, float* redf) {
  const int pad = FL / 2;
  const bool reflect = n > pad;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int f = wave; f < nf; f += SVF_THREADS / 64) {
    float acc = 0.f;
    for (int c = lane; c < FL; c += 64) {
      const int j = f * hop + c - pad;
      float v = 0.f;
      if (reflect) v = yb[ssv_reflect(j, n)];
      else if (j >= 0 && j < n) v = yb[j];
      acc = fmaf(v, v, acc);
    }
    acc = svf_wave_sum(acc);
    if (lane == 0) mse[f] = acc / (float)FL;
  }
  __syncthreads();
  float m = 0.f;
  for (int f = threadIdx.x; f < nf; f += SVF_THREADS) m = fmaxf(m, mse[f]);
  redf[threadIdx.x] = m;
  __syncthreads();
  for (int s = SVF_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) redf[threadIdx.x] = fmaxf(redf[threadIdx.x], redf[threadIdx.x + s]);
    __syncthreads();
  }
  return 10.0 * log10(fmax(1e-10, (double)redf[0]));
}

// power_to_db of one frame against the loudest (1e-10 floor, as librosa has it)
__device__ __forceinline__ double svf_frame_db(float e, double ref) { return 10.0 * log10(fmax(1e-10, (double)e)) - ref; }

__global__ __launch_bounds__(SVF_THREADS) void trim_bounds_kernel(const float* __restrict__ y, const int* __restrict__ n_in,
                                                                  int* __restrict__ bounds, int n_max, double top_db, int FL, int hop) {
  __shared__ float mse[SVF_TRIM_FRAMES_MAX];
  __shared__ float redf[SVF_THREADS];
  __shared__ int redlo[SVF_THREADS], redhi[SVF_THREADS];
  const int b = blockIdx.x;
  int n = n_in[b];
  n = n < 0 ? 0 : (n > n_max ? n_max : n);
  const int nf = 1 + n / hop;
  const double ref = svf_frame_energies(y + (long)b * n_max, n, nf, FL, hop, mse, redf);
  int lo = nf, hi = -1;
  for (int f = threadIdx.x; f < nf; f += SVF_THREADS) {
    if (svf_frame_db(mse[f], ref) > -top_db) { lo = min(lo, f); hi = max(hi, f); }
  }
  redlo[threadIdx.x] = lo;
  redhi[threadIdx.x] = hi;
  __syncthreads();
  for (int s = SVF_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      redlo[threadIdx.x] = min(redlo[threadIdx.x], redlo[threadIdx.x + s]);
      redhi[threadIdx.x] = max(redhi[threadIdx.x], redhi[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int start = 0, end = 0;
    if (redhi[0] >= 0) {
      start = redlo[0] * hop;
      const long e = (long)(redhi[0] + 1) * hop;
      end = e < n ? (int)e : n;
      if (start > end) start = end;
    }
    bounds[2 * b] = start;
    bounds[2 * b + 1] = end;
  }
}

// ---- librosa.effects.split(y, top_db) of librosa 0.7.0 (synthetic_data_preprocess.py:35; host form: vocoder.split_silence) -------------
// Number of set flags in the threads below this one, and in the whole workgroup (total): a ballot per wave, the waves' counts through
// wsum (SVF_THREADS / 64 ints of LDS).  Every thread of the workgroup calls it; two barriers, the first keeps a previous call's wsum.
__device__ __forceinline__ int svf_block_rank(bool flag, int* wsum, int& total) {
  const unsigned long long m = __ballot(flag);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int below = __popcll(m & ((1ull << lane) - 1ull));
  total = 0;
  for (int w = 0; w < SVF_THREADS / 64; ++w) {
    const int c = wsum[w];
    if (w < wave) below += c;
    total += c;
  }
  return below;
}

// One workgroup per row, the energy stage of trim.  Every maximal run [f0, f1) of frames above -top_db is one interval
// (f0 * hop, min(n, f1 * hop)); the rank of a run is the number of runs that begin before it: a workgroup prefix count over the "a run
// begins here" flags, SVF_THREADS frames at a time, the count carried from chunk to chunk.  The thread of a run's first frame writes
// its start, the thread of its last frame its end.  intervals (B, K, 2): runs past K are counted, not stored; entries from
// min(count, K) on are (0, 0).  An empty row has no run.
__global__ __launch_bounds__(SVF_THREADS) void split_intervals_kernel(const float* __restrict__ y, const int* __restrict__ n_in,
                                                                      int* __restrict__ intervals, int* __restrict__ count, int n_max, int K,
                                                                      double top_db, int FL, int hop) {
  __shared__ float mse[SVF_TRIM_FRAMES_MAX];               // energies, then flags (1.f: above the threshold)
  __shared__ float redf[SVF_THREADS];
  __shared__ int wsum[SVF_THREADS / 64];
  const int b = blockIdx.x;
  int n = n_in[b];
  n = n < 0 ? 0 : (n > n_max ? n_max : n);
  int* iv = intervals + (long)b * K * 2;
  int runs = 0;
  if (n > 0) {                                             // (block-uniform)
    const int nf = 1 + n / hop;
    const double ref = svf_frame_energies(y + (long)b * n_max, n, nf, FL, hop, mse, redf);
    for (int f = threadIdx.x; f < nf; f += SVF_THREADS) mse[f] = svf_frame_db(mse[f], ref) > -top_db ? 1.f : 0.f;   // each thread its own frames
    __syncthreads();
    for (int base = 0; base < nf; base += SVF_THREADS) {
      const int f = base + threadIdx.x;
      const bool live = f < nf && mse[f] != 0.f;
      const bool first = live && (f == 0 || mse[f - 1] == 0.f);
      const bool last = live && (f == nf - 1 || mse[f + 1] == 0.f);
      int begun;
      const int before = runs + svf_block_rank(first, wsum, begun);        // runs that begin before frame f
      const int r = first ? before : before - 1;                             // the run frame f lies in, if it lies in one
      if (first && r < K) iv[2 * r] = f * hop;
      if (last && r < K) {
        const long e = (long)(f + 1) * hop;
        iv[2 * r + 1] = e < n ? (int)e : n;
      }
      runs += begun;
    }
  }
  for (int k = min(runs, K) + threadIdx.x; k < K; k += SVF_THREADS) iv[2 * k] = iv[2 * k + 1] = 0;
  if (threadIdx.x == 0) count[b] = runs;
}

// ---- `for interval in intervals: if (interval[1] - interval[0]) > utter_min_len` (synthetic_data_preprocess.py:36-37) across rows --------
// One workgroup walks the (B, K) spans in (row, interval) order, SVF_THREADS at a time; span k of row b passes when k < min(count[b], K),
// it fits its row (ssv_clamp_span leaves it as it is) and end - start > min_len.  Its global index g is the prefix count of the passes;
// table[g - first] = (row, start, end) for first <= g < first + R, the rows after the last one (-1, 0, 0); total[0] = all passes.
__global__ __launch_bounds__(SVF_THREADS) void select_spans_kernel(const int* __restrict__ intervals, const int* __restrict__ count,
                                                                   int* __restrict__ table, int* __restrict__ total, int B, int K, int n_max,
                                                                   int min_len, int first, int R) {
  __shared__ int wsum[SVF_THREADS / 64];
  const long n_spans = (long)B * K;                        // < 2^31, checked on the host
  int passed = 0;
  for (long base = 0; base < n_spans; base += SVF_THREADS) {
    const long i = base + threadIdx.x;
    bool pass = false;
    int b = 0, start = 0, end = 0;
    if (i < n_spans) {
      b = (int)(i / K);
      start = intervals[2 * i];
      end = intervals[2 * i + 1];
      int s = start, e = end;
      ssv_clamp_span(s, e, n_max);
      pass = (int)(i % K) < min(count[b], K) && s == start && e == end && end - start > min_len;
    }
    int here;
    const long g = (long)passed + svf_block_rank(pass, wsum, here) - first;
    if (pass && g >= 0 && g < R) {
      table[3 * g] = b;
      table[3 * g + 1] = start;
      table[3 * g + 2] = end;
    }
    passed += here;
  }
  const long used = (long)passed - first;
  for (long r = (used < 0 ? 0 : used) + threadIdx.x; r < R; r += SVF_THREADS) {
    table[3 * r] = -1;
    table[3 * r + 1] = table[3 * r + 2] = 0;
  }
  if (threadIdx.x == 0) total[0] = passed;
}

// ---- the framing of librosa.stft(utter, n_fft, hop, win_length) restricted to S[:, :T] and S[:, -T:] (data_preprocess.py:48-60) ----------
// fr[2b + s][c][t] = reflect_pad(seg, N / 2)[(f0 + t) * hop + c], seg = y[b][start:end], f0 = 0 (s = 0) or 1 + len / hop - T (s = 1);
// valid[b] = len > min_len (strict, :48), frames of an invalid row are zeros.
__global__ __launch_bounds__(128) void tisv_frames_kernel(const float* __restrict__ y, const int* __restrict__ bounds,
                                                          float* __restrict__ fr, int* __restrict__ valid, int n_max, int N, int hop,
                                                          int T, int min_len) {
  const int t = blockIdx.x * 128 + threadIdx.x, c = blockIdx.y, b = blockIdx.z >> 1, s = blockIdx.z & 1;
  int start = bounds[2 * b], end = bounds[2 * b + 1];
  ssv_clamp_span(start, end, n_max);
  const int len = end - start;
  const bool ok = len > min_len;                        // min_len >= max(N / 2, T * hop): reflect padding and T frames exist
  if (blockIdx.x == 0 && c == 0 && s == 0 && threadIdx.x == 0) valid[b] = ok ? 1 : 0;
  if (t >= T) return;
  float v = 0.f;
  if (ok) {
    const int f0 = s ? 1 + len / hop - T : 0;
    v = y[(long)b * n_max + start + ssv_reflect((f0 + t) * hop + c - N / 2, len)];
  }
  fr[((long)blockIdx.z * N + c) * T + t] = v;
}

// ---- the same two slices for the spans of a table (synthetic_data_preprocess.py:38-45), through the staged core of frame_stage.h -----
// table (R, 3) int: (row, start, end) as select_spans_kernel writes it.  fr[2r + s][c][t] as above with seg = y[row][start:end].  A
// workgroup takes one tile of at most SVF_TILE frames of one slice: it stages the samples the tile reads once in LDS and every wave
// writes whole sample rows as runs of the tile's frames.  A row of -1, one that does not fit the batch or one with
// end - start <= min_len gets zero frames and valid = 0, and is never followed.
#define SVF_TILE 64                // frames of a tile: one 256-byte run per sample row and wave store
#define SVF_TILE_SPAN_MAX 12288    // floats of a tile's staged sample range, (SVF_TILE - 1) * hop + n_fft; 10,592 at hop 160, n_fft 512
#define SVF_SKEW_SHIFT 5           // ssv_skew's shift: conflict-free at hop = 160 = 5 * 32
__global__ __launch_bounds__(SVF_THREADS) void tisv_frames_table_kernel(const float* __restrict__ y, const int* __restrict__ table,
                                                                        float* __restrict__ fr, int* __restrict__ valid, int B, int n_max,
                                                                        int n_tiles, int N, int hop, int T, int min_len) {
  __shared__ float sm[SVF_TILE_SPAN_MAX + SVF_TILE_SPAN_MAX / 32 + 1];
  const int item = blockIdx.x / n_tiles, t0 = (blockIdx.x % n_tiles) * SVF_TILE, r = item >> 1, s = item & 1;
  const int row = table[3 * r], start = table[3 * r + 1], end = table[3 * r + 2];
  const int len = end - start;
  const int cnt = min(SVF_TILE, T - t0);
  // min_len >= max(N / 2, T * hop), checked on the host: reflect padding and T frames exist (block-uniform)
  const bool ok = row >= 0 && row < B && start >= 0 && end <= n_max && len > min_len;
  if (t0 == 0 && s == 0 && threadIdx.x == 0) valid[r] = ok ? 1 : 0;
  float* dst = fr + (long)item * N * T + t0;
  if (!ok) {
    for (int e = threadIdx.x; e < N * cnt; e += SVF_THREADS) dst[(long)(e / cnt) * T + e % cnt] = 0.f;
    return;
  }
  const int f0 = (s ? 1 + len / hop - T : 0) + t0;
  frame_stage_load<false, SVF_THREADS>(sm, y + (long)row * n_max + start, len, f0 * hop - N / 2, (cnt - 1) * hop + N, SVF_SKEW_SHIFT, 0.f);   // count <= SVF_TILE_SPAN_MAX, checked on the host
  __syncthreads();
  const int wave = threadIdx.x >> 6, t = threadIdx.x & 63;
  if (t >= cnt) return;
  frame_stage_store(sm, dst + t, T, t * hop, wave, SVF_THREADS / 64, N, SVF_SKEW_SHIFT);
}

// ---- np.abs(S) ** 2, np.dot(mel_basis, S), np.log10(. + 1e-6)  (data_preprocess.py:50-52), frames-major output ------------------------------
// A workgroup takes SVF_TT frames of one row: the F powers of each in LDS, then out[t][m] = log10(sum_f mel[m][f] * pw[f][t] + eps),
// plain fp32 FMA, f ascending.
#define SVF_TT 16
__global__ __launch_bounds__(SVF_THREADS) void power_mel_log_kernel(const float* __restrict__ spec, const float* __restrict__ mel,
                                                                    float* __restrict__ out, int F, int T, int nmels, float eps) {
  extern __shared__ float pw[];                          // (F, SVF_TT)
  const int r = blockIdx.y, t0 = blockIdx.x * SVF_TT;
  const float* sp = spec + (long)r * 2 * F * T;
  for (int i = threadIdx.x; i < F * SVF_TT; i += SVF_THREADS) {
    const int f = i / SVF_TT, t = t0 + i % SVF_TT;
    float p = 0.f;
    if (t < T) {
      const float re = sp[(long)f * T + t], im = sp[(long)(F + f) * T + t];
      p = fmaf(im, im, re * re);
    }
    pw[i] = p;
  }
  __syncthreads();
  const int tt = min(SVF_TT, T - t0);
  for (int i = threadIdx.x; i < tt * nmels; i += SVF_THREADS) {
    const int tl = i / nmels, m = i % nmels;
    const float* w = mel + (long)m * F;
    float acc = 0.f;
    for (int f = 0; f < F; ++f) acc = fmaf(w[f], pw[f * SVF_TT + tl], acc);
    out[((long)r * T + t0) * nmels + i] = log10f(acc + eps);
  }
}

// ---- generate_test_utterances.py:135-139 after the trim: clip, peak by the row's maximum (not its absolute maximum) ------------------
// out[b][i] = y[b][start + i] / max(seg) * peak for i < len = min(end - start, clip), zeros after; n_out[b] = len.
__global__ __launch_bounds__(SVF_THREADS) void segment_peak_kernel(const float* __restrict__ y, const int* __restrict__ bounds,
                                                                   float* __restrict__ out, int* __restrict__ n_out, int n_max, int clip,
                                                                   float peak) {
  __shared__ float red[SVF_THREADS];
  const int b = blockIdx.x;
  int start = bounds[2 * b], end = bounds[2 * b + 1];
  ssv_clamp_span(start, end, n_max);
  const int len = min(end - start, clip);
  const float* yb = y + (long)b * n_max + start;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < len; i += SVF_THREADS) m = fmaxf(m, yb[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = SVF_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  m = red[0];
  float* ob = out + (long)b * clip;
  for (int i = threadIdx.x; i < clip; i += SVF_THREADS) ob[i] = i < len ? yb[i] / m * peak : 0.f;
  if (threadIdx.x == 0) n_out[b] = len;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------
extern "C" int ssv_resample_sinc(const float* x, const int* n_in, const float* bank, float* y, int* n_out, int B, int n_max, int m_max,
                                 int up, int down, int taps, int left, ssv_stream_t stream) {
  SSV_CHECK(x && n_in && y && n_out && x != y && B > 0 && B <= 65535 && n_max > 0 && m_max > 0 && up > 0 && down > 0 && taps >= 0 && left >= 0 &&
            left <= taps, SSV_BAD_SHAPE, "resample_sinc: bad argument B=%d n_max=%d m_max=%d up=%d down=%d taps=%d left=%d", B, n_max, m_max, up, down, taps, left);
  SSV_CHECK(up == down || (bank && taps > 0), SSV_BAD_SHAPE, "resample_sinc: rates differ (up=%d down=%d) but no filter bank was given", up, down);
  const int t = up == down ? 0 : taps;
  SSV_CHECK((long)up * t <= (1L << 20) && (long)(SVF_THREADS - 1) * down / up + t + 2 <= SVF_SPAN_MAX, SSV_UNSUPPORTED,
            "resample_sinc: the ratio %d/%d needs a filter bank of %d x %d taps or an input span of %ld samples per workgroup (limits: 2^20 taps, %d samples)",
            up, down, up, t, (long)(SVF_THREADS - 1) * down / up + t + 2, SVF_SPAN_MAX);
  SSV_CHECK((long)ceil((double)n_max * ((double)up / (double)down)) <= (long)m_max && (long)m_max * down < (1L << 40), SSV_BAD_SHAPE,
            "resample_sinc: m_max=%d is smaller than ceil(n_max * up / down) (n_max=%d up=%d down=%d)", m_max, n_max, up, down);
  hipLaunchKernelGGL(resample_sinc_kernel, dim3(ssv_cdiv(m_max, SVF_THREADS), B), dim3(SVF_THREADS), 0, (hipStream_t)stream, x, n_in, bank, y, n_out,
                     n_max, m_max, up, down, t, left, (double)up / (double)down);
  return ssv_check_launch("resample_sinc");
}

extern "C" int ssv_trim_bounds(const float* y, const int* n_in, int* bounds, int B, int n_max, float top_db, int frame_length, int hop,
                               ssv_stream_t stream) {
  SSV_CHECK(y && n_in && bounds && B > 0 && n_max > 0 && frame_length >= 2 && frame_length % 2 == 0 && hop > 0 && hop <= frame_length && top_db > 0.f,
            SSV_BAD_SHAPE, "trim_bounds: bad argument B=%d n_max=%d frame_length=%d hop=%d top_db=%g", B, n_max, frame_length, hop, (double)top_db);
  SSV_CHECK(1 + n_max / hop <= SVF_TRIM_FRAMES_MAX, SSV_UNSUPPORTED, "trim_bounds: n_max=%d gives %d frames per row (limit %d)", n_max, 1 + n_max / hop,
            SVF_TRIM_FRAMES_MAX);
  hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(SVF_THREADS), 0, (hipStream_t)stream, y, n_in, bounds, n_max, (double)top_db, frame_length, hop);
  return ssv_check_launch("trim_bounds");
}

extern "C" int ssv_tisv_frames(const float* y, const int* bounds, float* fr, int* valid, int B, int n_max, int n_fft, int hop, int tisv_frame,
                               int min_len, ssv_stream_t stream) {
  SSV_CHECK(y && bounds && fr && valid && B > 0 && 2 * B <= 65535 && n_max > 0 && n_fft >= 2 && n_fft <= 65535 && n_fft % 2 == 0 && hop > 0 &&
            hop <= n_fft && tisv_frame > 0, SSV_BAD_SHAPE, "tisv_frames: bad argument B=%d n_max=%d n_fft=%d hop=%d tisv_frame=%d", B, n_max, n_fft, hop, tisv_frame);
  SSV_CHECK(min_len >= n_fft / 2 && (long)min_len >= (long)tisv_frame * hop, SSV_BAD_SHAPE,
            "tisv_frames: min_len=%d must be at least n_fft/2 and tisv_frame*hop (n_fft=%d hop=%d tisv_frame=%d)", min_len, n_fft, hop, tisv_frame);
  hipLaunchKernelGGL(tisv_frames_kernel, dim3(ssv_cdiv(tisv_frame, 128), n_fft, 2 * B), dim3(128), 0, (hipStream_t)stream, y, bounds, fr, valid, n_max,
                     n_fft, hop, tisv_frame, min_len);
  return ssv_check_launch("tisv_frames");
}

extern "C" int ssv_split_intervals(const float* y, const int* n_in, int* intervals, int* count, int B, int n_max, int K, float top_db,
                                   int frame_length, int hop, ssv_stream_t stream) {
  SSV_CHECK(y && n_in && intervals && count && B > 0 && n_max > 0 && K > 0 && frame_length >= 2 && frame_length % 2 == 0 && hop > 0 &&
            hop <= frame_length && top_db > 0.f, SSV_BAD_SHAPE, "split_intervals: bad argument B=%d n_max=%d K=%d frame_length=%d hop=%d top_db=%g", B, n_max,
            K, frame_length, hop, (double)top_db);
  SSV_CHECK(1 + n_max / hop <= SVF_TRIM_FRAMES_MAX, SSV_UNSUPPORTED, "split_intervals: n_max=%d gives %d frames per row (limit %d)", n_max, 1 + n_max / hop,
            SVF_TRIM_FRAMES_MAX);
  hipLaunchKernelGGL(split_intervals_kernel, dim3(B), dim3(SVF_THREADS), 0, (hipStream_t)stream, y, n_in, intervals, count, n_max, K, (double)top_db,
                     frame_length, hop);
  return ssv_check_launch("split_intervals");
}

extern "C" int ssv_select_spans(const int* intervals, const int* count, int* table, int* total, int B, int K, int n_max, int min_len, int first, int R,
                                ssv_stream_t stream) {
  SSV_CHECK(intervals && count && table && total && B > 0 && K > 0 && n_max > 0 && min_len >= 0 && first >= 0 && R > 0, SSV_BAD_SHAPE,
            "select_spans: bad argument B=%d K=%d n_max=%d min_len=%d first=%d R=%d", B, K, n_max, min_len, first, R);
  SSV_CHECK((long)B * K < (1L << 30) && R < (1 << 29), SSV_UNSUPPORTED, "select_spans: B=%d rows of K=%d spans or R=%d table rows exceed the int index range", B, K, R);
  hipLaunchKernelGGL(select_spans_kernel, dim3(1), dim3(SVF_THREADS), 0, (hipStream_t)stream, intervals, count, table, total, B, K, n_max, min_len, first, R);
  return ssv_check_launch("select_spans");
}

extern "C" int ssv_tisv_frames_table(const float* y, const int* table, float* fr, int* valid, int B, int n_max, int R, int n_fft, int hop, int tisv_frame,
                                     int min_len, ssv_stream_t stream) {
  SSV_CHECK(y && table && fr && valid && B > 0 && n_max > 0 && R > 0 && n_fft >= 2 && n_fft % 2 == 0 && hop > 0 && hop <= n_fft && tisv_frame > 0,
            SSV_BAD_SHAPE, "tisv_frames_table: bad argument B=%d n_max=%d R=%d n_fft=%d hop=%d tisv_frame=%d", B, n_max, R, n_fft, hop, tisv_frame);
  SSV_CHECK(min_len >= n_fft / 2 && (long)min_len >= (long)tisv_frame * hop, SSV_BAD_SHAPE,
            "tisv_frames_table: min_len=%d must be at least n_fft/2 and tisv_frame*hop (n_fft=%d hop=%d tisv_frame=%d)", min_len, n_fft, hop, tisv_frame);
  SSV_CHECK((long)(SVF_TILE - 1) * hop + n_fft <= SVF_TILE_SPAN_MAX, SSV_UNSUPPORTED,
            "tisv_frames_table: a tile of %d frames at hop=%d n_fft=%d reads %ld samples (LDS tile: %d)", SVF_TILE, hop, n_fft,
            (long)(SVF_TILE - 1) * hop + n_fft, SVF_TILE_SPAN_MAX);
  const int n_tiles = ssv_cdiv(tisv_frame, SVF_TILE);
  SSV_CHECK(2L * R * n_tiles < (1L << 31), SSV_UNSUPPORTED, "tisv_frames_table: R=%d table rows of %d tiles exceed the grid", R, n_tiles);
  hipLaunchKernelGGL(tisv_frames_table_kernel, dim3((unsigned)(2L * R * n_tiles)), dim3(SVF_THREADS), 0, (hipStream_t)stream, y, table, fr, valid, B, n_max,
                     n_tiles, n_fft, hop, tisv_frame, min_len);
  return ssv_check_launch("tisv_frames_table");
}

extern "C" int ssv_power_mel_log(const float* spec, const float* mel, float* out, int R, int F, int T, int nmels, float eps, ssv_stream_t stream) {
  SSV_CHECK(spec && mel && out && R > 0 && R <= 65535 && F > 0 && T > 0 && nmels > 0 && eps >= 0.f, SSV_BAD_SHAPE,
            "power_mel_log: bad argument R=%d F=%d T=%d nmels=%d", R, F, T, nmels);
  SSV_CHECK(F <= 1024, SSV_UNSUPPORTED, "power_mel_log: F=%d frequency bins do not fit the workgroup's LDS tile (limit 1024)", F);
  hipLaunchKernelGGL(power_mel_log_kernel, dim3(ssv_cdiv(T, SVF_TT), R), dim3(SVF_THREADS), (size_t)F * SVF_TT * sizeof(float), (hipStream_t)stream,
                     spec, mel, out, F, T, nmels, eps);
  return ssv_check_launch("power_mel_log");
}

extern "C" int ssv_segment_peak(const float* y, const int* bounds, float* out, int* n_out, int B, int n_max, int clip, float peak, ssv_stream_t stream) {
  SSV_CHECK(y && bounds && out && n_out && y != out && B > 0 && n_max > 0 && clip > 0, SSV_BAD_SHAPE, "segment_peak: bad argument B=%d n_max=%d clip=%d",
            B, n_max, clip);
  hipLaunchKernelGGL(segment_peak_kernel, dim3(B), dim3(SVF_THREADS), 0, (hipStream_t)stream, y, bounds, out, n_out, n_max, clip, peak);
  return ssv_check_launch("segment_peak");
}
