// Index arithmetic and per-thread loops of the LDS FFT back end of the vocoder (fft.hip): the butterfly schedule, the split that turns an
// N / 2-point complex transform into an N-point real one (and back), and the span / reflect arithmetic of the fused Griffin-Lim step.
// Plain C++ as well as HIP: every function takes (tid, nth) instead of reading threadIdx, so a host program can run a workgroup's
// loops thread after thread, a barrier being the end of one call -- a wrong index is found on the CPU (tests/test_fft_vocoder_cpu.py
// compiles tests/fft_core_check.cpp with the address sanitizer), where the LDS images are heap blocks of their exact size.
//
// A real frame x[0 .. N) is packed as z[m] = x[2m] + i x[2m+1], m < M = N / 2.  Z = FFT_M(z) by radix-2 decimation in frequency, in
// place, natural order in, bit-reversed order out: bin k sits at slot bitrev(k).  With w = exp(-2 pi i k / N), E = (Z[k] + conj Z[M-k]) / 2
// and O = -i (Z[k] - conj Z[M-k]) / 2:  X[k] = E + w O and X[M-k] = conj(E - w O), Z[M] = Z[0].  The inverse builds Z from X by the same
// pair (imaginary parts of X[0] and X[M] dropped, as numpy.fft.irfft does), stores it bit-reversed and runs decimation in time, natural
// order out; its factors 1/2 and 1/M are one exact power of two applied with the synthesis window.
//
// LDS image of a tile: frame f, slot c at fr[f * (M + 1) + c] (8-byte complex).  Inside the butterfly stages a wave runs along the
// slots of one frame (consecutive 8-byte words: a 32-lane group covers one 256-byte bank row, two rows in the stages with a span below 32);
// the loops that touch the T-fastest spectra run along the FRAMES, where a stride of M would put every lane in one bank: M + 1 is odd,
// so 32 frames meet 32 different bank pairs.  (By the bank rules, not by a counter run.  The split / merge loops give each frame 4 consecutive
// bins per wave, whose bit-reversed slots differ by multiples of M / 4: those lanes DO share a bank pair.)
#pragma once
#if defined(__HIPCC__)
#define SSV_HD __host__ __device__ __forceinline__
#else
#define SSV_HD inline
#endif

#define SSV_FFT_MIN 64
#define SSV_FFT_MAX 2048
#define SSV_FFT_TILE_FLOATS 16384        // samples of all frames of a tile
#define SSV_FFT_TILE_MAX 64

struct alignas(8) ssv_cpx { float re, im; };

SSV_HD bool ssv_fft_supported(int n) { return n >= SSV_FFT_MIN && n <= SSV_FFT_MAX && (n & (n - 1)) == 0; }
// frames per workgroup: 8 (2048), 16 (1024), 32 (512), 64 below -- a power of two
SSV_HD int ssv_fft_tile(int n) { return SSV_FFT_TILE_FLOATS / n > SSV_FFT_TILE_MAX ? SSV_FFT_TILE_MAX : SSV_FFT_TILE_FLOATS / n; }
SSV_HD int ssv_fft_log2(int n) { int b = 0; while ((1 << b) < n) ++b; return b; }
SSV_HD int ssv_fft_bitrev(int v, int bits) {
  unsigned r = (unsigned)v;
  r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
  r = ((r >> 2) & 0x33333333u) | ((r & 0x33333333u) << 2);
  r = ((r >> 4) & 0x0f0f0f0fu) | ((r & 0x0f0f0f0fu) << 4);
  r = ((r >> 8) & 0x00ff00ffu) | ((r & 0x00ff00ffu) << 8);
  r = (r >> 16) | (r << 16);
  return (int)(r >> (32 - bits));
}
SSV_HD int ssv_fft_frame_stride(int M) { return M + 1; }
// table of ssv_fft_tables_host: window [0, N), cos(2 pi k / N) [N, N + N/2), sin(2 pi k / N) [N + N/2, 2N)
SSV_HD int ssv_fft_tab_floats(int N) { return 2 * N; }
// LDS image: twiddles (N / 2 complex), frames (tile * (M + 1) complex), then the staged span (floats) of the Griffin-Lim step
SSV_HD int ssv_fft_lds_cpx(int N) { return N / 2 + ssv_fft_tile(N) * ssv_fft_frame_stride(N / 2); }
// one reflection, -len < j < 2 * len - 1 (frame_stage.h, ssv_reflect)
SSV_HD int ssv_fft_reflect(int j, int len) { return j < 0 ? -j : (j >= len ? 2 * (len - 1) - j : j); }

// tw[k] = exp(-2 pi i k / N), k < N / 2
SSV_HD void ssv_fft_stage_twiddles(ssv_cpx* tw, const float* tab, int N, int tid, int nth) {
  for (int k = tid; k < N / 2; k += nth) tw[k] = ssv_cpx{tab[N + k], -tab[N + N / 2 + k]};
}

// ---- butterfly stages: h = M/2, M/4, ... 1 forward; h = 1, 2, ... M/2 inverse; a barrier after each ----------------------------------
// butterfly j < M / 2 of span h joins slots i and i + h, i = 2 (j - j % h) + j % h, with the twiddle exp(-+2 pi i (j % h) / (2 h))
SSV_HD int ssv_fft_bfly_slot(int j, int h) { const int pos = j & (h - 1); return ((j - pos) << 1) + pos; }
SSV_HD int ssv_fft_bfly_twiddle(int j, int h, int N) { return (j & (h - 1)) * (N / (2 * h)); }      // index into tw[0 .. N/2)

SSV_HD void ssv_fft_dif_stage(ssv_cpx* fr, const ssv_cpx* tw, int N, int nf, int h, int tid, int nth) {
  const int M = N >> 1, lg = ssv_fft_log2(M) - 1, FS = ssv_fft_frame_stride(M);
  for (int u = tid; u < (nf << lg); u += nth) {
    const int f = u >> lg, j = u & ((1 << lg) - 1);
    ssv_cpx* p = fr + f * FS + ssv_fft_bfly_slot(j, h);
    const ssv_cpx a = p[0], b = p[h], w = tw[ssv_fft_bfly_twiddle(j, h, N)];
    const float dr = a.re - b.re, di = a.im - b.im;
    p[0] = ssv_cpx{a.re + b.re, a.im + b.im};
    p[h] = ssv_cpx{dr * w.re - di * w.im, dr * w.im + di * w.re};
  }
}
SSV_HD void ssv_fft_dit_stage(ssv_cpx* fr, const ssv_cpx* tw, int N, int nf, int h, int tid, int nth) {
  const int M = N >> 1, lg = ssv_fft_log2(M) - 1, FS = ssv_fft_frame_stride(M);
  for (int u = tid; u < (nf << lg); u += nth) {
    const int f = u >> lg, j = u & ((1 << lg) - 1);
    ssv_cpx* p = fr + f * FS + ssv_fft_bfly_slot(j, h);
    const ssv_cpx a = p[0], c = p[h], w = tw[ssv_fft_bfly_twiddle(j, h, N)];
    const float br = c.re * w.re + c.im * w.im, bi = c.im * w.re - c.re * w.im;       // c * conj(w)
    p[0] = ssv_cpx{a.re + br, a.im + bi};
    p[h] = ssv_cpx{a.re - br, a.im - bi};
  }
}

// ---- real <-> packed complex ---------------------------------------------------------------------------------------------------------
SSV_HD void ssv_fft_rsplit(ssv_cpx zk, ssv_cpx zm, ssv_cpx w, ssv_cpx& xk, ssv_cpx& xm) {
  const float er = 0.5f * (zk.re + zm.re), ei = 0.5f * (zk.im - zm.im);
  const float orr = 0.5f * (zk.im + zm.im), oi = -0.5f * (zk.re - zm.re);
  const float pr = w.re * orr - w.im * oi, pi = w.re * oi + w.im * orr;
  xk = ssv_cpx{er + pr, ei + pi};
  xm = ssv_cpx{er - pr, pi - ei};
}
// twice Z[k] and Z[M-k] (the half goes into the output scale)
SSV_HD void ssv_fft_rmerge(ssv_cpx xk, ssv_cpx xm, ssv_cpx w, ssv_cpx& zk, ssv_cpx& zm) {
  const float er = xk.re + xm.re, ei = xk.im - xm.im, dr = xk.re - xm.re, di = xk.im + xm.im;
  const float orr = dr * w.re + di * w.im, oi = di * w.re - dr * w.im;                // D * conj(w)
  zk = ssv_cpx{er - oi, ei + orr};
  zm = ssv_cpx{er + oi, orr - ei};
}

// Spectrum of the tile's transformed frames: sink(f, k, X[k]) for every k in [0, M] of every frame f < nf, once each.  An item is the
// pair (k, M - k), k <= M / 2; the threads run along the frames (ftile, the tile size, is a power of two).
template <class Sink>
SSV_HD void ssv_fft_emit_spectrum(const ssv_cpx* fr, const ssv_cpx* tw, int N, int nf, int ftile, int tid, int nth, Sink sink) {
  const int M = N >> 1, bits = ssv_fft_log2(M), FS = ssv_fft_frame_stride(M), lt = ssv_fft_log2(ftile);
  for (int u = tid; u < ((M / 2 + 1) << lt); u += nth) {
    const int f = u & (ftile - 1), k = u >> lt, km = M - k;
    if (f >= nf) continue;
    const ssv_cpx zk = fr[f * FS + ssv_fft_bitrev(k, bits)], zm = fr[f * FS + ssv_fft_bitrev(km & (M - 1), bits)];
    ssv_cpx xk, xm;
    ssv_fft_rsplit(zk, zm, tw[k], xk, xm);
    sink(f, k, xk);
    if (km != k) sink(f, km, xm);
  }
}
// The reverse: src(f, k) = X[k], k in [0, M]; leaves twice Z in bit-reversed order, ready for the decimation-in-time stages.
template <class Src>
SSV_HD void ssv_fft_gather_spectrum(ssv_cpx* fr, const ssv_cpx* tw, int N, int nf, int ftile, int tid, int nth, Src src) {
  const int M = N >> 1, bits = ssv_fft_log2(M), FS = ssv_fft_frame_stride(M), lt = ssv_fft_log2(ftile);
  for (int u = tid; u < ((M / 2 + 1) << lt); u += nth) {
    const int f = u & (ftile - 1), k = u >> lt, km = M - k;
    if (f >= nf) continue;
    ssv_cpx xk = src(f, k), xm = src(f, km);
    if (k == 0) xk.im = xm.im = 0.f;                   // DC and Nyquist are real
    ssv_cpx zk, zm;
    ssv_fft_rmerge(xk, xm, tw[k], zk, zm);
    fr[f * FS + ssv_fft_bitrev(k, bits)] = zk;
    if (k != 0 && km != k) fr[f * FS + ssv_fft_bitrev(km, bits)] = zm;
  }
}
// windowed inverse frames: sink(f, m, w[2m] x[2m], w[2m+1] x[2m+1]), m < M; the threads run along the samples of a frame
template <class Sink>
SSV_HD void ssv_fft_emit_frames(const ssv_cpx* fr, const float* win, int N, int nf, int tid, int nth, Sink sink) {
  const int M = N >> 1, lg = ssv_fft_log2(M), FS = ssv_fft_frame_stride(M);
  const float s = 1.f / (float)N;
  for (int u = tid; u < (nf << lg); u += nth) {
    const int f = u >> lg, m = u & (M - 1);
    const ssv_cpx z = fr[f * FS + m];
    sink(f, m, z.re * (win[2 * m] * s), z.im * (win[2 * m + 1] * s));
  }
}

// ---- analysis frames into the LDS image ---------------------------------------------------------------------------------------------
// from a waveform y[0 .. n), reflect-padded by N / 2: frame t0 + f, packed and windowed (needs n > N / 2 and (t0 + nf - 1) * hop <= n)
SSV_HD void ssv_fft_load_signal(ssv_cpx* fr, const float* y, int n, const float* win, int N, int hop, int t0, int nf, int tid, int nth) {
  const int M = N >> 1, lg = ssv_fft_log2(M), FS = ssv_fft_frame_stride(M);
  for (int u = tid; u < (nf << lg); u += nth) {
    const int f = u >> lg, m = u & (M - 1), p = (t0 + f) * hop + 2 * m - M;
    fr[f * FS + m] = ssv_cpx{y[ssv_fft_reflect(p, n)] * win[2 * m], y[ssv_fft_reflect(p + 1, n)] * win[2 * m + 1]};
  }
}
// from the staged span of the Griffin-Lim step: span[s] is the padded waveform at t0 * hop + s
SSV_HD void ssv_fft_load_span(ssv_cpx* fr, const float* span, const float* win, int N, int hop, int nf, int tid, int nth) {
  const int M = N >> 1, lg = ssv_fft_log2(M), FS = ssv_fft_frame_stride(M);
  for (int u = tid; u < (nf << lg); u += nth) {
    const int f = u >> lg, m = u & (M - 1);
    const float* s = span + f * hop + 2 * m;
    fr[f * FS + m] = ssv_cpx{s[0] * win[2 * m], s[1] * win[2 * m + 1]};
  }
}

// ---- overlap-add from frame-major inverse frames frb (T, N) ---------------------------------------------------------------------------
// ola(m) = sum over frames t with 0 <= m - t * hop < N of frb[t][m - t * hop], added in increasing t (librosa's istft loop), times
// inv_env[m]; m indexes the untrimmed signal of N + hop * (T - 1) samples
SSV_HD float ssv_ola_fm(const float* frb, const float* inv_env, int m, int N, int T, int hop) {
  int t1 = m / hop;
  if (t1 > T - 1) t1 = T - 1;
  const int t0 = m - N + 1 <= 0 ? 0 : (m - N + hop) / hop;       // ceil((m - N + 1) / hop)
  float acc = 0.f;
  for (int t = t0; t <= t1; ++t) acc += frb[(long)t * N + (m - t * hop)];
  return acc * inv_env[m];
}
// samples of the padded waveform that frames t0 .. t0 + nf - 1 cover, and where sample s of them lies in the untrimmed overlap-add:
// trim N / 2, reflect over the hop * (T - 1) samples that remain (one reflection: needs hop * (T - 1) > N / 2), add N / 2 again
SSV_HD int ssv_gl_span_count(int nf, int hop, int N) { return (nf - 1) * hop + N; }
SSV_HD int ssv_gl_span_index(int s, int t0, int N, int T, int hop) { return ssv_fft_reflect(t0 * hop + s - N / 2, hop * (T - 1)) + N / 2; }
SSV_HD void ssv_gl_stage_span(float* span, const float* frb, const float* inv_env, int t0, int nf, int N, int T, int hop, int tid, int nth) {
  const int count = ssv_gl_span_count(nf, hop, N);
  for (int s = tid; s < count; s += nth) span[s] = ssv_ola_fm(frb, inv_env, ssv_gl_span_index(s, t0, N, T, hop), N, T, hop);
}
