// Host run of the loops of spoofsv_amd/csrc/fft_core.h, one emulated workgroup per frame tile: every loop is called for tid = 0 .. NTH - 1
// in turn, the end of such a round standing for the kernel's barrier.  The LDS images are heap blocks of exactly the size the kernels ask
// for, so the address sanitizer this is compiled with (tests/test_fft_vocoder_cpu.py) sees an index that leaves them.
//   fft_core_check stft  N hop n  y.f32      tab.f32 out.f32              out: spectrum (2F, T), T = 1 + n / hop
//   fft_core_check istft N hop T  spec.f32   tab.f32 out.f32              out: windowed inverse frames (T, N)
//   fft_core_check gl    N hop T  frames.f32 env.f32 tab.f32 out.f32      out: spectrum (2F, T) of the overlap-added, re-framed signal
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../spoofsv_amd/csrc/fft_core.h"

static const int NTH = 192;

static std::vector<float> read_f32(const char* path, size_t count) {
  std::vector<float> v(count);
  FILE* f = fopen(path, "rb");
  if (!f || fread(v.data(), sizeof(float), count, f) != count) { fprintf(stderr, "cannot read %zu floats from %s\n", count, path); exit(2); }
  fclose(f);
  return v;
}
static void write_f32(const char* path, const std::vector<float>& v) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}
template <class Fn> static void round_of(Fn fn) { for (int tid = 0; tid < NTH; ++tid) fn(tid); }

static void forward_stages(ssv_cpx* fr, const ssv_cpx* tw, int N, int nf) {
  for (int h = N >> 2; h >= 1; h >>= 1) round_of([&](int tid) { ssv_fft_dif_stage(fr, tw, N, nf, h, tid, NTH); });
}
static void emit(const ssv_cpx* fr, const ssv_cpx* tw, int N, int nf, int tile, int t0, int T, std::vector<float>& out, std::vector<int>& hits) {
  const int F = N / 2 + 1;
  round_of([&](int tid) {
    ssv_fft_emit_spectrum(fr, tw, N, nf, tile, tid, NTH, [&](int f, int k, ssv_cpx x) {
      out[(size_t)k * T + t0 + f] = x.re;
      out[(size_t)(F + k) * T + t0 + f] = x.im;
      ++hits[(size_t)k * T + t0 + f];
    });
  });
}

int main(int argc, char** argv) {
  if (argc < 8) { fprintf(stderr, "usage: see the head of fft_core_check.cpp\n"); return 2; }
  const char* mode = argv[1];
  const int N = atoi(argv[2]), hop = atoi(argv[3]), M = N / 2, F = M + 1;
  if (!ssv_fft_supported(N) || hop <= 0 || hop > N) { fprintf(stderr, "unsupported N / hop\n"); return 2; }
  const int tile = ssv_fft_tile(N);
  if (!strcmp(mode, "stft")) {
    const int n = atoi(argv[4]), T = 1 + n / hop;
    std::vector<float> y = read_f32(argv[5], n), tab = read_f32(argv[6], ssv_fft_tab_floats(N)), out((size_t)2 * F * T);
    std::vector<int> hits((size_t)F * T, 0);
    for (int t0 = 0; t0 < T; t0 += tile) {
      const int nf = tile < T - t0 ? tile : T - t0;
      ssv_cpx* sm = new ssv_cpx[ssv_fft_lds_cpx(N)];
      ssv_cpx *tw = sm, *fr = sm + M;
      round_of([&](int tid) {
        ssv_fft_stage_twiddles(tw, tab.data(), N, tid, NTH);
        ssv_fft_load_signal(fr, y.data(), n, tab.data(), N, hop, t0, nf, tid, NTH);
      });
      forward_stages(fr, tw, N, nf);
      emit(fr, tw, N, nf, tile, t0, T, out, hits);
      delete[] sm;
    }
    for (int h : hits) if (h != 1) { fprintf(stderr, "a spectrum element was written %d times\n", h); return 3; }
    write_f32(argv[7], out);
  } else if (!strcmp(mode, "istft")) {
    const int T = atoi(argv[4]);
    std::vector<float> spec = read_f32(argv[5], (size_t)2 * F * T), tab = read_f32(argv[6], ssv_fft_tab_floats(N)), out((size_t)T * N);
    std::vector<int> hits((size_t)T * M, 0);
    for (int t0 = 0; t0 < T; t0 += tile) {
      const int nf = tile < T - t0 ? tile : T - t0;
      ssv_cpx* sm = new ssv_cpx[ssv_fft_lds_cpx(N)];
      ssv_cpx *tw = sm, *fr = sm + M;
      round_of([&](int tid) { ssv_fft_stage_twiddles(tw, tab.data(), N, tid, NTH); });
      round_of([&](int tid) {
        ssv_fft_gather_spectrum(fr, tw, N, nf, tile, tid, NTH, [&](int f, int k) {
          return ssv_cpx{spec[(size_t)k * T + t0 + f], spec[(size_t)(F + k) * T + t0 + f]};
        });
      });
      for (int h = 1; h < M; h <<= 1) round_of([&](int tid) { ssv_fft_dit_stage(fr, tw, N, nf, h, tid, NTH); });
      round_of([&](int tid) {
        ssv_fft_emit_frames(fr, tab.data(), N, nf, tid, NTH, [&](int f, int m, float a, float b) {
          out[(size_t)(t0 + f) * N + 2 * m] = a;
          out[(size_t)(t0 + f) * N + 2 * m + 1] = b;
          ++hits[(size_t)(t0 + f) * M + m];
        });
      });
      delete[] sm;
    }
    for (int h : hits) if (h != 1) { fprintf(stderr, "a frame element was written %d times\n", h); return 3; }
    write_f32(argv[7], out);
  } else if (!strcmp(mode, "gl") && argc >= 9) {
    const int T = atoi(argv[4]);
    if ((long)hop * (T - 1) <= N / 2) { fprintf(stderr, "hop * (T - 1) <= N / 2\n"); return 2; }
    std::vector<float> frames = read_f32(argv[5], (size_t)T * N), env = read_f32(argv[6], (size_t)N + (size_t)hop * (T - 1));
    std::vector<float> tab = read_f32(argv[7], ssv_fft_tab_floats(N)), out((size_t)2 * F * T);
    std::vector<int> hits((size_t)F * T, 0);
    for (int t0 = 0; t0 < T; t0 += tile) {          // the first and the last tile of the signal among them
      const int nf = tile < T - t0 ? tile : T - t0;
      ssv_cpx* sm = new ssv_cpx[ssv_fft_lds_cpx(N)];
      float* span = new float[ssv_gl_span_count(nf, hop, N)];       // (the kernel reserves the full tile's span: this is the part it may touch)
      ssv_cpx *tw = sm, *fr = sm + M;
      round_of([&](int tid) {
        ssv_fft_stage_twiddles(tw, tab.data(), N, tid, NTH);
        ssv_gl_stage_span(span, frames.data(), env.data(), t0, nf, N, T, hop, tid, NTH);
      });
      round_of([&](int tid) { ssv_fft_load_span(fr, span, tab.data(), N, hop, nf, tid, NTH); });
      forward_stages(fr, tw, N, nf);
      emit(fr, tw, N, nf, tile, t0, T, out, hits);
      delete[] span;
      delete[] sm;
    }
    for (int h : hits) if (h != 1) { fprintf(stderr, "a spectrum element was written %d times\n", h); return 3; }
    write_f32(argv[8], out);
  } else {
    fprintf(stderr, "unknown mode %s\n", mode);
    return 2;
  }
  return 0;
}
