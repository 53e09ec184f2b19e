// FFT back end of the vocoder, gfx950: STFT, ISTFT and one Griffin-Lim round trip with every frame of a tile resident in LDS.  fp32
// throughout, no atomics, no arithmetic mode: the results depend on the inputs alone.  The loops and their index arithmetic are in
// fft_core.h (they also run on the host); this file holds the kernels' global-memory sides and the C ABI.
//
// Spectra are (B, 2F, T) float32, rows [0, F) real, rows [F, 2F) imaginary, T fastest.  Inverse frames are FRAME-major, (B, T, N): a
// frame is one contiguous run.  A workgroup owns ssv_fft_tile(N) consecutive frames of one batch item, so its accesses to the
// T-fastest arrays are runs of tile floats (64 bytes at N = 1024, 32 at N = 2048, where 16 frames and their span exceed the LDS).
#include "ssv_common.h"
#include "fft_core.h"
#include <math.h>
#include <atomic>

#define FFT_THREADS 512
extern __shared__ ssv_cpx fft_sm[];       // [twiddles N/2 | frames tile * (M + 1) | span floats (Griffin-Lim step only)]

__device__ __forceinline__ void fft_forward_stages(ssv_cpx* fr, const ssv_cpx* tw, int N, int nf) {
  for (int h = N >> 2; h >= 1; h >>= 1) {
    ssv_fft_dif_stage(fr, tw, N, nf, h, threadIdx.x, FFT_THREADS);
    __syncthreads();
  }
}

// reflect padding, window and real FFT of the tile's frames of waveform y (B, n)
__global__ __launch_bounds__(FFT_THREADS) void stft_fft_kernel(const float* __restrict__ y, const float* __restrict__ tab,
                                                               float* __restrict__ spec, int n, int N, int hop, int T) {
  const int M = N >> 1, F = M + 1, tile = ssv_fft_tile(N), t0 = blockIdx.x * tile, nf = min(tile, T - t0);
  ssv_cpx* tw = fft_sm;
  ssv_cpx* fr = fft_sm + M;
  ssv_fft_stage_twiddles(tw, tab, N, threadIdx.x, FFT_THREADS);
  ssv_fft_load_signal(fr, y + (long)blockIdx.y * n, n, tab, N, hop, t0, nf, threadIdx.x, FFT_THREADS);
  __syncthreads();
  fft_forward_stages(fr, tw, N, nf);
  float* sb = spec + (long)blockIdx.y * 2 * F * T + t0;
  ssv_fft_emit_spectrum(fr, tw, N, nf, tile, threadIdx.x, FFT_THREADS, [=](int f, int k, ssv_cpx x) {
    sb[(long)k * T + f] = x.re;
    sb[(long)(F + k) * T + f] = x.im;
  });
}

// inverse real FFT and synthesis window: spectrum (B, 2F, T) -> frames (B, T, N)
__global__ __launch_bounds__(FFT_THREADS) void istft_frames_fft_kernel(const float* __restrict__ spec, const float* __restrict__ tab,
                                                                       float* __restrict__ frames, int N, int T) {
  const int M = N >> 1, F = M + 1, tile = ssv_fft_tile(N), t0 = blockIdx.x * tile, nf = min(tile, T - t0);
  ssv_cpx* tw = fft_sm;
  ssv_cpx* fr = fft_sm + M;
  ssv_fft_stage_twiddles(tw, tab, N, threadIdx.x, FFT_THREADS);
  __syncthreads();
  const float* sb = spec + (long)blockIdx.y * 2 * F * T + t0;
  ssv_fft_gather_spectrum(fr, tw, N, nf, tile, threadIdx.x, FFT_THREADS, [=](int f, int k) {
    return ssv_cpx{sb[(long)k * T + f], sb[(long)(F + k) * T + f]};
  });
  __syncthreads();
  for (int h = 1; h < M; h <<= 1) {
    ssv_fft_dit_stage(fr, tw, N, nf, h, threadIdx.x, FFT_THREADS);
    __syncthreads();
  }
  float* ob = frames + ((long)blockIdx.y * T + t0) * N;
  ssv_fft_emit_frames(fr, tab, N, nf, threadIdx.x, FFT_THREADS, [=](int f, int m, float a, float b) {
    *(float2*)(ob + (long)f * N + 2 * m) = make_float2(a, b);
  });
}

// One Griffin-Lim round trip: overlap-add of the inverse frames that touch the tile's span of the padded waveform, envelope, centre trim
// and reflect padding (staged once in LDS), window, real FFT, and the phase step a = reb - alpha * tprev, proj = mag * a / (|a| + 1e-16).
__global__ __launch_bounds__(FFT_THREADS) void gl_step_fft_kernel(const float* __restrict__ frames, const float* __restrict__ inv_env,
                                                                  const float* __restrict__ tab, const float* __restrict__ mag,
                                                                  const float* __restrict__ tprev, float alpha, float* __restrict__ reb,
                                                                  float* __restrict__ proj, int N, int T, int hop) {
  const int M = N >> 1, F = M + 1, tile = ssv_fft_tile(N), t0 = blockIdx.x * tile, nf = min(tile, T - t0);
  ssv_cpx* tw = fft_sm;
  ssv_cpx* fr = fft_sm + M;
  float* span = (float*)(fft_sm + ssv_fft_lds_cpx(N));
  ssv_fft_stage_twiddles(tw, tab, N, threadIdx.x, FFT_THREADS);
  ssv_gl_stage_span(span, frames + (long)blockIdx.y * T * N, inv_env, t0, nf, N, T, hop, threadIdx.x, FFT_THREADS);
  __syncthreads();
  ssv_fft_load_span(fr, span, tab, N, hop, nf, threadIdx.x, FFT_THREADS);
  __syncthreads();
  fft_forward_stages(fr, tw, N, nf);
  const long FT = (long)F * T, so = (long)blockIdx.y * 2 * FT + t0;
  const float* mb = mag + (long)blockIdx.y * FT + t0;
  ssv_fft_emit_spectrum(fr, tw, N, nf, tile, threadIdx.x, FFT_THREADS, [=](int f, int k, ssv_cpx x) {
    const long o = so + (long)k * T + f;
    reb[o] = x.re;
    reb[o + FT] = x.im;
    float ar = x.re, ai = x.im;
    if (tprev) { ar -= alpha * tprev[o]; ai -= alpha * tprev[o + FT]; }
    const float m = mb[(long)k * T + f] / (sqrtf(ar * ar + ai * ai) + 1e-16f);
    proj[o] = ar * m;
    proj[o + FT] = ai * m;
  });
}

// overlap-add, envelope and centre trim from frame-major frames: (B, T, N) -> (B, hop * (T - 1))
__global__ __launch_bounds__(256) void ola_signal_fm_kernel(const float* __restrict__ frames, const float* __restrict__ inv_env,
                                                            float* __restrict__ y, int N, int T, int hop) {
  const int len = hop * (T - 1), i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  y[(long)blockIdx.y * len + i] = ssv_ola_fm(frames + (long)blockIdx.y * T * N, inv_env, i + N / 2, N, T, hop);
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" size_t ssv_fft_tables_floats(int n_fft) { return ssv_fft_supported(n_fft) ? (size_t)ssv_fft_tab_floats(n_fft) : 0; }

extern "C" int ssv_fft_tables_host(float* out, int n_fft) {
  SSV_CHECK(out, SSV_BAD_SHAPE, "fft_tables_host: null pointer");
  SSV_CHECK(ssv_fft_supported(n_fft), SSV_UNSUPPORTED, "fft_tables_host: n_fft=%d is not a power of two in [%d, %d]", n_fft, SSV_FFT_MIN, SSV_FFT_MAX);
  const int N = n_fft;
  for (int i = 0; i < N; ++i) out[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)N));      // periodic Hann
  for (int k = 0; k < N / 2; ++k) {            // the argument k / N needs no reduction: k < N / 2
    const double a = 2.0 * M_PI * (double)k / (double)N;
    out[N + k] = (float)cos(a);
    out[N + N / 2 + k] = (float)sin(a);
  }
  return 0;
}

extern "C" int ssv_fft_frame_tile(int n_fft) {
  SSV_CHECK(ssv_fft_supported(n_fft), SSV_UNSUPPORTED, "fft_frame_tile: n_fft=%d is not a power of two in [%d, %d]", n_fft, SSV_FFT_MIN, SSV_FFT_MAX);
  return ssv_fft_tile(n_fft);
}

// the kernels take up to 160 KB of dynamic LDS: say so once per device
static int fft_lds_limit() {
  static std::atomic<int> done[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return ssv_fail(-(int)e, "fft: hipGetDevice: %s", hipGetErrorString(e));
  if (dev >= 0 && dev < 64 && done[dev].load(std::memory_order_acquire)) return 0;
  const void* ks[3] = {(const void*)stft_fft_kernel, (const void*)istft_frames_fft_kernel, (const void*)gl_step_fft_kernel};
  for (int i = 0; i < 3; ++i) {
    e = hipFuncSetAttribute(ks[i], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return ssv_fail(-(int)e, "fft: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(e));
  }
  if (dev >= 0 && dev < 64) done[dev].store(1, std::memory_order_release);
  return 0;
}

static size_t fft_lds_bytes(int N, int span_floats) { return (size_t)ssv_fft_lds_cpx(N) * sizeof(ssv_cpx) + (size_t)span_floats * sizeof(float); }
#define FFT_CHECK_N(what, n_fft) \
  SSV_CHECK(ssv_fft_supported(n_fft), SSV_UNSUPPORTED, what ": n_fft=%d is not a power of two in [%d, %d]", n_fft, SSV_FFT_MIN, SSV_FFT_MAX)
// sizes of a T-frame problem: centred frames need hop * (T - 1) > N / 2 for the one reflection
static bool fft_frames_ok(int B, int N, int T, int hop) {
  return B <= 65535 && hop <= N && T >= 2 && (long)hop * (T - 1) > N / 2 && (long)hop * (T - 1) + N < (1L << 30) && (long)B * N * T < (1L << 40);
}

extern "C" int ssv_stft_fft(const float* y, const float* tab, float* spec, int B, int n, int n_fft, int hop, int T, ssv_stream_t stream) {
  SSV_CHECK(y && tab && spec && B > 0 && n > 0 && n_fft > 0 && hop > 0 && T > 0, SSV_BAD_SHAPE,
            "stft_fft: bad argument B=%d n=%d n_fft=%d hop=%d T=%d", B, n, n_fft, hop, T);
  FFT_CHECK_N("stft_fft", n_fft);
  SSV_CHECK(B <= 65535 && hop <= n_fft && n > n_fft / 2 && n < (1 << 30) && T == 1 + n / hop, SSV_BAD_SHAPE,
            "stft_fft: bad argument B=%d n=%d n_fft=%d hop=%d T=%d (need hop <= n_fft, n > n_fft/2, T = 1 + n/hop)", B, n, n_fft, hop, T);
  SSV_TRY(fft_lds_limit());
  hipLaunchKernelGGL(stft_fft_kernel, dim3(ssv_cdiv(T, ssv_fft_tile(n_fft)), B), dim3(FFT_THREADS), fft_lds_bytes(n_fft, 0), (hipStream_t)stream,
                     y, tab, spec, n, n_fft, hop, T);
  return ssv_check_launch("stft_fft");
}

extern "C" int ssv_istft_frames_fft(const float* spec, const float* tab, float* fr, int B, int n_fft, int T, ssv_stream_t stream) {
  SSV_CHECK(spec && tab && fr && B > 0 && n_fft > 0 && T > 0, SSV_BAD_SHAPE, "istft_frames_fft: bad argument B=%d n_fft=%d T=%d", B, n_fft, T);
  FFT_CHECK_N("istft_frames_fft", n_fft);
  SSV_CHECK(B <= 65535 && (long)B * n_fft * T < (1L << 40), SSV_BAD_SHAPE, "istft_frames_fft: bad argument B=%d n_fft=%d T=%d", B, n_fft, T);
  SSV_CHECK(((uintptr_t)fr & 7) == 0, SSV_BAD_SHAPE, "istft_frames_fft: fr must be 8-byte aligned (the frames are stored two floats at a time)");
  SSV_TRY(fft_lds_limit());
  hipLaunchKernelGGL(istft_frames_fft_kernel, dim3(ssv_cdiv(T, ssv_fft_tile(n_fft)), B), dim3(FFT_THREADS), fft_lds_bytes(n_fft, 0), (hipStream_t)stream,
                     spec, tab, fr, n_fft, T);
  return ssv_check_launch("istft_frames_fft");
}

extern "C" int ssv_ola_signal_fm(const float* fr, const float* inv_env, float* y, int B, int N, int T, int hop, ssv_stream_t stream) {
  SSV_CHECK(fr && inv_env && y && B > 0 && N >= 2 && N % 2 == 0 && hop > 0 && T > 0 && fft_frames_ok(B, N, T, hop), SSV_BAD_SHAPE,
            "ola_signal_fm: bad argument B=%d N=%d T=%d hop=%d (need hop <= N, hop*(T-1) > N/2)", B, N, T, hop);
  hipLaunchKernelGGL(ola_signal_fm_kernel, dim3(ssv_cdiv((long)hop * (T - 1), 256), B), dim3(256), 0, (hipStream_t)stream, fr, inv_env, y, N, T, hop);
  return ssv_check_launch("ola_signal_fm");
}

extern "C" int ssv_gl_step_fft(const float* fr, const float* inv_env, const float* tab, const float* mag, const float* tprev, float alpha,
                               float* reb, float* proj, int B, int n_fft, int T, int hop, ssv_stream_t stream) {
  SSV_CHECK(fr && inv_env && tab && mag && reb && proj && reb != tprev && B > 0 && n_fft > 0 && T > 0 && hop > 0, SSV_BAD_SHAPE,
            "gl_step_fft: bad argument B=%d n_fft=%d T=%d hop=%d (reb must not alias tprev)", B, n_fft, T, hop);
  FFT_CHECK_N("gl_step_fft", n_fft);
  SSV_CHECK(fft_frames_ok(B, n_fft, T, hop), SSV_BAD_SHAPE, "gl_step_fft: bad argument B=%d n_fft=%d T=%d hop=%d (need hop <= n_fft, hop*(T-1) > n_fft/2)",
            B, n_fft, T, hop);
  SSV_TRY(fft_lds_limit());
  const int tile = ssv_fft_tile(n_fft);
  hipLaunchKernelGGL(gl_step_fft_kernel, dim3(ssv_cdiv(T, tile), B), dim3(FFT_THREADS), fft_lds_bytes(n_fft, ssv_gl_span_count(tile, hop, n_fft)),
                     (hipStream_t)stream, fr, inv_env, tab, mag, tprev, alpha, reb, proj, n_fft, T, hop);
  return ssv_check_launch("gl_step_fft");
}
