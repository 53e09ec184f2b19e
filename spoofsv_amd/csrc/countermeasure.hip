// The spoof countermeasure's own kernels (gfx950): the fused classifier head of anti_spoofing/discriminator.py:129-131 with the
// binary cross-entropy of anti_spoofing/main_spoof_conv1d.py:87, and the optimizer that trainer uses (main_spoof_conv1d.py:52):
// Adam with L2 weight decay and AMSGrad as one multi-tensor launch.
//
// Head: z_b = bias + sum_c w[c] * mean_t leaky_relu(x[b,c,t]) -- conv5 (one output channel, k = 1) and AdaptiveAvgPool1d(1) commute,
// so the convolution never runs as a product over T columns and its weight gradient is a (B x C) contraction of saved means.
// Every launch has ONE workgroup per batch item (a wave per (b, c) row) or ONE workgroup in all (the sums over the batch, in a
// fixed order): no atomics, nothing passes between workgroups inside a launch, the same inputs give the same bits.
#include "ssv_common.h"

#define CM_MAX_C 16

// sum over the 64 lanes in double, the pairing of a xor butterfly (every lane gets it)
__device__ __forceinline__ double cm_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// The scalar tail of one item, in double (a few dozen operations per ITEM; the per-element work above it is fp32).
//   p = sigmoid(z), q = 1 - p evaluated as sigmoid(-z).
// q by subtraction is what the reference computes (`1-pred`, main_spoof_conv1d.py:87) and it loses every digit of q in float32
// once z exceeds about 17 (p rounds to 1, q to 0): log(q + 1e-6) is then log(1e-6) instead of log(1e-6 + e^-z); just below that
// q keeps only a few bits, and the float32 term of an item on the wrong label is off by up to 0.06 (at z = 16.6, 7e-3 already at
// z = 12); its gradient p q (...) is exactly 0 from z = 17 on.  Evaluated as
// sigmoid(-z) both tails keep full relative accuracy.  z itself is summed in double from the fp32 means: q = e^-z turns an ABSOLUTE
// error of z into a RELATIVE error of q, and one float32 rounding of z = 40 is already 1.9e-6.
struct CmItem { double p, q; };
__device__ __forceinline__ CmItem cm_item(const float* __restrict__ am, const float* __restrict__ w, const float* __restrict__ bias, int C) {
  double z = (double)bias[0];
  for (int c = 0; c < C; ++c) z += (double)w[c] * (double)am[c];
  CmItem r;
  r.p = 1.0 / (1.0 + exp(-z));
  r.q = 1.0 / (1.0 + exp(z));
  return r;
}
__device__ __forceinline__ double cm_bce(CmItem s, double y) { return -y * log(s.p + 1e-6) - (1.0 - y) * log(s.q + 1e-6); }
// d per_b / d z_b = p q (-y / (p + 1e-6) + (1 - y) / (q + 1e-6))
__device__ __forceinline__ double cm_dz(CmItem s, double y) { return s.p * s.q * (-y / (s.p + 1e-6) + (1.0 - y) / (s.q + 1e-6)); }

// The live width of a padded item (the _len entries): its first clamp(live[0], 1, T) columns, live a DEVICE int read when the kernel
// runs, so that one captured launch serves every batch of its bucket.  LEN = false is the dense head: Tl = T, nothing is read.
template <bool LEN>
__device__ __forceinline__ int cm_live(const int* __restrict__ live, int T) {
  return LEN ? min(max(live[0], 1), T) : T;
}

// ---- forward, launch 1: grid = B, 256 threads.  Wave v sums the activated rows c = v, v + 4, ... of its item (lanes stride the
// row, 16-byte loads when the row starts on a 16-byte boundary, then the wave butterfly), the means meet in LDS, and thread 0
// finishes the item.  Rows are T apart; the sums and the mean run over the first Tl columns, and nothing at or past Tl is loaded.
template <bool LEN>
__global__ __launch_bounds__(256) void cm_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ labels, float slope, float* __restrict__ pred,
                                                          float* __restrict__ amean, float* __restrict__ per, int C, int T,
                                                          const int* __restrict__ live) {
  __shared__ float am[CM_MAX_C];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Tl = cm_live<LEN>(live, T);
  const float inv_t = 1.f / (float)Tl;
  for (int c = wave; c < C; c += 4) {
    const float* __restrict__ xr = x + ((long)b * C + c) * T;
    float s = 0.f;
    int t0 = 0;
    if ((((uintptr_t)xr) & 15) == 0) {
      const int n4 = Tl >> 2;
      const f32x4* __restrict__ x4 = reinterpret_cast<const f32x4*>(xr);
      for (int i = lane; i < n4; i += 64) {
        const f32x4 v = x4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) s += v[k] > 0.f ? v[k] : slope * v[k];
      }
      t0 = n4 << 2;
    }
    for (int t = t0 + lane; t < Tl; t += 64) {
      const float v = xr[t];
      s += v > 0.f ? v : slope * v;
    }
    s = ssv_wave_sum(s) * inv_t;
    if (lane == 0) am[c] = s;
  }
  __syncthreads();
  if (threadIdx.x < C && amean) amean[(long)b * C + threadIdx.x] = am[threadIdx.x];
  if (threadIdx.x == 0) {
    const CmItem s = cm_item(am, w, bias, C);
    pred[b] = (float)s.p;
    if (labels) per[b] = (float)cm_bce(s, (double)labels[b]);
  }
}
// ---- forward, launch 2: one wave, loss = (sum_b per_b) / B.  Lane l adds items l, l + 64, ... in that order, then the butterfly.
__global__ __launch_bounds__(64) void cm_loss_kernel(const float* __restrict__ per, float* __restrict__ loss, int B) {
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += 64) s += (double)per[b];
  s = cm_wave_sum_f64(s);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)B);
}

// ---- backward, launch 1: grid = B, 256 threads.  dz_b once per item (recomputed from the saved means: the saved float32 pred
// cannot give q back), then dx[b,c,t] = dz_b / Tl * w[c] * (x > 0 ? 1 : slope) over the item's C * T elements; with LEN the columns at or
// past Tl are written as exact zeros whatever x holds there (a NaN compares false and is then discarded).
template <bool LEN>
__global__ __launch_bounds__(256) void cm_head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ labels, const float* __restrict__ amean,
                                                          const float* __restrict__ gscale, float slope, float* __restrict__ dx,
                                                          float* __restrict__ dz, int B, int C, int T, const int* __restrict__ live) {
  __shared__ float wz[CM_MAX_C];      // dz_b / Tl * w[c]
  __shared__ float dzs;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    const CmItem s = cm_item(amean + (long)b * C, w, bias, C);
    const float d = (float)((double)gscale[0] / (double)B * cm_dz(s, (double)labels[b]));
    dzs = d;
    dz[b] = d;
  }
  __syncthreads();
  const unsigned uTl = (unsigned)cm_live<LEN>(live, T);
  if (threadIdx.x < C) wz[threadIdx.x] = dzs / (float)uTl * w[threadIdx.x];
  __syncthreads();
  const unsigned n = (unsigned)C * (unsigned)T, uT = (unsigned)T;      // T <= 2^26 (checked by the entry point): an item's index fits 32 bits
  const float* __restrict__ xb = x + (long)b * n;
  float* __restrict__ db = dx + (long)b * n;
  unsigned e0 = 0;
  if (((((uintptr_t)xb) | ((uintptr_t)db)) & 15) == 0) {
    const unsigned n4 = n >> 2;
    for (unsigned i = threadIdx.x; i < n4; i += 256) {
      const f32x4 v = reinterpret_cast<const f32x4*>(xb)[i];
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned c = (4 * i + k) / uT;
        const float g = wz[c];
        o[k] = v[k] > 0.f ? g : g * slope;
        if (LEN && 4 * i + k - c * uT >= uTl) o[k] = 0.f;
      }
      reinterpret_cast<f32x4*>(db)[i] = o;
    }
    e0 = n4 << 2;
  }
  for (unsigned e = e0 + threadIdx.x; e < n; e += 256) {
    const unsigned c = e / uT;
    const float g = wz[c];
    db[e] = (LEN && e - c * uT >= uTl) ? 0.f : (xb[e] > 0.f ? g : g * slope);
  }
}
// ---- backward, launch 2: one wave.  dw[c] = sum_b dz_b amean[b,c] (lane c, items in order), dbias = sum_b dz_b (lane 16).
__global__ __launch_bounds__(64) void cm_head_bwd_params_kernel(const float* __restrict__ dz, const float* __restrict__ amean, float* __restrict__ dw,
                                                                float* __restrict__ dbias, int B, int C) {
  const int c = threadIdx.x;
  if (c < C) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)dz[b] * (double)amean[(long)b * C + c];
    dw[c] = (float)s;
  } else if (c == CM_MAX_C) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)dz[b];
    dbias[0] = (float)s;
  }
}

// One body for the dense entries (live == NULL) and the _len ones: the same kernels, instantiated with and without the live width.
static int cm_head_fwd_run(const char* name, bool len, const float* x, const float* w, const float* bias, const float* labels, float slope,
                           float* pred, float* amean, float* per, float* loss, int B, int C, int T, const int* live, ssv_stream_t stream) {
  SSV_CHECK(B > 0 && C > 0 && T > 0, SSV_BAD_SHAPE, "%s: need B, C, T > 0, got B=%d C=%d T=%d", name, B, C, T);
  SSV_CHECK(C <= CM_MAX_C, SSV_BAD_SHAPE, "%s: C=%d exceeds the %d channels the head is built for", name, C, CM_MAX_C);
  SSV_CHECK(x && w && bias && pred, SSV_BAD_SHAPE, "%s: null x, w, bias or pred", name);
  SSV_CHECK(!len || live, SSV_BAD_SHAPE, "%s: null live", name);
  SSV_CHECK(!labels || (amean && per && loss), SSV_BAD_SHAPE, "%s: with labels, amean, per and loss are outputs and must not be null", name);
  hipStream_t st = (hipStream_t)stream;
  if (len)
    hipLaunchKernelGGL(cm_head_fwd_kernel<true>, dim3(B), dim3(256), 0, st, x, w, bias, labels, slope, pred, amean, per, C, T, live);
  else
    hipLaunchKernelGGL(cm_head_fwd_kernel<false>, dim3(B), dim3(256), 0, st, x, w, bias, labels, slope, pred, amean, per, C, T, live);
  SSV_TRY(ssv_check_launch(name));
  if (labels) {
    hipLaunchKernelGGL(cm_loss_kernel, dim3(1), dim3(64), 0, st, (const float*)per, loss, B);
    return ssv_check_launch("cm_loss");
  }
  return 0;
}
static int cm_head_bwd_run(const char* name, bool len, const float* x, const float* w, const float* bias, const float* labels, const float* amean,
                           const float* gscale, float slope, float* dx, float* dw, float* dbias, float* dz, int B, int C, int T, const int* live,
                           ssv_stream_t stream) {
  SSV_CHECK(B > 0 && C > 0 && T > 0, SSV_BAD_SHAPE, "%s: need B, C, T > 0, got B=%d C=%d T=%d", name, B, C, T);
  SSV_CHECK(C <= CM_MAX_C && T <= (1 << 26), SSV_BAD_SHAPE, "%s: C=%d exceeds the %d channels the head is built for (or T=%d exceeds 2^26)", name, C, CM_MAX_C, T);
  SSV_CHECK(x && w && bias && labels && amean && gscale && dx && dw && dbias && dz && (!len || live), SSV_BAD_SHAPE, "%s: null argument", name);
  hipStream_t st = (hipStream_t)stream;
  if (len)
    hipLaunchKernelGGL(cm_head_bwd_kernel<true>, dim3(B), dim3(256), 0, st, x, w, bias, labels, amean, gscale, slope, dx, dz, B, C, T, live);
  else
    hipLaunchKernelGGL(cm_head_bwd_kernel<false>, dim3(B), dim3(256), 0, st, x, w, bias, labels, amean, gscale, slope, dx, dz, B, C, T, live);
  SSV_TRY(ssv_check_launch(name));
  hipLaunchKernelGGL(cm_head_bwd_params_kernel, dim3(1), dim3(64), 0, st, (const float*)dz, amean, dw, dbias, B, C);
  return ssv_check_launch("cm_head_bwd_params");
}

extern "C" int ssv_cm_head_fwd(const float* x, const float* w, const float* bias, const float* labels, float slope, float* pred, float* amean,
                               float* per, float* loss, int B, int C, int T, ssv_stream_t stream) {
  return cm_head_fwd_run("cm_head_fwd", false, x, w, bias, labels, slope, pred, amean, per, loss, B, C, T, nullptr, stream);
}
extern "C" int ssv_cm_head_bwd(const float* x, const float* w, const float* bias, const float* labels, const float* amean, const float* gscale,
                               float slope, float* dx, float* dw, float* dbias, float* dz, int B, int C, int T, ssv_stream_t stream) {
  return cm_head_bwd_run("cm_head_bwd", false, x, w, bias, labels, amean, gscale, slope, dx, dw, dbias, dz, B, C, T, nullptr, stream);
}
extern "C" int ssv_cm_head_fwd_len(const float* x, const float* w, const float* bias, const float* labels, float slope, float* pred, float* amean,
                                   float* per, float* loss, int B, int C, int T, const int* live, ssv_stream_t stream) {
  return cm_head_fwd_run("cm_head_fwd_len", true, x, w, bias, labels, slope, pred, amean, per, loss, B, C, T, live, stream);
}
extern "C" int ssv_cm_head_bwd_len(const float* x, const float* w, const float* bias, const float* labels, const float* amean, const float* gscale,
                                   float slope, float* dx, float* dw, float* dbias, float* dz, int B, int C, int T, const int* live,
                                   ssv_stream_t stream) {
  return cm_head_bwd_run("cm_head_bwd_len", true, x, w, bias, labels, amean, gscale, slope, dx, dw, dbias, dz, B, C, T, live, stream);
}

// ---- multi-tensor Adam with L2 weight decay and AMSGrad ---------------------------------------------------------------------
// torch.optim.Adam's single-tensor path: g' = g + wd p; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; vmax = max(vmax, v);
// denom = sqrt(vmax)/sqrt(1-b2^t) + eps; p -= (lr/(1-b1^t)) * m / denom.  AMS = false: v in place of vmax, which is neither read nor
// written.  The structure is adam_multi_kernel's (misc.hip): one workgroup per chunk, 16-byte accesses when every pointer of the
// chunk allows it, two vectors per thread in flight, the scalar loop otherwise and for the tail.  g is only read.
template <bool AMS>
__global__ __launch_bounds__(256) void adam_ex_multi_kernel(const ssv_adam_ex_chunk* __restrict__ chunks, float lr, float b1, float b2, float eps,
                                                            float wd, int step_host, const int* __restrict__ step_dev) {
  const int step = step_dev ? step_dev[0] + 1 : step_host;
  const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
  const float step_size = (float)((double)lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const ssv_adam_ex_chunk ch = chunks[blockIdx.x];
  auto upd = [&](float& p, float g, float& m, float& v, float& x) {
    g = fmaf(wd, p, g);                       // one rounding; wd = 0 leaves g as it is
    m = b1 * m + (1.f - b1) * g;
    v = b2 * v + (1.f - b2) * g * g;
    float vh = v;
    if (AMS) { x = fmaxf(x, v); vh = x; }
    p -= step_size * (m / (sqrtf(vh) * inv_sqrt_bc2 + eps));
  };
  typedef float vf4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(1))) vf4 gf4;
  typedef __attribute__((address_space(1))) float gf1;
  long i0 = 0;
  uintptr_t bits = (uintptr_t)ch.p | (uintptr_t)ch.g | (uintptr_t)ch.m | (uintptr_t)ch.v;
  if (AMS) bits |= (uintptr_t)ch.vmax;
  if ((bits & 15) == 0) {
    const long n4 = ch.n >> 2;
    auto upd4 = [&](vf4& p, const vf4 g, vf4& m, vf4& v, vf4& x) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pp = p[k], mm = m[k], vv = v[k], xx = x[k];
        upd(pp, g[k], mm, vv, xx);
        p[k] = pp; m[k] = mm; v[k] = vv; x[k] = xx;
      }
    };
    gf4* __restrict__ p4 = (gf4*)ch.p; const gf4* __restrict__ g4 = (const gf4*)ch.g;
    gf4* __restrict__ m4 = (gf4*)ch.m; gf4* __restrict__ v4 = (gf4*)ch.v; gf4* __restrict__ x4 = (gf4*)ch.vmax;
    const vf4 zero = {0.f, 0.f, 0.f, 0.f};
    long i = threadIdx.x;
    for (; i + 256 < n4; i += 512) {
      vf4 p = p4[i], m = m4[i], v = v4[i], q = p4[i + 256], n = m4[i + 256], w = v4[i + 256];
      vf4 x = AMS ? x4[i] : zero, y = AMS ? x4[i + 256] : zero;
      const vf4 g = g4[i], h = g4[i + 256];
      upd4(p, g, m, v, x);
      upd4(q, h, n, w, y);
      p4[i] = p; m4[i] = m; v4[i] = v;
      p4[i + 256] = q; m4[i + 256] = n; v4[i + 256] = w;
      if (AMS) { x4[i] = x; x4[i + 256] = y; }
    }
    for (; i < n4; i += 256) {
      vf4 p = p4[i], m = m4[i], v = v4[i];
      vf4 x = AMS ? x4[i] : zero;
      const vf4 g = g4[i];
      upd4(p, g, m, v, x);
      p4[i] = p; m4[i] = m; v4[i] = v;
      if (AMS) x4[i] = x;
    }
    i0 = n4 << 2;
  }
  gf1* __restrict__ p1 = (gf1*)ch.p; const gf1* __restrict__ g1 = (const gf1*)ch.g;
  gf1* __restrict__ m1 = (gf1*)ch.m; gf1* __restrict__ v1 = (gf1*)ch.v; gf1* __restrict__ x1 = (gf1*)ch.vmax;
  for (long i = i0 + threadIdx.x; i < ch.n; i += 256) {
    float p = p1[i], m = m1[i], v = v1[i], x = AMS ? x1[i] : 0.f;
    upd(p, g1[i], m, v, x);
    p1[i] = p; m1[i] = m; v1[i] = v;
    if (AMS) x1[i] = x;
  }
}
__global__ void cm_step_inc_kernel(int* step_dev) { step_dev[0] += 1; }
extern "C" int ssv_adam_ex_multi(const ssv_adam_ex_chunk* chunks, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                                 int amsgrad, int step, int* step_dev, ssv_stream_t stream) {
  SSV_CHECK(chunks && nchunks > 0 && (step_dev || step > 0), SSV_BAD_SHAPE, "adam_ex_multi: nchunks=%d step=%d", nchunks, step);
  SSV_CHECK(weight_decay >= 0.f && (amsgrad == 0 || amsgrad == 1), SSV_BAD_SHAPE, "adam_ex_multi: weight_decay=%g amsgrad=%d", weight_decay, amsgrad);
  hipStream_t st = (hipStream_t)stream;
  if (amsgrad)
    hipLaunchKernelGGL(adam_ex_multi_kernel<true>, dim3(nchunks), dim3(256), 0, st, chunks, lr, beta1, beta2, eps, weight_decay, step, (const int*)step_dev);
  else
    hipLaunchKernelGGL(adam_ex_multi_kernel<false>, dim3(nchunks), dim3(256), 0, st, chunks, lr, beta1, beta2, eps, weight_decay, step, (const int*)step_dev);
  SSV_TRY(ssv_check_launch("adam_ex_multi"));
  if (step_dev) {
    hipLaunchKernelGGL(cm_step_inc_kernel, dim3(1), dim3(1), 0, st, step_dev);
    return ssv_check_launch("step_inc");
  }
  return 0;
}
