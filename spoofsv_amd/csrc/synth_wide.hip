// Wide column-incremental synthesis step (models/TTSModel.py:275-300 as driven by generate_test_utterances.py:98-139), gfx950.
//
// The column step of synth.hip is built for a handful of items: fp32 dot products, one output row per wave, a workgroup per item in
// the LayerNorm / gate / attention kernels.  Here the batch is the long axis.  Step activations are CHANNEL-MAJOR, (C, Bw) with the
// items contiguous and Bw = the batch rounded up to the 32-column tile (pad columns hold zeros) -- the operand layout of the
// convolution kernels with L := Bw -- so a layer of the step is a matrix product over the batch on the MFMA units, in the arithmetic
// mode of ssv_set_precision, reading the resident pre-split weight planes as they are.  A workgroup owns ALL output rows of its 32
// columns (as gemm_pwln_kernel does), so bias, LayerNorm, activation or highway gate and the store happen in its epilogue: one launch
// per layer.  The three taps of a causal k = 3 layer are three K segments that come from three different column buffers, frames
// t - 2d, t - d of the layer's input history (Tmax, C, Bw) and the current column, addressed from the device-side frame counter.
// split-fp16: the operand scale is the power of two of the workgroup's own tile (its 32 columns of all segments, scanned once before
// the product), so no scale lists travel between the layers and an item's rounding depends only on the items of its 32-column tile.
#include "bf3_common.h"
#include "ssv_host.h"

#define WD_BN 32                      // columns per workgroup
#define WD_LDT (WD_BN + 1)            // row pitch of the fp32 pre-activation tile in LDS
#define WD_MAXM 512                   // output rows a workgroup can own (8 waves x 4 row blocks x 16)
#define WD_EPS 1e-5f

struct WideArgs {
  const unsigned short* Ahi; const unsigned short* Alo; const float* a_inv;    // split modes: resident planes of the (M, Cin, KT) weight
  const float* w;                                                              // exact fp32 mode: the weight itself
  const float* bias;                  // M
  const float* add;                   // (M, Bw) per-item term added before the LayerNorm, or null
  const float* cur;                   // (Cin, Bw): the last K segment
  float* hist;                        // (Tmax, Cin, Bw) or null (KT = 1)
  const int* t_dev; int Tmax, dil;
  const float* g1; const float* b1; const float* g2; const float* b2;
  float* out;                         // highway: (M / 2, Bw); link: (M, Bw)
  int M, Cin, KT, B, Bw, act, hw;
};

__device__ __forceinline__ float wd_sigmoid(float v) { return 1.f / (1.f + __expf(-v)); }

// MODE 0: v_mfma_f32_16x16x4_f32 on the fp32 weight; 1: split-bf16 planes; 2: split-fp16 planes.  WMB: 16-row blocks per wave.
template <int MODE, int WMB>
__global__ __launch_bounds__(512) void wide_link_kernel(const WideArgs p) {
  constexpr int F16 = MODE == 2;
  __shared__ uint4 stage[2][2 * 4 * WD_BN];               // per chunk of 32 channels: hi [k-group][column], lo likewise (fp32 mode: [channel][column] floats)
  __shared__ float tile[WMB * 128 * WD_LDT];
  __shared__ float red[2][16][WD_BN];
  __shared__ float amx[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, nq = lane & 15;
  const int n0 = blockIdx.x * WD_BN;
  const int M = p.M, Cin = p.Cin, KT = p.KT, Bw = p.Bw;
  const int MB = (M + 15) >> 4, NCH = (Cin + 31) >> 5, G = KT * NCH;
  const int t = p.t_dev ? p.t_dev[0] : 0;
  // the K segments' column buffers (null: a tap before frame 0, or outside the history -- reads as zero)
  const float* seg[3] = {nullptr, nullptr, nullptr};
  for (int j = 0; j < KT; ++j) {
    if (j == KT - 1) seg[j] = p.cur;
    else {
      const int col = t - (KT - 1 - j) * p.dil;
      if (col >= 0 && col < p.Tmax) seg[j] = p.hist + (long)col * Cin * Bw;
    }
  }
  float* hcol = (p.hist && t >= 0 && t < p.Tmax) ? p.hist + (long)t * Cin * Bw : nullptr;

  float xs = 1.f, xinv = 1.f;
  if constexpr (F16) {
    float am = 0.f;
    for (int j = 0; j < KT; ++j) {
      const float* s = seg[j];
      if (!s) continue;
      for (int c = tid >> 5; c < Cin; c += 16) am = fmaxf(am, fabsf(s[(long)c * Bw + n0 + (tid & 31)]));
    }
    am = ssv_wg_max<8>(am, amx);
    float sc, inv;
    ssv_pow2_scale(am, sc, inv);
    xs = ssv_uniform(sc); xinv = ssv_uniform(inv);
  }

  f32x4 acc[WMB][2];
#pragma unroll
  for (int i = 0; i < WMB; ++i) { acc[i][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[i][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  uint4 Ah_[2][WMB], Al_[2][WMB];                        // fp32 mode: the 8 weights of a lane per row block, in the two registers
  float rx[8];
  const bool stager = tid < 4 * WD_BN;
  const int skg = (tid >> 5) & 3, scol = tid & 31;
  const uint4* Hp = reinterpret_cast<const uint4*>(p.Ahi);
  const uint4* Lp = reinterpret_cast<const uint4*>(p.Alo);

  auto prefetchX = [&](int g) __attribute__((always_inline)) {
    const int j = g / NCH, ch = g - j * NCH;
    const float* s = seg[j];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = ch * 32 + skg * 8 + i;
      rx[i] = (stager && s && c < Cin) ? s[(long)c * Bw + n0 + scol] : 0.f;
    }
    if (stager && j == KT - 1 && hcol) {                 // the layer's input column is filed in its history
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = ch * 32 + skg * 8 + i;
        if (c < Cin) hcol[(long)c * Bw + n0 + scol] = rx[i];
      }
    }
  };
  auto loadA = [&](auto setc, int g) __attribute__((always_inline)) {
    constexpr int set = decltype(setc)::value;
    const int j = g / NCH, ch = g - j * NCH;
#pragma unroll
    for (int i = 0; i < WMB; ++i) {
      const int mb = min(wave * WMB + i, MB - 1);
      if constexpr (MODE == 0) {
        const int m = mb * 16 + nq;
        float a[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int c = ch * 32 + 4 * s + kq;
          a[s] = (m < M && c < Cin) ? p.w[((long)m * Cin + c) * KT + j] : 0.f;
        }
        Ah_[set][i] = make_uint4(__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3]));
        Al_[set][i] = make_uint4(__float_as_uint(a[4]), __float_as_uint(a[5]), __float_as_uint(a[6]), __float_as_uint(a[7]));
      } else {
        const long o = (((long)j * MB + mb) * NCH + ch) * 64 + lane;
        Ah_[set][i] = Hp[o]; Al_[set][i] = Lp[o];
      }
    }
  };
  auto commitX = [&](int g) __attribute__((always_inline)) {
    if (!stager) return;
    if constexpr (MODE == 0) {
      float* sf = reinterpret_cast<float*>(stage[g & 1]);
#pragma unroll
      for (int i = 0; i < 8; ++i) sf[(skg * 8 + i) * WD_BN + scol] = rx[i];
    } else {
      uint4 h, l;
      split8s<F16>(rx, xs, h, l);
      stage[g & 1][tid] = h; stage[g & 1][4 * WD_BN + tid] = l;
    }
  };
  auto mma = [&](auto setc, int g) __attribute__((always_inline)) {
    constexpr int set = decltype(setc)::value;
    if constexpr (MODE == 0) {
      const float* sf = reinterpret_cast<const float*>(stage[g & 1]);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float b0 = sf[(4 * s + kq) * WD_BN + nq], b1 = sf[(4 * s + kq) * WD_BN + 16 + nq];
#pragma unroll
        for (int i = 0; i < WMB; ++i) {
          const uint4 q = s < 4 ? Ah_[set][i] : Al_[set][i];
          const unsigned u = (s & 3) == 0 ? q.x : (s & 3) == 1 ? q.y : (s & 3) == 2 ? q.z : q.w;
          const float a = __uint_as_float(u);
          acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[i][0], 0, 0, 0);
          acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[i][1], 0, 0, 0);
        }
      }
    } else {
      const uint4* Xh = stage[g & 1];
      const uint4* Xl = stage[g & 1] + 4 * WD_BN;
      uint4 bh[2], bl[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) { const int s_ = kq * WD_BN + c * 16 + nq; bh[c] = Xh[s_]; bl[c] = Xl[s_]; }
#pragma unroll
      for (int i = 0; i < WMB; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          acc[i][c] = mma16<F16>(Al_[set][i], bh[c], acc[i][c]);
          acc[i][c] = mma16<F16>(Ah_[set][i], bl[c], acc[i][c]);
          acc[i][c] = mma16<F16>(Ah_[set][i], bh[c], acc[i][c]);
        }
    }
  };
  typedef std::integral_constant<int, 0> S0;
  typedef std::integral_constant<int, 1> S1;
  // chunk g: its input values (prefetched into rx) are split into image g & 1; behind the barrier the next chunk's loads are
  // issued, then this chunk's MFMAs run.  Image g & 1 is written again two chunks later, behind the barrier of chunk g + 1, which
  // every wave reaches only after its reads of chunk g.
  prefetchX(0);
  loadA(S0{}, 0);
  for (int g = 0; g < G; g += 2) {
    commitX(g);
    __syncthreads();
    if (g + 1 < G) { prefetchX(g + 1); loadA(S1{}, g + 1); }
    mma(S0{}, g);
    if (g + 1 < G) {
      commitX(g + 1);
      __syncthreads();
      if (g + 2 < G) { prefetchX(g + 2); loadA(S0{}, g + 2); }
      mma(S1{}, g + 1);
    }
  }

  // ---- epilogue: pre-activations -> LDS tile, LayerNorm over the rows of every column (two-pass), activation or gate, store
  const float us = F16 ? ssv_uniform(xinv * p.a_inv[0]) : 1.f;
#pragma unroll
  for (int i = 0; i < WMB; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (wave * WMB + i) * 16 + kq * 4 + r;
      if (row < M) {
        const float bv = p.bias ? p.bias[row] : 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float v = acc[i][c][r] * us + bv;
          if (p.add) v += p.add[(long)row * Bw + n0 + c * 16 + nq];
          tile[row * WD_LDT + c * 16 + nq] = v;
        }
      }
    }
  __syncthreads();
  const int col = tid & 31, rg = tid >> 5;
  const int NH = p.hw ? 2 : 1, Ch = p.hw ? M / 2 : M;
  const float invC = 1.f / (float)Ch;
  float mu[2] = {0.f, 0.f}, rs[2] = {0.f, 0.f};
  for (int h = 0; h < NH; ++h) {
    float s = 0.f;
    for (int rr = rg; rr < Ch; rr += 16) s += tile[(h * Ch + rr) * WD_LDT + col];
    red[h][rg][col] = s;
  }
  __syncthreads();
  for (int h = 0; h < NH; ++h) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[h][k][col];
    mu[h] = s * invC;
  }
  __syncthreads();
  for (int h = 0; h < NH; ++h) {
    float s = 0.f;
    for (int rr = rg; rr < Ch; rr += 16) { const float d = tile[(h * Ch + rr) * WD_LDT + col] - mu[h]; s += d * d; }
    red[h][rg][col] = s;
  }
  __syncthreads();
  for (int h = 0; h < NH; ++h) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[h][k][col];
    rs[h] = rsqrtf(s * invC + WD_EPS);
  }
  const bool live = n0 + col < p.B;                      // pad columns are written as zeros
  for (int rr = rg; rr < Ch; rr += 16) {
    float y;
    const float n1 = (tile[rr * WD_LDT + col] - mu[0]) * rs[0] * p.g1[rr] + p.b1[rr];
    if (p.hw) {
      const float n2 = (tile[(Ch + rr) * WD_LDT + col] - mu[1]) * rs[1] * p.g2[rr] + p.b2[rr];
      const float sg = wd_sigmoid(n1);
      y = sg * n2 + (1.f - sg) * p.cur[(long)rr * Bw + n0 + col];
    } else {
      y = n1;
      if (p.act == 1) y = fmaxf(y, 0.f);
      else if (p.act == 2) y = wd_sigmoid(y);
    }
    p.out[(long)rr * Bw + n0 + col] = live ? y : 0.f;
  }
}

static int wide_launch(const WideArgs& a, const char* what, hipStream_t st) {
  const int mode = ssv_precision();
  const int wmb = a.M <= 128 ? 1 : (a.M <= 256 ? 2 : 4);
  const dim3 grid(a.Bw / WD_BN), block(512);
#define WD_GO(MODE_, W_) if (mode == MODE_ && wmb == W_) { hipLaunchKernelGGL((wide_link_kernel<MODE_, W_>), grid, block, 0, st, a); return ssv_check_launch(what); }
  WD_GO(0, 1) WD_GO(0, 2) WD_GO(0, 4) WD_GO(1, 1) WD_GO(1, 2) WD_GO(1, 4) WD_GO(2, 1) WD_GO(2, 2) WD_GO(2, 4)
#undef WD_GO
  return ssv_fail(SSV_UNSUPPORTED, "%s: no instantiation for %d rows in mode %d", what, a.M, mode);
}
static int wide_weights(WideArgs& a, const float* w, const void* w_packed, int M, int Cin, int k, const char* what) {
  a.w = w;
  a.Ahi = a.Alo = nullptr; a.a_inv = nullptr;
  if (ssv_precision() == 0) return 0;
  SSV_CHECK(w_packed, SSV_BAD_SHAPE, "%s: the split-MFMA modes read the weight's resident planes (w_packed is null)", what);
  const SplitPlanes pl = packed_planes(w_packed, M, Cin, k).fwd;
  a.Ahi = pl.hi; a.Alo = pl.lo; a.a_inv = pl.inv;
  return 0;
}

extern "C" int ssv_column_wide_tile(void) { return WD_BN; }

extern "C" int ssv_column_highway_wide(const float* w, const void* w_packed, const float* bias, const float* g1, const float* b1, const float* g2,
                                       const float* b2, const float* cur, float* hist, int Tmax, const int* t_dev, int dilation, float* out,
                                       int B, int Bw, int C, int k, ssv_stream_t stream) {
  SSV_CHECK(w && bias && g1 && b1 && g2 && b2 && cur && hist && t_dev && out, SSV_BAD_SHAPE, "column_highway_wide: null argument");
  SSV_CHECK(B > 0 && Bw >= B && C > 0 && Tmax > 0 && dilation > 0, SSV_BAD_SHAPE, "column_highway_wide: bad shape B=%d Bw=%d C=%d Tmax=%d dilation=%d", B, Bw, C, Tmax, dilation);
  SSV_CHECK(k == 3, SSV_UNSUPPORTED, "column_highway_wide: kernel size %d (causal kernel size 3 only)", k);
  SSV_CHECK(C % 8 == 0 && 2 * C <= WD_MAXM, SSV_UNSUPPORTED, "column_highway_wide: C = %d must be a multiple of 8 (whole staging slots), at most %d", C, WD_MAXM / 2);
  SSV_CHECK(Bw % WD_BN == 0, SSV_UNSUPPORTED, "column_highway_wide: Bw = %d must be a multiple of the column tile (%d)", Bw, WD_BN);
  SSV_CHECK(out != cur, SSV_BAD_SHAPE, "column_highway_wide: the output column must not be the input column");
  WideArgs a;
  SSV_TRY(wide_weights(a, w, w_packed, 2 * C, C, 3, "column_highway_wide"));
  a.bias = bias; a.add = nullptr; a.cur = cur; a.hist = hist; a.t_dev = t_dev; a.Tmax = Tmax; a.dil = dilation;
  a.g1 = g1; a.b1 = b1; a.g2 = g2; a.b2 = b2; a.out = out;
  a.M = 2 * C; a.Cin = C; a.KT = 3; a.B = B; a.Bw = Bw; a.act = 0; a.hw = 1;
  return wide_launch(a, "column_highway_wide", (hipStream_t)stream);
}

extern "C" int ssv_column_pwln_wide(const float* x, const float* w, const void* w_packed, const float* bias, const float* s, const float* gamma,
                                    const float* beta, float* y, int B, int Bw, int Cin, int Cout, int act, ssv_stream_t stream) {
  SSV_CHECK(x && w && bias && gamma && beta && y, SSV_BAD_SHAPE, "column_pwln_wide: null argument");
  SSV_CHECK(B > 0 && Bw >= B && Cin > 0 && Cout > 0 && act >= 0 && act <= 2, SSV_BAD_SHAPE, "column_pwln_wide: bad shape B=%d Bw=%d Cin=%d Cout=%d act=%d", B, Bw, Cin, Cout, act);
  SSV_CHECK(Cout <= WD_MAXM && Cin <= 4096, SSV_UNSUPPORTED, "column_pwln_wide: %d -> %d channels (at most 4096 -> %d)", Cin, Cout, WD_MAXM);
  SSV_CHECK(Bw % WD_BN == 0, SSV_UNSUPPORTED, "column_pwln_wide: Bw = %d must be a multiple of the column tile (%d)", Bw, WD_BN);
  SSV_CHECK(y != x, SSV_BAD_SHAPE, "column_pwln_wide: the output column must not be the input column");
  WideArgs a;
  SSV_TRY(wide_weights(a, w, w_packed, Cout, Cin, 1, "column_pwln_wide"));
  a.bias = bias; a.add = s; a.cur = x; a.hist = nullptr; a.t_dev = nullptr; a.Tmax = 0; a.dil = 1;
  a.g1 = gamma; a.b1 = beta; a.g2 = nullptr; a.b2 = nullptr; a.out = y;
  a.M = Cout; a.Cin = Cin; a.KT = 1; a.B = B; a.Bw = Bw; a.act = act; a.hw = 0;
  return wide_launch(a, "column_pwln_wide", (hipStream_t)stream);
}

// ---- attention for one new frame (models/TTSModel.py:281-295) with q and [r ; q] in the wide layout -------------------------------
// The arithmetic of attention_column_kernel (synth.hip), operation for operation -- the arg-max path has to agree with the reference
// bit for bit -- with the item's query read from column b of q (d, Bw) into LDS first and rq (2d, Bw) written by column.  K | V may be
// shared: item b reads text b % U of kv (U, 2d, N).
#define WACOL_MAXN 1024
#define WACOL_MAXD 1024
__global__ __launch_bounds__(256) void attention_column_wide_kernel(const float* __restrict__ kv, long kv_bs, int U, const float* __restrict__ q,
                                                                    int64_t* __restrict__ pma, float* __restrict__ a, int a_T,
                                                                    const int* __restrict__ t_dev, float* __restrict__ rq, int Bw, int d, int N, float scale) {
  __shared__ float logit[WACOL_MAXN];
  __shared__ float part[4][WACOL_MAXN];
  __shared__ float qs[WACOL_MAXD];
  __shared__ float red[4];
  __shared__ int redi[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = t_dev[0];
  const float* kb = kv + (long)(b % U) * kv_bs;
  const float* vb = kb + (long)d * N;
  const int64_t p0 = pma[b];
  for (int c = tid; c < d; c += 256) qs[c] = q[(long)c * Bw + b];
  __syncthreads();
  {
    const int c0 = (int)((long)wave * d / 4), c1 = (int)((long)(wave + 1) * d / 4);
    for (int n = lane; n < N; n += 64) {
      float s0 = 0.f, s1 = 0.f;
      int c = c0;
      for (; c + 1 < c1; c += 2) { s0 = fmaf(kb[(long)c * N + n], qs[c], s0); s1 = fmaf(kb[(long)(c + 1) * N + n], qs[c + 1], s1); }
      if (c < c1) s0 = fmaf(kb[(long)c * N + n], qs[c], s0);
      part[wave][n] = s0 + s1;
    }
  }
  __syncthreads();
  for (int n = tid; n < N; n += 256) {
    float s = ((part[0][n] + part[1][n]) + (part[2][n] + part[3][n])) * scale;
    if (n < p0 || n >= p0 + 3) s = -4294967296.f;
    logit[n] = s;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int n = tid; n < N; n += 256) mx = fmaxf(mx, logit[n]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int n = tid; n < N; n += 256) { const float e = expf(logit[n] - mx); logit[n] = e; sum += e; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  sum = (red[0] + red[1]) + (red[2] + red[3]);
  const float inv = 1.f / sum;
  float best = -1.f; int bi = N;
  for (int n = tid; n < N; n += 256) {
    const float pr = logit[n] * inv;
    logit[n] = pr;
    if (col >= 0 && col < a_T) a[((long)b * N + n) * a_T + col] = pr;
    if (pr > best) { best = pr; bi = n; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  __syncthreads();
  if (lane == 0) { red[wave] = best; redi[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (red[w] > best || (red[w] == best && redi[w] < bi)) { best = red[w]; bi = redi[w]; }
    pma[b] = bi;
  }
  __syncthreads();
  for (int c = tid; c < d; c += 256) {
    const float* vr = vb + (long)c * N;
    float s0 = 0.f, s1 = 0.f;
    int n = 0;
    for (; n + 1 < N; n += 2) { s0 = fmaf(vr[n], logit[n], s0); s1 = fmaf(vr[n + 1], logit[n + 1], s1); }
    if (n < N) s0 = fmaf(vr[n], logit[n], s0);
    rq[(long)c * Bw + b] = s0 + s1;
  }
  for (int c = tid; c < d; c += 256) rq[(long)(d + c) * Bw + b] = qs[c];
}

extern "C" int ssv_attention_column_wide(const float* kv, long kv_bs, int U, const float* q, int64_t* pma, float* a, int a_T, const int* t_dev,
                                         float* rq, int B, int Bw, int d, int N, ssv_stream_t stream) {
  SSV_CHECK(kv && q && pma && a && t_dev && rq, SSV_BAD_SHAPE, "attention_column_wide: null argument");
  SSV_CHECK(B > 0 && Bw >= B && d > 0 && N > 0 && a_T > 0 && kv_bs >= 2L * d * N, SSV_BAD_SHAPE, "attention_column_wide: bad shape B=%d Bw=%d d=%d N=%d", B, Bw, d, N);
  SSV_CHECK(U > 0 && B % U == 0, SSV_BAD_SHAPE, "attention_column_wide: %d items do not divide into %d shared texts", B, U);
  SSV_CHECK(N <= WACOL_MAXN && d <= WACOL_MAXD, SSV_UNSUPPORTED, "attention_column_wide: N=%d d=%d (at most %d, %d)", N, d, WACOL_MAXN, WACOL_MAXD);
  hipLaunchKernelGGL(attention_column_wide_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, kv, kv_bs, U, q, pma, a, a_T, t_dev, rq, Bw, d, N,
                     1.f / sqrtf((float)d));
  return ssv_check_launch("attention_column_wide");
}

// ---- end of a step: frame t of Y (T, F, Bw) = y_cur (F, Bw), mel_cur = y_cur (the next step's input column), t += 1 ----------------
__global__ __launch_bounds__(256) void synth_wide_feed_kernel(const float* __restrict__ y_cur, float* __restrict__ Y, float* __restrict__ mel_cur,
                                                              const int* __restrict__ t_dev, long n, int T) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = t_dev[0];
  if (i < n) {
    const float v = y_cur[i];
    if (t >= 0 && t < T) Y[(long)t * n + i] = v;
    mel_cur[i] = v;
  }
}
__global__ void synth_wide_inc_kernel(int* t_dev) { t_dev[0] += 1; }
extern "C" int ssv_synth_column_advance_wide(const float* y_cur, float* Y, float* mel_cur, int* t_dev, int Bw, int F, int T, ssv_stream_t stream) {
  SSV_CHECK(y_cur && Y && mel_cur && t_dev && Bw > 0 && F > 0 && T > 0, SSV_BAD_SHAPE, "synth_column_advance_wide: bad argument");
  const long n = (long)F * Bw;
  hipLaunchKernelGGL(synth_wide_feed_kernel, dim3(ssv_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, y_cur, Y, mel_cur, (const int*)t_dev, n, T);
  SSV_TRY(ssv_check_launch("synth_wide_feed"));
  hipLaunchKernelGGL(synth_wide_inc_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t_dev);
  return ssv_check_launch("synth_wide_inc");
}
