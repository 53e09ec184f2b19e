// Host layer (see api.hip), GE2E speaker embedder: the LSTM forward (inference, cached weights, training), the projection + L2 norm,
// and backpropagation through time.  No kernel here.
#include "ssv_host.h"

// ---- GE2E speaker embedder ---------------------------------------------------------------------------------
// Layer-by-layer paths: input frames [T][F][Bn], a layer's input projection [T][4H][Bn], the sequences of two layers (ping-pong), gates and
// cell state of one frame, the pre-split weights of one layer (hi, lo planes)
struct LstmWs { size_t xt, xp, seq0, seq1, g, c, wih, whh, total; };
static LstmWs lstm_ws(int Bn, int T, int F, int H) {
  WsTake t;
  LstmWs s;
  s.xt = t.take((size_t)T * F * Bn * sizeof(float));
  s.xp = t.take((size_t)T * 4 * H * Bn * sizeof(float));
  s.seq0 = t.take((size_t)T * H * Bn * sizeof(float));
  s.seq1 = t.take((size_t)T * H * Bn * sizeof(float));
  s.g = t.take((size_t)4 * H * Bn * sizeof(float));
  s.c = t.take((size_t)H * Bn * sizeof(float));
  s.wih = t.take(2 * split_bytes(4 * H, F > H ? F : H, 1));
  s.whh = t.take(2 * split_bytes(4 * H, H, 1));
  s.total = t.off;
  return s;
}
// C = A X (+ bias + bias_b + R) with A (M x K) row-major weights and X, C as [rows][Bn] activations; "batch" of nb
// independent problems strided by sxb / scb.  fp32 MFMA path (the split-bf16 path is spelled out in ssv_lstm_fwd).
int lstm_gemm_f32(const float* A, const float* X, long sxb, float* C, long scb, const float* bias, const float* bias_b,
                         const float* R, int M, int K, int Bn, int nb, hipStream_t st) {
  GemmNN g;
  g.A = A; g.sam = K; g.sac = 1; g.saj = 1;
  g.X = X; g.sxb = sxb; g.sxc = Bn; g.Lx = Bn;
  g.C = C; g.scb = scb; g.scm = Bn;
  g.bias = bias; g.bias_b = bias_b; g.sbb = 0;
  if (R) { g.R = R; g.srm = Bn; }
  g.M = M; g.N = Bn; g.Kc = K; g.B = nb;
  return ssv_launch_gemm_nn(g, st);
}
// Wavefront (split-bf16) layout: h of every layer lives in a 2-frame ring, weights of layer l >= 1 are [W_ih | W_hh] side by side.
// split-fp16 scales of the wavefront (floats at `aux`): [0, 64) partial maxima over ALL weight matrices (one scale for every layer: a
// launch batches layers over grid.y and has one epilogue factor), [64] its inverse scale, [128, 192) partial maxima of the input frames
// (layer 0's projection).  The recurrent activations need no list: |h| = |o tanh c| < 1, their scale is the constant 2^14 (x_namax = 0).
#define LSTM_AUX_FLOATS 192
LstmWave lstm_wave_ws(int Bn, int T, int F, int H, int layers) {
  WsTake t;
  LstmWave s;
  s.xt = t.take((size_t)T * F * Bn * sizeof(float));
  s.xp = t.take((size_t)T * 4 * H * Bn * sizeof(float));
  s.out = t.take((size_t)layers * 2 * H * Bn * sizeof(float));
  s.c = t.take((size_t)layers * H * Bn * sizeof(float));
  s.bias = t.take((size_t)layers * 8 * H * sizeof(float));
  s.ih0 = t.take(2 * split_bytes(4 * H, F, 1));
  s.hh0 = t.take(2 * split_bytes(4 * H, H, 1));
  s.comb_stride = 2 * split_bytes(4 * H, 2 * H, 1);
  s.comb = t.take((size_t)(layers > 1 ? layers - 1 : 0) * s.comb_stride);
  s.aux = t.take(LSTM_AUX_FLOATS * sizeof(float));
  // pre-split recurrent activations (GemmNNB::hs_planes): hi and lo planes of [H / 8][npad][8 halves] per (layer, ring slot); npad = whole 128-column tiles
  s.npad = (Bn + 127) / 128 * 128;
  s.hp_plane = (H % 8 == 0) ? (size_t)(H / 8) * s.npad * 16 : 0;
  s.hp = t.take((size_t)layers * 2 * 2 * s.hp_plane);
  // layer 0's input as the first K segment of its product (GemmNNB::x0_planes): the planes of [W_ih (F padded to whole chunk pairs) | W_hh] and the
  // input frames pre-split, a (hi, lo) plane pair of the recurrent activations' size per frame (only its first 4 * xsplit0 k-groups are used)
  s.xsplit0 = 2 * ((F + 63) / 64);
  s.l0c = t.take(2 * split_bytes(4 * H, 32 * s.xsplit0 + H, 1));
  s.x0p = t.take((size_t)T * 2 * s.hp_plane);
  s.total = t.off;
  return s;
}
static bool lstm_wave_ok(int Bn, int H) { return Bn >= 64 && H >= 32 && H % 32 == 0; }
extern "C" size_t ssv_lstm_fwd_workspace(int Bn, int T, int F, int H, int layers) {
  return zmax(lstm_ws(Bn, T, F, H).total, lstm_wave_ws(Bn, T, F, H, layers).total);
}
// LSTM forward as a wavefront over (layer, frame): in step s layer l computes frame s - l, so the layers' recurrent products
// (each too small to fill the chip: 672 workgroups of 24 K-chunks) run side by side in ONE launch, and a layer's input
// projection rides along as the first K segment of the same product instead of a separate pass over all frames.
// T + layers - 1 steps of two launches (layer 0, whose input projection W_ih x_t is precomputed for all frames, and layers
// 1.. batched over grid.y) instead of layers * T sequential products.
// Training (keep != null): every frame of h, c and the activated gates is kept in the caller's buffers (D = T instead of the 2-frame ring).
int lstm_fwd_wave(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                  const float* const* b_hh, float* h_last, int Bn, int T, int F, int H, int layers, char* base, hipStream_t st,
                  float* keep_xt, float* keep_hs, float* keep_cs, float* keep_gates, bool packed) {
  const LstmWave s = lstm_wave_ws(Bn, T, F, H, layers);
  const int D = keep_hs ? T : 2;
  float* xt = keep_xt ? keep_xt : ws_f32(base, s.xt);
  float* xp = ws_f32(base, s.xp);
  float* out = keep_hs ? keep_hs : ws_f32(base, s.out);
  float* cbuf = keep_cs ? keep_cs : ws_f32(base, s.c);
  float* bias = ws_f32(base, s.bias);
  const long HN = (long)H * Bn;
  // Arithmetic of the products: split-fp16 in the default mode (the reference's nn.LSTM computes in fp32,
  // GE2E/speech_embedder_net.py:19,28), split-bf16 when that mode is selected.
  const bool f16 = use_f16() && 2 * layers <= 64;
  // One launch per wavefront step (SSV_LSTM_MERGE=0 keeps the two launches: tuning), and in the split-fp16 mode the cells write h already split into the
  // consumers' staging order (GemmNNB::hs_planes): no split, no masks and a quarter of the load instructions in the products' input staging.  The input
  // frames are then pre-split the same way and layer 0's W_ih x_t is the first K segment of its product (GemmNNB::x0_planes): no projection of all frames
  // (0.42 ms and 1.3 GB written, then read back by the cells, at config 5's shape).
  const char* mk = ssv_tuning(SSV_T_LSTM_MERGE);
  const bool merge = !(mk && atoi(mk) == 0);
  // (inference and the training forward alike -- every frame's h, c and gates kept: 36.0 -> 35.7 ms, small because the epilogue then writes them and the planes)
  const bool presplit = f16 && merge && layers >= 2 && H % 32 == 0 && s.hp_plane > 0 && s.hp_plane < ((size_t)1 << 31) && !(mk && atoi(mk) == 2);
  const bool x0fold = presplit && 4 * s.xsplit0 <= H / 8;
  if (!x0fold || keep_xt) SSV_TRY(ssv_launch_lstm_in_transpose(x, xt, Bn, T, F, st));    // [T][F][Bn]  (training keeps it for W_ih[0]'s gradient)
  // packed: the workspace still holds what a previous call of the same shape and arithmetic mode prepared from the SAME weight values -- bias
  // rows, split weight planes, the weights' scale (ssv_lstm_fwd_cached: d-vector extraction runs batch after batch on fixed weights; the six
  // absmax scans over 48 MB of weights and the six packs were ~0.35 ms of an 11.6 ms forward)
  for (int l = 0; !packed && l < layers; ++l) {                   // biases side by side: [layer][b_ih (4H) | b_hh (4H)]
    SSV_TRY(ssv_copy_rows(b_ih[l], 0, bias + (long)l * 8 * H, 0, 1, (long)4 * H, st));
    SSV_TRY(ssv_copy_rows(b_hh[l], 0, bias + (long)l * 8 * H + 4 * H, 0, 1, (long)4 * H, st));
  }
  // weights, rows gate-interleaved (row 4u + gate) so that the product can finish the cell in its epilogue
  unsigned short* ih0_hi = ws_u16(base, s.ih0);
  unsigned short* ih0_lo = ws_u16(base, s.ih0 + split_bytes(4 * H, F, 1));
  unsigned short* hh0_hi = ws_u16(base, s.hh0);
  unsigned short* hh0_lo = ws_u16(base, s.hh0 + split_bytes(4 * H, H, 1));
  unsigned short* l0c_hi = ws_u16(base, s.l0c);
  unsigned short* l0c_lo = ws_u16(base, s.l0c + split_bytes(4 * H, 32 * s.xsplit0 + H, 1));
  float* aux = ws_f32(base, s.aux);
  if (f16) {
    const int npb = 64 / (2 * layers);                            // partial maxima per weight matrix
    if (!packed) {
      SSV_TRY(ssv_launch_fill(aux, 0.f, LSTM_AUX_FLOATS, st));      // (a kernel, not a memset node: see ssv_lstm_bwd)
      for (int l = 0; l < layers; ++l) {
        SSV_TRY(ssv_launch_absmax(w_ih[l], 0, 1, (long)4 * H * (l == 0 ? F : H), aux + (2 * l) * npb, npb, st));
        SSV_TRY(ssv_launch_absmax(w_hh[l], 0, 1, (long)4 * H * H, aux + (2 * l + 1) * npb, npb, st));
      }
    }
    SSV_TRY(ssv_launch_absmax(x0fold ? x : xt, 0, 1, (long)T * F * Bn, aux + 128, 64, st));       // (writes all 64 entries of the input's list; the same values either way)
  }
  auto pack = [&](const float* w, unsigned short* hi, unsigned short* lo, int K, int Kpad, int nch_total, int ch_off) -> int {
    if (f16) return ssv_launch_pack_split_f16_list(w, hi, lo, 4 * H, K, Kpad, 1, K, 1, 1, H, aux, 64, aux + 64, st, nch_total, ch_off);
    return ssv_launch_pack_split(w, hi, lo, 4 * H, K, Kpad, 1, K, 1, 1, H, st, nch_total, ch_off);
  };
  const int hch = H / 32;
  if (!packed && !x0fold) {
    SSV_TRY(pack(w_ih[0], ih0_hi, ih0_lo, F, pad32(F), 0, 0));
    SSV_TRY(pack(w_hh[0], hh0_hi, hh0_lo, H, H, 0, 0));
  }
  if (!packed && x0fold) {                                       // [W_ih (zero-padded to xsplit0 chunks) | W_hh], one row of chunks per 16 output rows
    SSV_TRY(pack(w_ih[0], l0c_hi, l0c_lo, F, 32 * s.xsplit0, s.xsplit0 + hch, 0));
    SSV_TRY(pack(w_hh[0], l0c_hi, l0c_lo, H, H, s.xsplit0 + hch, s.xsplit0));
  }
  for (int l = 1; !packed && l < layers; ++l) {
    unsigned short* hi = ws_u16(base, s.comb + (size_t)(l - 1) * s.comb_stride);
    unsigned short* lo = (unsigned short*)((char*)hi + split_bytes(4 * H, 2 * H, 1));
    SSV_TRY(pack(w_ih[l], hi, lo, H, H, 2 * hch, 0));
    SSV_TRY(pack(w_hh[l], hi, lo, H, H, 2 * hch, hch));
  }
  // layer 0's input projection for every frame at once (biases are left to the cell): xp[t] = W_ih x_t
  if (x0fold) SSV_TRY(ssv_launch_lstm_x_planes(x, aux + 128, base + s.x0p, (long)s.hp_plane, Bn, T, F, 4 * s.xsplit0, s.npad, st));
  else {
    GemmNNB g;
    g.Ahi = ih0_hi; g.Alo = ih0_lo; g.Kpad = pad32(F); g.Kc = F;
    g.X = xt; g.sxb = (long)F * Bn; g.sxc = Bn; g.Lx = Bn;
    g.C = xp; g.scb = (long)4 * H * Bn; g.scm = Bn;
    g.M = 4 * H; g.N = Bn; g.B = T; g.perm_h = H;
    if (f16) { g.f16 = 1; g.a_inv = aux + 64; g.x_amax = aux + 128; g.x_namax = 64; g.x_amax_bs = 0; }
    SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
  }
  GemmNNB g;
  g.sxc = Bn; g.Lx = Bn; g.scm = Bn; g.srm = Bn;
  g.M = 4 * H; g.N = Bn; g.perm_h = H; g.epi = 1; g.cstate = cbuf;
  if (f16) { g.f16 = 1; g.a_inv = aux + 64; g.x_amax = nullptr; g.x_namax = 0; g.x_amax_bs = 0; }     // activations: |h| < 1, the fixed scale 2^14
  g.lstm_out = out; g.lstm_D = D; g.sbb = (long)8 * H; g.gates_out = keep_gates;
  g.X = out; g.C = out;                        // placeholders: the kernel derives X, X2 and C from (layer, frame)
  // One launch per wavefront step (round 5): layer 0 (K = H: its own h_{t-1}; the input projection xp[t] through R) rides in the launch of the
  // layers above it (K = 2 H) as entry 0.  Before, a step was two launches -- 336 workgroups with 24 chunks, then 672 with 48 -- each with a
  // half-empty last round; together they are 1008 workgroups = two full rounds of 512.  SSV_LSTM_MERGE=0 keeps the two launches (tuning).
  if (presplit) {
    SSV_TRY(ssv_launch_fill((float*)(base + s.hp), 0.f, (long)((size_t)layers * s.hp_plane), st));      // layers * 2 * 2 * hp_plane bytes
    g.hs_planes = ws_u16(base, s.hp); g.hs_plane_bytes = (long)s.hp_plane; g.hs_npad = s.npad;
  }
  for (int step = 0; merge && layers >= 2 && step < T + layers - 1; ++step) {
    g.lstm_s = step;
    g.hs_keep_h = !presplit || keep_hs || step == T + layers - 2;   // (pre-split h at inference: the fp32 copy is read by nobody but the caller, from the last step)
    const int lo = step - T + 1 > 0 ? step - T + 1 : 0, hi = step < layers - 1 ? step : layers - 1;
    const int lo1 = lo > 1 ? lo : 1;           // the first layer >= 1 of the launch: its planes are the launch's Ahi
    g.Ahi = ws_u16(base, s.comb + (size_t)(lo1 - 1) * s.comb_stride);
    g.Alo = (unsigned short*)((char*)g.Ahi + split_bytes(4 * H, 2 * H, 1));
    g.sab = (long)(s.comb_stride / sizeof(unsigned short));
    g.Kpad = 2 * H; g.Kc = 2 * H;
    g.xsplit = hch; g.lstm_lo = lo; g.B = hi - lo + 1;
    g.bias = bias + (long)lo * 8 * H; g.bias_b = g.bias + 4 * H;
    g.x0_planes = nullptr;
    if (lo == 0 && x0fold) {
      g.A0hi = l0c_hi; g.A0lo = l0c_lo; g.R = nullptr;
      g.x0_planes = ws_u16(base, s.x0p); g.x0_amax = aux + 128; g.xsplit0 = s.xsplit0;
    }
    else if (lo == 0) { g.A0hi = hh0_hi; g.A0lo = hh0_lo; g.R = xp + (long)step * 4 * H * Bn; g.srb = 0; }
    else { g.A0hi = g.A0lo = nullptr; g.R = nullptr; }
    SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
  }
  for (int step = 0; !(merge && layers >= 2) && step < T + layers - 1; ++step) {
    g.lstm_s = step;
    if (step < T) {                            // layer 0: gates = W_hh h_{t-1} + xp[t] + b
      g.Ahi = hh0_hi; g.Alo = hh0_lo; g.Kpad = H; g.Kc = H; g.sab = 0;
      g.xsplit = 0; g.lstm_lo = 0; g.B = 1;
      g.R = xp + (long)step * 4 * H * Bn;
      g.bias = bias; g.bias_b = bias + 4 * H;
      SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
    }
    const int lo = step - T + 1 > 1 ? step - T + 1 : 1, hi = step < layers - 1 ? step : layers - 1;
    if (lo <= hi) {                            // layers lo..hi: gates = [W_ih | W_hh] [h^{l-1}_t ; h^l_{t-1}] + b
      g.Ahi = ws_u16(base, s.comb + (size_t)(lo - 1) * s.comb_stride);
      g.Alo = (unsigned short*)((char*)g.Ahi + split_bytes(4 * H, 2 * H, 1));
      g.sab = (long)(s.comb_stride / sizeof(unsigned short));
      g.Kpad = 2 * H; g.Kc = 2 * H;
      g.xsplit = hch; g.lstm_lo = lo; g.B = hi - lo + 1;
      g.R = nullptr;
      g.bias = bias + (long)lo * 8 * H; g.bias_b = g.bias + 4 * H;
      SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
    }
  }
  (void)HN;
  return ssv_launch_transpose_out(out + ((long)(layers - 1) * D + (T - 1) % D) * H * Bn, h_last, H, Bn, st);
}

static int lstm_fwd_impl(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* h_last,
                         int Bn, int T, int F, int H, int layers, void* ws, size_t ws_bytes, ssv_stream_t stream, bool packed) {
  SSV_CHECK(x && w_ih && w_hh && b_ih && b_hh && h_last && Bn > 0 && T > 0 && F > 0 && H > 0 && layers > 0, SSV_BAD_SHAPE, "lstm_fwd: bad argument");
  SSV_CHECK(T <= 65535, SSV_UNSUPPORTED, "lstm_fwd: T=%d exceeds grid.y", T);
  const LstmWs s = lstm_ws(Bn, T, F, H);
  SSV_CHECK(ws && ws_bytes >= ssv_lstm_fwd_workspace(Bn, T, F, H, layers), SSV_BAD_SHAPE, "lstm_fwd: workspace too small (%zu < %zu)", ws_bytes,
            ssv_lstm_fwd_workspace(Bn, T, F, H, layers));
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  if (ssv_precision() >= 1 && lstm_wave_ok(Bn, H))
    return lstm_fwd_wave(x, w_ih, w_hh, b_ih, b_hh, h_last, Bn, T, F, H, layers, base, st, nullptr, nullptr, nullptr, nullptr, packed);
  // (the layer-by-layer paths below re-pack per layer into ONE buffer: nothing to keep)
  float* xt = ws_f32(base, s.xt);
  float* xp = ws_f32(base, s.xp);
  float* seq[2] = {ws_f32(base, s.seq0), ws_f32(base, s.seq1)};
  float* gbuf = ws_f32(base, s.g);
  float* cbuf = ws_f32(base, s.c);
  const bool bf3 = ssv_precision() >= 1 && Bn >= 64 && H >= 32;
  SSV_TRY(ssv_launch_lstm_in_transpose(x, xt, Bn, T, F, st));    // [T][F][Bn]
  if (bf3) SSV_TRY(ssv_launch_fill(gbuf, 0.f, (long)H * Bn, st));
  const float* in = xt;
  int Fin = F;
  float* out = nullptr;
  for (int l = 0; l < layers; ++l) {
    out = seq[l & 1];
    if (!bf3) {
      // input projection for every frame at once: xp[t] = W_ih in[t] + b_ih + b_hh    ("batch" = frame)
      SSV_TRY(lstm_gemm_f32(w_ih[l], in, (long)Fin * Bn, xp, (long)4 * H * Bn, b_ih[l], b_hh[l], nullptr, 4 * H, Fin, Bn, T, st));
      for (int t = 0; t < T; ++t) {
        const float* gates = xp + (long)t * 4 * H * Bn;
        if (t > 0) {  // gates = W_hh h_{t-1} + xp[t]
          SSV_TRY(lstm_gemm_f32(w_hh[l], out + (long)(t - 1) * H * Bn, 0, gbuf, 0, nullptr, nullptr, gates, 4 * H, H, Bn, 1, st));
          gates = gbuf;
        }
        SSV_TRY(ssv_launch_lstm_cell(gates, cbuf, out + (long)t * H * Bn, H, Bn, t == 0, st));
      }
    } else {
      // Split-bf16 path.  The layer's weights are used by T + 1 products: split them once, with the 4H output rows
      // re-ordered gate-interleaved (row 4u + gate) so that the recurrent product can finish the cell in its epilogue.
      unsigned short* ih_hi = ws_u16(base, s.wih);
      unsigned short* ih_lo = ws_u16(base, s.wih + split_bytes(4 * H, Fin, 1));
      unsigned short* hh_hi = ws_u16(base, s.whh);
      unsigned short* hh_lo = ws_u16(base, s.whh + split_bytes(4 * H, H, 1));
      SSV_TRY(ssv_launch_pack_split(w_ih[l], ih_hi, ih_lo, 4 * H, Fin, pad32(Fin), 1, Fin, 1, 1, H, st));
      SSV_TRY(ssv_launch_pack_split(w_hh[l], hh_hi, hh_lo, 4 * H, H, pad32(H), 1, H, 1, 1, H, st));
      GemmNNB g;
      g.X = in; g.sxb = (long)Fin * Bn; g.sxc = Bn; g.Lx = Bn;
      g.bias_b = nullptr; g.sbb = 0; g.R = nullptr; g.srb = 0; g.srm = Bn;
      g.M = 4 * H; g.N = Bn; g.KT = 1;
      g.shift[0] = g.shift[1] = g.shift[2] = 0;
      g.perm_h = H; g.first = 0; g.cstate = nullptr;
      // input projection for every frame at once, biases left to the cell: xp[t] = W_ih in[t]  (gate-interleaved rows)
      g.Ahi = ih_hi; g.Alo = ih_lo; g.Kpad = pad32(Fin); g.Kc = Fin;
      g.C = xp; g.scb = (long)4 * H * Bn; g.scm = Bn; g.bias = nullptr; g.B = T; g.epi = 0;
      SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
      // recurrent product with the cell finished in its epilogue: h_t, c_t from W_hh h_{t-1} + xp[t] + b_ih + b_hh.
      // t = 0 has no recurrent term; it runs the same kernel on an all-zero h_{-1} (gbuf, zeroed above; one product in T).
      g.Ahi = hh_hi; g.Alo = hh_lo; g.Kpad = pad32(H); g.Kc = H;
      g.sxb = 0; g.scb = 0; g.scm = Bn;
      g.bias = b_ih[l]; g.bias_b = b_hh[l]; g.sbb = 0;
      g.srb = 0; g.srm = Bn;
      g.B = 1; g.epi = 1; g.cstate = cbuf;
      for (int t = 0; t < T; ++t) {
        g.X = (t > 0) ? out + (long)(t - 1) * H * Bn : gbuf;
        g.C = out + (long)t * H * Bn;
        g.R = xp + (long)t * 4 * H * Bn;
        g.first = (t == 0);
        SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
      }
    }
    in = out;
    Fin = H;
  }
  return ssv_launch_transpose_out(out + (long)(T - 1) * H * Bn, h_last, H, Bn, st);
}
extern "C" int ssv_lstm_fwd(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                            const float* const* b_hh, float* h_last, int Bn, int T, int F, int H, int layers,
                            void* ws, size_t ws_bytes, ssv_stream_t stream) {
  return lstm_fwd_impl(x, w_ih, w_hh, b_ih, b_hh, h_last, Bn, T, F, H, layers, ws, ws_bytes, stream, false);
}
extern "C" int ssv_lstm_fwd_cached(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                   const float* const* b_hh, float* h_last, int Bn, int T, int F, int H, int layers,
                                   void* ws, size_t ws_bytes, int weights_packed, ssv_stream_t stream) {
  return lstm_fwd_impl(x, w_ih, w_hh, b_ih, b_hh, h_last, Bn, T, F, H, layers, ws, ws_bytes, stream, weights_packed != 0);
}

extern "C" size_t ssv_proj_l2norm_fwd_workspace(int Bn, int P) { return align256((size_t)Bn * P * sizeof(float)); }
extern "C" int ssv_proj_l2norm_fwd(const float* h, const float* w, const float* bias, float* e, float* norms, int Bn, int H, int P,
                                   void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(h && w && e && Bn > 0 && H > 0 && P > 0, SSV_BAD_SHAPE, "proj_l2norm_fwd: bad argument");
  SSV_CHECK(ws && ws_bytes >= ssv_proj_l2norm_fwd_workspace(Bn, P), SSV_BAD_SHAPE, "proj_l2norm_fwd: workspace too small");
  GemmNN g;                        // y[p][b] = sum_c w[p][c] h[b][c] + bias[p]
  g.A = w; g.sam = H; g.sac = 1; g.saj = 1;
  g.X = h; g.sxc = 1; g.sxn = H; g.Lx = Bn;
  g.C = (float*)ws; g.scm = Bn;
  g.bias = bias;
  g.M = P; g.N = Bn; g.Kc = H; g.B = 1;
  SSV_TRY(ssv_launch_gemm_nn(g, (hipStream_t)stream));
  return ssv_launch_l2norm_rows((const float*)ws, e, norms, P, Bn, (hipStream_t)stream);
}
// Backward of the above: dy = (de - e <e,de>) / |y|;  dh = dy W,  dW = dy^T h,  dbias = column sums of dy.
extern "C" size_t ssv_proj_l2norm_bwd_workspace(int Bn, int P) { return align256((size_t)Bn * P * sizeof(float)); }
extern "C" int ssv_proj_l2norm_bwd(const float* de, const float* e, const float* norms, const float* h, const float* w, float* dh, float* dw,
                                   float* dbias, int Bn, int H, int P, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(de && e && norms && h && w && dh && dw && dbias && Bn > 0 && H > 0 && P > 0, SSV_BAD_SHAPE, "proj_l2norm_bwd: bad argument");
  SSV_CHECK(ws && ws_bytes >= ssv_proj_l2norm_bwd_workspace(Bn, P), SSV_BAD_SHAPE, "proj_l2norm_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* dy = (float*)ws;                      // (Bn, P)
  SSV_TRY(ssv_launch_l2norm_bwd(de, e, norms, dy, P, Bn, st));
  SSV_TRY(ssv_launch_colsum(dy, dbias, P, Bn, st));
  GemmNN g;                        // dh (Bn,H): rows b, reduction over p
  g.A = dy; g.sam = P; g.sac = 1; g.saj = 1;
  g.X = w; g.sxc = H; g.Lx = H;
  g.C = dh; g.scm = H;
  g.M = Bn; g.N = H; g.Kc = P; g.B = 1;
  SSV_TRY(ssv_launch_gemm_nn(g, st));
  GemmNN q;                        // dW (P,H) = dy^T h: rows p, reduction over b
  q.A = dy; q.sam = 1; q.sac = P; q.saj = 1;
  q.X = h; q.sxc = H; q.Lx = H;
  q.C = dw; q.scm = H;
  q.M = P; q.N = H; q.Kc = Bn; q.B = 1;
  return ssv_launch_gemm_nn(q, st);
}
