// Host layer (see api.hip), GE2E speaker embedder, training: the LSTM forward that keeps every frame, and backpropagation through
// time (the forward's wavefront and its workspace layout are api_lstm.hip's).  No kernel here.
#include "ssv_host.h"

// ---- LSTM training: forward that keeps every frame, and backpropagation through time ------------------------------------
// saved (caller-owned, ssv_lstm_saved_bytes): xt [T][F][Bn] | hs [layers][T][H][Bn] | cs [layers][T][H][Bn] |
// gates [layers][T][4H][Bn] (activated i, f, g, o; torch row order).
struct LstmSaved { size_t xt, hs, cs, gates, total; };
static LstmSaved lstm_saved(int Bn, int T, int F, int H, int layers) {
  WsTake t;
  LstmSaved s;
  s.xt = t.take((size_t)T * F * Bn * sizeof(float));
  s.hs = t.take((size_t)layers * T * H * Bn * sizeof(float));
  s.cs = t.take((size_t)layers * T * H * Bn * sizeof(float));
  s.gates = t.take((size_t)layers * T * 4 * H * Bn * sizeof(float));
  s.total = t.off;
  return s;
}
extern "C" size_t ssv_lstm_saved_bytes(int Bn, int T, int F, int H, int layers) { return lstm_saved(Bn, T, F, H, layers).total; }
// The wavefront kernels exist in the split modes, for hidden sizes that are multiples of 32 and at least 8 utterances.  Everything else -- the
// exact-fp32 mode (ssv_set_precision(0)), any hidden size, any batch -- trains on the exact-fp32 MFMA GEMMs below: layer by layer and frame by
// frame (nn.LSTM + autograd of the reference have no such limits: GE2E/speech_embedder_net.py:19, GE2E/train_speech_embedder.py:82-86).
// Same saved-tensor layout, same cell backward kernel; only the products differ.
static bool lstm_train_split_ok(int Bn, int H) { return ssv_precision() >= 1 && H % 32 == 0 && Bn >= 8; }
static int lstm_train_fwd_f32(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih, const float* const* b_hh,
                              float* h_last, int Bn, int T, int F, int H, int layers, char* base, hipStream_t st,
                              float* xt, float* hs, float* cs, float* gates) {
  const LstmWave s = lstm_wave_ws(Bn, T, F, H, layers);
  float* xp = ws_f32(base, s.xp);                               // [T][4H][Bn]: the layer's input projection of every frame, biases included
  const long HN = (long)H * Bn;
  SSV_TRY(ssv_launch_lstm_in_transpose(x, xt, Bn, T, F, st));     // [T][F][Bn]
  for (int l = 0; l < layers; ++l) {
    const float* in = l == 0 ? xt : hs + (long)(l - 1) * T * HN;
    const int Fin = l == 0 ? F : H;
    SSV_TRY(lstm_gemm_f32(w_ih[l], in, (long)Fin * Bn, xp, 4 * HN, b_ih[l], b_hh[l], nullptr, 4 * H, Fin, Bn, T, st));
    for (int t = 0; t < T; ++t) {
      float* gt = gates + ((long)l * T + t) * 4 * HN;
      const float* pre = xp + (long)t * 4 * HN;
      if (t > 0) {                                                  // pre-activations = W_hh h_{t-1} + xp[t], into the saved slot (activated in place)
        SSV_TRY(lstm_gemm_f32(w_hh[l], hs + ((long)l * T + t - 1) * HN, 0, gt, 0, nullptr, nullptr, pre, 4 * H, H, Bn, 1, st));
        pre = gt;
      }
      SSV_TRY(ssv_launch_lstm_cell_train(pre, gt, t > 0 ? cs + ((long)l * T + t - 1) * HN : nullptr, cs + ((long)l * T + t) * HN,
                                         hs + ((long)l * T + t) * HN, H, Bn, st));
    }
  }
  return ssv_launch_transpose_out(hs + ((long)(layers - 1) * T + (T - 1)) * HN, h_last, H, Bn, st);
}
extern "C" size_t ssv_lstm_train_fwd_workspace(int Bn, int T, int F, int H, int layers) { return lstm_wave_ws(Bn, T, F, H, layers).total; }
extern "C" int ssv_lstm_train_fwd(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                  const float* const* b_hh, float* h_last, void* saved, int Bn, int T, int F, int H, int layers,
                                  void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(x && w_ih && w_hh && b_ih && b_hh && h_last && saved && Bn > 0 && T > 0 && F > 0 && H > 0 && layers > 0, SSV_BAD_SHAPE, "lstm_train_fwd: bad argument");
  SSV_CHECK(ws && ws_bytes >= ssv_lstm_train_fwd_workspace(Bn, T, F, H, layers), SSV_BAD_SHAPE, "lstm_train_fwd: workspace too small");
  const LstmSaved sv = lstm_saved(Bn, T, F, H, layers);
  char* sb = (char*)saved;
  if (!lstm_train_split_ok(Bn, H))
    return lstm_train_fwd_f32(x, w_ih, w_hh, b_ih, b_hh, h_last, Bn, T, F, H, layers, (char*)ws, (hipStream_t)stream,
                              ws_f32(sb, sv.xt), ws_f32(sb, sv.hs), ws_f32(sb, sv.cs), ws_f32(sb, sv.gates));
  return lstm_fwd_wave(x, w_ih, w_hh, b_ih, b_hh, h_last, Bn, T, F, H, layers, (char*)ws, (hipStream_t)stream,
                       ws_f32(sb, sv.xt), ws_f32(sb, sv.hs), ws_f32(sb, sv.cs), ws_f32(sb, sv.gates));
}

struct LstmBwdWs { size_t dgates, dxa, dxa_slab, dcarry, dhtop, rs, wta, wta_stride, cmax, aux, slabs, total; };
// split-fp16 scales of the backward (floats at `aux`): [0, 64) partial maxima of the weights of the data-gradient products (one scale for all
// layers, as in the forward), [64] its inverse scale, [128, 192) the input frames' list, [192] 1.0 -- the list of the recurrent activations
// (|h| < 1) --, then 64 entries per layer: that layer's dgates over all frames (the weight gradients' list), reduced from cmax.
#define LSTM_BWD_AUX_FLOATS(layers) (256 + 64 * (layers))
static size_t lstm_dw_slab_bytes(int Bn, int T, int H, int Fin) {
  return (size_t)dw_splits(T, 4 * H, Fin, 1, Bn) * 4 * H * Fin * sizeof(float);        // "batch" = frames, reduction length = utterances
}
// dxa: the data-gradient products of one reverse wavefront step, [K range z][step parity][layer][2H][Bn] -- layer l's product at frame t is
// [dh^{l-1}_t ; dh^l_{t-1}] (layer 0: only the second half is used), written at step s = l + t under parity s & 1 and read by the cells of step s - 1:
// two parities are the whole life of these values, so the buffer stays in the last-level cache instead of walking through T frames of HBM.
static LstmBwdWs lstm_bwd_ws(int Bn, int T, int F, int H, int layers) {
  WsTake t;
  LstmBwdWs s;
  s.dgates = t.take((size_t)layers * T * 4 * H * Bn * sizeof(float));
  s.dxa_slab = align256((size_t)2 * layers * 2 * H * Bn * sizeof(float));   // (a stride: one K range of dxa)
  s.dxa = t.take(2 * s.dxa_slab);
  s.dcarry = t.take((size_t)layers * H * Bn * sizeof(float));
  s.dhtop = t.take((size_t)H * Bn * sizeof(float));
  s.rs = t.take((size_t)layers * T * 4 * H * sizeof(float));       // the bias gradients' per-frame terms, [layer][frame][4H] (lstm_cell_bwd_kernel)
  s.wta_stride = 2 * split_bytes(2 * H, 4 * H, 1);                 // [W_ih | W_hh]^T of a layer (layer 0: the W_ih half stays zero)
  s.wta = t.take((size_t)layers * s.wta_stride);
  s.cmax = t.take((size_t)layers * T * H * sizeof(float));         // max |dgates| per (layer, frame, hidden unit), left by lstm_cell_bwd_kernel
  s.aux = t.take(LSTM_BWD_AUX_FLOATS(layers) * sizeof(float));
  // every (items, M, Nc) lstm_weight_grad is called with: W_ih over T frames (Fin = F or H), W_hh over T - 1
  s.slabs = t.take(zmax(zmax(lstm_dw_slab_bytes(Bn, T, H, H), lstm_dw_slab_bytes(Bn, T > 1 ? T - 1 : 1, H, H)), lstm_dw_slab_bytes(Bn, T, H, F)));
  s.total = t.off;
  return s;
}
extern "C" size_t ssv_lstm_bwd_workspace(int Bn, int T, int F, int H, int layers) { return lstm_bwd_ws(Bn, T, F, H, layers).total; }
// dW (M x Nc) = sum over `items` frames of A_item (M x Bn) X_item^T (Nc x Bn): the conv weight-gradient kernel with time = batch.
// al / xl (split-fp16): the operands' scale lists, one per operand over all frames; null in the other modes.
static int lstm_weight_grad(const float* A, long sab, const float* X, long sxb, float* dw, int M, int Nc, int Bn, int items, void* slabs, hipStream_t st,
                            bool f32 = false, const AmaxList* al = nullptr, const AmaxList* xl = nullptr) {
  GemmNT g;
  if (al && xl) { g.f16 = 1; g.a_amax = al->p; g.a_namax = al->n; g.x_amax = xl->p; g.x_namax = xl->n; }
  const int Z = dw_splits(items, M, Nc, 1, Bn);
  const long n = (long)M * Nc;
  g.A = A; g.sab = sab; g.sam = Bn; g.La = Bn;
  g.X = X; g.sxb = sxb; g.sxc = Bn; g.Lx = Bn;
  if (Z == 1) { g.C = dw; g.scz = n; g.scm = Nc; g.scc = 1; g.scj = 0; }
  else { g.C = (float*)slabs; g.scz = n; g.scm = Nc; g.scc = 1; g.scj = 0; }
  g.M = M; g.Nc = Nc; g.KT = 1; g.B = items; g.Z = Z; g.bstep = Z;
  if (f32) SSV_TRY(ssv_launch_gemm_nt(g, st));
  else {
    SSV_CHECK(ssv_nt_bf3_fits(g), SSV_UNSUPPORTED, "lstm_bwd: sequence buffers exceed the weight-gradient kernel's 32-bit offsets");
    SSV_TRY(ssv_launch_gemm_nt_bf3(g, st));
  }
  if (Z > 1) SSV_TRY(ssv_launch_reduce_slabs((const float*)slabs, dw, n, Z, n, st));
  return 0;
}
extern "C" int ssv_lstm_bwd(const float* dh_last, const void* saved, const float* const* w_ih, const float* const* w_hh,
                            float* const* dw_ih, float* const* dw_hh, float* const* db_ih, float* const* db_hh,
                            int Bn, int T, int F, int H, int layers, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dh_last && saved && w_ih && w_hh && dw_ih && dw_hh && db_ih && db_hh && Bn > 0 && T > 0 && F > 0 && H > 0 && layers > 0, SSV_BAD_SHAPE, "lstm_bwd: bad argument");
  const bool f32 = !lstm_train_split_ok(Bn, H);                    // the exact-fp32 products (see lstm_train_fwd_f32)
  // split-fp16 products in the default mode, as in the forward (lstm_fwd_wave; one weight scale for all layers: at most 32 of them), split-bf16 in its mode
  const bool f16 = !f32 && use_f16() && 2 * layers <= 64;
  const LstmBwdWs s = lstm_bwd_ws(Bn, T, F, H, layers);
  SSV_CHECK(ws && ws_bytes >= s.total, SSV_BAD_SHAPE, "lstm_bwd: workspace too small (%zu < %zu)", ws_bytes, s.total);
  hipStream_t st = (hipStream_t)stream;
  const LstmSaved sv = lstm_saved(Bn, T, F, H, layers);
  const char* sb = (const char*)saved;
  const float* xt = ws_f32(sb, sv.xt);
  const float* hs = ws_f32(sb, sv.hs);
  const float* cs = ws_f32(sb, sv.cs);
  const float* gates = ws_f32(sb, sv.gates);
  char* base = (char*)ws;
  float* dgates = ws_f32(base, s.dgates);
  float* dxa = ws_f32(base, s.dxa);
  float* dcarry = ws_f32(base, s.dcarry);
  float* dhtop = ws_f32(base, s.dhtop);
  float* rs = ws_f32(base, s.rs);
  float* cmax = f16 ? ws_f32(base, s.cmax) : nullptr;
  float* aux = ws_f32(base, s.aux);
  const long HN = (long)H * Bn;
  const long zstride = (long)(s.dxa_slab / sizeof(float));
  SSV_TRY(ssv_launch_transpose_out(dh_last, dhtop, Bn, H, st));               // (Bn, H) -> [H][Bn]
  // the transposed product dX [H][Bn] = W^T dG with W (4H x H) row-major, on the exact-fp32 kernel: A(m = q, c = r) = W[r][q]
  auto wt_gemm_f32 = [&](const float* W, const float* dg, float* out) -> int {
    GemmNN q;
    q.A = W; q.sam = 1; q.sac = H; q.saj = 1;
    q.X = dg; q.sxc = Bn; q.Lx = Bn;
    q.C = out; q.scm = Bn;
    q.M = H; q.N = Bn; q.Kc = 4 * H; q.B = 1;
    return ssv_launch_gemm_nn(q, st);
  };
  for (int step = T + layers - 2; f32 && step >= 0; --step) {
    const int lo = step - T + 1 > 0 ? step - T + 1 : 0, hi = step < layers - 1 ? step : layers - 1;
    SSV_TRY(ssv_launch_lstm_cell_bwd(gates, cs, dxa, zstride, 1, dhtop, dgates, dcarry, rs, nullptr, H, Bn, T, layers, step, lo, hi - lo + 1, st));
    float* outp = dxa + (long)(step & 1) * layers * 2 * HN;                   // this step's parity
    if (lo == 0 && step >= 1) SSV_TRY(wt_gemm_f32(w_hh[0], dgates + (long)step * 4 * HN, outp + HN));
    for (int l = lo > 1 ? lo : 1; l <= hi; ++l) {                            // [dh^{l-1}_t ; dh^l_{t-1}] = [W_ih | W_hh]^T dgates^l_t
      const float* dg = dgates + ((long)l * T + (step - l)) * 4 * HN;
      SSV_TRY(wt_gemm_f32(w_ih[l], dg, outp + (long)l * 2 * HN));
      SSV_TRY(wt_gemm_f32(w_hh[l], dg, outp + (long)l * 2 * HN + HN));
    }
  }
  // transposed weights for the data-gradient products: rows = inputs of the layer, reduction over the 4H gate rows
  const size_t rows_h = (size_t)(H / 16) * (4 * H / 32) * 512;               // elements of the first H rows of a [2H x 4H] plane
  if (f16) {                                                                 // the weights' partial maxima: W_ih[l >= 1] and W_hh[l] (layer 0's W_ih half is zero)
    const int npb = 64 / (2 * layers);
    // (zeroed by a kernel, as everything below that clears memory: a memset NODE of a captured iteration was seen to run out of order with the kernels around
    // it on the first replay of a process -- the maxima cleared after they were written, the planes split with a zero scale, layer 0's gradients zero)
    SSV_TRY(ssv_launch_fill(aux, 0.f, 64, st));
    for (int l = 0; l < layers; ++l) {
      if (l > 0) SSV_TRY(ssv_launch_absmax(w_ih[l], 0, 1, (long)4 * H * H, aux + (2 * l) * npb, npb, st));
      SSV_TRY(ssv_launch_absmax(w_hh[l], 0, 1, (long)4 * H * H, aux + (2 * l + 1) * npb, npb, st));
    }
  }
  auto pack_t = [&](const float* w, unsigned short* hi, unsigned short* lo) -> int {           // (m=q, k=r) = W[r][q]
    if (f16) return ssv_launch_pack_split_f16_list(w, hi, lo, H, 4 * H, 4 * H, 1, 1, H, 1, 0, aux, 64, aux + 64, st);
    return ssv_launch_pack_split(w, hi, lo, H, 4 * H, 4 * H, 1, 1, H, 1, 0, st);
  };
  for (int l = 0; !f32 && l < layers; ++l) {
    unsigned short* hi = ws_u16(base, s.wta + (size_t)l * s.wta_stride);
    unsigned short* lo = (unsigned short*)((char*)hi + split_bytes(2 * H, 4 * H, 1));
    if (l == 0) {                                                            // no data gradient of the utterance itself: zero rows (mostly skipped, see skip_rows)
      SSV_TRY(ssv_launch_fill((float*)hi, 0.f, (long)(rows_h / 2), st));           // rows_h is a multiple of 512 elements
      SSV_TRY(ssv_launch_fill((float*)lo, 0.f, (long)(rows_h / 2), st));
    } else SSV_TRY(pack_t(w_ih[l], hi, lo));
    SSV_TRY(pack_t(w_hh[l], hi + rows_h, lo + rows_h));
  }
  // ONE product launch per reverse wavefront step: every active layer (layer 0 included) x two K ranges of 2H gate rows, on the forward wavefront's
  // 128 x 128 tile -- 3 layers x 12 x 7 x 2 = 504 tiles less layer 0's 84 skipped ones for config 5 (before round 6's end: a 768-row and a 1536-row product
  // on 128 x 32 tiles, 47 + 87 us per step)
  GemmNNB g;
  g.Kpad = 4 * H; g.Kc = 2 * H; g.ksplit = 2; g.sxc = Bn; g.Lx = Bn; g.scm = Bn; g.N = Bn; g.M = 2 * H;
  g.sab = (long)(s.wta_stride / sizeof(unsigned short)); g.sxb = (long)(T - 1) * 4 * HN; g.scb = 2 * HN; g.scz = zstride;
  // split-fp16: item b (layer lo + b at frame step - lo - b) takes the H maxima its cells just left, at the same (T - 1)-frame stride as its dgates
  if (f16) { g.f16 = 1; g.a_inv = aux + 64; g.x_namax = H; g.x_amax_bs = (long)(T - 1) * H; }
  for (int step = T + layers - 2; !f32 && step >= 0; --step) {
    const int lo = step - T + 1 > 0 ? step - T + 1 : 0, hi = step < layers - 1 ? step : layers - 1;
    SSV_TRY(ssv_launch_lstm_cell_bwd(gates, cs, dxa, zstride, 2, dhtop, dgates, dcarry, rs, cmax, H, Bn, T, layers, step, lo, hi - lo + 1, st));
    if (step == 0) break;                                                    // frame 0 of layer 0: its product would be the gradient of the initial state
    g.Ahi = ws_u16(base, s.wta + (size_t)lo * s.wta_stride);
    g.Alo = (unsigned short*)((char*)g.Ahi + split_bytes(2 * H, 4 * H, 1));
    g.X = dgates + ((long)lo * T + (step - lo)) * 4 * HN;
    if (f16) g.x_amax = cmax + ((long)lo * T + (step - lo)) * H;
    g.C = dxa + ((long)(step & 1) * layers + lo) * 2 * HN;
    g.B = hi - lo + 1;
    g.skip_rows = lo == 0 ? H : 0;
    SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
  }
  // parameter gradients: one reduction over all frames per matrix
  // split-fp16 scale lists: the input frames' (one scan of xt), the recurrent activations' constant 1.0 (|h| < 1), a layer's dgates from its cells' maxima
  AmaxList xl = {nullptr, 0}, hl = {aux + 192, 1};
  if (f16) {
    SSV_TRY(ssv_launch_fill(aux + 192, 1.f, 1, st));
    SSV_TRY(amax_of(xt, 0, 1, (long)T * F * Bn, nullptr, 0, aux + 128, &xl, st));
  }
  for (int l = 0; l < layers; ++l) {
    const float* dg = dgates + (long)l * T * 4 * HN;
    const int Fin = l == 0 ? F : H;
    const float* in = l == 0 ? xt : hs + (long)(l - 1) * T * HN;
    AmaxList al = {nullptr, 0};
    if (f16) SSV_TRY(amax_of(cmax + (long)l * T * H, 0, 1, (long)T * H, nullptr, 0, aux + 256 + 64 * l, &al, st));
    SSV_TRY(lstm_weight_grad(dg, 4 * HN, in, (long)Fin * Bn, dw_ih[l], 4 * H, Fin, Bn, T, base + s.slabs, st, f32, f16 ? &al : nullptr, l == 0 ? &xl : &hl));
    if (T > 1) SSV_TRY(lstm_weight_grad(dg + 4 * HN, 4 * HN, hs + (long)l * T * HN, HN, dw_hh[l], 4 * H, H, Bn, T - 1, base + s.slabs, st, f32, f16 ? &al : nullptr, &hl));
    else SSV_TRY(ssv_launch_fill(dw_hh[l], 0.f, (long)4 * H * H, st));
    SSV_TRY(ssv_launch_reduce_slabs(rs + (long)l * T * 4 * H, db_ih[l], 4 * H, T, 4 * H, st));      // sum over frames of sum_b dgates[l][t][r][b] (the cell kernel's row sums)
    SSV_TRY(ssv_copy_rows(db_ih[l], 0, db_hh[l], 0, 1, (long)4 * H, st));
  }
  return 0;
}
