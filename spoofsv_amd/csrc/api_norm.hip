// Host layer (see api.hip), LayerNorm module: LayerNorm over channels, the 1x1 conv + LayerNorm links, the highwayConv blocks, and
// their second-order entries (gradient penalty through the critics).  No kernel here.
#include "ssv_host.h"

// ---- LayerNorm over channels ------------------------------------------------------------------------
extern "C" size_t ssv_channel_ln_act_fwd_workspace(int B, int C, int L) { (void)B; (void)C; (void)L; return 256; }   // none needed; kept in the ABI
extern "C" int ssv_channel_ln_act_fwd(const float* x, long x_bs, const float* gamma, const float* beta, float* y, long y_bs, float* y_amax, float* stats,
                                      int B, int C, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(x && gamma && beta && y && B > 0 && C > 0 && L > 0 && act >= 0 && act <= 2, SSV_BAD_SHAPE, "channel_ln_act_fwd: bad argument");
  SSV_CHECK(B <= 65535, SSV_UNSUPPORTED, "channel_ln_act_fwd: batch %d exceeds grid.y", B);
  (void)ws; (void)ws_bytes;
  return ssv_launch_ln_act_fwd(x, x_bs, gamma, beta, y, y_bs, stats, B, C, L, act, (hipStream_t)stream, y_amax);
}
// bytes of `rows_per_block` rows of C partial sums for every block a LayerNorm backward launch may write (one region: the whole workspace
// of the LayerNorm-only entries, the `part` region of the links')
static size_t ln_part_bytes(int B, int C, int L, int rows_per_block) { return align256((size_t)ssv_ln_gate_bwd_nblk(B, L) * rows_per_block * C * sizeof(float)); }
extern "C" size_t ssv_channel_ln_act_bwd_workspace(int B, int C, int L) { return ln_part_bytes(B, C, L, 3); }
extern "C" int ssv_channel_ln_act_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* stats, const float* gamma, const float* beta,
                                      float* dx, long dx_bs, float* pgrads, int B, int C, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dy && x && stats && gamma && beta && dx && B > 0 && C > 0 && L > 0 && act >= 0 && act <= 2, SSV_BAD_SHAPE, "channel_ln_act_bwd: bad argument");   // pgrads may be NULL
  SSV_CHECK(ws && ws_bytes >= ssv_channel_ln_act_bwd_workspace(B, C, L), SSV_BAD_SHAPE, "channel_ln_act_bwd: workspace too small");
  return ssv_launch_ln_act_bwd(dy, dy_bs, x, x_bs, stats, gamma, beta, dx, dx_bs, (float*)ws, pgrads, B, C, L, act, (hipStream_t)stream);
}

// ---- 1x1 conv + LayerNorm (+ activation), forward ---------------------------------------------------------------------------
// y = act(LN(conv1x1(x) + bias [+ s])) with pre = the LayerNorm's input and stats (B,2,L) = mean / rstd per column kept for the backward.
// One launch (gemm_pwln_kernel: a workgroup owns all output rows of its column tile and finishes the LayerNorm from its accumulators)
// where that form is the faster one in-step, else the product followed by the LayerNorm kernel -- same results up to summation order.
// (round 4, in-step and same box, fused against product + LayerNorm kernel: 513 x 1300 139.8 against 111.7 + 43.6 us; M = 256 / N = 325 29.1 against 19.5 + 12.5;
//  M = 512 / N = 186 33.9 against 29.1 + ~13; M = 512 / N = 1300 90.9 against 70.2 + 24: the fused form everywhere the split-MFMA kernels run)
static bool pwln_fused(int B, int Cin, int Cout, int L) { return use_bf3(B, L, Cin, Cout) && Cout <= 640 && B <= 65535; }
extern "C" size_t ssv_pointwise_conv_ln_act_fwd_workspace(int Cin, int Cout) { return conv_fwd_ws(Cin, Cout, 1).total; }
extern "C" int ssv_pointwise_conv_ln_act_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                                             const float* s, const float* gamma, const float* beta, float* pre, float* stats, float* y, long y_bs, float* y_amax,
                                             int B, int Cin, int Cout, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(x && w && gamma && beta && pre && y && B > 0 && Cin > 0 && Cout > 0 && L > 0 && act >= 0 && act <= 2, SSV_BAD_SHAPE, "pointwise_conv_ln_act_fwd: bad argument");
  SSV_CHECK(x_bs >= (long)Cin * L && y_bs >= (long)Cout * L, SSV_BAD_SHAPE, "pointwise_conv_ln_act_fwd: batch stride smaller than C*L");
  if (pwln_fused(B, Cin, Cout, L) && y_bs == (long)Cout * L && (!y_amax || ssv_amax_rows_(L) >= ssv_cdiv(L, 64))) {
    const ConvWs l = conv_fwd_ws(Cin, Cout, 1);
    SSV_CHECK((w_packed && !(use_f16() && !x_amax)) || (ws && ws_bytes >= l.total), SSV_BAD_SHAPE, "pointwise_conv_ln_act_fwd: workspace too small");
    int shift[3] = {0, 0, 0};
    PwLnArgs pw = {gamma, beta, y, y_bs, stats, y_amax, ssv_amax_rows_(L), act};
    return conv_nn(x, x_bs, w, packed_planes(w_packed, Cout, Cin, 1).fwd, (long)Cin, 1, bias, s, nullptr, 0, pre, (long)Cout * L, B, Cin, Cout, L, 1, shift, true,
                   ws, l, (hipStream_t)stream, x_amax, x_namax, nullptr, &pw);
  }
  SSV_TRY(ssv_conv1d_fwd(x, x_bs, x_amax, x_namax, w, w_packed, bias, s, pre, (long)Cout * L, nullptr, B, Cin, Cout, L, 1, 1, 0, ws, ws_bytes, stream));
  return ssv_channel_ln_act_fwd(pre, (long)Cout * L, gamma, beta, y, y_bs, y_amax, stats, B, Cout, L, act, nullptr, 0, stream);
}

// ---- highwayConv ---------------------------------------------------------------------------------------
// Column statistics of h come out of the conv kernel's epilogue (64-row groups) when the split-MFMA kernel runs and the two
// halves are whole groups; the LayerNorm / gate forward is then a streaming kernel without reductions (norm.hip).
static inline bool hw_colstats(int B, int C, int L) { return use_bf3(B, L, C, 2 * C) && C % 64 == 0 && C <= 512; }
// the convolution's workspace, then (where they are computed) the column statistics
struct HwFwdWs { ConvWs conv; size_t colstats, total; };
static HwFwdWs hw_fwd_ws(int B, int C, int L, int k) {
  HwFwdWs l;
  l.conv = conv_fwd_ws(C, 2 * C, k);
  WsTake t;
  t.take(l.conv.total);
  l.colstats = t.take(hw_colstats(B, C, L) ? (size_t)B * (2 * C / 64) * L * 2 * sizeof(float) : 0);
  l.total = t.off;
  return l;
}
extern "C" size_t ssv_highway_conv1d_fwd_workspace(int B, int C, int L, int k) { return hw_fwd_ws(B, C, L, k).total; }
extern "C" int ssv_highway_conv1d_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                                      const float* g1, const float* b1, const float* g2, const float* b2, float* h, float* stats, float* y, long y_bs,
                                      float* y_amax, int B, int C, int L, int k, int dilation, int causal, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(x && w && g1 && b1 && g2 && b2 && h && y, SSV_BAD_SHAPE, "highway_conv1d_fwd: null argument");
  SSV_CHECK(B > 0 && C > 0 && L > 0 && B <= 65535, SSV_BAD_SHAPE, "highway_conv1d_fwd: bad shape B=%d C=%d L=%d", B, C, L);
  if (hw_colstats(B, C, L)) {
    const HwFwdWs l = hw_fwd_ws(B, C, L, k);
    SSV_CHECK(ws && ws_bytes >= l.total, SSV_BAD_SHAPE, "highway_conv1d_fwd: workspace too small");
    SSV_CHECK(x_bs >= (long)C * L && y_bs >= (long)C * L, SSV_BAD_SHAPE, "highway_conv1d_fwd: batch stride smaller than C*L");
    float* cs = ws_f32(ws, l.colstats);
    int shift[3];
    SSV_TRY(conv_shifts(k, dilation, causal, shift));
    SSV_TRY(conv_nn(x, x_bs, w, packed_planes(w_packed, 2 * C, C, k).fwd, (long)C * k, k, bias, nullptr, nullptr, 0, h, (long)2 * C * L, B, C, 2 * C, L, k, shift, true,
                    ws, l.conv, (hipStream_t)stream, x_amax, x_namax, cs));
    return ssv_launch_ln_gate_fwd_stream(h, x, x_bs, cs, g1, b1, g2, b2, y, y_bs, stats, y_amax, B, C, L, (hipStream_t)stream);
  }
  SSV_TRY(ssv_conv1d_fwd(x, x_bs, x_amax, x_namax, w, w_packed, bias, nullptr, h, (long)2 * C * L, nullptr, B, C, 2 * C, L, k, dilation, causal, ws, ws_bytes, stream));
  return ssv_launch_ln_gate_fwd(h, (long)2 * C * L, x, x_bs, g1, b1, g2, b2, y, y_bs, stats, B, C, L, (hipStream_t)stream, y_amax);
}

// ---- 1x1 conv + LayerNorm (+ activation), whole backward ------------------------------------------------------------------
// y = act(LN(conv1x1(x) [+ s])) -- models/TTSModel.py:128-131, :173-180, :218-231, :343-361.  One entry for the backward so that
// the LayerNorm partial rows and the weight-gradient slabs are summed by ONE launch (as in ssv_highway_conv1d_bwd).
// LayerNorm / activation backward + the k = 1 data gradient of a link: ONE launch (round 5, pwln_bwd_kernel) when the transposed weight's planes
// are resident and the shape fits, else ln_act_bwd*, then the data-gradient GEMM.  dpre (B, Cout, L) dense; part: ssv_ln_act_bwd_rows rows.
static int pw_bwd_ln_and_data(const float* dy, long dy_bs, const float* w, const void* w_packed, const float* gamma, const float* beta, const float* pre,
                              const float* stats, float* dx, long dx_bs, float* dpre, float* dpre_amax, float* part, int B, int Cin, int Cout, int L, int act,
                              void* ws, size_t ws_bytes, ssv_stream_t stream) {
  const long pbs = (long)Cout * L;
  if (dx && w_packed && use_bf3(B, L, Cout, Cin) && (!use_f16() || dpre_amax) && ssv_pwln_bwd_fused_ok(B, Cin, Cout, L)) {
    const bool has_amax = dpre_amax != nullptr;
    const SplitPlanes pl = packed_planes(w_packed, Cout, Cin, 1).tr;
    PwLnBw q;
    q.dy = dy; q.dy_bs = dy_bs; q.pre = pre; q.stats = stats; q.gamma = gamma; q.beta = beta;
    q.dpre = dpre; q.part = part; q.part_rows = ssv_ln_act_bwd_rows(1, Cout, L, has_amax); q.part_q = 4 / ssv_ln_act_bwd_vec(Cout, L, has_amax);
    q.amax = dpre_amax; q.namax = ssv_amax_rows_(L);
    q.Ahi = pl.hi; q.Alo = pl.lo; q.a_inv = pl.inv;
    q.dx = dx; q.dx_bs = dx_bs;
    q.xrow_w = (Cin > 128 && Cin % 128 == 1) ? w + (Cin - 1) : nullptr; q.xrow_sk = Cin;       // w[o][Cin - 1], o < Cout
    q.M = Cout; q.Cin = Cin; q.L = L; q.act = act;
    return ssv_launch_pwln_bwd(q, B, use_f16() ? 1 : 0, (hipStream_t)stream);
  }
  SSV_TRY(ssv_launch_ln_act_bwd(dy, dy_bs, pre, pbs, stats, gamma, beta, dpre, pbs, part, nullptr, B, Cout, L, act, (hipStream_t)stream, dpre_amax));
  if (dx) SSV_TRY(ssv_conv1d_bwd_data(dpre, pbs, dpre_amax, ssv_amax_rows_(L), w, w_packed, nullptr, dx, dx_bs, B, Cin, Cout, L, 1, 1, 0, ws, ws_bytes, stream));
  return 0;
}
// Workspace of the whole backward of a link or a highway block: the gradient at the LayerNorm's input (B, rows, L), the LayerNorm's partial rows,
// max |that gradient| per LayerNorm tile (split-fp16 scales), the workspaces of the data gradient and of the weight gradient
struct LinkBwdWs { size_t dpre, part, amax, data, data_bytes, wgrad, wgrad_bytes, total; };
static LinkBwdWs link_bwd_ws(int B, int Cin, int Cout, int L, int k) {
  WsTake t;
  LinkBwdWs l;
  l.dpre = t.take((size_t)B * Cout * L * sizeof(float));
  l.part = t.take(ln_part_bytes(B, Cout, L, 3));                     // 3 rows of Cout per block (a highway block's 6 rows of C: Cout = 2 C)
  l.amax = t.take((size_t)B * ssv_amax_rows_(L) * sizeof(float));
  l.data_bytes = ssv_conv1d_bwd_data_workspace(Cin, Cout, k);
  l.data = t.take(l.data_bytes);
  l.wgrad_bytes = ssv_conv1d_bwd_weight_workspace(B, Cin, Cout, L, k);
  l.wgrad = t.take(l.wgrad_bytes);
  l.total = t.off;
  return l;
}
static LinkBwdWs pw_ws(int B, int Cin, int Cout, int L) { return link_bwd_ws(B, Cin, Cout, L, 1); }
static LinkBwdWs hw_ws(int B, int C, int L, int k) { return link_bwd_ws(B, C, 2 * C, L, k); }                     // dH has 2 C rows
extern "C" size_t ssv_pointwise_conv_ln_act_bwd_workspace(int B, int Cin, int Cout, int L) { return pw_ws(B, Cin, Cout, L).total; }
extern "C" int ssv_pointwise_conv_ln_act_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* x_amax, int x_namax, const float* w,
                                             const void* w_packed, const float* gamma,
                                             const float* beta, const float* pre, const float* stats, float* dx, long dx_bs, float* dw, float* pgrads,
                                             float* ds, int B, int Cin, int Cout, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dy && x && w && gamma && beta && pre && stats && dw && pgrads, SSV_BAD_SHAPE, "pointwise_conv_ln_act_bwd: null argument");
  SSV_CHECK(B > 0 && B <= 65535 && Cin > 0 && Cout > 0 && L > 0 && act >= 0 && act <= 2, SSV_BAD_SHAPE, "pointwise_conv_ln_act_bwd: bad shape");
  const LinkBwdWs s = pw_ws(B, Cin, Cout, L);
  SSV_CHECK(ws && ws_bytes >= s.total, SSV_BAD_SHAPE, "pointwise_conv_ln_act_bwd: workspace too small (%zu < %zu)", ws_bytes, s.total);
  float* dpre = ws_f32(ws, s.dpre);
  const long pbs = (long)Cout * L;
  float* da = use_f16() ? ws_f32(ws, s.amax) : nullptr;
  const int dn = ssv_amax_rows_(L);
  SSV_TRY(pw_bwd_ln_and_data(dy, dy_bs, w, w_packed, gamma, beta, pre, stats, dx, dx_bs, dpre, da, ws_f32(ws, s.part), B, Cin, Cout, L, act,
                             ws_f32(ws, s.data), s.data_bytes, stream));
  if (ds) SSV_TRY(ssv_rowsum(dpre, pbs, ds, B, Cout, L, stream));               // gradient of the broadcast (B, Cout, 1) term
  return conv1d_bwd_weight_impl(dpre, pbs, x, x_bs, dw, B, Cin, Cout, L, 1, 1, 0, ws_f32(ws, s.wgrad), s.wgrad_bytes, stream,
                                ws_f32(ws, s.part), pgrads, 3 * Cout, ssv_ln_act_bwd_rows(B, Cout, L, da != nullptr), da, dn, x_amax, x_namax);
}

// ---- second order (gradient penalty through the critics) and the gate forward alone ------------------------------------
extern "C" size_t ssv_channel_ln_bwd2_workspace(int B, int C, int L) { return ln_part_bytes(B, C, L, 1); }
extern "C" int ssv_channel_ln_bwd2(const float* v, long v_bs, const float* gn, long gn_bs, const float* x, long x_bs, const float* stats,
                                   const float* gamma, float* d_gn, long dgn_bs, float* d_x, long dx_bs, float* dgamma,
                                   int B, int C, int L, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(v && gn && x && stats && gamma && d_gn && d_x && dgamma && B > 0 && B <= 65535 && C > 0 && L > 0, SSV_BAD_SHAPE, "channel_ln_bwd2: bad argument");
  SSV_CHECK(ws && ws_bytes >= ssv_channel_ln_bwd2_workspace(B, C, L), SSV_BAD_SHAPE, "channel_ln_bwd2: workspace too small");
  return ssv_launch_ln_bwd2(v, v_bs, gn, gn_bs, x, x_bs, stats, gamma, d_gn, dgn_bs, d_x, dx_bs, (float*)ws, dgamma, B, C, L, (hipStream_t)stream);
}
extern "C" int ssv_highway_gate_fwd(const float* h, const float* x, long x_bs, const float* g1, const float* b1, const float* g2, const float* b2,
                                    float* stats, float* y, long y_bs, float* y_amax, int B, int C, int L, ssv_stream_t stream) {
  SSV_CHECK(h && x && g1 && b1 && g2 && b2 && y && B > 0 && B <= 65535 && C > 0 && L > 0, SSV_BAD_SHAPE, "highway_gate_fwd: bad argument");
  return ssv_launch_ln_gate_fwd(h, (long)2 * C * L, x, x_bs, g1, b1, g2, b2, y, y_bs, stats, B, C, L, (hipStream_t)stream, y_amax);
}
extern "C" size_t ssv_highway_gate_bwd2_workspace(int B, int C, int L) { return ln_part_bytes(B, C, L, 4); }
extern "C" int ssv_highway_gate_bwd2(const float* vh, const float* vx, long vx_bs, const float* gy, long gy_bs, const float* h, const float* x, long x_bs,
                                     const float* stats, const float* g1, const float* b1, const float* g2, const float* b2,
                                     float* d_gy, long dgy_bs, float* d_h, float* d_x, long dx_bs, float* pgrads,
                                     int B, int C, int L, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(vh && vx && gy && h && x && stats && g1 && b1 && g2 && b2 && d_gy && d_h && d_x && pgrads && B > 0 && B <= 65535 && C > 0 && L > 0,
            SSV_BAD_SHAPE, "highway_gate_bwd2: bad argument");
  SSV_CHECK(ws && ws_bytes >= ssv_highway_gate_bwd2_workspace(B, C, L), SSV_BAD_SHAPE, "highway_gate_bwd2: workspace too small");
  return ssv_launch_ln_gate_bwd2(vh, vx, vx_bs, gy, gy_bs, h, x, x_bs, stats, g1, b1, g2, b2, d_gy, dgy_bs, d_h, d_x, dx_bs, (float*)ws, pgrads,
                                 B, C, L, (hipStream_t)stream);
}

// ---- highway gate alone (building block: lets a caller overlap the two conv gradients on different streams) ---------------
extern "C" size_t ssv_highway_gate_bwd_workspace(int B, int C, int L) { return ln_part_bytes(B, C, L, 6); }
extern "C" int ssv_highway_gate_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* g1, const float* b1,
                                    const float* g2, const float* b2, const float* h, const float* stats, float* dh, float* dxres,
                                    long dx_bs, float* pgrads, int B, int C, int L, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dy && x && g1 && b1 && g2 && b2 && h && stats && dh && dxres && B > 0 && C > 0 && L > 0 && B <= 65535, SSV_BAD_SHAPE, "highway_gate_bwd: bad argument");   // pgrads may be NULL
  SSV_CHECK(ws && ws_bytes >= ssv_highway_gate_bwd_workspace(B, C, L), SSV_BAD_SHAPE, "highway_gate_bwd: workspace too small");
  return ssv_launch_ln_gate_bwd(dy, dy_bs, h, x, x_bs, stats, g1, b1, g2, b2, dh, dxres, dx_bs, (float*)ws, pgrads, B, C, L, (hipStream_t)stream);
}

extern "C" size_t ssv_highway_conv1d_bwd_workspace(int B, int C, int L, int k) { return hw_ws(B, C, L, k).total; }
extern "C" int ssv_highway_conv1d_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed,
                                      const float* g1, const float* b1,
                                      const float* g2, const float* b2, const float* h, const float* stats, float* dx, long dx_bs, float* dw,
                                      float* pgrads, int B, int C, int L, int k, int dilation, int causal, void* ws, size_t ws_bytes,
                                      ssv_stream_t stream) {
  SSV_CHECK(dy && x && w && g1 && b1 && g2 && b2 && h && stats && dx && dw && pgrads, SSV_BAD_SHAPE, "highway_conv1d_bwd: null argument");
  SSV_CHECK(B > 0 && C > 0 && L > 0 && B <= 65535, SSV_BAD_SHAPE, "highway_conv1d_bwd: bad shape B=%d C=%d L=%d", B, C, L);
  const LinkBwdWs s = hw_ws(B, C, L, k);
  SSV_CHECK(ws && ws_bytes >= s.total, SSV_BAD_SHAPE, "highway_conv1d_bwd: workspace too small (%zu < %zu)", ws_bytes, s.total);
  float* dH = ws_f32(ws, s.dpre);
  // gate + both LayerNorms backward: dH (B,2C,L), the residual-path gradient dy*(1-g) into dx, parameter partials
  // (its partial rows are summed at the end, by the launch that also sums the weight-gradient slabs)
  float* da = use_f16() ? ws_f32(ws, s.amax) : nullptr;
  const int dn = ssv_amax_rows_(L);
  SSV_TRY(ssv_launch_ln_gate_bwd(dy, dy_bs, h, x, x_bs, stats, g1, b1, g2, b2, dH, dx, dx_bs, ws_f32(ws, s.part), nullptr, B, C, L, (hipStream_t)stream, da));
  // dx += conv^T(dH)
  SSV_TRY(ssv_conv1d_bwd_data(dH, (long)2 * C * L, da, dn, w, w_packed, dx, dx, dx_bs, B, C, 2 * C, L, k, dilation, causal, ws_f32(ws, s.data), s.data_bytes, stream));
  return conv1d_bwd_weight_impl(dH, (long)2 * C * L, x, x_bs, dw, B, C, 2 * C, L, k, dilation, causal, ws_f32(ws, s.wgrad), s.wgrad_bytes, stream,
                                ws_f32(ws, s.part), pgrads, 6 * C, ssv_ln_gate_bwd_rows(B, C, L, da != nullptr), da, dn, x_amax, x_namax);
}

extern "C" int ssv_ln_partial_rows(int B, int L) { return ssv_ln_gate_bwd_nblk(B, L); }
extern "C" int ssv_ln_bwd_partial_rows(int gate, int B, int C, int L, int with_amax) {
  return gate ? ssv_ln_gate_bwd_rows(B, C, L, with_amax != 0) : ssv_ln_act_bwd_rows(B, C, L, with_amax != 0);
}
extern "C" size_t ssv_highway_conv1d_bwd_data_workspace(int B, int C, int L, int k) { (void)B; (void)L; return ssv_conv1d_bwd_data_workspace(C, 2 * C, k); }
extern "C" int ssv_highway_conv1d_bwd_data(const float* dy, long dy_bs, const float* x, long x_bs, const float* w, const void* w_packed,
                                           const float* g1, const float* b1, const float* g2, const float* b2, const float* h, const float* stats,
                                           float* dx, long dx_bs, float* dh, float* dh_amax, float* part, int B, int C, int L, int k, int dilation, int causal,
                                           void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dy && x && w && g1 && b1 && g2 && b2 && h && stats && dx && dh && part, SSV_BAD_SHAPE, "highway_conv1d_bwd_data: null argument");
  SSV_CHECK(B > 0 && C > 0 && L > 0 && B <= 65535, SSV_BAD_SHAPE, "highway_conv1d_bwd_data: bad shape B=%d C=%d L=%d", B, C, L);
  SSV_TRY(ssv_launch_ln_gate_bwd(dy, dy_bs, h, x, x_bs, stats, g1, b1, g2, b2, dh, dx, dx_bs, part, nullptr, B, C, L, (hipStream_t)stream, dh_amax));
  return ssv_conv1d_bwd_data(dh, (long)2 * C * L, dh_amax, ssv_amax_rows_(L), w, w_packed, dx, dx, dx_bs, B, C, 2 * C, L, k, dilation, causal, ws, ws_bytes, stream);
}
extern "C" size_t ssv_pointwise_conv_ln_act_bwd_data_workspace(int B, int Cin, int Cout, int L) { (void)B; (void)L; return ssv_conv1d_bwd_data_workspace(Cin, Cout, 1); }
extern "C" int ssv_pointwise_conv_ln_act_bwd_data(const float* dy, long dy_bs, const float* w, const void* w_packed, const float* gamma, const float* beta,
                                                  const float* pre, const float* stats, float* dx, long dx_bs, float* ds, float* dpre, float* dpre_amax,
                                                  float* part, int B, int Cin, int Cout, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dy && w && gamma && beta && pre && stats && dpre && part, SSV_BAD_SHAPE, "pointwise_conv_ln_act_bwd_data: null argument");
  SSV_CHECK(B > 0 && B <= 65535 && Cin > 0 && Cout > 0 && L > 0 && act >= 0 && act <= 2, SSV_BAD_SHAPE, "pointwise_conv_ln_act_bwd_data: bad shape");
  const long pbs = (long)Cout * L;
  SSV_TRY(pw_bwd_ln_and_data(dy, dy_bs, w, w_packed, gamma, beta, pre, stats, dx, dx_bs, dpre, dpre_amax, part, B, Cin, Cout, L, act, ws, ws_bytes, stream));
  if (ds) SSV_TRY(ssv_rowsum(dpre, pbs, ds, B, Cout, L, stream));
  return 0;
}
