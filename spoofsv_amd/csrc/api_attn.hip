// Host layer (see api.hip), attention module: the guided attention of Text2Mel, forward (plain, with the decoder's cat(R, Q), length-masked)
// and backward.  No kernel here.
#include "ssv_host.h"

// ---- attention -------------------------------------------------------------------------------------------
extern "C" int ssv_attention_apply(const float* v, long kv_bs, const float* a, int a_T, float* r, long r_bs, int B, int d, int N, int T, ssv_stream_t stream) {
  SSV_CHECK(v && a && r && B > 0 && d > 0 && N > 0 && T > 0 && a_T >= T, SSV_BAD_SHAPE, "attention_apply: bad argument");
  GemmNN g;
  g.A = v; g.sab = kv_bs; g.sam = N; g.sac = 1; g.saj = 0;
  g.X = a; g.sxb = (long)N * a_T; g.sxc = a_T; g.Lx = T;
  g.C = r; g.scb = r_bs; g.scm = T;
  g.M = d; g.N = T; g.Kc = N; g.B = B;
  return ssv_launch_gemm_nn(g, (hipStream_t)stream);
}
extern "C" int ssv_attention_train_fwd(const float* k, const float* v, long kv_bs, const float* q, long q_bs, float* a, float* r, long r_bs,
                                       int B, int d, int N, int T, ssv_stream_t stream) {
  SSV_CHECK(k && v && q && a && r && B > 0 && d > 0 && N > 0 && T > 0, SSV_BAD_SHAPE, "attention_train_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (ssv_attn_fused_ok(B, d, N, T)) return ssv_launch_attn_fwd_fused(k, v, kv_bs, q, q_bs, a, r, r_bs, 0, B, d, N, T, st);
  GemmNN g;                       // scores(b,n,t) = sum_c k(b,c,n) q(b,c,t) / sqrt(d)
  g.A = k; g.sab = kv_bs; g.sam = 1; g.sac = N; g.saj = 0;
  g.X = q; g.sxb = q_bs; g.sxc = T; g.Lx = T;
  g.C = a; g.scb = (long)N * T; g.scm = T;
  g.M = N; g.N = T; g.Kc = d; g.B = B; g.alpha = 1.f / sqrtf((float)d);
  SSV_TRY(ssv_launch_gemm_nn(g, st));
  SSV_TRY(ssv_launch_softmax_cols(a, B, N, T, st));
  return ssv_attention_apply(v, kv_bs, a, T, r, r_bs, B, d, N, T, stream);
}
// The decoder's input cat(R, Q) (models/TTSModel.py:270) in the same call: rq (B, 2d, T) receives R in rows [0, d) and a copy of Q in rows [d, 2d).
extern "C" int ssv_attention_train_fwd_rq(const float* k, const float* v, long kv_bs, const float* q, long q_bs, float* a, float* rq, long rq_bs,
                                          int B, int d, int N, int T, ssv_stream_t stream) {
  SSV_CHECK(k && v && q && a && rq && B > 0 && d > 0 && N > 0 && T > 0 && rq_bs >= (long)2 * d * T, SSV_BAD_SHAPE, "attention_train_fwd_rq: bad argument");
  if (ssv_attn_fused_ok(B, d, N, T)) return ssv_launch_attn_fwd_fused(k, v, kv_bs, q, q_bs, a, rq, rq_bs, 1, B, d, N, T, (hipStream_t)stream);
  SSV_TRY(ssv_attention_train_fwd(k, v, kv_bs, q, q_bs, a, rq, rq_bs, B, d, N, T, stream));
  return ssv_copy_rows(q, q_bs, rq + (long)d * T, rq_bs, B, (long)d * T, stream);
}
// Length-masked form: scores on the general product, the masked column softmax (attn.hip), V A.  The fused one-launch kernel has no mask; the
// backward is ssv_attention_train_bwd unchanged (A is exactly 0 on the masked sets, hence so are dS, dK, dV and dQ there).
extern "C" int ssv_attention_train_fwd_rq_len(const float* k, const float* v, long kv_bs, const float* q, long q_bs, float* a, float* rq, long rq_bs,
                                              int B, int d, int N, int T, const int* live, ssv_stream_t stream) {
  SSV_CHECK(k && v && q && a && rq && live && B > 0 && d > 0 && N > 0 && T > 0 && rq_bs >= (long)2 * d * T, SSV_BAD_SHAPE,
            "attention_train_fwd_rq_len: bad argument");
  hipStream_t st = (hipStream_t)stream;
  GemmNN g;
  g.A = k; g.sab = kv_bs; g.sam = 1; g.sac = N; g.saj = 0;
  g.X = q; g.sxb = q_bs; g.sxc = T; g.Lx = T;
  g.C = a; g.scb = (long)N * T; g.scm = T;
  g.M = N; g.N = T; g.Kc = d; g.B = B; g.alpha = 1.f / sqrtf((float)d);
  SSV_TRY(ssv_launch_gemm_nn(g, st));
  SSV_TRY(ssv_launch_softmax_cols_len(a, B, N, T, live, st));
  SSV_TRY(ssv_attention_apply(v, kv_bs, a, T, rq, rq_bs, B, d, N, T, stream));
  return ssv_copy_rows(q, q_bs, rq + (long)d * T, rq_bs, B, (long)d * T, stream);
}
// dA / dScores (B, N, T), then the two fallback scale lists of nt_per_batch
struct AttnBwdWs { size_t dA, fb, total; };
static AttnBwdWs attn_bwd_ws(int B, int N, int T) {
  WsTake t;
  AttnBwdWs l;
  l.dA = t.take((size_t)B * N * T * sizeof(float));
  l.fb = t.take(2 * AMAX_FB_BYTES);
  l.total = t.off;
  return l;
}
extern "C" size_t ssv_attention_train_bwd_workspace(int B, int d, int N, int T) { (void)d; return attn_bwd_ws(B, N, T).total; }
// Per-batch-item products reduced over time (attention dV, dK): the split-bf16 weight-gradient kernel with one slab per batch
// item and no slab sum (21 -> ~100 TFLOP/s at d = 256, N = 186, T = 325; the fp32 kernel's 128 x 96 tiles leave the chip idle).
// fb: 2 * SSV_AMAX_FB_FLOATS floats of workspace for the operands' scale lists (split-fp16)
static int nt_per_batch(GemmNT& g, int T, hipStream_t st, float* fb) {
  g.KT = 1;
  g.scj = 1;
  if (ssv_precision() >= 1 && (long)g.B * T >= 256 && ssv_nt_bf3_fits(g)) {
    if (use_f16()) {
      AmaxList la, lx;
      SSV_TRY(amax_of(g.A, g.sab, g.B, (long)g.M * T, nullptr, 0, fb, &la, st));
      SSV_TRY(amax_of(g.X, g.sxb, g.B, (long)g.Nc * T, nullptr, 0, fb + SSV_AMAX_FB_FLOATS, &lx, st));
      g.f16 = 1; g.a_amax = la.p; g.a_namax = la.n * g.B; g.x_amax = lx.p; g.x_namax = lx.n * g.B;
    }
    return ssv_launch_gemm_nt_bf3(g, st);
  }
  return ssv_launch_gemm_nt(g, st);
}

extern "C" int ssv_attention_train_bwd(const float* dr, long dr_bs, const float* da_ext, const float* dq_add, long dq_add_bs,
                                       const float* k, const float* v, long kv_bs, const float* q, long q_bs, const float* a,
                                       float* dk, float* dv, long dkv_bs, float* dq, long dq_bs, int B, int d, int N, int T,
                                       void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dr && k && v && q && a && dk && dv && dq && B > 0 && d > 0 && N > 0 && T > 0, SSV_BAD_SHAPE, "attention_train_bwd: bad argument");
  const AttnBwdWs l = attn_bwd_ws(B, N, T);
  SSV_CHECK(ws && ws_bytes >= l.total, SSV_BAD_SHAPE, "attention_train_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* dA = ws_f32(ws, l.dA);
  float* fb = ws_f32(ws, l.fb);
  // out(b,c,n) = sum_t A(b,c,t) X(b,n,t): the two reductions over time (dv, dk) stay on the weight-gradient kernel in both forms
  auto over_time = [&](const float* A, long a_bs, const float* X, float* out) -> int {
    GemmNT g;
    g.A = A; g.sab = a_bs; g.sam = T; g.La = T;
    g.X = X; g.sxb = (long)N * T; g.sxc = T; g.Lx = T;
    g.C = out; g.scz = dkv_bs; g.scm = N; g.scc = 1;
    g.M = d; g.Nc = N; g.B = B; g.Z = B; g.bstep = B;
    return nt_per_batch(g, T, st, fb);
  };
  if (ssv_attn_fused_ok(B, d, N, T)) {
    // dA, dS (left in ws for dk) and dq in ONE launch
    SSV_TRY(ssv_launch_attn_bwd_fused(dr, dr_bs, da_ext, dq_add, dq_add_bs, k, v, kv_bs, a, dA, dq, dq_bs, B, d, N, T, st));
    SSV_TRY(over_time(dr, dr_bs, a, dv));          // dv(b,c,n) = sum_t dr(b,c,t) a(b,n,t)
    return over_time(q, q_bs, dA, dk);             // dk(b,c,n) = sum_t q(b,c,t) ds(b,n,t)
  }
  {  // dA(b,n,t) = sum_c v(b,c,n) dr(b,c,t)
    GemmNN g;
    g.A = v; g.sab = kv_bs; g.sam = 1; g.sac = N;
    g.X = dr; g.sxb = dr_bs; g.sxc = T; g.Lx = T;
    g.C = dA; g.scb = (long)N * T; g.scm = T;
    g.M = N; g.N = T; g.Kc = d; g.B = B;
    SSV_TRY(ssv_launch_gemm_nn(g, st));
  }
  SSV_TRY(over_time(dr, dr_bs, a, dv));            // dv(b,c,n) = sum_t dr(b,c,t) a(b,n,t)
  SSV_TRY(ssv_launch_softmax_cols_bwd(a, dA, da_ext, 1.f / sqrtf((float)d), B, N, T, st));   // dA now holds dScores
  SSV_TRY(over_time(q, q_bs, dA, dk));             // dk(b,c,n) = sum_t q(b,c,t) ds(b,n,t)
  GemmNN g;                                        // dq(b,c,t) = sum_n k(b,c,n) ds(b,n,t) + dq_add
  g.A = k; g.sab = kv_bs; g.sam = N; g.sac = 1;
  g.X = dA; g.sxb = (long)N * T; g.sxc = T; g.Lx = T;
  g.C = dq; g.scb = dq_bs; g.scm = T;
  if (dq_add) { g.R = dq_add; g.srb = dq_add_bs; g.srm = T; }
  g.M = d; g.N = T; g.Kc = N; g.B = B;
  return ssv_launch_gemm_nn(g, st);
}
