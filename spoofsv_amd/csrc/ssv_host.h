// Internal header of the C-ABI host layer (api.hip and the per-module api_*.hip files): the helpers several modules share, the ONE
// description of a resident weight's planes, the running-offset workspace layout, and the declarations of the launchers that
// norm.hip, attn*.hip and lstm.hip define.  No kernel, no entry point.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssv_common.h"
#include <type_traits>
static_assert(std::is_trivially_copyable<GemmNN>::value && std::is_trivially_copyable<GemmNT>::value && std::is_trivially_copyable<GemmNNB>::value,
              "the GEMM argument structs are kernel arguments");
#define SSV_HIP(expr) do { hipError_t _he = (expr); if (_he != hipSuccess) { ssv_fail(0, "%s: %s", #expr, hipGetErrorString(_he)); return -(int)_he; } } while (0)

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
static inline size_t zmax(size_t a, size_t b) { return a > b ? a : b; }
static inline int pad32(int n) { return (n + 31) & ~31; }

// The host copy of an offsets array (n + 1 entries, optional): [off[0], off[n]) must lie inside the `total` items and no entry descend.
// `arg` names the array, `one` one of its intervals, `items` what they index: the words of the two messages.
static inline int host_offsets_ok(const char* who, const char* arg, const char* one, const char* items, const long* off, int n, long total) {
  if (!off) return 0;
  SSV_CHECK(off[0] >= 0 && off[n] <= total, SSV_BAD_SHAPE, "%s: %ss [%ld, %ld) leave the %ld %s", who, one, off[0], off[n], total, items);
  for (int i = 0; i < n; ++i)
    SSV_CHECK(off[i] <= off[i + 1], SSV_BAD_SHAPE, "%s: %s descends at %s %d (%ld > %ld)", who, arg, one, i, off[i], off[i + 1]);
  return 0;
}

// ---- workspace layout ------------------------------------------------------------------------------------------------
// The regions of a workspace are taken in order, each from a 256-byte boundary; `off` after the last take is the size.  Every
// workspace has ONE layout function built on this: the public *_workspace query returns its total and the entry point carves
// with its offsets, so a region cannot be added to an entry point without growing its query.
struct WsTake {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t at = off; off += align256(bytes); return at; }
};
static inline float* ws_f32(void* ws, size_t off) { return (float*)((char*)ws + off); }
static inline const float* ws_f32(const void* ws, size_t off) { return (const float*)((const char*)ws + off); }
static inline unsigned short* ws_u16(void* ws, size_t off) { return (unsigned short*)((char*)ws + off); }

// ---- arithmetic mode ---------------------------------------------------------------------------------------------------
// Channel counts below 32 (the tail of the WGAN-GP critics: 64 -> 16 -> 8 -> 1 channels, models/discriminator.py:31-38) take the exact-fp32
// kernels in all three products of a convolution: such a launch is 5 us either way, and the split-MFMA path would need a scale list per
// operand -- one ssv_absmax launch each for tensors whose producers (pooling, dropout, second-order LayerNorm) emit none (ops._tiny_conv).
#define SSV_MIN_SPLIT_CHANNELS 32
static inline bool use_bf3(int B, int L, int Cin, int Cout) {
  return ssv_precision() >= 1 && (long)B * L >= 128 && Cin >= SSV_MIN_SPLIT_CHANNELS && Cout >= SSV_MIN_SPLIT_CHANNELS;
}
static inline bool use_f16() { return ssv_precision() == 2; }

// ---- split planes of a weight ------------------------------------------------------------------------------------------
// bytes of ONE plane of a (rows, K, k) operand; the lo plane follows the hi plane
static inline size_t split_bytes(int rows, int K, int k) { return align256((size_t)k * ((rows + 15) / 16 * 16) * pad32(K) * sizeof(unsigned short)); }
// The resident planes of a (Cout, Cin, k) weight (ssv_conv_pack_bytes; written by ssv_conv_pack_multi from the plan of ssv_conv_pack_plan):
// the forward hi / lo planes (rows = Cout), the transposed hi / lo planes (rows = Cin), then 256 bytes that keep 2^-ea of the forward
// planes at +0 and of the transposed planes at +128 (split-fp16).  This is the only place that spells the layout out.  All null
// when w_packed is null: "no resident planes", the callers split into their workspace instead.
struct SplitPlanes { unsigned short* hi; unsigned short* lo; float* inv; };
struct PackedPlanes { SplitPlanes fwd, tr; size_t bytes; };
static inline PackedPlanes packed_planes(const void* w_packed, int Cout, int Cin, int k) {
  const size_t f = split_bytes(Cout, Cin, k), t = split_bytes(Cin, Cout, k);
  PackedPlanes p = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, 2 * f + 2 * t + 256};
  if (char* b = (char*)w_packed) {
    p.fwd = {(unsigned short*)b, (unsigned short*)(b + f), (float*)(b + 2 * f + 2 * t)};
    p.tr = {(unsigned short*)(b + 2 * f), (unsigned short*)(b + 2 * f + t), (float*)(b + 2 * f + 2 * t + 128)};
  }
  return p;
}

#pragma GCC visibility push(hidden)      // the host layer's own functions: shared between its files, not exported
// ---- split-fp16 operand scales (ssv_common.h, "split-fp16") ------------------------------------------------------------
// A list of partial maxima of |x|: n entries per batch item, items consecutive.  Either the caller's (written by the kernel
// that produced x, or by ssv_absmax) or computed by amax_of into `fb`, SSV_AMAX_FB_FLOATS floats of the call's workspace.
#define SSV_AMAX_FB_FLOATS 4096
#define SSV_F16_AUX_BYTES (SSV_F16_AUX_FLOATS * sizeof(float))
static const size_t AMAX_FB_BYTES = SSV_AMAX_FB_FLOATS * sizeof(float);
struct AmaxList { const float* p; int n; };
int amax_of(const float* x, long x_bs, int B, long n_item, const float* given, int ngiven, float* fb, AmaxList* out, hipStream_t st);

// ---- convolution products shared by the modules (api_conv.hip) -----------------------------------------------------------
int conv_shifts(int k, int dilation, int causal, int* shift);
// Workspace of one conv_nn call: `main` bytes at offset 0 (the weight split here when no resident planes are given, or its fp32
// transpose), the pack kernel's aux floats, the fallback scale list of x.
struct ConvWs { size_t main, aux, fb, total; };
ConvWs conv_ws(size_t main_bytes);
ConvWs conv_fwd_ws(int Cin, int Cout, int k);
ConvWs conv_bwd_data_ws(int Cin, int Cout, int k);
// (pw != null: the 1x1 product finishes LayerNorm + activation in its own launch, gemm_pwln_kernel; y is then `pre`)
struct PwLnArgs { const float* gamma; const float* beta; float* y; long ybs; float* stats; float* y_amax; int namax; int act; };
// y = conv(x, w): shared by forward (rows = Cout) and data gradient (rows = Cin, transposed weights, negated shifts)
// `packed`: resident pre-split planes of this operand and where they keep 2^-ea (packed.hi null -> split into ws here).
// split-fp16: xa_given / xa_n = the caller's scale list of x or null (computed into the workspace's fallback list).
int conv_nn(const float* x, long x_bs, const float* w, SplitPlanes packed, long w_sm, long w_sk, const float* bias, const float* bias_b,
            const float* r, long r_bs, float* y, long y_bs, int B, int K, int M, int L, int k, const int* shift,
            bool bf3, void* ws, const ConvWs& l, hipStream_t st, const float* xa_given = nullptr, int xa_n = 0,
            float* colstats = nullptr, const PwLnArgs* pw = nullptr);
// Number of batch slabs of a weight-gradient launch.  L: the reduction length per batch item.  Required: a caller whose workspace
// query has no length (the transposed conv) passes SSV_NOMINAL_L so that query and launch agree by construction.
#define SSV_NOMINAL_L 325
int dw_splits(int B, int M, int Nc, int k, int L);
// part / pgrads / n2 / nblk: partial rows of another reduction (the LayerNorm / bias gradients of the same layer) summed by the
// SAME launch that sums the weight-gradient slabs (highwayConv backward); part == nullptr: weight gradient only.
// dy_amax / x_amax (n entries per batch item each): the operands' scale lists for the split-fp16 arithmetic, or null (computed here).
int conv1d_bwd_weight_impl(const float* dy, long dy_bs, const float* x, long x_bs, float* dw, int B, int Cin, int Cout, int L, int k, int dilation,
                           int causal, void* ws, size_t ws_bytes, ssv_stream_t stream, const float* part, float* pgrads, int n2, int nblk,
                           const float* dy_amax, int dy_namax, const float* x_amax, int x_namax);

// ---- GE2E LSTM pieces that inference and training share (api_lstm.hip) -------------------------------------------------------
// Wavefront (split-MFMA) layout: h of every layer lives in a 2-frame ring, weights of layer l >= 1 are [W_ih | W_hh] side by side.
// (comb_stride, hp_plane, npad, xsplit0: strides and counts of the regions, not offsets.)
struct LstmWave { size_t xt, xp, out, c, bias, ih0, hh0, comb, comb_stride, aux, hp, hp_plane, l0c, x0p, total; int npad, xsplit0; };
LstmWave lstm_wave_ws(int Bn, int T, int F, int H, int layers);
// Training (keep_* != null): every frame of h, c and the activated gates is kept in the caller's buffers.  packed: see ssv_lstm_fwd_cached.
int lstm_fwd_wave(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                  const float* const* b_hh, float* h_last, int Bn, int T, int F, int H, int layers, char* base, hipStream_t st,
                  float* keep_xt = nullptr, float* keep_hs = nullptr, float* keep_cs = nullptr, float* keep_gates = nullptr, bool packed = false);
// C = A X (+ bias + bias_b + R) on the exact-fp32 kernel, A (M x K) row-major weights and X, C as [rows][Bn] activations
int lstm_gemm_f32(const float* A, const float* X, long sxb, float* C, long scb, const float* bias, const float* bias_b,
                  const float* R, int M, int K, int Bn, int nb, hipStream_t st);

#pragma GCC visibility pop

// ---- launchers defined in norm.hip --------------------------------------------------------------------------------------
// amax (last argument of the four LayerNorm launchers): where the kernel leaves its tiles' max |output| (ssv_amax_rows(L) per batch item), or null
int ssv_launch_ln_gate_fwd(const float* H, long h_bs, const float* X, long x_bs, const float* g1, const float* b1, const float* g2, const float* b2,
                           float* Y, long y_bs, float* stats, int B, int C, int L, hipStream_t st, float* amax = nullptr);
int ssv_launch_ln_gate_fwd_stream(const float* H, const float* X, long x_bs, const float* colstats, const float* g1, const float* b1, const float* g2, const float* b2,
                                  float* Y, long y_bs, float* stats, float* amax, int B, int C, int L, hipStream_t st);
int ssv_launch_ln_gate_bwd(const float* dY, long dy_bs, const float* H, const float* X, long x_bs, const float* stats, const float* g1, const float* b1,
                           const float* g2, const float* b2, float* dH, float* dXres, long dx_bs, float* part, float* pgrads /* [6][C] */,
                           int B, int C, int L, hipStream_t st, float* amax = nullptr);
int ssv_launch_ln_act_fwd(const float* X, long x_bs, const float* gam, const float* bet, float* Y, long y_bs, float* stats,
                          int B, int C, int L, int act, hipStream_t st, float* amax = nullptr);
int ssv_launch_ln_act_bwd(const float* dY, long dy_bs, const float* X, long x_bs, const float* stats, const float* gam, const float* bet,
                          float* dX, long dx_bs, float* part, float* pgrads /* [3][C] */, int B, int C, int L, int act, hipStream_t st, float* amax = nullptr);
int ssv_launch_ln_bwd2(const float* V, long v_bs, const float* GN, long gn_bs, const float* X, long x_bs, const float* stats, const float* gam,
                       float* dGN, long dgn_bs, float* dX, long dx_bs, float* part, float* dgamma, int B, int C, int L, hipStream_t st);
int ssv_launch_ln_gate_bwd2(const float* VH, const float* VX, long vx_bs, const float* GY, long gy_bs, const float* H, const float* X, long x_bs,
                            const float* stats, const float* g1, const float* b1, const float* g2, const float* b2, float* dGY, long dgy_bs,
                            float* dH, float* dX, long dx_bs, float* part, float* pgrads /* [4][C] */, int B, int C, int L, hipStream_t st);
int ssv_ln_gate_bwd_nblk(int B, int L);                            // upper bound of the partial rows a backward launch writes (buffer sizes)
int ssv_ln_gate_bwd_rows(int B, int C, int L, bool has_amax);      // partial rows the backward launch of this shape writes
int ssv_ln_act_bwd_rows(int B, int C, int L, bool has_amax);
int ssv_ln_act_bwd_vec(int C, int L, bool has_amax);
int ssv_reduce_partial_rows(const float* part, float* out, int n, int nblk, hipStream_t st);

// ---- launchers defined in attn.hip and attn_fused.hip ------------------------------------------------------------------
int ssv_launch_softmax_cols(float* s, int B, int N, int T, hipStream_t st);
int ssv_launch_softmax_cols_bwd(const float* a, float* da, const float* da_ext, float scale, int B, int N, int T, hipStream_t st);
int ssv_launch_softmax_cols_len(float* s, int B, int N, int T, const int* live, hipStream_t st);
bool ssv_attn_fused_ok(int B, int d, int N, int T);        // scores, softmax and V A (backward: dA, dS, dQ) in one launch
int ssv_launch_attn_fwd_fused(const float* k, const float* v, long kv_bs, const float* q, long q_bs, float* a, float* rq, long rq_bs, int copy_q,
                              int B, int d, int N, int T, hipStream_t st);
int ssv_launch_attn_bwd_fused(const float* dr, long dr_bs, const float* da_ext, const float* dq_add, long dq_add_bs, const float* k, const float* v, long kv_bs,
                              const float* a, float* ds, float* dq, long dq_bs, int B, int d, int N, int T, hipStream_t st);

// ---- launchers defined in lstm.hip --------------------------------------------------------------------------------------
int ssv_launch_lstm_in_transpose(const float* x, float* xt, int Bn, int T, int F, hipStream_t st);
int ssv_launch_lstm_x_planes(const float* x, const float* amax, void* planes, long plane_bytes, int Bn, int T, int F, int kgroups, int npad, hipStream_t st);
int ssv_launch_lstm_cell(const float* g, float* c, float* h, int H, int Bn, int first, hipStream_t st);
int ssv_launch_lstm_cell_train(const float* pre, float* act, const float* cprev, float* c, float* h, int H, int Bn, hipStream_t st);
int ssv_launch_lstm_cell_bwd(const float* gates, const float* cs, const float* dxa, long zstride, int nz, const float* dh_top, float* dgates, float* dcarry,
                             float* dbp, float* amax, int H, int Bn, int T, int layers, int s, int lo, int nl, hipStream_t st);
int ssv_launch_transpose_out(const float* src, float* dst, int R, int Bn, hipStream_t st);
int ssv_launch_l2norm_rows(const float* y, float* e, float* norms, int P, int Bn, hipStream_t st);
int ssv_launch_l2norm_bwd(const float* de, const float* e, const float* norms, float* dy, int P, int Bn, hipStream_t st);
int ssv_launch_colsum(const float* x, float* out, int P, int Bn, hipStream_t st);
