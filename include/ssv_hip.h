/* libssv_hip.so -- C ABI of the MI355X (gfx950) hot path of SpoofSV.
 *
 * The reference (MingruiYuan/SpoofSV) is pure Python on torch and has NO plugin / operator / FFI
 * interface: its hot path is the nn.Module surface of models/TTSModel.py and
 * GE2E/speech_embedder_net.py.  Each entry point below therefore replaces a *module forward (or its
 * autograd backward)* of the reference, cited as file:line; a binding is a ctypes stub
 * (INTEGRATION.md shows the one a maintainer of the reference would add).
 *
 * Conventions (all entries):
 *   - every pointer is a DEVICE pointer to caller-owned memory; fp32 unless stated; text ids and
 *     attention indices are int64.  Activations are (B, C, T) with T fastest and rows contiguous
 *     (channel stride = T); `*_bs` arguments are the batch stride in floats (C*T when dense), which
 *     lets a caller pass channel slices of a wider tensor (K|V halves, the R|Q concatenation).
 *   - no allocation, no ownership transfer, no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t; NULL = default stream) and the call returns.  Safe under hipGraph capture.
 *   - scratch memory is passed as (ws, ws_bytes); the matching *_workspace() query gives the size.
 *   - return value: 0 on success, -1 bad shape/argument, -2 unsupported configuration, otherwise
 *     -(int)hipError_t.  ssv_last_error() returns a thread-local message for the last failure.
 *   - re-entrant; callable from any host thread (torch's autograd thread calls the *_bwd entries).
 *   - outputs listed as "saved" are the tensors the matching backward needs; the caller owns them.
 */
#ifndef SSV_HIP_H
#define SSV_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* ssv_stream_t; /* hipStream_t */

int ssv_version(void);            /* ABI version, currently 7 (7 = ssv_spec_losses_fwd_bwd, ssv_deinterleave2_rows_amax, w_packed / y_amax of ssv_deconv1d_k2s2_fwd, ssv_bias_grad; 6 = ssv_shift_right_amax, ssv_deinterleave2_amax, ssv_lstm_fwd_cached, GE2E training without shape / mode limits; 5 = ssv_attention_train_fwd_rq; 2 = split-fp16 operand scales; 3 = max_shift of ssv_conv1d_bwd_weight_multi, ssv_pointwise_conv_ln_act_fwd;
                                    4 = compact partial rows: the nblk of a weight-gradient job is ssv_ln_bwd_partial_rows(...), not ssv_ln_partial_rows(B, L)) */
const char* ssv_arch(void);       /* "gfx950" */
const char* ssv_last_error(void); /* thread-local, valid until the next failing call on this thread */
/* Arithmetic of the conv GEMMs (the reference computes in fp32: requirements.txt:5, nn.Conv1d at models/TTSModel.py:59):
 *   0 = fp32-in MFMA: bit-exact fp32 fma chains (157 TFLOP/s peak);
 *   1 = split-bf16 MFMA: each fp32 operand as bf16 hi+lo, three bf16 MFMAs per product, fp32 accumulate; ~2^-16 per
 *       product -- NARROWER than the reference's arithmetic, opt-in only;
 *   2 = split-fp16 MFMA (default): each operand is scaled by a power of two (per tensor / per batch item, from its
 *       maximum magnitude) and split into fp16 hi+lo = 22 significand bits, three fp16 MFMAs per product (every
 *       fp16 x fp16 product is exact in fp32), fp32 accumulate, result rescaled; ~2^-22 per product = fp32-grade at
 *       the bf16/fp16 MFMA rate.  The LSTM products of the GE2E embedder run in this arithmetic too (one power-of-two scale for all
 *       weight matrices of a launch; the recurrent activations, |h| < 1, take the fixed scale 2^14).
 * Env SSV_PRECISION = fp32 | bf16x3 | f16x2 selects the mode at load.  Returns the previous mode.  Process-wide.
 *
 * Operand scales (mode 2).  A kernel that reads an fp32 tensor as an MFMA operand needs max |x| BEFORE it starts.  The
 * convention: a "scale list" of x (B, C, L) is `namax` floats per batch item, items consecutive, whose maximum per item
 * is max |x(b)| -- partial maxima, in any partition.  The LayerNorm / gate kernels write such a list for their output as
 * a by-product (ssv_amax_rows(L) entries per item: one per kernel tile, unused ones zeroed), ssv_absmax computes one for any tensor, and
 * every entry below that takes `*_amax, *_namax` arguments accepts NULL, 0: it then computes the list itself in its
 * workspace (one extra small launch).  Outside mode 2 the arguments are ignored (amax outputs are still written, except y_amax of
 * ssv_deconv1d_k2s2_fwd: mode 2 only).  A NaN element does not enter a list (fmaxf drops it): the entry is the maximum of the others. */
int ssv_set_precision(int mode);
int ssv_get_precision(void);
int ssv_amax_rows(int L);         /* entries per batch item of the lists the LayerNorm / gate kernels write: 4 * ceil(L / 64) */
/* amax[b * namax + i] = max |x| over the i-th of namax equal pieces of item b (n dense floats at x + b * x_bs). */
int ssv_absmax(const float* x, long x_bs, int B, long n, float* amax, int namax, ssv_stream_t stream);
/* Two layout changes of the trainers that also deliver the result's scale list (one launch instead of a copy kernel + ssv_absmax; amax may be
 * NULL).  Teacher forcing, train/ordinary.py:226 = train/adversarial_wasserstein_gp.py:277 (`torch.cat((zeros, mel[:, :, :-1]), -1)`):
 * y (B, C, T) dense, y(b, c, 0) = 0, y(b, c, t) = x(b, c, t - 1); x items x_bs apart. */
int ssv_shift_right_amax(const float* x, long x_bs, float* y, int B, int C, int T, float* amax, int namax, ssv_stream_t stream);
/* out[j][b][i] = x[b][2 i + j] for j = 0, 1, i < n: the two taps of a ConvTranspose1d(k = 2, s = 2) output gradient (models/TTSModel.py:309,314,
 * backward), each then a dense (B, n) operand of a k = 1 weight gradient; amax: namax partial maxima of |x| per item. */
int ssv_deinterleave2_amax(const float* x, long x_bs, float* out, int B, long n, float* amax, int namax, ssv_stream_t stream);
/* The same, row by row (ABI 7): out(b, 2 r + j, t) = x(b, r, 2 t + j), x (B, rows, 2 L) with items x_bs apart, out (B, 2 rows, L) dense.  A
 * ConvTranspose1d(k = 2, s = 2) is the 1x1 convolution u = W2 x, W2 = w.view(Cin, 2 Cout), followed by y(b, o, 2 t + j) = u(b, 2 o + j, t): with its
 * output gradient in this layout, dx is ONE ssv_conv1d_fwd of it with the weight w.view(Cin, 2 Cout, 1) and dw ONE ssv_conv1d_bwd_weight that lands in
 * the weight's own (Cin, Cout, 2) layout (spoofsv_amd/ops.py, DeconvK2S2Fn.backward). */
int ssv_deinterleave2_rows_amax(const float* x, long x_bs, float* out, int B, int rows, int L, float* amax, int namax, ssv_stream_t stream);

/* ---- Conv1d (stride 1, kernel 1 or 3, dilated, "same" or causal zero padding) -------------------
 * Replaces nn.Conv1d as used at models/TTSModel.py:59,78 (highway), :115-117, :154-158, :203-214,
 * :323-339 (kernel 1) and nn.Linear on (B, D, 1) speaker codes (:150-151, :174, :179).
 * y(b,o,t) = bias[o] + bias_b[b*Cout+o] + sum_{c,j} w[o,c,j] * x(b,c,t + (j-j0)*dilation),
 * j0 = (k-1)/2 ("same", :57-59) or k-1 (causal: 2*pad zeros on the left, :72-74).
 * bias and bias_b (the broadcast speaker term of :175,:180) may be NULL. */
/* w_packed (every entry that takes it): NULL, or the weight's resident pre-split planes written by
 * ssv_conv_pack_multi (see "Resident pre-split weights" below) -- then the call skips its own weight split.  The
 * caller vouches that the planes are current for w. */
size_t ssv_conv1d_fwd_workspace(int Cin, int Cout, int k);   /* holds the pre-split weights */
/* y_colstats (may be NULL; split-MFMA modes, Cout % 64 == 0, dense y): per batch item, 64-row group of output channels and
 * column, the mean and the sum of squared deviations of y over the group's 64 channels, (B, Cout/64, L, 2) floats -- the
 * channel-axis LayerNorm that follows merges the groups instead of reducing over y again (ssv_highway_conv1d_fwd does). */
int ssv_conv1d_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                   const float* bias_b, float* y, long y_bs, float* y_colstats,
                   int B, int Cin, int Cout, int L, int k, int dilation, int causal,
                   void* ws, size_t ws_bytes, ssv_stream_t stream);
/* dx = conv1d_transpose(dy, w) [+ dx_add if non-NULL, same layout as dx]; ws holds w transposed. */
size_t ssv_conv1d_bwd_data_workspace(int Cin, int Cout, int k);
int ssv_conv1d_bwd_data(const float* dy, long dy_bs, const float* dy_amax, int dy_namax, const float* w, const void* w_packed,
                        const float* dx_add, float* dx, long dx_bs,
                        int B, int Cin, int Cout, int L, int k, int dilation, int causal,
                        void* ws, size_t ws_bytes, ssv_stream_t stream);
/* dw(o,c,j) = sum_{b,t} dy(b,o,t) x(b,c,t+(j-j0)*dilation); split over the batch into slabs, summed
 * in a fixed order (bitwise reproducible).  With batch strides larger than C*L the kernels READ the floats between two items of dy and of x
 * (their windows run past a row's end, never past the tensor's last element) and count them as zeros whatever they hold -- NaN, Inf or
 * the gradient of the other half of a torch.cat; they write nothing outside dw and ws. */
size_t ssv_conv1d_bwd_weight_workspace(int B, int Cin, int Cout, int L, int k);
int ssv_conv1d_bwd_weight(const float* dy, long dy_bs, const float* dy_amax, int dy_namax, const float* x, long x_bs, const float* x_amax, int x_namax,
                          float* dw, int B, int Cin, int Cout, int L, int k, int dilation, int causal,
                          void* ws, size_t ws_bytes, ssv_stream_t stream);
/* out(b,c) = sum_t x(b,c,t): gradient of a (B,C,1) broadcast term / of a bias per batch item. */
int ssv_rowsum(const float* x, long x_bs, float* out, int B, int C, int L, ssv_stream_t stream);
/* out(c) = sum_{b,t} x(b,c,t): the bias gradient of a conv layer in one launch (ABI 7; ssv_rowsum + ssv_sum_slabs before), fixed summation order. */
int ssv_bias_grad(const float* x, long x_bs, float* out, int B, int C, int L, ssv_stream_t stream);
/* out[i] = sum_{z<Z} slabs[z*stride + i], i < n.  The order is fixed, so the result is bitwise reproducible, but it is NOT index order: four
 * accumulators a_u take slabs u, u + 4, u + 8, ... of the first 4 * (Z / 4) slabs in increasing z, the remaining Z % 4 slabs are then added
 * to a_0 in increasing z, and out[i] = (a_0 + a_1) + (a_2 + a_3). */
int ssv_sum_slabs(const float* slabs, float* out, long n, int Z, long stride, ssv_stream_t stream);
/* dst(b, 0:n) = src(b, 0:n) for B rows with independent row strides (the Q half of torch.cat((R, Q), 1),
 * models/TTSModel.py:270). */
int ssv_copy_rows(const float* src, long src_bs, float* dst, long dst_bs, int B, long n, ssv_stream_t stream);

/* ---- LayerNorm over channels (+ activation) ----------------------------------------------------
 * Replaces `ln(x.permute(0,2,1)).permute(0,2,1)` followed by F.relu / F.sigmoid,
 * models/TTSModel.py:129-131, :175-180, :219-231, :344-361.  act: 0 none, 1 relu, 2 sigmoid.
 * stats (B,2,L) = mean, rstd: saved for backward (may be NULL for inference). */
size_t ssv_channel_ln_act_fwd_workspace(int B, int C, int L);
/* y_amax (may be NULL): scale list of y, ssv_amax_rows(L) entries per item, for the convolution that reads y next. */
int ssv_channel_ln_act_fwd(const float* x, long x_bs, const float* gamma, const float* beta,
                           float* y, long y_bs, float* y_amax, float* stats, int B, int C, int L, int act,
                           void* ws, size_t ws_bytes, ssv_stream_t stream);
/* The whole forward of such a link: y = act(LN(conv1x1(x) + bias [+ s])) -- models/TTSModel.py:128-131, :173-180 (s = fc(spk), (B,Cout)),
 * :218-231, :343-361.  pre (B,Cout,L) dense = the LayerNorm's input and stats (B,2,L) (may be NULL) are kept for
 * ssv_pointwise_conv_ln_act_bwd.  One launch where the library has the fused kernel for the shape (a workgroup owns all output rows of
 * its column tile), otherwise the product followed by the LayerNorm kernel; x_amax / w_packed / y_amax as in ssv_conv1d_fwd /
 * ssv_channel_ln_act_fwd. */
size_t ssv_pointwise_conv_ln_act_fwd_workspace(int Cin, int Cout);
int ssv_pointwise_conv_ln_act_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                                  const float* s, const float* gamma, const float* beta, float* pre, float* stats, float* y, long y_bs, float* y_amax,
                                  int B, int Cin, int Cout, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream);
size_t ssv_channel_ln_act_bwd_workspace(int B, int C, int L);
/* dx: gradient w.r.t. the pre-LN input; pgrads (3,C) = dgamma, dbeta, sum_{b,t} dx (bias gradient of
 * the producing conv).   pgrads may be NULL: the parameter gradients are not wanted
 * (the partial rows stay unsummed in ws) -- the gradient penalty's input-gradient pass, train/adversarial_wasserstein_gp.py:303-304. */
int ssv_channel_ln_act_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* stats,
                           const float* gamma, const float* beta, float* dx, long dx_bs, float* pgrads,
                           int B, int C, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* The whole backward of y = act(LN(conv1x1(x) [+ s])) (models/TTSModel.py:128-131, :173-180, :218-231, :343-361) in one call,
 * so that the LayerNorm partial sums and the weight-gradient slabs share one reduction launch.  pre (B,Cout,L) dense and stats
 * (B,2,L) are what the forward saved; dx may be NULL (first layer: the input needs no gradient); ds (B,Cout) = gradient of
 * the broadcast term s, or NULL; pgrads (3,Cout) = dgamma, dbeta, dbias. */
size_t ssv_pointwise_conv_ln_act_bwd_workspace(int B, int Cin, int Cout, int L);
int ssv_pointwise_conv_ln_act_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* x_amax, int x_namax,
                                  const float* w, const void* w_packed,
                                  const float* gamma, const float* beta, const float* pre, const float* stats,
                                  float* dx, long dx_bs, float* dw, float* pgrads, float* ds,
                                  int B, int Cin, int Cout, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* ---- Weight gradients of several equal-shaped conv layers in ONE launch ------------------------------------------
 * The weight gradient is off the critical path of backward (nothing downstream reads dW), and a single layer's reduction over
 * (batch, time) must be cut into Z slabs only to fill the chip (C = 256, L = 325: 16 output tiles x 32 slabs = 49 MiB of partial
 * sums written and read back per layer).  A trainer can therefore run backward with the *_bwd_data entries below (LayerNorm /
 * gate backward + data gradient only; dH and the LayerNorm partial rows are left in caller-owned buffers), collect one job per
 * layer, and hand all layers of one shape to ssv_conv1d_bwd_weight_multi: njobs x tiles x Z workgroups with a Z that is njobs
 * times smaller, then one reduction launch for all jobs (slabs -> dw, partial rows -> pgrads).  Same arithmetic per product;
 * only the slab boundaries (hence the fp32 summation order over the batch) differ from the one-layer entry.
 * jobs_dev: device array of njobs jobs.  Per job: dy (B,Cout,L) = dH, x (B,Cin,L), dw (Cout,Cin,k) out, part (nblk, n2) partial
 * rows or NULL, pgrads (n2) out or NULL, shift[j] = (j - j0) * dilation as ssv_conv_shifts returns them.
 * max_shift: the caller's bound on |shift[j]| over all jobs (the table lives on the device; the entry plans its kernel from the
 * bound), or -1 for "unknown" (the general kernel).  A job whose shifts exceed a stated bound gets NaN gradients, not wrong ones.
 * dy_bs / x_bs may exceed C*L: what lies between two items of a job's dy or x is read and counted as zeros, as in ssv_conv1d_bwd_weight.
 * Split-bf16 mode only, B*L >= 256 (ssv_conv1d_bwd_weight_multi_ok). */
typedef struct {
  const float* dy; const float* x; float* dw; const float* part; float* pgrads;
  int shift[3]; int pad_;
  const float* dy_amax; const float* x_amax;   /* split-fp16 (mode 2): the two operands' scale lists, WHOLE lists (all batch items) ... */
  int dy_namax, x_namax;                       /* ... and their total entry counts (B * entries per item); ignored in the other modes */
} ssv_wgrad_job;
int ssv_conv_shifts(int k, int dilation, int causal, int* shift3);
int ssv_conv1d_bwd_weight_multi_ok(int B, int Cin, int Cout, int L, int k);
int ssv_conv1d_bwd_weight_multi_splits(int njobs, int B, int Cin, int Cout, int L, int k);   /* the Z the entry will use */
size_t ssv_conv1d_bwd_weight_multi_workspace(int njobs, int B, int Cin, int Cout, int L, int k);
int ssv_conv1d_bwd_weight_multi(const ssv_wgrad_job* jobs_dev, int njobs, long dy_bs, long x_bs, int B, int Cin, int Cout, int L, int k, int max_shift,
                                int n2, int nblk, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* highwayConv backward without the weight gradient: dx, plus dh (B,2C,L) dense and the partial rows `part` for the job.
 * `part` has room for ssv_ln_partial_rows(B, L) rows (of 6C floats; 3 Cout for the pointwise entry); the launch WRITES the first
 * ssv_ln_bwd_partial_rows(gate, B, C, L, with_amax) of them -- one per column tile of the kernel it picks for the shape (gate = 1: highway
 * gate over C channels, 0: LayerNorm + activation over C = Cout channels; with_amax = whether the call passes a scale-list output) -- and
 * that count is the `nblk` of the job (the rest of the buffer is not read). */
int ssv_ln_partial_rows(int B, int L);
int ssv_ln_bwd_partial_rows(int gate, int B, int C, int L, int with_amax);
size_t ssv_highway_conv1d_bwd_data_workspace(int B, int C, int L, int k);
int ssv_highway_conv1d_bwd_data(const float* dy, long dy_bs, const float* x, long x_bs, const float* w, const void* w_packed,
                                const float* g1, const float* b1, const float* g2, const float* b2, const float* h, const float* stats,
                                float* dx, long dx_bs, float* dh, float* dh_amax, float* part, int B, int C, int L, int k, int dilation, int causal,
                                void* ws, size_t ws_bytes, ssv_stream_t stream);   /* dh_amax (B * ssv_amax_rows(L), may be NULL): scale list of dh for the job */
/* The same for y = act(LN(conv1x1(x) [+ s])): dx (may be NULL), ds (may be NULL), dpre (B,Cout,L) dense and part (rows, 3 Cout). */
size_t ssv_pointwise_conv_ln_act_bwd_data_workspace(int B, int Cin, int Cout, int L);
int ssv_pointwise_conv_ln_act_bwd_data(const float* dy, long dy_bs, const float* w, const void* w_packed, const float* gamma, const float* beta,
                                       const float* pre, const float* stats, float* dx, long dx_bs, float* ds, float* dpre, float* dpre_amax,
                                       float* part, int B, int Cin, int Cout, int L, int act, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* ---- highwayConv ---------------------------------------------------------------------------------
 * Replaces highwayConv.forward, models/TTSModel.py:63-84:
 *   h = conv(x) (2C channels); y = sigmoid(LN1(h[:C])) * LN2(h[C:]) + (1 - sigmoid(LN1(h[:C]))) * x.
 * h (B,2C,L) dense and stats (B,4,L) = mean1, rstd1, mean2, rstd2 are saved for backward. */
size_t ssv_highway_conv1d_fwd_workspace(int B, int C, int L, int k);
int ssv_highway_conv1d_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                           const float* g1, const float* b1, const float* g2, const float* b2,
                           float* h, float* stats, float* y, long y_bs, float* y_amax,
                           int B, int C, int L, int k, int dilation, int causal,
                           void* ws, size_t ws_bytes, ssv_stream_t stream);   /* y_amax: as in ssv_channel_ln_act_fwd */
size_t ssv_highway_conv1d_bwd_workspace(int B, int C, int L, int k);
/* Outputs: dx (B,C,L), dw (2C,C,k), pgrads (6,C) = dgamma1, dbeta1, dgamma2, dbeta2, dbias[:C], dbias[C:]. */
int ssv_highway_conv1d_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed,
                           const float* g1, const float* b1, const float* g2, const float* b2,
                           const float* h, const float* stats, float* dx, long dx_bs, float* dw, float* pgrads,
                           int B, int C, int L, int k, int dilation, int causal,
                           void* ws, size_t ws_bytes, ssv_stream_t stream);

/* Building block of the above: only the gate + two LayerNorm backward.  dh (B,2C,L) dense = dL/dh (the conv output
 * gradient), dxres = dy*(1-gate) (the residual-path part of dL/dx), pgrads (6,C) as above.  A caller can then run
 * ssv_conv1d_bwd_data(dh, ..., dx_add = dxres) and ssv_conv1d_bwd_weight(dh, x, ...) on two different streams.  pgrads may be NULL (as in ssv_channel_ln_act_bwd). */
size_t ssv_highway_gate_bwd_workspace(int B, int C, int L);
int ssv_highway_gate_bwd(const float* dy, long dy_bs, const float* x, long x_bs,
                         const float* g1, const float* b1, const float* g2, const float* b2,
                         const float* h, const float* stats, float* dh, float* dxres, long dx_bs, float* pgrads,
                         int B, int C, int L, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* ---- textEmbedding -------------------------------------------------------------------------------
 * Replaces textEmbedding.forward, models/TTSModel.py:25-35 (one-hot scatter + Linear):
 * y(b,e,n) = w[e, ids(b,0,n)] + bias[e]; w is the nn.Linear weight (E, vocab).  ids int64 (B,1,N);
 * an id outside [0, vocab) contributes the bias only (the reference would raise in scatter_). */
int ssv_text_embed_fwd(const int64_t* ids, const float* w, const float* bias, float* y,
                       int B, int N, int E, int vocab, ssv_stream_t stream);
int ssv_text_embed_bwd(const int64_t* ids, const float* dy, float* dw, float* dbias,
                       int B, int N, int E, int vocab, ssv_stream_t stream);

/* ---- attention (training) ------------------------------------------------------------------------
 * Replaces models/TTSModel.py:266-270: A = softmax_N(K^T Q / sqrt(d)); R = V A; cat(R, Q).
 * k, v: (B,d,N) with batch stride kv_bs; q: (B,d,T); a: (B,N,T) dense (returned attention, saved);
 * r: (B,d,T) with batch stride r_bs (pass the first half of the (B,2d,T) decoder input). */
int ssv_attention_train_fwd(const float* k, const float* v, long kv_bs, const float* q, long q_bs,
                            float* a, float* r, long r_bs, int B, int d, int N, int T, ssv_stream_t stream);
/* ABI 5: the decoder's input cat(R, Q) (models/TTSModel.py:270) in the same call -- rq (B, 2d, T): R in rows [0, d), a copy of Q in rows [d, 2d).
 * For d % 64 == 0, d <= 256, N <= 192 scores, softmax and V A run in ONE launch (exact-fp32 MFMA, attn_fused.hip). */
int ssv_attention_train_fwd_rq(const float* k, const float* v, long kv_bs, const float* q, long q_bs, float* a, float* rq, long rq_bs,
                               int B, int d, int N, int T, ssv_stream_t stream);
size_t ssv_attention_train_bwd_workspace(int B, int d, int N, int T);
/* dr: grad of R; da_ext: extra dL/dA (guided-attention loss), may be NULL; dq_add: gradient reaching
 * Q through the concatenation, added into dq (may be NULL).  dk, dv have batch stride dkv_bs. */
int ssv_attention_train_bwd(const float* dr, long dr_bs, const float* da_ext, const float* dq_add, long dq_add_bs,
                            const float* k, const float* v, long kv_bs, const float* q, long q_bs, const float* a,
                            float* dk, float* dv, long dkv_bs, float* dq, long dq_bs,
                            int B, int d, int N, int T, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* ---- attention (one synthesis step) ---------------------------------------------------------------
 * Replaces models/TTSModel.py:281-291 for the newest frame: logits of the last query column, masked
 * outside the text window [pma, pma+2] with -2^32 (:282-286), softmax over N, argmax -> pma_out.
 * q_last: (B,d) column t of Q (element stride q_cs between channels, batch stride q_bs);
 * a: (B,N,a_T) attention buffer, column `col` is written.  pma_in/pma_out int64 (B). */
int ssv_attention_step(const float* k, long kv_bs, const float* q_last, long q_bs, long q_cs,
                       const int64_t* pma_in, float* a, int a_T, int col, const int* col_dev, int64_t* pma_out,
                       int B, int d, int N, ssv_stream_t stream);
/* col_dev (DEVICE int*, may be NULL): when given, the frame index is *col_dev instead of `col` and q_last must point at
 * column 0 of Q -- one captured hipGraph of a fixed-shape synthesis step can then be replayed for every frame.
 * With col_dev the frame index is NOT range-checked, on the host or in the kernel: the caller must keep *col_dev below a_T.
 * ssv_synth_advance closes such a step: mel_in[b][f][*col_dev + 1] = y[b][f][*col_dev] (both (B,F,T) dense; the frame just
 * synthesised is the next input, synthesize.py:108-109), then *col_dev += 1. */
int ssv_synth_advance(const float* y, float* mel_in, int* col_dev, int B, int F, int T, ssv_stream_t stream);
/* r(b,c,t) = sum_n v(b,c,n) a(b,n,t) for t < T (a has row stride a_T). */
int ssv_attention_apply(const float* v, long kv_bs, const float* a, int a_T, float* r, long r_bs,
                        int B, int d, int N, int T, ssv_stream_t stream);

/* ---- ConvTranspose1d(kernel 2, stride 2) ----------------------------------------------------------
 * Replaces upsampling.deconv, models/TTSModel.py:309,314.  w: (Cin, Cout, 2) as nn.ConvTranspose1d.
 * y(b,o,2t+j) = bias[o] + sum_c w[c,o,j] x(b,c,t). */
size_t ssv_deconv1d_k2s2_fwd_workspace(int Cin, int Cout);   /* pre-split weights (when no resident planes are given) */
/* ABI 7: w_packed = the resident planes of the 1x1 weight w.view(Cin, 2 Cout, 1) (ssv_conv_pack_multi; NULL: split here) -- the forward is ONE product over
 * 2 Cout rows whose epilogue interleaves the row pairs --, and y_amax (may be NULL) receives y's operand-scale list, y_namax entries per item
 * (mode 2 only; the other modes leave it untouched.  One entry per tile of the product; with more tiles per item than y_namax -- long sequences, small batches --
 * the product runs without the list and one ssv_absmax launch over y fills it: every length works). */
int ssv_deconv1d_k2s2_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                          float* y, long y_bs, float* y_amax, int y_namax, int B, int Cin, int Cout, int L, void* ws, size_t ws_bytes, ssv_stream_t stream);
size_t ssv_deconv1d_k2s2_bwd_workspace(int B, int Cin, int Cout);
/* dw may be NULL: the weight gradient is then left to the caller -- dw[:, :, j] is the k = 1 conv weight gradient of
 * (dy' = x, x' = dy[:, :, j::2]) and runs on the split-precision kernel through ssv_conv1d_bwd_weight once dy is de-interleaved,
 * which the stride-2 operand of this entry's own product (an exact-fp32 MFMA kernel) cannot; spoofsv_amd/ops.py does so. */
int ssv_deconv1d_k2s2_bwd(const float* dy, long dy_bs, const float* dy_amax, int dy_namax, const float* x, long x_bs, const float* w,
                          float* dx, long dx_bs, float* dw, float* dbias,
                          int B, int Cin, int Cout, int L, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* ---- losses ----------------------------------------------------------------------------------------
 * Replaces train/ordinary.py:230-231 / :249-250: out[0] = mean|gt - y|,
 * out[1] = mean(-gt*log(y+1e-8) - (1-gt)*log(1-y+1e-8)) over n elements (dense tensors). */
size_t ssv_spec_losses_workspace(long n);
int ssv_spec_losses_fwd(const float* y, const float* gt, long n, float* out, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* dy = gscale[0] * dl1/dy + gscale[1] * dbd/dy; gscale is a DEVICE pointer to 2 floats. */
int ssv_spec_losses_bwd(const float* y, const float* gt, long n, const float* gscale, float* dy, ssv_stream_t stream);
/* Both of the above in one pass over (y, gt) (ABI 7): `out` as ssv_spec_losses_fwd, `dy` as ssv_spec_losses_bwd for the gradient seed `gscale` (DEVICE pointer
 * to 2 floats) that the caller will hand to the backward -- a trainer knows it before the forward runs (train/ordinary.py:237,253: loss.backward()
 * seeds every term with 1).  The sums are taken in another order than ssv_spec_losses_fwd's (same value to fp32 rounding of a mean over n). */
int ssv_spec_losses_fwd_bwd(const float* y, const float* gt, long n, const float* gscale, float* out, float* dy, void* ws, size_t ws_bytes,
                            ssv_stream_t stream);
/* Replaces train/ordinary.py:232-234: out[0] = sum(a * gaw[:N,:T]) / (B*N*T); gaw row stride gaw_T. */
size_t ssv_guided_att_loss_workspace(int B, int N, int T);
int ssv_guided_att_loss_fwd(const float* a, const float* gaw, int gaw_T, float* out, int B, int N, int T,
                            void* ws, size_t ws_bytes, ssv_stream_t stream);
int ssv_guided_att_loss_bwd(const float* gaw, int gaw_T, const float* gscale, float* da, int B, int N, int T,
                            ssv_stream_t stream);

/* ---- length-masked training steps (additions; ABI version unchanged) ---------------------------------------------------------
 * One hipGraph captured at a bucket shape (N, T) serves every batch whose own maxima N_b <= N, T_b <= T (the reference's collates pad to
 * the batch's longest item, data/dataset.py:187-258).  `live` is a DEVICE int pointer to the live length (N_b or T_b), read by the
 * kernels at run time; `mult` scales it inside SSRN's upsampled stages (2 T_b, 4 T_b).  Live lengths are clamped to the tensor's extent.
 * ssv_mask_cols: x(b, c, t) = 0 for t >= mult * live[0] (x: (B, C, L), rows of L, batch stride x_bs); writes only the tail columns.
 * A layer's output masked this way, and its incoming gradient masked the same way before its backward runs, make every convolution see
 * the zero padding of the unpadded shape, and parameter gradients receive nothing from the padded columns. */
int ssv_mask_cols(float* x, long x_bs, int B, int C, int L, const int* live, int mult, ssv_stream_t stream);
/* models/TTSModel.py:266-270 on a padded batch: live[0] = N_b, live[1] = T_b.  Keys n >= N_b are left out of the column softmax (A = 0
 * there); columns t >= T_b of A and of R are 0.  Same outputs as ssv_attention_train_fwd_rq otherwise; the backward is
 * ssv_attention_train_bwd (A = 0 makes dS, dK, dV, dQ zero on the masked sets). */
int ssv_attention_train_fwd_rq_len(const float* k, const float* v, long kv_bs, const float* q, long q_bs, float* a, float* rq, long rq_bs,
                                   int B, int d, int N, int T, const int* live, ssv_stream_t stream);
/* train/ordinary.py:230-231 / :249-250 over the live columns t < mult * live[0] of (B, C, L) tensors, divided by B * C * (mult * live[0]);
 * dy (may be NULL; then gscale may be NULL too) receives the gradient for the DEVICE seed gscale (2 floats) inside the live columns and 0
 * outside.  Workspace ssv_spec_losses_workspace(B * C * L). */
int ssv_spec_losses_len(const float* y, const float* gt, int B, int C, int L, const int* live, int mult, const float* gscale,
                        float* out, float* dy, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* train/ordinary.py:232-234 over the live block n < live[0], t < live[1]: sum(a * gaw) / (B * N_b * T_b); the backward writes 0 outside the
 * block.  Workspace ssv_guided_att_loss_workspace(B, N, T). */
int ssv_guided_att_loss_fwd_len(const float* a, const float* gaw, int gaw_T, float* out, int B, int N, int T, const int* live,
                                void* ws, size_t ws_bytes, ssv_stream_t stream);
int ssv_guided_att_loss_bwd_len(const float* gaw, int gaw_T, const float* gscale, float* da, int B, int N, int T, const int* live,
                                ssv_stream_t stream);

/* ---- Resident pre-split weights ------------------------------------------------------------------
 * The split-bf16 conv kernels read weights as bf16 hi/lo planes in MFMA fragment order.  Splitting a weight costs one
 * small launch per conv call (forward order for the forward, transposed order for the data gradient): ~100 launches
 * per training step.  Instead a trainer can keep one caller-owned buffer of ssv_conv_pack_bytes() per weight and
 * refresh ALL of them with one launch after each optimizer step; the conv entry points then take that buffer as
 * w_packed.  A job table is planned once on the host (ssv_conv_pack_plan), copied to the device by the caller, and
 * replayed by ssv_conv_pack_multi (safe inside hipGraph capture). */
typedef struct { const float* w; void* planes; int M, K, Kpad, KT; long sm, sk; int first_block, pad_; float* inv_out; } ssv_pack_job;
size_t ssv_conv_pack_bytes(int Cout, int Cin, int k);   /* forward + transposed planes of one weight (Cout,Cin,k) + their two inverse scales (mode 2) */
/* Fills 2*n HOST jobs (forward, transposed per weight) for weights w[i] (DEVICE pointers, torch layout (Cout,Cin,k))
 * and their DEVICE buffers planes[i]; returns the number of workgroups ssv_conv_pack_multi must launch, or < 0. */
int ssv_conv_pack_plan(int n, const float* const* w, void* const* planes, const int* Cout, const int* Cin, const int* k,
                       ssv_pack_job* jobs_host);
/* The planes are written in the arithmetic mode in force at the call (bf16 or scaled fp16 halves): re-pack after ssv_set_precision.
 * ws (mode 2 only): ssv_conv_pack_multi_workspace(njobs) bytes for the weights' partial maxima. */
size_t ssv_conv_pack_multi_workspace(int njobs);
int ssv_conv_pack_multi(const ssv_pack_job* jobs_dev, int njobs, int nblocks, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* ---- Adam -------------------------------------------------------------------------------------------
 * Replaces optim.Adam(...).step(), train/ordinary.py:182,238 (config.json:41-46), for many tensors in
 * one launch.  `chunks` is a DEVICE array describing contiguous pieces of parameters. */
typedef struct { float* p; const float* g; float* m; float* v; long n; } ssv_adam_chunk;
/* step: 1-based step count.  If step_dev (DEVICE int*) is non-NULL the count is *step_dev + 1 and the
 * counter is incremented on the stream after the update, so a captured hipGraph advances on replay. */
int ssv_adam_multi(const ssv_adam_chunk* chunks, int nchunks, float lr, float beta1, float beta2, float eps,
                   int step, int* step_dev, ssv_stream_t stream);

/* ---- GE2E speaker embedder --------------------------------------------------------------------------
 * Replaces SpeechEmbedder.forward, GE2E/speech_embedder_net.py:27-33: 3-layer nn.LSTM(batch_first) ->
 * last frame -> Linear -> x / ||x||.  x: (Bn, T, F) row-major as the reference feeds it.
 * Weights in torch layout: w_ih[l] (4H, F or H), w_hh[l] (4H, H), b_ih[l], b_hh[l] (4H), gate order
 * i, f, g, o.  h_last: (Bn, H) output of the top layer at the last frame. */
size_t ssv_lstm_fwd_workspace(int Bn, int T, int F, int H, int layers);
int ssv_lstm_fwd(const float* x, const float* const* w_ih, const float* const* w_hh,
                 const float* const* b_ih, const float* const* b_hh, float* h_last,
                 int Bn, int T, int F, int H, int layers, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* The same forward for a caller that runs it again and again on FIXED weights (d-vector extraction, GE2E/dvector_create.py:100, batch after
 * batch): weights_packed != 0 promises that `ws` is the buffer of an earlier call with the same shape, arithmetic mode and weight VALUES, not
 * written by anyone since -- the call then skips the weights' scale scans and the split into fp16 / bf16 planes.  0 = ssv_lstm_fwd. */
int ssv_lstm_fwd_cached(const float* x, const float* const* w_ih, const float* const* w_hh,
                        const float* const* b_ih, const float* const* b_hh, float* h_last,
                        int Bn, int T, int F, int H, int layers, void* ws, size_t ws_bytes, int weights_packed, ssv_stream_t stream);
/* e = normalize(h W^T + b): h (Bn,H), w (P,H), e (Bn,P).  norms (Bn, may be NULL): |h W^T + b| per row, kept for the backward. */
size_t ssv_proj_l2norm_fwd_workspace(int Bn, int P);
int ssv_proj_l2norm_fwd(const float* h, const float* w, const float* bias, float* e, float* norms, int Bn, int H, int P,
                        void* ws, size_t ws_bytes, ssv_stream_t stream);
/* Backward: de (Bn,P) -> dh (Bn,H), dw (P,H), dbias (P). */
size_t ssv_proj_l2norm_bwd_workspace(int Bn, int P);
int ssv_proj_l2norm_bwd(const float* de, const float* e, const float* norms, const float* h, const float* w,
                        float* dh, float* dw, float* dbias, int Bn, int H, int P, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* Training (GE2E/train_speech_embedder.py:77-83): the same LSTM forward, keeping every frame of h, c and
 * the activated gates in `saved` (caller-owned, ssv_lstm_saved_bytes), and backpropagation through time from dh_last
 * (Bn,H) to the gradients of all weights and biases (arrays of `layers` DEVICE pointers, torch layouts).  No shape or mode
 * limits (nn.LSTM + autograd have none, GE2E/speech_embedder_net.py:19): in a split mode with hidden % 32 == 0 and
 * batch >= 8 the (layer, frame) wavefront kernels run in that mode's arithmetic; every other case -- mode 0, any other
 * hidden size, fewer than 8 utterances -- runs frame by frame on the exact-fp32 MFMA GEMMs.  One `saved` layout for both;
 * forward and backward of one iteration must run in the same mode. */
size_t ssv_lstm_saved_bytes(int Bn, int T, int F, int H, int layers);
size_t ssv_lstm_train_fwd_workspace(int Bn, int T, int F, int H, int layers);
int ssv_lstm_train_fwd(const float* x, const float* const* w_ih, const float* const* w_hh,
                       const float* const* b_ih, const float* const* b_hh, float* h_last, void* saved,
                       int Bn, int T, int F, int H, int layers, void* ws, size_t ws_bytes, ssv_stream_t stream);
size_t ssv_lstm_bwd_workspace(int Bn, int T, int F, int H, int layers);
int ssv_lstm_bwd(const float* dh_last, const void* saved, const float* const* w_ih, const float* const* w_hh,
                 float* const* dw_ih, float* const* dw_hh, float* const* db_ih, float* const* db_hh,
                 int Bn, int T, int F, int H, int layers, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* Replaces GE2ELoss.forward, GE2E/speech_embedder_net.py:43-49 with GE2E/utils.py:16-55.
 * emb (N,M,D); w, b device scalars; loss[0] = total; per (N,M) per-embedding losses (may be NULL). */
size_t ssv_ge2e_loss_fwd_workspace(int N, int M, int D);
int ssv_ge2e_loss_fwd(const float* emb, const float* w, const float* b, float* loss, float* per,
                      int N, int M, int D, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* Backward of the above (autograd of GE2ELoss.forward; GE2E/train_speech_embedder.py:82): dloss is the upstream gradient
 * of the scalar loss (DEVICE float, NULL = 1).  demb (N,M,D), dw, db (DEVICE scalars). */
size_t ssv_ge2e_loss_bwd_workspace(int N, int M, int D);
int ssv_ge2e_loss_bwd(const float* emb, const float* w, const float* b, const float* dloss, float* demb, float* dw, float* db,
                      int N, int M, int D, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* GE2E training on a corpus held on the device: the batch assembly and the tail of one iteration.
 *
 * Replaces SpeakerDatasetTIMITPreprocessed.__getitem__, GE2E/data_load.py:77-85 (`utters[utter_index]`, `np.transpose(.., (0,2,1))`,
 * then the DataLoader's stack and upload), for a whole batch: corpus (U_total, nmels, frames) holds every speaker's utterances,
 * rows (Bn = N*M int32, DEVICE) the batch's global utterance rows, out (Bn, frames, nmels) is what ssv_lstm_train_fwd takes:
 * out[b][t][f] = corpus[rows[b]][f][t].  Rows may repeat (np.random.randint draws with replacement).  The table is not read on
 * the host: the caller, who drew it, validates it before the upload.  A row outside [0, U_total) is never dereferenced; its
 * utterance is written as NaN.  Any (nmels, frames): the transpose is tiled. */
int ssv_tisv_batch_gather(const float* corpus, long U_total, const int* rows, float* out, int Bn, int nmels, int frames, ssv_stream_t stream);
/* Replaces clip_grad_norm_(embedder_net.parameters(), 3.0), clip_grad_norm_(ge2e_loss.parameters(), 1.0) and
 * optimizer.step() (optim.SGD), GE2E/train_speech_embedder.py:84-86, for all parameters in two launches.  `chunks` is a DEVICE array
 * of contiguous pieces of parameters (any n >= 1) with their clipping group, 0 <= group < ngroups <= SSV_CLIP_SGD_MAX_GROUPS;
 * max_norm is a HOST array of ngroups floats, read during the call.  Per group: S = sum g^2 in double (one partial per piece, added
 * in piece order), norms[group] = sqrt(S) (DEVICE floats, ngroups of them: what clip_grad_norm_ returns),
 * coef = min(1, max_norm / (sqrt(S) + 1e-6)) in double, rounded once to float, step = lr * coef in float, p <- p - step * g
 * (product and difference each rounded once).  No atomics and no arrival order anywhere: the same inputs give the same bits.  A
 * non-finite gradient propagates as with error_if_nonfinite=False.
 * DIFFERENCE from the reference: the gradients are NOT rescaled in memory (clip_grad_norm_ multiplies them by coef in place; nothing
 * reads them before the next zero_grad()).
 * loss, loss_hist, hist_len, step_dev (DEVICE, optional): loss_hist[*step_dev % hist_len] = *loss and *step_dev += 1, inside the second
 * launch, so that a replayed hipGraph fills successive slots and the host reads losses back when it wants them (the step_dev
 * convention of ssv_adam_multi).  step_dev alone counts the calls.  ws: ssv_clip_sgd_workspace(nchunks) bytes (a long, like the n of
 * the tables: one double per piece). */
#define SSV_CLIP_SGD_MAX_GROUPS 8
typedef struct { float* p; const float* g; long n; int group; int pad_; } ssv_clip_sgd_chunk;
long ssv_clip_sgd_workspace(int nchunks);
int ssv_clip_sgd_multi(const ssv_clip_sgd_chunk* chunks, int nchunks, const float* max_norm, int ngroups, float lr, float* norms,
                       const float* loss, float* loss_hist, int hist_len, int* step_dev, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* The speaker-verification test on the device: trial scores, threshold sweep, accept rate.  No workspace: every table is the caller's and
 * its size follows from the arguments.
 *
 * Replaces get_centroids + get_cossim as the tests call them, GE2E/train_speech_embedder.py:151-164 and :244-257 (GE2E/utils.py), in ONE
 * launch: enr (N, E, D) enrolment embeddings, ver (N, ver_stride, D) verification embeddings of which each speaker's first V rows are used
 * (test_nospoof scores the first 2*eval_num only), sim (N, V, N) out, cent (N, D) out or NULL: the enrolment centroids enr.mean(1).
 *   sim[i,v,j] = cos(ver[i,v], cent[j]) + 1e-6                                  for j != i,
 *   sim[i,v,i] = cos(ver[i,v], (sum_v' ver[i,v'] - ver[i,v]) / (V - 1)) + 1e-6  (the sum over the V rows in use; utils.py:42-43),
 * cos(a, b) = a.b / (max(|a|, 1e-8) * max(|b|, 1e-8)) as the reference's F.cosine_similarity clamps each norm.  fp32; every sum in a fixed order
 * that depends on D alone (not on the grid or the run).  Centroids and the speaker's sum are staged in LDS, tiled over j when N * D does
 * not fit; any size runs.  N < 2, V < 2, E < 1, V > ver_stride or D < 1: -1 before anything is launched. */
int ssv_sv_trial_scores(const float* enr, const float* ver, float* sim, float* cent, int N, int E, int V, int ver_stride, int D, ssv_stream_t stream);
/* Replaces the threshold loops of GE2E/train_speech_embedder.py:174-194 (test) and :264-284 (test_nospoof).  sim (N, V, N); thr: DEVICE
 * array of nthr float32 thresholds (the caller uploads the float32 roundings of 0.01*i + 0.5 once); head / tail: rows of the own-speaker
 * column that form the genuine / the spoofing half (0, 0: the no-spoof variant, gt_FRR and spoof_rate are then 0).  counts (nthr, 4) int32
 * OUT: per threshold the trials with sim > thr (strict) over the whole matrix, the own-speaker column, its first `head` rows, its last
 * `tail` rows.  Then, in float64 and in the reference's operation order, with the host-computed constants den, pos (full sweep) and
 * hden, hpos (half sweep):
 *   FAR = (all - own) / (N - 1.0) / den / N,  FRR = (N * pos - own) / den / N,  the FIRST threshold with the smallest |FAR - FRR| (strict
 *   <, starting from 1.0) wins;  gt_FRR = (N * hpos - own_head) / hden / N,  spoof_rate = own_tail / hden / N at that threshold.
 * hist (hist_len, 6) float64: row *step_dev % hist_len = (EER = (FAR + FRR) / 2, index of the threshold, FAR, FRR, gt_FRR, spoof_rate),
 * then *step_dev += 1 (the step_dev convention of ssv_clip_sgd_multi: a replayed hipGraph fills successive rows).  Two launches. */
int ssv_sv_eer_sweep(const float* sim, int N, int V, const float* thr, int nthr, int head, int tail, double den, double pos, double hden,
                     double hpos, int* counts, double* hist, int hist_len, int* step_dev, ssv_stream_t stream);
/* Replaces the body of the spoof-rate pass, GE2E/train_speech_embedder.py:313-321, over a DEVICE stack of nmat matrices (N, V, N):
 * rates[m] (float32) = trials of the own-speaker column in the last `tail` rows with sim > thres, / float(tail) / N.  The comparison is
 * float32 against the float32 rounding of the threshold, as the reference's `mat > thres` compares a float32 matrix with a Python float. */
int ssv_sv_accept_rate(const float* sim_stack, int nmat, int N, int V, int tail, float thres, float* rates, ssv_stream_t stream);
/* The counting of the GE2E sweep of curve.py:15-25 (5,000 thresholds over a similarity matrix), over a DEVICE stack of nmat matrices
 * (N, V, N) in ONE launch that reads every matrix once per tile of ssv_sv_curve_tile() thresholds (ssv_sv_eer_sweep reads it once per
 * threshold).  thr: DEVICE array of nthr float32 thresholds, NON-DECREASING (duplicates allowed; not checked on the device: the caller
 * checks before the upload).  counts (nmat, nthr, 4) int32 OUT, the four columns of ssv_sv_eer_sweep per matrix: trials with
 * sim > thr[t] (strict, float32) over the whole matrix, the own-speaker column, its first `head` rows, its last `tail` rows
 * (head + tail > V is allowed: a row may be in both).  A NaN score is accepted by no threshold, +inf by every finite one, -inf by none.
 * Every element of counts is written and nothing is added to what it held.  Integer sums in LDS, no global atomics: the same bits on
 * every run.  nmat, N, V, nthr < 1, head or tail outside [0, V]: -1 before anything is launched; more than 2^31 - 1 trials per matrix
 * (or more than 65535 matrices): -2. */
int ssv_sv_score_curve(const float* sim_stack, int nmat, int N, int V, int head, int tail, const float* thr, int nthr, int* counts, ssv_stream_t stream);
/* The same for a list of n scores with a class code each -- the counting of the i-vector sweep of curve.py:45-49 (real and fake score
 * arrays against 8,000 thresholds) and of kaldi_ivectors/ivector_spoofrate.py:18-22 (one threshold): counts (nthr, nclass) int32 OUT,
 * counts[t][c] = items with cls[e] == c and scores[e] > thr[t] (strict, in the scores' own type); 1 <= nclass <= 4, an item whose code
 * is >= nclass is counted nowhere.  scores, cls, thr on the DEVICE, thr non-decreasing.  _f64 compares float64 scores with float64
 * thresholds as the reference's numpy arrays do; _f32 serves float32 score vectors.  n < 1, nthr < 1, nclass outside [1, 4]: -1;
 * n > 2^31 - 1: -2. */
int ssv_score_list_curve_f32(const float* scores, const unsigned char* cls, long n, int nclass, const float* thr, int nthr, int* counts, ssv_stream_t stream);
int ssv_score_list_curve_f64(const double* scores, const unsigned char* cls, long n, int nclass, const double* thr, int nthr, int* counts, ssv_stream_t stream);
int ssv_sv_curve_tile(void);      /* thresholds one workgroup of the three entries above owns (tests put nthr on its edges) */

/* ---- I-vector groundwork: cepstral features, diagonal UBM, Baum-Welch statistics (additions; ABI version unchanged) ----
 * The bottom of the reference's kaldi_ivectors/run.sh (MFCC -> VAD -> diagonal UBM -> ...), as far as the diagonal UBM and the
 * per-utterance statistics.  Kaldi's binaries are NOT reproduced (its MFCC window, snip-edges, energy, VAD and the recipe's conf/ values
 * are unknown here); the algorithms are the ones stated below.  All arithmetic is independent of ssv_set_precision: the two products run
 * on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains).  No float atomics, the same inputs give the same bits; nothing is read on the host
 * except where an argument is said to be a HOST array.  Bad arguments: -1; a shape beyond a kernel's tiles: -2; both before any launch.
 *
 * Features.  mel (G, M): the compact frames-major log-mel array of the d-vector path; utt_off (U + 1) int64 DEVICE, ascending: frames
 * [utt_off[u], utt_off[u+1]) are utterance u (T frames; T = 0 writes nothing; frames in no utterance are not written).  dct (Cc, M) or
 * NULL (then the statics are mel itself and Cc must equal M).  out (G, Cc * (delta_order + 1)), rows [s, d, dd]:
 *   s_t = dct . mel_t;   d_t = sum_{j=-w..w} c_j s_{clamp(t+j)},  c_j = j / (2 sum_{i=1..w} i^2);   dd_t = sum_{j=-2w..2w} (c (*) c)_j s_{clamp(t+j)},
 *   clamp to [0, T-1] (the order of sid/train_diag_ubm.sh: add-deltas, then sliding CMN);  then on ALL columns the centred sliding mean over
 *   W = cmn_window frames: lo = t - W/2, hi = lo + W; lo < 0: lo = 0, hi = min(T, W); hi > T: hi = T, lo = max(0, T - W);
 *   out_t = v_t - mean(v[lo:hi]), no variance normalisation.  The window sum is slid in double (never a float32 prefix sum).
 * ws: ssv_ivec_features_workspace bytes (the rows before the mean subtraction).  Cc <= 128, delta_window <= 8, else -2. */
long ssv_ivec_features_workspace(long G, int Cc, int delta_order);      /* bytes (a long, like its G; 0 for arguments the entry refuses) */
int ssv_ivec_features(const float* mel, const long* utt_off, const float* dct, float* out, long G, int M, int U, int Cc, int delta_window,
                      int delta_order, int cmn_window, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* Gaussian selection and posteriors of a diagonal-covariance GMM.  X (F, D); planes A = mu / var (C, D), B = -1/2 / var (C, D),
 * g (C) = log w_c - 1/2 sum_d (log 2 pi var_cd + mu_cd^2 / var_cd), float32 (ssv_gmm_diag_update / ssv_gmm_diag_planes write them; with
 * D % 4 == 0 the planes must be 16-byte aligned).  L_fc = sum_d A_cd x_fd + sum_d B_cd x_fd^2 + g_c, one (F x 2D)(2D x C) product whose
 * tile of ssv_gmm_frame_tile(D, C) frames x ALL C columns stays in LDS.  Per frame: the nsel largest L, by descending L and, among equal
 * values, ascending index -> idx (F, nsel) int32; loglik (F) = log-sum-exp over the selected; post (F, nsel) = the soft max over the
 * selected, entries below min_post set to 0 and the rest renormalised to sum 1 (min_post = 0: no pruning; the largest is never pruned).
 * The dense (F, C) posterior matrix is never written.  Range: 1 <= D <= 128, nsel <= C <= 2048, nsel <= 32, any F >= 1; beyond: -2. */
int ssv_gmm_frame_tile(int D, int C);      /* host-only query: frames one workgroup of ssv_gmm_diag_gselect owns (tests put F on its edges) */
int ssv_gmm_diag_gselect(const float* X, const float* A, const float* B, const float* g, int* idx, float* post, float* loglik, long F, int D, int C,
                         int nsel, float min_post, ssv_stream_t stream);
/* Sufficient statistics per segment: slab (S, C, 1 + order * D) float32, slab[s][c] = sum over f in [seg_off[s], seg_off[s+1]) of
 * gamma_fc [1, x_f, x_f^2] (order = 1: [1, x_f]), gamma given sparsely by idx / post (F, nsel) as ssv_gmm_diag_gselect writes them: the
 * product Gamma^T [1, X, X^2] with K = frames, a workgroup per (segment, 64 Gaussians).  seg_off (S + 1) int64 DEVICE.  seg_off_host: the
 * same table as a HOST array, or NULL: when given it is checked here -- ascending, inside [0, F], else -1; the device clamps what it reads
 * to [0, F] and takes a descending pair as empty, so nothing is followed out of bounds either way.  A segment of length 0 gives exact
 * zeros; an idx outside [0, C) is skipped; a repeated idx in a row adds.  Segments = utterances, order 1: the Baum-Welch statistics
 * (N_u, F_u); segments = runs of <= 2048 frames, order 2: the partial sums of an EM pass.  A sum is fp32 chains over 64 frames each, added
 * in double along the segment and rounded once to float32.
 * ssv_gmm_stats_reduce: out (n) float64 = sum over s of slab (S, n), added in ascending s, in double. */
int ssv_gmm_diag_stats(const float* X, const int* idx, const float* post, const long* seg_off, const long* seg_off_host, float* slab, long F, int D,
                       int C, int nsel, int S, int order, ssv_stream_t stream);
int ssv_gmm_stats_reduce(const float* slab, double* out, int S, long n, ssv_stream_t stream);
/* M-step, one launch, all in float64.  stats (C, 1 + 2 D) float64 = (N_c, F_c, S_c); w (C) OUT, mu, var (C, D) IN / OUT:
 *   w_c = N_c / sum N;  mu = F / N;  var = max(S / N - mu^2, var_floor);  a Gaussian with N_c < min_count (or N_c <= 0) keeps its mu and var
 *   and takes weight max(w_c, min_weight); then the weights are renormalised to sum 1.  (This rule is the project's own: Kaldi removes or
 *   splits such a Gaussian.)  A, B (C, D) and g (C) float32 OUT: the planes of the new parameters, each rounded once from double.
 * ssv_gmm_diag_planes: the planes alone, of given w, mu, var.  C <= 2048, D <= 128, else -2. */
int ssv_gmm_diag_update(const double* stats, double* w, double* mu, double* var, float* A, float* B, float* g, int C, int D, double var_floor,
                        double min_count, double min_weight, ssv_stream_t stream);
int ssv_gmm_diag_planes(const double* w, const double* mu, const double* var, float* A, float* B, float* g, int C, int D, ssv_stream_t stream);

/* ---- I-vector groundwork: full-covariance UBM (additions; ABI version unchanged) ----
 * The second link of kaldi_ivectors/run.sh (sid/train_full_ubm.sh), between the diagonal UBM above and the extractor below.  The model is
 * OURS, stated here; Kaldi's fgmm-global-* binaries (eigenvalue flooring, Gaussian removal) are NOT reproduced.  All arithmetic is
 * independent of ssv_set_precision; no float atomics; the order of every sum follows from the shapes and the selection lists alone, so
 * the same inputs give the same bits.  Limits: 1 <= D <= 128, 1 <= C <= 2048, 1 <= nsel <= 32, F nsel < 2^31.  Bad arguments: -1; beyond
 * the limits: -2; both before any launch.
 *
 * Mixture: w (C), mu (C, D), cov (C, Pd) float64, Pd = D (D + 1) / 2, cov_c the PACKED lower triangle of Sigma_c, row-major (element
 * (i, j), j <= i, at i (i + 1) / 2 + j).  Sigma_c = L_c L_c^T (Cholesky), W_c = L_c^-1 (lower triangular).  The log-likelihood is taken
 * in the centred, whitened form, in which nothing cancels:
 *   z = W_c (x - mu_c),   L_fc = g_c - 1/2 |z|^2,   g_c = log w_c - 1/2 (D log 2 pi + log|Sigma_c|),
 * x - mu_c being ONE float32 subtraction on mu rounded once, before any product.  Planes: Wt (C, D, D) float32, Wt[c][i][j] = W_c (i, j),
 * exact zeros above the diagonal; muf (C, D) and g (C) float32; each rounded once from double; icov (C, Pd) float64 = packed Sigma_c^-1
 * (for ssv_ivec_tv_planes_full).
 *
 * ssv_fgmm_planes: a workgroup per Gaussian, float64, the packed triangle in LDS: Cholesky, the triangular inverse, W^T W (LAPACK's
 * potrf / trtri / lauum forms, as ssv_ivec_estep), log|Sigma| from the pivots.  A pivot that is not positive: that Gaussian's Wt, muf,
 * g and icov are NaN and nothing else is touched. */
int ssv_fgmm_planes(const double* w, const double* mu, const double* cov, float* Wt, float* muf, float* g, double* icov, int C, int D,
                    ssv_stream_t stream);
/* The Gaussian-major selection lists of idx (F, nsel) int32 as ssv_gmm_diag_gselect writes it.  Slot f * nsel + j belongs to the list of
 * Gaussian idx[f][j]; start (C + 1) int32 and pairs (F nsel) int32 OUT: pairs[start[c] : start[c + 1]] = the slots of c in ASCENDING slot
 * order (a stable counting sort on the device; integer counts, and no position depends on the order in which anything ran).  An idx
 * outside [0, C) belongs to no list; pairs beyond start[C] are not written.  ws: ssv_fgmm_group_workspace bytes.
 * ssv_fgmm_pair_tile: pairs of a list one workgroup of the two product entries below owns per step (tests put list lengths on its edges).
 * A list is split into runs of whole tiles, ssv_fgmm_stats_runs(F, nsel, C) of them for the statistics: the count follows from the shapes
 * alone and a run's extent from the list's length alone.  The *_workspace queries return bytes, 0 for arguments the entries refuse. */
int ssv_fgmm_pair_tile(void);
int ssv_fgmm_stats_runs(long F, int nsel, int C);
long ssv_fgmm_group_workspace(long F, int nsel, int C);
long ssv_fgmm_post_workspace(long F, int nsel);
long ssv_fgmm_stats_workspace(long F, int nsel, int C, int D);
int ssv_fgmm_group_selection(const int* idx, int* start, int* pairs, long F, int nsel, int C, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* Posteriors over a given selection.  A workgroup owns (Gaussian c, run of its list): Wt_c is staged in LDS once and serves every pair of
 * the run; per tile the pairs' frame rows are gathered into LDS and centred on muf_c, Z = Xc Wt_c^T runs on v_mfma_f32_16x16x4_f32 (K = D:
 * the fp32 rate does not limit it), |z|^2 is added along the row and L is written per slot.  A frame-major finish then takes, over the
 * frame's slots in idx's order: loglik (F) = log-sum-exp of L, post (F, nsel) = the soft max, entries below min_post set to 0 (never the
 * first largest) and the rest renormalised.  A slot whose idx lies outside [0, C) has posterior 0 and takes no part; a frame with no slot
 * inside has posteriors 0 and loglik -inf.  A frame's post and loglik do not depend on the other frames of the call: a row of the product
 * depends on its own K chain only.  ws: ssv_fgmm_post_workspace bytes (L per slot). */
int ssv_fgmm_select_post(const float* X, const float* Wt, const float* muf, const float* g, const int* idx, const int* start, const int* pairs,
                         float* post, float* loglik, long F, int D, int C, int nsel, float min_post, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* Statistics centred on the CURRENT mean, over each Gaussian's list: out (C, 1 + D + Pd) float64 = [N_c, S1_c, S2_c],
 *   N_c = sum gamma,   S1_c = sum gamma (x - mu_c),   S2_c = sum gamma (x - mu_c)(x - mu_c)^T (packed),   gamma = post[slot],
 * x - mu_c as above (muf).  Centring on the old mean is what keeps the M-step's Sigma = S2 / N - delta delta^T from cancelling.  Per tile
 * of 64 pairs S2 = (gamma Xc)^T Xc runs on the fp32 MFMA (K = the 64 pairs in list order) and S1, N are fp32 chains over the same pairs;
 * the tiles are added in double along the run, the run's sums rounded once to float32 into ws and the runs added in ascending order in
 * double (ssv_gmm_stats_reduce's kernel).  A pair of posterior 0 (pruned) is MULTIPLIED by its zero, not skipped.  An empty list gives
 * exact zeros.  ws: ssv_fgmm_stats_workspace bytes. */
int ssv_fgmm_stats(const float* X, const float* muf, const float* post, const int* start, const int* pairs, double* out, long F, int D, int C,
                   int nsel, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* M-step, a workgroup per Gaussian plus one launch for the weights, all in float64.  stats as ssv_fgmm_stats writes them;
 * w (C) OUT, mu (C, D) and cov (C, Pd) IN / OUT, kept (C) int32 OUT:
 *   delta = S1 / N;   mu <- mu + delta;   Sigma <- S2 / N - delta delta^T.
 * A Gaussian KEEPS its mu and cov bit for bit and has kept[c] = 1 when N_c < min_count (or N_c <= 0), or when the new Sigma has a
 * Cholesky pivot L_ii^2 < var_floor (or not positive) -- L_ii^2 is the conditional variance of dimension i given the dimensions before
 * it.  (The project's own rule: Kaldi floors eigenvalues and removes Gaussians.)  w_c = N_c / sum N, a kept Gaussian taking
 * max(w_c, min_weight), then renormalised to sum 1 (ssv_gmm_diag_update's rule).  Wt, muf, g, icov OUT: the planes of the result. */
int ssv_fgmm_update(const double* stats, double* w, double* mu, double* cov, float* Wt, float* muf, float* g, double* icov, int* kept, int C,
                    int D, double var_floor, double min_count, double min_weight, ssv_stream_t stream);

/* ---- I-vector extractor: total-variability EM, extraction, cosine trials (additions; ABI version unchanged) ----
 * The middle of kaldi_ivectors/run.sh (extractor training, i-vector extraction, trial scores) on the Baum-Welch statistics above.  The
 * model is OURS, stated here; Kaldi's ivector-extractor-* binaries (prior offset, weight projection, full covariances) are NOT reproduced
 * (the back end is the next section; the trial entry here scores by cosine on length-normalised vectors).  All arithmetic is independent of ssv_set_precision; no float
 * atomics; the order of every sum follows from the shapes alone.  Bad arguments: -1; a shape beyond a kernel: -2; both before any launch.
 * Limits of every entry that takes them: 1 <= R <= 192 (the packed float64 triangle of R = 192, 148,224 bytes, is the most one
 * workgroup's LDS holds), C <= 2048, D <= 128.
 *
 * Notation: UBM of C Gaussians in D dimensions (mu, var (C, D) float64); rank R, P = R (R + 1) / 2; T (C, D, R) float64.  A symmetric
 * R x R matrix is PACKED as its lower triangle, row-major: element (i, j), j <= i, at i (i + 1) / 2 + j.
 *
 * ssv_ivec_tv_planes: G (C * D, R) float32 = diag(1 / var_c) T_c and Pk (C, P) float32 = packed T_c^T diag(1 / var_c) T_c, summed over d
 * in double and rounded once.
 * ssv_ivec_centre_stats: Ft (U, C, D) = F - N mu, one float32 fused multiply-add per element (mu rounded once); Ft may be F. */
int ssv_ivec_tv_planes(const double* T, const double* var, float* G, float* Pk, int C, int D, int R, ssv_stream_t stream);
int ssv_ivec_centre_stats(const float* N, const float* F, const double* mu, float* Ft, long U, int C, int D, ssv_stream_t stream);
/* The same planes on a full-covariance UBM: icov (C, Pd) float64 = packed Sigma_c^-1 as ssv_fgmm_planes / ssv_fgmm_update write it;
 * G_c = Sigma_c^-1 T_c and Pk_c = packed T_c^T G_c, summed over d in double (ascending) and rounded once; outputs and layout as
 * ssv_ivec_tv_planes, and nothing below the planes knows the difference.  R < 1: -1; R > 192, C > 2048 or D > 128: -2. */
int ssv_ivec_tv_planes_full(const double* T, const double* icov, float* G, float* Pk, int C, int D, int R, ssv_stream_t stream);
/* The product family, on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains), all operands row-major:
 *   ssv_ivec_product:     out (m, n) float32 = A (m, K) B (K, n), rounded once;
 *   ssv_ivec_product_tn:  acc (m, n) float64 += A (U, m)^T B (U, n)  (K = U; acc persists across the passes of an accumulation).
 * K is walked in runs of ssv_ivec_product_run() = 256 elements, each an fp32 chain from zero accumulators, and the runs are added in
 * double registers: a single fp32 chain over K = C D = 61,440 would cost more digits than a blocked float32 product does.  Every
 * output element belongs to one workgroup (a tile of ssv_ivec_product_tile() = 64 rows and columns); the order of its sum depends on K
 * alone, so a row of the output does not depend on the rows that share its launch.  Used as Lp (U, P) = N Pk, b (U, R) = Ft G,
 * A (C, P) += N^T M, Cm (C D, R) += Ft^T w, Nc (C, 1) += N^T 1.  More than 65535 x 64 rows: -2. */
int ssv_ivec_product_run(void);
int ssv_ivec_product_tile(void);
int ssv_ivec_product(const float* A, const float* B, float* out, long m, long n, long K, ssv_stream_t stream);
int ssv_ivec_product_tn(const float* A, const float* B, double* acc, long U, long m, long n, ssv_stream_t stream);
/* E-step, a workgroup per utterance, in double on the packed triangle in LDS:  L_u = I + unpack(Lp_u),  w_u = L_u^-1 b_u (Cholesky, the
 * forward substitution on the way, then the back substitution),  obj_u = -1/2 log|L_u| + 1/2 b_u . w_u -- with posteriors and covariances
 * fixed, the utterance's marginal log-likelihood up to a constant in T -- and, when M is not NULL (training), the inverse in place
 * (LAPACK's trtri + lauum forms) and M_u = L_u^-1 + w_u w_u^T, packed.  w (U, R), M (U, P) float32, obj (U) float64.  M == NULL: nothing of M
 * is touched and w, obj are the same bits.  A pivot that is not positive cannot happen for N >= 0 (L >= I); met anyway (NaN input), the
 * utterance's w, obj and M are NaN and nothing else is touched. */
int ssv_ivec_estep(const float* Lp, const float* b, float* w, float* M, double* obj, long U, int R, ssv_stream_t stream);
/* M-step, a workgroup per Gaussian, all in float64:  T_c <- Cm_c A_c^-1 (A_c (P) packed, inverted in LDS by the E-step's functions; the D
 * rows of Cm_c stream past it), then T_c <- T_c J when J (R, R) is not NULL (the minimum-divergence step; J = chol_lower(mean M_u),
 * factorised by the caller).  A Gaussian with Nc[c] < min_count (or Nc[c] <= 0) keeps its T_c bit for bit -- J included; the project's own
 * rule, as for the starved Gaussian of ssv_gmm_diag_update.  A (C, P), Cm (C D, R), Nc (C) float64 as ssv_ivec_product_tn accumulates them;
 * T (C, D, R) IN / OUT. */
int ssv_ivec_tv_update(const double* A, const double* Cm, const double* Nc, const double* J, double* T, int C, int D, int R, double min_count,
                       ssv_stream_t stream);
/* Cosine trials in one launch: enroll (n_enroll, R), evalv (E, R) float32; spk_off (S + 1) int64 DEVICE, speaker s owning the enrolment
 * rows [spk_off[s], spk_off[s+1]) (spk_off_host: the same table as a HOST array or NULL; when given, checked here -- ascending, inside
 * [0, n_enroll], else -1; the device clamps what it reads and takes a descending pair as empty).  Every vector is length-normalised
 * (norm 0: the zero vector), a speaker model is the mean of its normalised enrolment vectors, normalised again and kept as float32 in
 * LDS, and scores (E, S) float32 = their dot products, summed in double and rounded once.  A zero vector, or a speaker without enrolment,
 * scores 0, never NaN.  S R 4 bytes beyond 128 KiB of LDS: -2. */
int ssv_ivec_cosine_trials(const float* enroll, const long* spk_off, const long* spk_off_host, const float* evalv, float* scores, long n_enroll, int S,
                           long E, int R, ssv_stream_t stream);

/* ---- I-vector back end: PLDA (additions; ABI version unchanged) ----
 * The last third of kaldi_ivectors/run.sh (ivector-compute-plda, ivector-plda-scoring --num-utts; compute-eer is host arithmetic in
 * spoofsv_amd/plda.py).  The model is OURS, stated here; Kaldi's binaries are NOT reproduced bit for bit.  1 <= R <= 192 as for the
 * extractor (R < 1: -1, R > 192: -2).  All arithmetic is independent of ssv_set_precision; no float atomics; the order of every sum follows
 * from the shapes alone.  Bad arguments: -1; a shape beyond a kernel: -2; both before any launch.  P = R (R + 1) / 2, packed as above.
 *
 * The model is two-covariance PLDA: x = mu + y_s + e, y_s ~ N(0, B) per speaker, e ~ N(0, W) per utterance.
 * Length normalisation: xh = x sqrt(R) / |x|; a zero vector stays zero.
 * Statistics: per speaker k with n_k >= 1 rows the mean m_k in double; the residual rows d_i = xh_i - m_s(i), rounded once to float32; the
 *   scatter Sigma = sum_i d_i d_i^T, taken on the residuals so that nothing cancels; mu = the unweighted mean over speakers of m_k.  Speakers
 *   without rows are left out of everything.
 * EM, from W = B = I, all in float64; per iteration, for every distinct count n among the speakers Mx_n = (B^-1 + n W^-1)^-1, then per speaker
 *   w_k = n_k Mx W^-1 (m_k - mu) and r_k = (m_k - mu) - w_k, and
 *   B <- (1/S) sum_k (Mx_{n_k} + w_k w_k^T),   W <- (Sigma + sum_k n_k (Mx_{n_k} + r_k r_k^T)) / N   (S speakers with rows, N rows).
 * Objective (the data's marginal log-likelihood up to a constant; EM may not decrease it):
 *   obj = (1/N) { -1/2 [(N - S) log|W| + tr(W^-1 Sigma)] - 1/2 sum_k [log|B + W/n_k| + (m_k - mu)^T (B + W/n_k)^-1 (m_k - mu)] }.
 * Finalise (host, float64, once per model): W = C C^T, C^-1 B C^-T = U diag(psi) U^T with psi floored at 0 and descending, A = U^T C^-1, each
 *   row's sign fixed so that its entry of largest magnitude is positive.  The model is (mu, A, psi).
 * Transform: u = A (xh - mu), then u <- u sqrt(R / sum_d u_d^2 / (psi_d + 1/n)), n the number of utterances behind the vector; the factor is
 *   1 where that sum is 0.
 * Speaker model: each enrolment row normalised, their mean, normalised again, transformed with n = the number of its rows.  Eval vectors are
 *   normalised and transformed with n = 1.
 * Score: c = n psi / (n psi + 1), v = 1 + psi / (n psi + 1), a = 1 / v,
 *   LLR(t | y, n) = -1/2 sum_d [log v_d + a_d (t_d - c_d y_d)^2] + 1/2 sum_d [log(psi_d + 1) + t_d^2 / (psi_d + 1)];  n = 0 scores exactly 0.
 *
 * ssv_plda_class_stats: X (n, R) float32; spk_off (S + 1) int64 DEVICE, speaker k owning rows [spk_off[k], spk_off[k+1]) (spk_off_host: the same
 * table as a HOST array or NULL; when given, checked here -- ascending, inside [0, n], else -1; the device clamps what it reads and takes a
 * descending pair as empty).  A workgroup per speaker: with length_norm != 0 each row's factor sqrt(R / |x|^2) in double, the mean in double
 * over the rows in ascending order.  Outputs, each optional (at least one): Xd (n, R) float32 the residual rows; means (S, R) float64; mu (R)
 * float64 (needs means); model (S, R) float32 = m_k sqrt(R) / |m_k| rounded once -- the speaker model before its transform.  A speaker without
 * rows leaves its rows of Xd and means untouched and gets a zero model row. */
int ssv_plda_class_stats(const float* X, const long* spk_off, const long* spk_off_host, float* Xd, double* means, double* mu, float* model, long n, int S,
                         int R, int length_norm, ssv_stream_t stream);
/* out_j (P) = (a + coef_j b_j)^-1, j < J, and when logdet is not NULL logdet_j = log|a + coef_j b_j|.  a (P) packed float64; b_j = b + j
 * b_stride, packed float64 (b_stride = 0: one b for all; b_stride >= P: J matrices); a == NULL: the inverse of coef_j b_j; coef (J) float64
 * DEVICE, NULL: ones (with a == NULL, J = 2 and b_stride = P two plain inverses, which serves W^-1 and B^-1 in one launch).  A workgroup
 * per matrix, the triangle in LDS (153,856 bytes at R = 192), by the extractor's Cholesky, trtri and lauum.  A pivot that is not
 * positive (a NaN among the inputs included) gives NaN in out_j and logdet_j and touches nothing else. */
int ssv_plda_mixed_inverse(const double* a, const double* b, long b_stride, const double* coef, double* out, double* logdet, int J, int R, ssv_stream_t stream);
/* The E-step, a workgroup per speaker, float64: with n = cnt[k] and Mx_{cls[k]} (Mx (J, P), the mixed inverses of B^-1 + n W^-1),
 * c = means_k - mu, t = Winv c, w_k = n Mx t, r_k = c - w_k and quad_k = n t . r_k, which is c^T (B + W/n)^-1 c by the matrix inversion
 * lemma.  cnt, cls (S) int32 DEVICE.  cnt[k] <= 0 (or cls[k] outside [0, J)): w_k = r_k = 0, quad_k = 0.  w, r (S, R), quad (S) float64. */
int ssv_plda_em_classes(const double* means, const double* mu, const int* cnt, const int* cls, const double* Mx, const double* Winv, double* w, double* r,
                        double* quad, int S, int J, int R, ssv_stream_t stream);
/* acc (R, R) float64 += V^T diag(c) V, V (S, R), c (S) float64 (NULL: ones).  Each element has one owner, which adds the rows in ascending
 * order. */
int ssv_plda_wsyrk_f64(const double* V, const double* c, double* acc, long S, int R, ssv_stream_t stream);
/* The M-step and the objective.  Per class j < J of equal counts: nspk_j speakers, nrow_j = nspk_j n_j rows (float64), Mx_j, ldMx_j =
 * log|B^-1 + n_j W^-1| (the logdet of ssv_plda_mixed_inverse).  WW = sum w w^T, RR = sum n r r^T, Sigma: (R, R) float64.  With W, B (P, packed)
 * not NULL:  B = (sum_j nspk_j Mx_j + WW) / Sn,  W = (Sigma + sum_j nrow_j Mx_j + RR) / N.  With obj (1) not NULL the objective above UNDER THE
 * PARAMETERS THE INPUTS WERE TAKEN FROM, where log|B + W/n| = ldW - R log n + ldB + ldMx and the quadratic forms are quad; ldW, ldB (1)
 * float64 DEVICE.  Sn: the speakers with rows, N: the rows.  W, B must not be the arrays Winv was computed into. */
int ssv_plda_em_update(const double* Mx, const double* ldMx, const double* nspk, const double* nrow, const double* WW, const double* RR, const double* Sigma,
                       const double* Winv, const double* ldW, const double* ldB, const int* cnt, const int* cls, const double* quad, double* W, double* B,
                       double* obj, int J, int S, int R, double Sn, double N, ssv_stream_t stream);
/* U (n, R) float32 = the transform of X (n, R): Xc = x f - mu, one float32 fused multiply-add per element BEFORE the product (f = sqrt(R /
 * |x|^2) rounded once, 1 with length_norm == 0; mu rounded once), then the product Xc At of ssv_ivec_product -- At (R, R) float32 = A^T, rounded
 * once from double by the caller -- then per row, a wave each, the sum over d of u_d^2 / (psi_d + 1/n) in double and the scaling, rounded
 * once.  n = nex[row] (int32 DEVICE) or, with nex == NULL, nex_all.  Xc (n, R): a workspace, distinct from X and U. */
int ssv_plda_transform(const float* X, const double* mu, const float* At, const double* psi, const int* nex, int nex_all, float* Xc, float* U, long n, int R,
                       int length_norm, ssv_stream_t stream);
/* The score's right operand, a workgroup per speaker, formed in double: H (S, 2 R) float32 = [-1/2 (a - 1/(psi + 1)), a c y] rounded once,
 * k (S) float64 = -1/2 sum a c^2 y^2 - 1/2 sum (log v - log(psi + 1)).  y (S, R) float32 the transformed speaker models, nspk (S) int32
 * DEVICE their row counts; nspk[s] <= 0: H_s and k_s are exactly zero. */
int ssv_plda_speaker_planes(const float* y, const int* nspk, const double* psi, float* H, double* k, int S, int R, ssv_stream_t stream);
/* scores (E, S) float32 = [t^2, t] H^T + k in one launch, T (E, R) float32 the transformed eval vectors: a workgroup owns a 64 x 64 tile;
 * the left operand is formed from the eval tile as it is staged (t^2 one float32 product), so no (E, 2 R) array exists; the product runs on
 * v_mfma_f32_16x16x4_f32 in fp32 chains of at most 256 elements of K = 2 R <= 384, added in double registers; k_s is added in double and the
 * result rounded once.  A row of the output does not depend on the rows that share its launch.  More than 65535 x 64 rows: -2. */
int ssv_plda_score(const float* T, const float* H, const double* k, float* scores, long E, long S, int R, ssv_stream_t stream);

/* ---- Vocoder and spectrogram front end ------------------------------------------------
 * Replaces the CPU tail of synthesis, synthesize.py:138-147 / generate_test_utterances.py:128-139
 * (`librosa.core.griffinlim(S, n_iter=64, hop_length, win_length)`, `signal.lfilter([1], [1, -PREEMPH], y)`, peak
 * normalisation) and the STFT front end of data/dataset.py:96-110, for a batch of equal-length utterances.
 * The DFTs are ssv_conv1d_fwd calls (k = 1) with windowed Fourier bases built by the host; these entries are the
 * steps between them.  Spectra are (B, 2F, T): rows [0,F) real, [F,2F) imaginary.  Frame matrices are (B, N, T):
 * row c holds sample c of every frame.  N = n_fft = 2(F-1), centred frames (librosa center=True, reflect padding),
 * so a T-frame spectrum is a waveform of hop*(T-1) samples.  inv_env: (N + hop*(T-1)) reciprocals of librosa's
 * window_sumsquare envelope (1 where the envelope vanishes). */
/* proj = mag * a / (|a| + 1e-16), a = reb - alpha*tprev (tprev NULL = 0): the Griffin-Lim phase update fused with S*angles. */
int ssv_gl_project(const float* mag, const float* reb, const float* tprev, float alpha, float* proj,
                   int B, int F, int T, ssv_stream_t stream);
/* mag = |spec| */
int ssv_complex_abs(const float* spec, float* mag, int B, int F, int T, ssv_stream_t stream);
/* istft overlap-add + envelope + centre trim, then stft reflect padding + framing, in one pass: windowed inverse frames
 * fr (B,N,T) -> analysis frames out (B,N,T) of the same waveform (out must not alias fr).  Needs hop*(T-1) > N/2. */
int ssv_ola_frames(const float* fr, const float* inv_env, float* out, int B, int N, int T, int hop, ssv_stream_t stream);
/* istft overlap-add + envelope + centre trim: fr (B,N,T) -> y (B, hop*(T-1)). */
int ssv_ola_signal(const float* fr, const float* inv_env, float* y, int B, int N, int T, int hop, ssv_stream_t stream);
/* stft framing: y (B,n) -> fr (B,N,T), T = 1 + n/hop, reflect padding by N/2 (n > N/2). */
int ssv_frame_signal(const float* y, float* fr, int B, int n, int N, int T, int hop, ssv_stream_t stream);
/* out[b] = max_i x[b][i];   y = (x / rowmax[b])^p * s   (synthesize.py:141-142,147; data/dataset.py:107-111). */
int ssv_rowmax(const float* x, float* out, int B, long n, ssv_stream_t stream);
int ssv_scale_pow(const float* x, const float* rowmax, float* y, float p, float s, int B, long n, ssv_stream_t stream);
/* y[n] = x[n] + a*y[n-1] per row, recurrence in double (scipy.signal.lfilter([1], [1, -a], x), synthesize.py:145). */
int ssv_deemphasis(const float* x, float* y, double a, int B, int n, ssv_stream_t stream);
/* y[0] = x[0], y[n] = x[n] - a*x[n-1] per row (data/dataset.py:96); y must not alias x. */
int ssv_preemphasis(const float* x, float* y, float a, int B, int n, ssv_stream_t stream);
/* LOG_FEATURE spectrograms (config.json:26-28).  y = exp(a*x + b): dB de-normalisation, 10^(dB/20) and the reconstruction
 * power of synthesize.py:133-135,142 folded into one pass.  y = clip((20 log10(max(1e-5, x)) - ref_db + max_db) / max_db,
 * 1e-8, 1): data/dataset.py:101-105. */
int ssv_exp_affine(const float* x, float* y, float a, float b, long n, ssv_stream_t stream);
int ssv_log_norm(const float* x, float* y, float ref_db, float max_db, long n, ssv_stream_t stream);

/* ---- FFT back end of the vocoder (additions; ABI version unchanged) -------------------------------------------------------------
 * The same transforms as the basis convolutions above -- librosa.stft / istft with a periodic Hann window, centred frames -- as
 * real FFTs that keep a tile of frames in LDS: fp32 throughout, no atomics, independent of ssv_set_precision.  n_fft: a power of two
 * in [64, 2048], else -2; 0 < hop <= n_fft.  Spectra as above, (B, 2F, T).  Inverse frames are FRAME-major here, (B, T, N): a private
 * workspace between ssv_istft_frames_fft and its two consumers.  tab: the ssv_fft_tables_floats(n_fft) floats that
 * ssv_fft_tables_host writes (host only, the caller uploads them): the window, then cos and sin of 2 pi k / n_fft for k < n_fft / 2,
 * computed in double and rounded once.  ssv_fft_frame_tile (host only): consecutive frames one workgroup owns, or -2.
 * Codes: NULL pointers, non-positive sizes, hop > n_fft, hop * (T - 1) <= n_fft / 2, n <= n_fft / 2: -1. */
size_t ssv_fft_tables_floats(int n_fft);
int ssv_fft_tables_host(float* out, int n_fft);
int ssv_fft_frame_tile(int n_fft);
/* y (B, n) -> spec (B, 2F, T), T = 1 + n / hop: reflect padding by n_fft / 2, window and real FFT in one launch (ssv_frame_signal and
 * the forward basis conv). */
int ssv_stft_fft(const float* y, const float* tab, float* spec, int B, int n, int n_fft, int hop, int T, ssv_stream_t stream);
/* spec (B, 2F, T) -> windowed inverse frames fr (B, T, N); the imaginary parts of the DC and Nyquist rows are ignored (numpy.fft.irfft).
 * fr must be 8-byte aligned (stored two floats at a time), else -1. */
int ssv_istft_frames_fft(const float* spec, const float* tab, float* fr, int B, int n_fft, int T, ssv_stream_t stream);
/* ssv_ola_signal for frame-major frames: fr (B, T, N) -> y (B, hop * (T - 1)), frames added in increasing index. */
int ssv_ola_signal_fm(const float* fr, const float* inv_env, float* y, int B, int N, int T, int hop, ssv_stream_t stream);
/* One Griffin-Lim round trip in one launch: what ssv_ola_frames does to fr (B, T, N), then window, real FFT and the phase step of
 * ssv_gl_project.  Writes reb (B, 2F, T), the rebuilt spectrum (the next call's tprev; must not alias it), and
 * proj = mag * a / (|a| + 1e-16), a = reb - alpha * tprev (tprev NULL = 0). */
int ssv_gl_step_fft(const float* fr, const float* inv_env, const float* tab, const float* mag, const float* tprev, float alpha,
                    float* reb, float* proj, int B, int n_fft, int T, int hop, ssv_stream_t stream);

/* ---- Speaker-verification front end: waveform -> GE2E features (additions; ABI version unchanged) ---------------------------
 * Replaces GE2E/data_preprocess.py:45-60 (`librosa.core.load(path, sr)`, `librosa.effects.trim(utter, 30)`, `librosa.core.stft`,
 * `np.abs(S)**2`, `np.dot(mel_basis, S)`, `np.log10(. + 1e-6)`, `S[:, :tisv_frame]` / `S[:, -tisv_frame:]`) for ragged batches:
 * waveforms are (B, n_max) float32 rows, each with a live length in a DEVICE int array, so nothing between the vocoder's output and
 * the embedder's input is read on the host and every shape is static.  The DFT between ssv_tisv_frames and ssv_power_mel_log is an
 * ssv_conv1d_fwd call (k = 1) with a (2F, n_fft, 1) basis whose window (win_length <= n_fft, centred, zero-padded) the host builds.
 * Codes: NULL pointers, non-positive sizes, hop > n_fft: -1; a ratio or size beyond the kernels' LDS tiles: -2. */
/* resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') as librosa.load applies it (:45), ratio up / down in lowest terms:
 * y[b][t] = sum_j bank[(t * down) % up][j] * x[b][(t * down) / up - left + j] (x = 0 outside [0, n_in[b])), fp32, j ascending;
 * bank (up, taps): the windowed-sinc table with resampy's linear interpolation and min(1, ratio) stretch folded in by the host.
 * int(n_in * ratio) samples are computed, n_out[b] = ceil(n_in * ratio) (librosa's fix_length), zeros up to m_max >= ceil(n_max * ratio).
 * up == down: a copy (bank may be NULL).  -2 when up * taps > 2^20 or a workgroup's input span exceeds 8192 samples. */
int ssv_resample_sinc(const float* x, const int* n_in, const float* bank, float* y, int* n_out, int B, int n_max, int m_max,
                      int up, int down, int taps, int left, ssv_stream_t stream);
/* librosa.effects.trim(y, top_db) of librosa 0.7.0 (:46): centred frames of frame_length every hop (reflect padding; zero padding for a
 * row no longer than frame_length / 2), mean square per frame in fp32, dB against the row's loudest frame;
 * bounds[b] = (start, end) = (first frame above -top_db) * hop, min(n_in[b], (last such frame + 1) * hop); an empty row gives (0, 0).
 * The loudest frame always passes, so a row of exact zeros keeps its whole length, as librosa's 1e-10 floor has it. */
int ssv_trim_bounds(const float* y, const int* n_in, int* bounds, int B, int n_max, float top_db, int frame_length, int hop,
                    ssv_stream_t stream);
/* The centred, reflect-padded frames of librosa.stft(seg, n_fft, hop) that :55-60 keep, seg = y[b][start:end] from bounds (B, 2):
 * fr (2B, n_fft, tisv_frame): item 2b the first tisv_frame frames, item 2b + 1 the last; valid[b] = (end - start) > min_len (:25, :48),
 * frames of an invalid row are zeros.  min_len >= max(n_fft / 2, tisv_frame * hop). */
int ssv_tisv_frames(const float* y, const int* bounds, float* fr, int* valid, int B, int n_max, int n_fft, int hop, int tisv_frame,
                    int min_len, ssv_stream_t stream);
/* out (R, T, nmels) = log10(mel (nmels, F) . |spec|^2 + eps), spec (R, 2F, T) as above (:50-52); plain fp32, f ascending; frames-major,
 * as SpeechEmbedder.forward takes them.  F <= 1024. */
int ssv_power_mel_log(const float* spec, const float* mel, float* out, int R, int F, int T, int nmels, float eps, ssv_stream_t stream);
/* generate_test_utterances.py:135-139 after the trim, on the device: out (B, clip) = y[b][start : start + len] / max(that segment) * peak,
 * len = min(end - start, clip), zeros after; n_out[b] = len.  The maximum, not the absolute maximum, as the reference has it. */
int ssv_segment_peak(const float* y, const int* bounds, float* out, int* n_out, int B, int n_max, int clip, float peak, ssv_stream_t stream);
/* The voiced-interval split of GE2E/synthetic_data_preprocess.py:36-47 (`librosa.effects.split(utter, top_db=30)`, every interval
 * longer than utter_min_len, its first and last tisv_frame frames), in three entries; same codes as above. */
/* librosa.effects.split(y, top_db) of librosa 0.7.0 (GE2E/synthetic_data_preprocess.py:36-47, the call at :35): frame energies and dB
 * exactly as ssv_trim_bounds computes them (one device function serves both); every maximal run [f0, f1) of frames above -top_db is the
 * interval (f0 * hop, min(n_in[b], f1 * hop)), ascending.  intervals (B, K, 2) int, entries from min(count[b], K) on are (0, 0);
 * count[b] is the number of runs, NOT capped at K (count[b] > K: the caller sees the overflow; nothing is written past entry K).
 * An empty row gives count 0, a row of exact zeros the one interval (0, n_in[b]).  -2 beyond 8192 frames per row, as ssv_trim_bounds. */
int ssv_split_intervals(const float* y, const int* n_in, int* intervals, int* count, int B, int n_max, int K, float top_db,
                        int frame_length, int hop, ssv_stream_t stream);
/* `for interval in intervals: if (interval[1] - interval[0]) > utter_min_len` (GE2E/synthetic_data_preprocess.py:36-47, the strict
 * compare at :37) across the rows of a batch, order kept: the spans k < min(count[b], K) of intervals (B, K, 2) are visited in (row,
 * interval) order; one passes when 0 <= start <= end <= n_max (a span that does not fit is skipped, never followed) and
 * end - start > min_len.  The passing span of global index g goes to table[g - first] = (row, start, end) for first <= g < first + R;
 * table (R, 3) int, rows past the last selected span are (-1, 0, 0); total[0] = the number of passing spans overall, whatever first
 * and R are (total[0] > first + R: run again with a larger first). */
int ssv_select_spans(const int* intervals, const int* count, int* table, int* total, int B, int K, int n_max, int min_len, int first, int R,
                     ssv_stream_t stream);
/* ssv_tisv_frames for the spans of a table (GE2E/synthetic_data_preprocess.py:36-47, the slices of :44-45): fr (2R, n_fft, tisv_frame),
 * item 2r the first tisv_frame centred frames of seg = y[row][start:end] of table row r (R, 3), item 2r + 1 the last, reflected at the
 * segment's own ends; valid[r] = 1.  A row of -1, one outside (B, n_max) or one with end - start <= min_len gets zero frames and
 * valid[r] = 0.  min_len >= max(n_fft / 2, tisv_frame * hop).  A workgroup stages one tile of at most 64 frames of one slice in LDS
 * and stores whole runs: -2 when (64 - 1) * hop + n_fft > 12288 floats. */
int ssv_tisv_frames_table(const float* y, const int* table, float* fr, int* valid, int B, int n_max, int R, int n_fft, int hop,
                          int tisv_frame, int min_len, ssv_stream_t stream);

/* ---- Whole-utterance d-vectors: every frame of every voiced span -> windows -> partition means (additions; ABI version unchanged) ----
 * Replaces GE2E/dvector_create.py:38-73 (`get_STFTs`: `librosa.core.stft` of every concatenated voiced segment, `S[:, j:j+24]` every 12
 * frames; `align_embeddings`: `np.average` over partitions of about 0.4 s) for ragged batches.  The host plans (which spans, which
 * windows, which partitions: spoofsv_amd/dvector.py) and ships int tables; a table entry that does not fit the buffers is skipped by
 * the kernel that reads it, never followed out of bounds.  Between ssv_span_frames and ssv_gather_windows run ssv_conv1d_fwd (k = 1,
 * the Fourier basis) and ssv_power_mel_log as above; between ssv_gather_windows and ssv_segment_mean the embedder.
 * Codes: NULL pointers, non-positive sizes, hop > n_fft, window * hop <= n_fft / 2: -1; a hop / n_fft beyond the LDS tile: -2. */
/* All centred frames of librosa.stft(seg, n_fft, hop) (:43) for the spans of a tile table.  tiles (n_tiles, 6) int on the device:
 * (row, span start, span end, first frame of the tile in its span, its first compact frame index g0, frame count <= 64), seg =
 * y[row][start:end], frame f = samples f * hop - n_fft / 2 + i (i < n_fft) of seg, reflected once at seg's own ends
 * (np.pad(mode="reflect") of the segment, not of the row; spans are at least window * hop > n_fft / 2 samples long).  Compact frame
 * g in [g_base, g_base + n_frames) goes to fr (R, n_fft, Tc) as column (g - g_base) % Tc of item (g - g_base) / Tc -- the layout
 * ssv_conv1d_fwd reads -- frames of a tile outside that range are left out, the columns past n_frames in the last item are zeroed:
 * (R - 1) * Tc < n_frames <= R * Tc.  A workgroup stages one tile's samples in LDS: (64 - 1) * hop + n_fft <= 12288 floats. */
int ssv_span_frames(const float* y, const int* tiles, float* fr, int B, int n_max, int n_tiles, int n_fft, int hop, int window, int Tc,
                    int R, int g_base, int n_frames, ssv_stream_t stream);
/* out (Nw, window, nmels)[w] = mel[g0[w] : g0[w] + window] of the frames-major log-mel array mel (G, nmels) (:48-52, transposed as :99
 * does), g0 (Nw) int on the device; 16-byte copies when nmels % 4 == 0.  A window that does not fit mel is written as zeros. */
int ssv_gather_windows(const float* mel, const int* g0, float* out, int G, int Nw, int window, int nmels, ssv_stream_t stream);
/* out (P, D)[p] = mean of rows offs[p] .. offs[p + 1] - 1 of e (Nw, D) (:70-72), offs (P + 1) int on the device; rows added in ascending
 * order in fp32 whatever the launch looks like; normalize != 0: the mean is divided by its L2 norm afterwards (the reference does not;
 * the utterance-level d-vector of the GE2E paper does).  An empty partition gives zeros. */
int ssv_segment_mean(const float* e, const int* offs, float* out, int Nw, int P, int D, int normalize, ssv_stream_t stream);

/* ---- Corpus spectrograms for ragged batches: trimmed waveforms -> the collated (mel, linear) training batch (additions; ABI version
 * unchanged) -------------------------------------------------------------------------------------------------------------------------
 * Replaces data/dataset.py:94-118 (`librosa.effects.trim(speech, 22)`, the pre-emphasis `np.append`, `librosa.stft`, `np.dot(mel_filterbank,
 * lin_spec)`, both normalisations, the time reduction) and the zero padding of collate_pad_2 / collate_pad_3 (:215-258) for B utterances
 * at once: waveforms (B, n_max) with (start, end) bounds (B, 2) int ON THE DEVICE, as ssv_trim_bounds (top_db = 22) writes them; resampling
 * in front (metagen.py:29-62) is ssv_resample_sinc.  Between the two entries run ssv_conv1d_fwd (k = 1, the Fourier basis), ssv_complex_abs,
 * ssv_conv1d_fwd (the mel basis) and, for the default normalisation, ssv_rowmax.
 * Codes: NULL pointers, non-positive sizes, an odd n_fft, hop > n_fft, a T_max below 1 + n_max / hop, r * RT_max > T_max, an output that is
 * its own input: -1; a hop / n_fft whose 16-frame tile does not fit the LDS image (12,800 floats): -2.  All checked before any launch. */
/* data/dataset.py:95-97 up to the DFT's input.  seg = y[b][start:end], len = end - start; p[0] = seg[0], p[i] = seg[i] - preemph * seg[i-1]
 * (:96, one fused multiply-add; the sample before `start` is not read); fr (B, n_fft, T_max)[b][i][t] = np.pad(p, n_fft / 2, "reflect")
 * [t * hop + i] for t < n_frames[b] = 1 + len / hop (librosa.stft, center=True), zeros for t >= n_frames[b].  A segment of
 * len <= n_fft / 2 (an empty one included) has nothing to reflect from: n_frames[b] = 0 and all-zero frames. */
int ssv_preemph_frames_ragged(const float* y, const int* bounds, float* fr, int* n_frames, int B, int n_max, int n_fft, int hop, int T_max,
                              float preemph, ssv_stream_t stream);
/* data/dataset.py:101-118 for magnitudes lin (B, F, T_max) and mel (B, M, T_max) whose columns >= n_frames[b] are zero, into the collated
 * layout: rt[b] = n_frames[b] / r (:115); mel_out (B, M, RT_max)[b][m][k] = norm(mel[b][m][k * r]) for k < rt[b] (:116-117); lin_out
 * (B, F, r * RT_max)[b][f][c] = norm(lin[b][f][c]) for c < r * rt[b] (:118); exact zeros after, as collate_pad_* pads.
 * log_feature == 0: norm(x) = (x / max)^power with max_lin[b] / max_mel[b] (B) the item's maxima (:108-112; ssv_rowmax over the padded
 * item); a maximum of 0 gives zeros where the reference gives NaN.  log_feature != 0: norm(x) = clip((20 log10(max(1e-5, x)) - ref_db +
 * max_db) / max_db, 1e-8, 1) (:102-105); the maxima are not read and may be NULL. */
int ssv_corpus_normalize_pack(const float* lin, const float* mel, const float* max_lin, const float* max_mel, const int* n_frames,
                              float* mel_out, float* lin_out, int* rt, int B, int F, int M, int T_max, int RT_max, int r, int log_feature,
                              float power, float ref_db, float max_db, ssv_stream_t stream);

/* ---- Text2Mel / SSRN batches from a spectrogram corpus held on the device (additions; ABI version unchanged) ----------------------
 * Replaces VCTKDataset.__getitem__, data/dataset.py:83-173 (`np.load` of the cached `_mel.npy` / `_lin.npy`, the text ids, the speaker
 * code, per item of every batch) and collate_pad_2 / collate_pad_3, data/dataset.py:187-258 (zero padding to the batch's longest item,
 * the stack, then the upload), for a whole batch in one launch per tensor.  The corpus lives in ragged arenas: item i is a
 * contiguous block at arena + off[i] (off: n_items int64, in ELEMENTS; len: n_items int32; both on the DEVICE).  rows (n_rows int32,
 * DEVICE) is the whole epoch's item order, uploaded once; a batch is its entries [row0, row0 + B), row0 a host integer.  Nothing is
 * read on the host.  An entry outside [0, n_items), a negative len, or a block that does not lie inside the arena_n elements of the
 * arena is never dereferenced: that item of the batch is written as NaN (ids: -1) and nothing else changes.
 * Codes: NULL pointers, non-positive sizes, [row0, row0 + B) outside the table, out_bs < F * width: -1; a grid that does not fit: -2. */
/* Item i is a row-major (F, len[i]) float block.  out[b * out_bs + f * width + t] = t < len[r] ? arena[off[r] + f * len[r] + t] : 0 for
 * b < B, f < F, t < width, r = rows[row0 + b]: width may exceed the batch's longest item (zeros after it) or fall below it (the item is
 * clipped); out_bs is the batch stride in elements.  Any len >= 0 and any off: 16-byte accesses where a row starts on a 16-byte
 * boundary on both sides, 4-byte ones elsewhere.  The speaker codes (B, D, 1) are this entry with F = 1, len = width = D over the
 * (n_speakers, D) table, off[i] = D * speaker(i). */
int ssv_corpus_gather(const float* arena, long arena_n, const long* off, const int* len, int n_items, const int* rows, long n_rows,
                      long row0, float* out, int B, int F, int width, long out_bs, ssv_stream_t stream);
/* Text ids (data/dataset.py:83-173, `text2id` at :175-185; collate at :187-258): item i is len[i] int32 ids at arena + off[i];
 * out (B, 1, width) int64, out[b][0][t] = t < len[r] ? arena[off[r] + t] : 0 ('P' = id 0 is the collate's padding). */
int ssv_corpus_gather_ids(const int* arena, long arena_n, const long* off, const int* len, int n_items, const int* rows, long n_rows,
                          long row0, long* out, int B, int width, ssv_stream_t stream);

/* The inverse of ssv_corpus_gather, for filling an arena on the device: replaces the per-item `lin_spec`, `mel_spec = self.get_spec(...)`
 * of ASVspoofDataset.__getitem__, anti_spoofing/spoof_conv1d.py:43-91, run again for every item of every epoch, by ONE extraction whose
 * collated batches (collate_pad_3, main_spoof_conv1d.py:64) are filed item by item.  src (B, F, width), batch stride src_bs elements, is
 * a collated batch; item i = item0 + b of the arena (off, len: n_items entries on the DEVICE, as above) receives
 * arena[off[i] + f * len[i] + t] = src[b * src_bs + f * width + t] for f < F, t < len[i].  Nothing is read on the host.  An item with
 * len[i] < 0 or len[i] > width, or whose block does not lie inside the arena_n elements of the arena, is left untouched and nothing else
 * changes.  16-byte accesses where a row starts on a 16-byte boundary on both sides, 4-byte ones elsewhere.
 * Codes: NULL pointers, non-positive sizes, [item0, item0 + B) outside the table, src_bs < F * width: -1; a grid that does not fit: -2. */
int ssv_corpus_scatter(const float* src, long src_bs, int B, int F, int width, float* arena, long arena_n, const long* off, const int* len,
                       int n_items, int item0, ssv_stream_t stream);

/* ---- Second order, for the critics' gradient penalty ------------------------------------------
 * train/adversarial_wasserstein_gp.py:300-308 differentiates the critic's input gradient
 * (`autograd.grad(..., create_graph=True)` then `loss.backward()`), so the LayerNorm / highway-gate BACKWARD kernels need
 * gradients of their own.  Critics only: at most 256 channels, no activation inside the LayerNorm.
 * ssv_channel_ln_bwd2: for dx = ssv_channel_ln_act_bwd(act = 0)(gn; x) and an upstream v (same shape as dx), the
 * gradients of <v, dx> w.r.t. gn (d_gn), x (d_x) and gamma (dgamma (C)); beta does not enter. */
size_t ssv_channel_ln_bwd2_workspace(int B, int C, int L);
int ssv_channel_ln_bwd2(const float* v, long v_bs, const float* gn, long gn_bs, const float* x, long x_bs, const float* stats,
                        const float* gamma, float* d_gn, long dgn_bs, float* d_x, long dx_bs, float* dgamma,
                        int B, int C, int L, void* ws, size_t ws_bytes, ssv_stream_t stream);
/* The highway gate alone (models/TTSModel_dropout.py:63-84 without the conv and the dropout, which the critics keep as
 * separate differentiable ops): h (B,2C,L) dense, y = sigmoid(LN1(h[:C])) * LN2(h[C:]) + (1 - sigmoid(..)) * x;
 * stats (B,4,L) saved for ssv_highway_gate_bwd. */
int ssv_highway_gate_fwd(const float* h, const float* x, long x_bs, const float* g1, const float* b1, const float* g2, const float* b2,
                         float* stats, float* y, long y_bs, float* y_amax, int B, int C, int L, ssv_stream_t stream);
/* For (dh, dxres) = ssv_highway_gate_bwd(gy; h, x) and upstreams vh (B,2C,L dense), vx: gradients of <vh, dh> + <vx, dxres>
 * w.r.t. gy (d_gy), h (d_h, dense), x (d_x) and pgrads (4,C) = dgamma1, dbeta1, dgamma2, dbeta2. */
size_t ssv_highway_gate_bwd2_workspace(int B, int C, int L);
int ssv_highway_gate_bwd2(const float* vh, const float* vx, long vx_bs, const float* gy, long gy_bs, const float* h, const float* x, long x_bs,
                          const float* stats, const float* g1, const float* b1, const float* g2, const float* b2,
                          float* d_gy, long dgy_bs, float* d_h, float* d_x, long dx_bs, float* pgrads,
                          int B, int C, int L, void* ws, size_t ws_bytes, ssv_stream_t stream);

/* ---- Column-incremental synthesis ------------------------------------------------------
 * The reference's free-running loop (synthesize.py:103-109, models/TTSModel.py:275-300) re-encodes the whole prefix at
 * every step.  The audio encoder and decoder are causal, so only column t of every layer is new at step t; these entries
 * compute that column.  Step activations are (B, C) matrices, channels contiguous; the input history of a causal k = 3
 * convolution is (B, Tmax, C); the frame counter is a DEVICE int so a captured step can be replayed for every frame.
 * ssv_column_matvec: out[b][m] = bias[m] + bias_b[b][m] + sum_{j,c} w[m][j][c] x_j[b][c] with w TAP-MAJOR, (M, k, C) =
 * nn.Conv1d's (M, C, k) weight with its last two axes swapped (the weights are frozen during synthesis: permute once; for
 * k = 1 the layouts coincide).  C a multiple of 4, buffers 16-byte aligned.  k = 1: x_0 = cur.  k = 3 (causal, `dilation`): x_2 = cur (frame t = *t_dev), x_1 = hist[t-d], x_0 = hist[t-2d]
 * (a tap outside [0, Tmax) is zero); cur is also stored as column t of hist when 0 <= t < Tmax.  A frame counter outside the history
 * (a replay past the last frame, as ssv_attention_column and ssv_synth_column_advance tolerate) reads and writes nothing outside hist;
 * out is still written.  bias, bias_b, and (k = 1) hist / t_dev may be NULL.  cur_bs and hist_bs are multiples of 4 floats. */
int ssv_column_matvec(const float* w, const float* bias, const float* bias_b, long bb_bs, const float* cur, long cur_bs,
                      float* hist, long hist_bs, int Tmax, const int* t_dev, int dilation, float* out, long out_bs,
                      int B, int C, int M, int k, ssv_stream_t stream);
/* LayerNorm over channels (+ activation, as ssv_channel_ln_act_fwd) and the highway gate (as ssv_highway_gate_fwd, h (B,2C)
 * dense) on one column per batch item, C <= 1024.  The mean is the correctly rounded sum / C: a column of one constant whose
 * sum is exact in float32 gives act(beta) to the bit. */
int ssv_column_ln_act(const float* x, long x_bs, const float* gamma, const float* beta, float* y, long y_bs, int B, int C, int act,
                      ssv_stream_t stream);
int ssv_column_gate(const float* h, const float* x, long x_bs, const float* g1, const float* b1, const float* g2, const float* b2,
                    float* y, long y_bs, int B, int C, ssv_stream_t stream);
/* One new attention frame, models/TTSModel.py:281-295: kv (B,2d,N) = K | V; q (B,d); pma (B) int64 is read and replaced by
 * the arg-max of the new column; column *t_dev of a (B,N,a_T) is written; rq (B,2d) = [V a ; q]. */
int ssv_attention_column(const float* kv, long kv_bs, const float* q, int64_t* pma, float* a, int a_T, const int* t_dev,
                         float* rq, int B, int d, int N, ssv_stream_t stream);
/* End of a step: Y[:, :, t] = y_cur (B,F), mel_cur = y_cur (the next step's input frame, synthesize.py:108-109), t += 1. */
int ssv_synth_column_advance(const float* y_cur, float* Y, float* mel_cur, int* t_dev, int B, int F, int T, ssv_stream_t stream);

/* ---- Wide column-incremental synthesis: many items per step (generate_test_utterances.py:98-139 walks the speakers one by one;
 * here S speakers x U sentences are the items of ONE free run) ---------------------------------------------------------------
 * Step activations are CHANNEL-MAJOR, (C, Bw): the B items contiguous, Bw = B rounded up to ssv_column_wide_tile() columns, the pad
 * columns B .. Bw-1 zero (every entry below writes them as zeros).  A layer is one launch: a matrix product over the batch on the
 * MFMA units in the mode of ssv_set_precision -- exact fp32 reads `w`, the split modes read the weight's resident planes `w_packed`
 * (ssv_conv_pack_multi) and fail with -1 when they are NULL -- whose workgroups own all output rows of their columns and finish bias,
 * LayerNorm and activation / gate in the epilogue.  split-fp16: the operand scale is that of the workgroup's own column tile.
 * Codes: NULL pointers, non-positive sizes, B > Bw, U = 0 or B % U != 0, an output that is its own input: -1; a shape the tile cannot take
 * (k != 3, C % 8 != 0 or C > 256 for the highway layer, Cout > 512, Bw not a multiple of the tile): -2.  All checked before any launch.
 * ssv_column_highway_wide: models/TTSModel.py:28-47 (highwayConv.forward, causal, kernel size 3) for frame t = *t_dev of every item:
 *   h = W0 x[t-2d] + W1 x[t-d] + W2 x[t] + bias (2C rows; a tap before frame 0 is zero), H1 | H2 = its halves,
 *   out = sigmoid(LN1(H1)) * LN2(H2) + (1 - sigmoid(LN1(H1))) * x[t];  x[t] = cur (C, Bw) is filed as frame t of hist (Tmax, C, Bw),
 *   the two earlier taps are read from there.  w (2C, C, 3) as nn.Conv1d keeps it. */
int ssv_column_wide_tile(void);
int ssv_column_highway_wide(const float* w, const void* w_packed, const float* bias, const float* g1, const float* b1, const float* g2,
                            const float* b2, const float* cur, float* hist, int Tmax, const int* t_dev, int dilation, float* out,
                            int B, int Bw, int C, int k, ssv_stream_t stream);
/* y (Cout, Bw) = act(LN(W x + bias [+ s])) for x (Cin, Bw): the 1x1 links, models/TTSModel.py:128-131, :173-180, :218-231.  s (Cout, Bw) or
 * NULL is the per-ITEM speaker term of the conditioned encoder (models/TTSModel.py:174,179).  act as ssv_channel_ln_act_fwd. */
int ssv_column_pwln_wide(const float* x, const float* w, const void* w_packed, const float* bias, const float* s, const float* gamma,
                         const float* beta, float* y, int B, int Bw, int Cin, int Cout, int act, ssv_stream_t stream);
/* ssv_attention_column (models/TTSModel.py:281-295) with q (d, Bw) and rq (2d, Bw) = [V a ; q] in the wide layout; item b reads text
 * b % U of kv (U, 2d, N) (U = B: a text per item).  pma (B) and a (B, N, a_T) as there. */
int ssv_attention_column_wide(const float* kv, long kv_bs, int U, const float* q, int64_t* pma, float* a, int a_T, const int* t_dev,
                              float* rq, int B, int Bw, int d, int N, ssv_stream_t stream);
/* End of a step (synthesize.py:108-109): frame t of Y (T, F, Bw) = y_cur (F, Bw), mel_cur = y_cur, t += 1. */
int ssv_synth_column_advance_wide(const float* y_cur, float* Y, float* mel_cur, int* t_dev, int Bw, int F, int T, ssv_stream_t stream);

/* ---- Critic glue: what models/discriminator.py:24-41 does between its convolutions and LayerNorms ----------
 * Dropout(p = 0.05) (always active: the reference never calls disc.eval()), leaky-ReLU(0.05), AvgPool1d, and the reduction of
 * the gradient penalty (train/adversarial_wasserstein_gp.py:305-308).  Each is (piecewise) linear, hence differentiable to any
 * order with ssv_mul / the pool adjoint.
 * ssv_act_dropout_fwd: y = leaky_relu(x, slope) * keep / (1 - p); d = y / x's factor, saved for ssv_mul.  slope = 1: plain
 * dropout, p = 0: plain leaky-ReLU.  The mask is Philox4x32-10 keyed by (seed, *ctr_dev); the call increments *ctr_dev on the
 * stream, so a replayed hipGraph draws a fresh mask every iteration. */
int ssv_act_dropout_fwd(const float* x, float* y, float* d, long n, float slope, float p, unsigned long long* ctr_dev, unsigned seed,
                        ssv_stream_t stream);
int ssv_mul(const float* x, const float* d, float* y, long n, ssv_stream_t stream);
/* nn.AvgPool1d(kernel_size = k) on rows of length L (rows = B * C): Lo = L / k outputs per row; the adjoint spreads dy / k. */
int ssv_avgpool1d_fwd(const float* x, float* y, long rows, int L, int k, ssv_stream_t stream);
int ssv_avgpool1d_bwd(const float* dy, float* dx, long rows, int L, int k, ssv_stream_t stream);
/* loss[0] = mean_b lam * (||g_b||_2 - 1)^2 for g (B, n); coef (B) = 2 lam (||g_b|| - 1) / (B ||g_b||) is saved for the backward
 * dg = gout[0] * coef[b] * g.  Fixed summation order. */
size_t ssv_grad_penalty_workspace(int B, long n);
int ssv_grad_penalty_fwd(const float* g, float* loss, float* coef, int B, long n, float lam, void* ws, size_t ws_bytes, ssv_stream_t stream);
int ssv_grad_penalty_bwd(const float* g, const float* coef, const float* gout, float* dg, int B, long n, ssv_stream_t stream);

/* ---- Spoof countermeasure: classifier head and its optimizer (additions; ABI version unchanged) -------------------------------
 * ssv_cm_head_fwd replaces `x = self.conv5(F.leaky_relu(x, 0.05)); x = self.pl3(x); x = F.sigmoid(x)`,
 * anti_spoofing/discriminator.py:129-131 (:91-93 for melDisc), and the loss of anti_spoofing/main_spoof_conv1d.py:87,
 * the mean over the batch of `-label*log(pred+1e-6)-(1-label)*log(1-pred+1e-6)`, for x (B, C, T) dense, the output of ln4, C <= 16:
 *   z_b = bias[0] + sum_c w[c] * mean_t leaky_relu(x[b,c,t], slope)   (the mean and the one-channel 1x1 convolution commute);
 *   pred[b] = p_b = sigmoid(z_b);  per[b] = -y_b log(p_b + 1e-6) - (1 - y_b) log(q_b + 1e-6);  loss[0] = mean_b per[b].
 * q_b = 1 - p_b is evaluated as sigmoid(-z_b): the subtraction the reference writes loses every digit of q in float32 once z
 * exceeds about 17 and puts a wrong-label item's term off by up to 0.06 just below that; here both tails keep their relative accuracy.  The
 * row sums are fp32 (a wave per (b, c) row); z, the sigmoids and the logarithms of an item are evaluated in double and rounded once.
 * labels (B floats) NULL = scoring: only pred is written (amean may be given, per and loss are not touched).  With labels, amean
 * (B, C), the activated means, is saved for the backward.  Two launches (one workgroup per item; one wave that adds the B terms
 * in a fixed order), no atomics: bitwise reproducible.
 * ssv_cm_head_bwd is autograd's backward of the above (`loss.backward()`, main_spoof_conv1d.py:89) down to ln4's output, gscale
 * (DEVICE float) the gradient arriving at the loss:
 *   dz[b] = gscale / B * p_b q_b (-y_b / (p_b + 1e-6) + (1 - y_b) / (q_b + 1e-6))   (B floats, scratch the caller provides);
 *   dx[b,c,t] = dz[b] / T * w[c] * (x[b,c,t] > 0 ? 1 : slope);  dw[c] = sum_b dz[b] amean[b,c];  dbias[0] = sum_b dz[b].
 * Codes: B, C, T <= 0, C > 16 or a NULL pointer: -1, before any launch. */
int ssv_cm_head_fwd(const float* x, const float* w, const float* bias, const float* labels, float slope, float* pred, float* amean,
                    float* per, float* loss, int B, int C, int T, ssv_stream_t stream);
int ssv_cm_head_bwd(const float* x, const float* w, const float* bias, const float* labels, const float* amean, const float* gscale,
                    float slope, float* dx, float* dw, float* dbias, float* dz, int B, int C, int T, ssv_stream_t stream);
/* ssv_cm_head_fwd / ssv_cm_head_bwd (anti_spoofing/discriminator.py:129-131, main_spoof_conv1d.py:87,89) on an x (B, C, T) of which only
 * the first Tl = clamp(live[0], 1, T) columns are live: a batch gathered into a wider static buffer, so that the iteration of
 * main_spoof_conv1d.py:84-90 can be replayed from one captured hipGraph per width.  live is a DEVICE int read when the kernels run.  The
 * means and the dz / T of the backward use Tl; columns t >= Tl of x are never used (they may hold anything, NaN included) and dx is
 * written as exact zeros there.  Same kernels as the dense entries (the same two launches each way, no atomics, the same summation
 * order, the double-precision scalar tail, q = sigmoid(-z)): with live[0] == T every output has the bits of ssv_cm_head_fwd / _bwd.
 * Codes: those of the dense entries; a NULL live: -1. */
int ssv_cm_head_fwd_len(const float* x, const float* w, const float* bias, const float* labels, float slope, float* pred, float* amean,
                        float* per, float* loss, int B, int C, int T, const int* live, ssv_stream_t stream);
int ssv_cm_head_bwd_len(const float* x, const float* w, const float* bias, const float* labels, const float* amean, const float* gscale,
                        float slope, float* dx, float* dw, float* dbias, float* dz, int B, int C, int T, const int* live, ssv_stream_t stream);
/* Replaces `optim.Adam(..., betas=(0.9, 0.98), eps=1e-09, weight_decay=1e-4, amsgrad=True)` and its .step(),
 * anti_spoofing/main_spoof_conv1d.py:52,90, for many tensors in one launch: ssv_adam_multi with L2 weight decay and AMSGrad, in the
 * arithmetic of torch's single-tensor path:  g' = g + wd p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  vmax = max(vmax, v);
 * p -= lr / (1 - b1^t) * m / (sqrt(vmax) / sqrt(1 - b2^t) + eps).  amsgrad == 0: v in place of vmax, and the vmax of a chunk is
 * neither read nor written (NULL allowed).  g is only read.  chunks / step / step_dev: as ssv_adam_multi.
 * Codes: nchunks <= 0, no step, weight_decay < 0, amsgrad not 0 / 1: -1.  The table lives on the device, so a NULL vmax under
 * amsgrad = 1 is the caller's to refuse (FusedAdamEx checks its rows on the host). */
typedef struct { float* p; const float* g; float* m; float* v; float* vmax; long n; } ssv_adam_ex_chunk;
int ssv_adam_ex_multi(const ssv_adam_ex_chunk* chunks, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                      int amsgrad, int step, int* step_dev, ssv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SSV_HIP_H */
