// Host layer (see api.hip), convolution module: Conv1d forward / data gradient / weight gradient, the resident pre-split weight
// planes, several weight gradients in one launch, and ConvTranspose1d(k=2, s=2).  No kernel here.
#include "ssv_host.h"

int conv_shifts(int k, int dilation, int causal, int* shift) {
  SSV_CHECK(k == 1 || k == 3, SSV_UNSUPPORTED, "conv1d: kernel_size %d not supported (1 or 3)", k);
  SSV_CHECK(dilation >= 1 && dilation * (k - 1) <= 54, SSV_UNSUPPORTED, "conv1d: dilation %d not supported (k=%d)", dilation, k);
  const int j0 = causal ? k - 1 : (k - 1) / 2;
  for (int j = 0; j < 3; ++j) shift[j] = j < k ? (j - j0) * dilation : 0;
  return 0;
}
extern "C" int ssv_conv_shifts(int k, int dilation, int causal, int* shift3) { return conv_shifts(k, dilation, causal, shift3); }

// ---- split-fp16 operand scales (ssv_host.h) -----------------------------------------------------------------------------
int amax_of(const float* x, long x_bs, int B, long n_item, const float* given, int ngiven, float* fb, AmaxList* out, hipStream_t st) {
  if (given) {
    SSV_CHECK(ngiven > 0, SSV_BAD_SHAPE, "operand scale list given with %d entries per item", ngiven);
    out->p = given; out->n = ngiven;
    return 0;
  }
  SSV_CHECK(fb, SSV_BAD_SHAPE, "split-fp16: no operand scales given and no workspace to compute them in");
  SSV_CHECK(B <= SSV_AMAX_FB_FLOATS, SSV_UNSUPPORTED, "split-fp16: batch %d needs caller-provided operand scales (ssv_absmax)", B);
  int npb = SSV_AMAX_FB_FLOATS / B;
  if (npb > 64) npb = 64;
  const long pieces = (n_item + 4095) / 4096;
  if (npb > pieces) npb = (int)(pieces > 0 ? pieces : 1);
  SSV_TRY(ssv_launch_absmax(x, x_bs, B, n_item, fb, npb, st));
  out->p = fb; out->n = npb;
  return 0;
}
extern "C" int ssv_amax_rows(int L) { return ssv_amax_rows_(L); }
extern "C" int ssv_absmax(const float* x, long x_bs, int B, long n, float* amax, int namax, ssv_stream_t stream) {
  SSV_CHECK(x && amax && B > 0 && B <= 65535 && n > 0 && namax > 0 && namax <= 65535, SSV_BAD_SHAPE, "absmax: bad argument");
  return ssv_launch_absmax(x, x_bs, B, n, amax, namax, (hipStream_t)stream);
}

// ---- Conv1d ----------------------------------------------------------------------------------------
ConvWs conv_ws(size_t main_bytes) {
  WsTake t;
  ConvWs l;
  l.main = t.take(main_bytes);
  l.aux = t.take(SSV_F16_AUX_BYTES);
  l.fb = t.take(AMAX_FB_BYTES);
  l.total = t.off;
  return l;
}
ConvWs conv_fwd_ws(int Cin, int Cout, int k) { return conv_ws(2 * split_bytes(Cout, Cin, k)); }
// (the exact-fp32 kernel reads the fp32 transpose of the weight from the same region)
ConvWs conv_bwd_data_ws(int Cin, int Cout, int k) { return conv_ws(zmax((size_t)Cin * Cout * k * sizeof(float), 2 * split_bytes(Cin, Cout, k))); }

int conv_nn(const float* x, long x_bs, const float* w, SplitPlanes packed, long w_sm, long w_sk, const float* bias, const float* bias_b,
            const float* r, long r_bs, float* y, long y_bs, int B, int K, int M, int L, int k, const int* shift,
            bool bf3, void* ws, const ConvWs& l, hipStream_t st, const float* xa_given, int xa_n, float* colstats, const PwLnArgs* pw) {
  if (bf3) {
    const int Kpad = pad32(K);
    const bool f16 = use_f16();
    float* aux = ws ? ws_f32(ws, l.aux) : nullptr;
    if (!packed.hi) {
      packed.hi = ws_u16(ws, l.main); packed.lo = ws_u16(ws, l.main + split_bytes(M, K, k));
      if (f16) { SSV_TRY(ssv_launch_pack_split_f16(w, (long)M * K * k, packed.hi, packed.lo, M, K, Kpad, k, w_sm, w_sk, 1, aux, st)); packed.inv = aux + 64; }
      else SSV_TRY(ssv_launch_pack_split(w, packed.hi, packed.lo, M, K, Kpad, k, w_sm, w_sk, 1, 0, st));
    }
    GemmNNB g;
    if (f16) {
      AmaxList xa;
      SSV_TRY(amax_of(x, x_bs, B, (long)K * L, xa_given, xa_n, ws ? ws_f32(ws, l.fb) : nullptr, &xa, st));
      g.f16 = 1; g.a_inv = packed.inv; g.x_amax = xa.p; g.x_namax = xa.n; g.x_amax_bs = xa.n;
    }
    g.colstats = colstats;
    g.Ahi = packed.hi; g.Alo = packed.lo; g.Kpad = Kpad;
    g.X = x; g.sxb = x_bs; g.sxc = L; g.Lx = L;
    g.C = y; g.scb = y_bs; g.scm = L;
    g.bias = bias; g.bias_b = bias_b; g.sbb = M;
    g.R = r; g.srb = r_bs; g.srm = L;
    g.M = M; g.N = L; g.Kc = K; g.KT = k; g.B = B;
    for (int j = 0; j < 3; ++j) g.shift[j] = shift[j];
    if (k == 1 && M > 128 && M % 128 == 1) { g.xrow_w = w + (long)(M - 1) * w_sm; g.xrow_sk = w_sk; }     // (GemmNNB::xrow_w; the launchers decide)
    if (pw) return ssv_launch_gemm_pwln(g, pw->gamma, pw->beta, pw->y, pw->ybs, pw->stats, pw->y_amax, pw->namax, pw->act, st);
    return ssv_launch_gemm_nn_bf3(g, st);
  }
  if (L == 1 && k == 1 && w_sk == 1 && w_sm == K && !r)          // nn.Linear on a (B, K) matrix (the speaker-code layers): see linear_len1_fwd_kernel
    return ssv_launch_linear_len1_fwd(x, x_bs, w, bias, bias_b, M, y, y_bs, B, K, M, st);
  GemmNN g;
  for (int j = 0; j < 3; ++j) g.shift[j] = shift[j];
  const float* a = w;
  if (w_sk != k) {                                   // transposed operand for the data gradient: wt[c][o][j] = w[o][c][j]
    SSV_TRY(ssv_launch_pack_wt(w, ws_f32(ws, l.main), K, M, k, st));
    a = ws_f32(ws, l.main);
  }
  g.A = a; g.sam = (long)K * k; g.sac = k; g.saj = 1;
  g.X = x; g.sxb = x_bs; g.sxc = L; g.Lx = L;
  g.C = y; g.scb = y_bs; g.scm = L;
  g.bias = bias; g.bias_b = bias_b; g.sbb = M;
  if (r) { g.R = r; g.srb = r_bs; g.srm = L; }
  g.M = M; g.N = L; g.Kc = K; g.KT = k; g.B = B;
  return ssv_launch_gemm_nn(g, st);
}

extern "C" size_t ssv_conv1d_fwd_workspace(int Cin, int Cout, int k) { return conv_fwd_ws(Cin, Cout, k).total; }
extern "C" int ssv_conv1d_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                              const float* bias_b, float* y, long y_bs, float* y_colstats,
                              int B, int Cin, int Cout, int L, int k, int dilation, int causal, void* ws, size_t ws_bytes,
                              ssv_stream_t stream) {
  SSV_CHECK(x && w && y && B > 0 && Cin > 0 && Cout > 0 && L > 0, SSV_BAD_SHAPE, "conv1d_fwd: bad argument B=%d Cin=%d Cout=%d L=%d", B, Cin, Cout, L);
  SSV_CHECK(x_bs >= (long)Cin * L && y_bs >= (long)Cout * L, SSV_BAD_SHAPE, "conv1d_fwd: batch stride smaller than C*L");
  int shift[3];
  SSV_TRY(conv_shifts(k, dilation, causal, shift));
  const bool bf3 = use_bf3(B, L, Cin, Cout);
  const ConvWs l = conv_fwd_ws(Cin, Cout, k);
  if (bf3 && (!w_packed || (use_f16() && !x_amax)))
    SSV_CHECK(ws && ws_bytes >= l.total, SSV_BAD_SHAPE, "conv1d_fwd: workspace too small");
  SSV_CHECK(!y_colstats || (bf3 && Cout % 64 == 0 && y_bs == (long)Cout * L), SSV_UNSUPPORTED,
            "conv1d_fwd: column statistics need a split-MFMA mode, Cout %% 64 == 0 and a dense output (Cout=%d)", Cout);
  return conv_nn(x, x_bs, w, packed_planes(w_packed, Cout, Cin, k).fwd, (long)Cin * k, k, bias, bias_b, nullptr, 0, y, y_bs, B, Cin, Cout, L, k, shift, bf3,
                 ws, l, (hipStream_t)stream, x_amax, x_namax, y_colstats);
}

extern "C" size_t ssv_conv1d_bwd_data_workspace(int Cin, int Cout, int k) { return conv_bwd_data_ws(Cin, Cout, k).total; }
extern "C" int ssv_conv1d_bwd_data(const float* dy, long dy_bs, const float* dy_amax, int dy_namax, const float* w, const void* w_packed,
                                   const float* dx_add, float* dx, long dx_bs,
                                   int B, int Cin, int Cout, int L, int k, int dilation, int causal,
                                   void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dy && w && dx && B > 0 && Cin > 0 && Cout > 0 && L > 0, SSV_BAD_SHAPE, "conv1d_bwd_data: bad argument");
  const ConvWs l = conv_bwd_data_ws(Cin, Cout, k);
  SSV_CHECK((w_packed && !(use_f16() && !dy_amax)) || (ws && ws_bytes >= l.total), SSV_BAD_SHAPE, "conv1d_bwd_data: workspace too small");
  int shift[3];
  SSV_TRY(conv_shifts(k, dilation, causal, shift));
  for (int j = 0; j < 3; ++j) shift[j] = -shift[j];
  // rows = input channels c, reduction over output channels o: element (c, o, j) = w[o][c][j] -- the transposed planes of a resident weight
  return conv_nn(dy, dy_bs, w, packed_planes(w_packed, Cout, Cin, k).tr, k, (long)Cin * k, nullptr, nullptr, dx_add, dx_bs, dx, dx_bs, B, Cout, Cin, L, k, shift,
                 use_bf3(B, L, Cout, Cin), ws, l, (hipStream_t)stream, dy_amax, dy_namax);
}

// ---- resident pre-split weights (layout: packed_planes, ssv_host.h) ---------------------------------------------------
extern "C" size_t ssv_conv_pack_bytes(int Cout, int Cin, int k) { return packed_planes(nullptr, Cout, Cin, k).bytes; }
extern "C" int ssv_conv_pack_plan(int n, const float* const* w, void* const* planes, const int* Cout, const int* Cin, const int* k,
                                  ssv_pack_job* jobs) {
  SSV_CHECK(n > 0 && w && planes && Cout && Cin && k && jobs, SSV_BAD_SHAPE, "conv_pack_plan: bad argument");
  long blocks = 0;
  for (int i = 0; i < n; ++i) {
    SSV_CHECK(w[i] && planes[i] && Cout[i] > 0 && Cin[i] > 0 && (k[i] == 1 || k[i] == 3), SSV_BAD_SHAPE, "conv_pack_plan: weight %d: bad shape", i);
    const PackedPlanes pp = packed_planes(planes[i], Cout[i], Cin[i], k[i]);
    for (int tr = 0; tr < 2; ++tr) {
      ssv_pack_job& j = jobs[2 * i + tr];
      const SplitPlanes& pl = tr ? pp.tr : pp.fwd;
      const int M = tr ? Cin[i] : Cout[i], K = tr ? Cout[i] : Cin[i];
      j.w = w[i];
      j.planes = pl.hi;
      j.M = M; j.K = K; j.Kpad = pad32(K); j.KT = k[i];
      j.sm = tr ? k[i] : (long)Cin[i] * k[i];            // element (m, kk, tap) = w[m*sm + kk*sk + tap]
      j.sk = tr ? (long)Cin[i] * k[i] : k[i];
      j.first_block = (int)blocks; j.pad_ = 0;
      j.inv_out = pl.inv;
      blocks += ssv_pack_job_blocks(j);
      SSV_CHECK(blocks < (1L << 30), SSV_UNSUPPORTED, "conv_pack_plan: too many elements");
    }
  }
  return (int)blocks;
}
extern "C" size_t ssv_conv_pack_multi_workspace(int njobs) { return align256((size_t)(njobs / 2) * SSV_PACK_AMAX_PER_WEIGHT * sizeof(float)); }
extern "C" int ssv_conv_pack_multi(const ssv_pack_job* jobs_dev, int njobs, int nblocks, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(jobs_dev && njobs > 0 && njobs % 2 == 0 && nblocks > 0, SSV_BAD_SHAPE, "conv_pack_multi: bad argument");
  const bool f16 = use_f16();
  SSV_CHECK(!f16 || (ws && ws_bytes >= ssv_conv_pack_multi_workspace(njobs)), SSV_BAD_SHAPE, "conv_pack_multi: workspace too small");
  return ssv_launch_pack_multi(jobs_dev, njobs, nblocks, f16 ? (float*)ws : nullptr, (hipStream_t)stream);
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
// Number of batch slabs Z a weight-gradient launch is cut into (njobs layers x output tiles x Z workgroups, each reducing over
// ceil(B / Z) batch items).  The launch lasts  rounds x (items per workgroup) x (time per item)  +  Z x (slab write + read back),
// rounds = ceil(workgroups / co-resident slots): the slots are few (2 workgroups per CU for the 128 x 64 x 3 tile = 512), so the
// count is a matter of wave quantisation -- 640 workgroups take TWO rounds of which the second runs a quarter full (the ten
// C = 512 / L = 186 layers of the text encoder with Z = 1: 905 us; Z = 4 -> 2,560 workgroups, 5 full rounds of 8 items: 660 us by
// this model).  Round 2 aimed at "about 512 workgroups" whatever the remainder.  L = 0: length unknown (325 assumed).
static int nt_slabs(long tiles_all, int njobs, int B, int L, int kt, int M, int Nc) {
  int wm, ntc;
  ssv_nt_bf3_tile(kt, M, Nc, &wm, &ntc);
  const int per_cu = ssv_nt_bf3_wg_per_cu(kt, wm, ntc);
  const long slots = 256L * per_cu;
  // per workgroup and batch item: 2 x (64 wm) x (16 ntc) x kt x L flop at ~0.55 TFLOP/s per resident workgroup (2 per CU; scaled
  // when more fit); per slab and job: the output written and read back at ~4 TB/s
  const double t_item = 2.0 * 64 * wm * 16 * ntc * kt * L / (0.55e12 * 2.0 / per_cu);
  const double t_slab = 8.0 * (double)M * Nc * kt / 4e12 * njobs;
  int best = 1;
  double best_t = 1e30;
  for (int z = 1; z <= B && z <= 64; ++z) {
    const long rounds = (tiles_all * z + slots - 1) / slots;
    const double t = (double)rounds * ssv_cdiv(B, z) * t_item + (z > 1 ? z * t_slab : 0.0);
    if (t < best_t * 0.98) { best_t = t; best = z; }          // ties and near-ties: the smaller count
  }
  return best;
}
// range slabs of the extra-row kernel (ssv_nt_bf3_xrow): as many slabs as fill the co-resident slots once -- every workgroup then reduces over
// the same number of 64-step chunks, not over a whole number of batch items
static int xrow_slabs(long tiles_all, int B, int L) {
  const long chunks = (long)B * ssv_cdiv(L, 64);
  long z = 512 / (tiles_all > 0 ? tiles_all : 1);
  if (z > chunks) z = chunks;
  if (z > 64) z = 64;
  return (int)(z < 1 ? 1 : z);
}
// THE predicate "this weight gradient runs the split-MFMA kernel", for dy (B, M, L) and x (B, Nc, L) with batch strides dy_bs / x_bs: asked by
// the launch with the operands' real strides, and by everything that must agree with it before the operands exist -- the slab count, the
// workspace queries, ssv_conv1d_bwd_weight_multi_ok -- with dense ones (wgrad_bf3_runs_dense).
static bool wgrad_bf3_runs(int B, int M, int Nc, int L, long dy_bs, long x_bs) {
  if (ssv_precision() < 1 || (long)B * L < 256 || Nc < SSV_MIN_SPLIT_CHANNELS || M < SSV_MIN_SPLIT_CHANNELS) return false;
  GemmNT g;
  g.sab = dy_bs; g.sam = L; g.La = L; g.sxb = x_bs; g.sxc = L; g.Lx = L;
  g.M = M; g.Nc = Nc; g.B = B;
  return ssv_nt_bf3_fits(g);
}
static bool wgrad_bf3_runs_dense(int B, int M, int Nc, int L) { return wgrad_bf3_runs(B, M, Nc, L, (long)M * L, (long)Nc * L); }
static int nt_force(int z, int M, int Nc, int k) {
  if (const char* e = ssv_tuning(SSV_T_NT_FORCE)) {      // "M:Nc:k=Z;..." -- one shape's slab count inside a whole step (tools/sweep_force.sh)
    char key[48];
    snprintf(key, sizeof key, "%d:%d:%d=", M, Nc, k);
    const char* hit = strstr(e, key);
    if (hit && (hit == e || hit[-1] == ';')) { const int v = atoi(hit + strlen(key)); if (v > 0) z = v; }
  }
  return z;
}
int dw_splits(int B, int M, int Nc, int k, int L) {
  const int tiles = ssv_nt_bf3_tiles(k == 3 ? 3 : 1, M, Nc);
  // range slabs only when the extra-row kernel will really run: the fp32 fallback cuts whole-item slabs, Z <= B
  if (k != 3 && ssv_nt_bf3_xrow(1, M, Nc) && wgrad_bf3_runs_dense(B, M, Nc, L)) {
    int z = nt_force(xrow_slabs(tiles, B, L), M, Nc, k);
    const long chunks = (long)B * ssv_cdiv(L, 64);
    if (z > chunks) z = (int)chunks;
    return z < 1 ? 1 : z;
  }
  int z = nt_force(nt_slabs(tiles, 1, B, L, k == 3 ? 3 : 1, M, Nc), M, Nc, k);
  if (z > B) z = B;
  if (z < 1) z = 1;
  return z;
}
// Z slabs [z][m][j][c], then the fallback scale lists of dy and of x
struct WgradWs { int Z; size_t slabs, fb_dy, fb_x, total; };
static WgradWs wgrad_ws(int B, int Cin, int Cout, int L, int k) {
  WsTake t;
  WgradWs l;
  l.Z = dw_splits(B, Cout, Cin, k, L);
  l.slabs = t.take((size_t)l.Z * Cout * Cin * k * sizeof(float));
  l.fb_dy = t.take(AMAX_FB_BYTES);
  l.fb_x = t.take(AMAX_FB_BYTES);
  l.total = t.off;
  return l;
}
extern "C" size_t ssv_conv1d_bwd_weight_workspace(int B, int Cin, int Cout, int L, int k) { return wgrad_ws(B, Cin, Cout, L, k).total; }
int conv1d_bwd_weight_impl(const float* dy, long dy_bs, const float* x, long x_bs, float* dw, int B, int Cin, int Cout, int L, int k, int dilation,
                           int causal, void* ws, size_t ws_bytes, ssv_stream_t stream, const float* part, float* pgrads, int n2, int nblk,
                           const float* dy_amax, int dy_namax, const float* x_amax, int x_namax) {
  SSV_CHECK(dy && x && dw && B > 0 && Cin > 0 && Cout > 0 && L > 0, SSV_BAD_SHAPE, "conv1d_bwd_weight: bad argument");
  const WgradWs l = wgrad_ws(B, Cin, Cout, L, k);
  SSV_CHECK(ws && ws_bytes >= l.total, SSV_BAD_SHAPE, "conv1d_bwd_weight: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  GemmNT g;
  SSV_TRY(conv_shifts(k, dilation, causal, g.shift));
  int Z = l.Z;
  const float* slabs = ws_f32(ws, l.slabs);
  const long n = (long)Cout * Cin * k;
  g.A = dy; g.sab = dy_bs; g.sam = L; g.La = L;
  g.X = x; g.sxb = x_bs; g.sxc = L; g.Lx = L;
  g.M = Cout; g.Nc = Cin; g.KT = k; g.B = B;
  const bool bf3 = wgrad_bf3_runs(B, Cout, Cin, L, dy_bs, x_bs);
  if (!bf3 && Z > B) Z = B;        // (range-slab count chosen for dense operands, strided ones do not fit the split kernel: whole-item slabs, no empty ones)
  if (Z == 1) { g.C = dw; g.scz = n; g.scm = (long)Cin * k; g.scc = k; g.scj = 1; }
  else { g.C = ws_f32(ws, l.slabs); g.scz = n; g.scm = (long)Cin * k; g.scc = 1; g.scj = Cin; }     // slabs [z][m][j][c]
  g.Z = Z; g.bstep = Z;
  if (bf3) {
    if (k != 3 && ssv_nt_bf3_xrow(1, Cout, Cin)) g.bstep = 0;            // range slabs (dw_splits chose Z for them; any Z <= chunks is valid)
    if (use_f16()) {
      AmaxList la, lx;
      SSV_TRY(amax_of(dy, dy_bs, B, (long)Cout * L, dy_amax, dy_namax, ws_f32(ws, l.fb_dy), &la, st));
      SSV_TRY(amax_of(x, x_bs, B, (long)Cin * L, x_amax, x_namax, ws_f32(ws, l.fb_x), &lx, st));
      g.f16 = 1; g.a_amax = la.p; g.a_namax = la.n * B; g.x_amax = lx.p; g.x_namax = lx.n * B;
    }
    SSV_TRY(ssv_launch_gemm_nt_bf3(g, st));
  } else if (L == 1 && k == 1) {                       // see linear_len1_wgrad_kernel; writes dw itself, whatever Z says
    SSV_TRY(ssv_launch_linear_len1_wgrad(dy, dy_bs, x, x_bs, dw, B, Cin, Cout, st));
    if (part) SSV_TRY(ssv_reduce_partial_rows(part, pgrads, n2, nblk, st));
    return 0;
  } else SSV_TRY(ssv_launch_gemm_nt(g, st));
  if (part) {
    if (Z > 1 && nblk <= 768) return ssv_launch_reduce_pair(slabs, dw, Cout, Cin, k, Z, part, pgrads, n2, nblk, st);
    SSV_TRY(ssv_reduce_partial_rows(part, pgrads, n2, nblk, st));
  }
  if (Z > 1) SSV_TRY(ssv_launch_reduce_slabs_perm(slabs, dw, Cout, Cin, k, Z, st));
  return 0;
}
extern "C" int ssv_conv1d_bwd_weight(const float* dy, long dy_bs, const float* dy_amax, int dy_namax, const float* x, long x_bs, const float* x_amax, int x_namax,
                                     float* dw, int B, int Cin, int Cout, int L, int k, int dilation, int causal,
                                     void* ws, size_t ws_bytes, ssv_stream_t stream) {
  return conv1d_bwd_weight_impl(dy, dy_bs, x, x_bs, dw, B, Cin, Cout, L, k, dilation, causal, ws, ws_bytes, stream, nullptr, nullptr, 0, 0,
                                dy_amax, dy_namax, x_amax, x_namax);
}

// ---- several equal-shaped weight gradients in one launch (see include/ssv_hip.h) ------------------------------------------
extern "C" int ssv_conv1d_bwd_weight_multi_ok(int B, int Cin, int Cout, int L, int k) {
  return (k == 1 || k == 3) && L >= 8 && wgrad_bf3_runs_dense(B, Cout, Cin, L) ? 1 : 0;
}
extern "C" int ssv_conv1d_bwd_weight_multi_splits(int njobs, int B, int Cin, int Cout, int L, int k) {
  const int kt = k == 3 ? 3 : 1;
  if (njobs < 1) njobs = 1;
  const long tiles = (long)ssv_nt_bf3_tiles(kt, Cout, Cin) * njobs;
  if (kt == 1 && ssv_nt_bf3_xrow(1, Cout, Cin)) return xrow_slabs(tiles, B, L);
  int z = nt_slabs(tiles, njobs, B, L, kt, Cout, Cin);
  if (z > B) z = B;
  if (z < 1) z = 1;
  return z;
}
extern "C" size_t ssv_conv1d_bwd_weight_multi_workspace(int njobs, int B, int Cin, int Cout, int L, int k) {      // one region: slabs [job][z][m][j][c]
  return align256((size_t)njobs * ssv_conv1d_bwd_weight_multi_splits(njobs, B, Cin, Cout, L, k) * Cout * Cin * k * sizeof(float));
}
extern "C" int ssv_conv1d_bwd_weight_multi(const ssv_wgrad_job* jobs_dev, int njobs, long dy_bs, long x_bs, int B, int Cin, int Cout, int L, int k, int max_shift,
                                           int n2, int nblk, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(jobs_dev && njobs > 0 && B > 0 && Cin > 0 && Cout > 0 && L > 0, SSV_BAD_SHAPE, "conv1d_bwd_weight_multi: bad argument");
  SSV_CHECK(ssv_conv1d_bwd_weight_multi_ok(B, Cin, Cout, L, k), SSV_UNSUPPORTED, "conv1d_bwd_weight_multi: shape or arithmetic mode not supported");
  SSV_CHECK(n2 == 0 || nblk <= 768, SSV_UNSUPPORTED, "conv1d_bwd_weight_multi: %d partial rows (max 768)", nblk);
  SSV_CHECK(ws && ws_bytes >= ssv_conv1d_bwd_weight_multi_workspace(njobs, B, Cin, Cout, L, k), SSV_BAD_SHAPE, "conv1d_bwd_weight_multi: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int Z = ssv_conv1d_bwd_weight_multi_splits(njobs, B, Cin, Cout, L, k);
  const long n = (long)Cout * Cin * k;
  GemmNT g;
  g.sab = dy_bs; g.sam = L; g.La = L;
  g.sxb = x_bs; g.sxc = L; g.Lx = L;
  g.C = (float*)ws; g.scz = n; g.scm = (long)Cin * k; g.scc = 1; g.scj = Cin;                 // slabs [job][z][m][j][c]
  g.M = Cout; g.Nc = Cin; g.KT = k; g.B = B; g.Z = Z; g.bstep = (k != 3 && ssv_nt_bf3_xrow(1, Cout, Cin)) ? 0 : Z;      // (0: range slabs)
  g.jobs = jobs_dev; g.njobs = njobs; g.max_shift = max_shift;
  g.f16 = use_f16() ? 1 : 0;                     // the jobs carry their operands' scale lists (the caller saw to that)
  SSV_TRY(ssv_launch_gemm_nt_bf3(g, st));
  return ssv_launch_reduce_pair_multi(jobs_dev, njobs, (const float*)ws, Cout, Cin, k, Z, n2, nblk, st);
}

// ---- ConvTranspose1d(k=2, s=2) -----------------------------------------------------------------------------
// Split-bf16 path of the two deconvolution halves: both taps' weights are split by ONE pack launch (tap-major planes);
// tap j is a k=1 product whose output (forward) or input (data gradient) columns have stride 2.
static ConvWs deconv_fwd_ws(int Cin, int Cout) { return conv_ws(2 * split_bytes(Cout, Cin, 2)); }
extern "C" size_t ssv_deconv1d_k2s2_fwd_workspace(int Cin, int Cout) { return deconv_fwd_ws(Cin, Cout).total; }
extern "C" int ssv_deconv1d_k2s2_fwd(const float* x, long x_bs, const float* x_amax, int x_namax, const float* w, const void* w_packed, const float* bias,
                                     float* y, long y_bs, float* y_amax, int y_namax, int B, int Cin, int Cout, int L, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(x && w && y && B > 0 && Cin > 0 && Cout > 0 && L > 0, SSV_BAD_SHAPE, "deconv1d_k2s2_fwd: bad argument");
  SSV_CHECK(!y_amax || y_namax > 0, SSV_BAD_SHAPE, "deconv1d_k2s2_fwd: scale list of %d entries", y_namax);
  hipStream_t st = (hipStream_t)stream;
  if (use_bf3(B, L, Cin, Cout)) {
    // ONE product over 2 Cout rows (round 6): u = W2^T x with W2 = w.view(Cin, 2 Cout) -- row 2 o + j of u is tap j of output channel o -- whose
    // epilogue interleaves row pairs into y(b, o, 2 t + j) (GemmNNB::row_pair).  The planes are the TRANSPOSED planes of the 1x1 weight
    // w.view(Cin, 2 Cout, 1): resident ones when the caller keeps them (w_packed, ssv_conv_pack_multi), else split here.
    // (Before: one stride-2 product per tap behind a per-call scan + split of the weight, and an ssv_absmax launch over y for the next layer.)
    const ConvWs l = deconv_fwd_ws(Cin, Cout);
    SSV_CHECK(ws && ws_bytes >= l.total, SSV_BAD_SHAPE, "deconv1d_k2s2_fwd: workspace too small");
    const int M2 = 2 * Cout, Kpad = pad32(Cin);
    const bool f16 = use_f16();
    float* aux = ws_f32(ws, l.aux);
    SplitPlanes pl = packed_planes(w_packed, Cin, M2, 1).tr;
    if (!pl.hi) {
      pl.hi = ws_u16(ws, l.main); pl.lo = ws_u16(ws, l.main + split_bytes(M2, Cin, 1));
      // (m = 2 o + j, k = c) = w[c][o][j] = w[c * 2 Cout + m]: row stride 1, column stride 2 Cout
      if (f16) { SSV_TRY(ssv_launch_pack_split_f16(w, (long)Cin * M2, pl.hi, pl.lo, M2, Cin, Kpad, 1, 1, (long)M2, 1, aux, st)); pl.inv = aux + 64; }
      else SSV_TRY(ssv_launch_pack_split(w, pl.hi, pl.lo, M2, Cin, Kpad, 1, 1, (long)M2, 1, 0, st));
    }
    GemmNNB g;
    if (f16) {
      AmaxList xa = {nullptr, 0};
      SSV_TRY(amax_of(x, x_bs, B, (long)Cin * L, x_amax, x_namax, ws_f32(ws, l.fb), &xa, st));
      g.f16 = 1; g.a_inv = pl.inv; g.x_amax = xa.p; g.x_namax = xa.n; g.x_amax_bs = xa.n;
    }
    g.Ahi = pl.hi; g.Alo = pl.lo; g.Kpad = Kpad;
    g.X = x; g.sxb = x_bs; g.sxc = L; g.Lx = L;
    g.C = y; g.scb = y_bs; g.scm = (long)2 * L; g.row_pair = 1;
    g.bias = bias;
    g.M = M2; g.N = L; g.Kc = Cin; g.B = B;
    if (y_amax && f16) { g.c_amax = y_amax; g.c_namax = y_namax; }
    const int rc = ssv_launch_gemm_nn_bf3(g, st);
    if (rc == SSV_UNSUPPORTED && g.c_amax) {                   // more tiles per item than list entries: the product without the list, then a scan
      g.c_amax = nullptr; g.c_namax = 0;
      SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
      return ssv_launch_absmax(y, y_bs, B, (long)Cout * 2 * L, y_amax, y_namax, st);
    }
    return rc;
  }
  for (int j = 0; j < 2; ++j) {               // y(b,o,2t+j) = bias[o] + sum_c w[c,o,j] x(b,c,t)
    GemmNN g;
    g.A = w + j; g.sam = 2; g.sac = (long)2 * Cout;
    g.X = x; g.sxb = x_bs; g.sxc = L; g.Lx = L;
    g.C = y + j; g.scb = y_bs; g.scm = (long)2 * L; g.scn = 2;
    g.bias = bias;
    g.M = Cout; g.N = L; g.Kc = Cin; g.B = B;
    SSV_TRY(ssv_launch_gemm_nn(g, st));
  }
  if (y_amax && use_f16()) return ssv_launch_absmax(y, y_bs, B, (long)Cout * 2 * L, y_amax, y_namax, st);
  return 0;
}
// Z weight-gradient slabs (the query has no length: SSV_NOMINAL_L), the bias gradient's row sums (B, Cout), both taps' planes (hi, then lo),
// the pack kernel's aux floats, the fallback scale list of dy
struct DeconvBwdWs { int Z; size_t slabs, rs, hi, lo, aux, fb, total; };
static DeconvBwdWs deconv_bwd_ws(int B, int Cin, int Cout) {
  WsTake t;
  DeconvBwdWs l;
  l.Z = dw_splits(B, Cin, Cout, 1, SSV_NOMINAL_L);
  l.slabs = t.take((size_t)l.Z * Cin * Cout * 2 * sizeof(float));
  l.rs = t.take((size_t)B * Cout * sizeof(float));
  l.hi = t.take(split_bytes(Cin, Cout, 2));
  l.lo = t.take(split_bytes(Cin, Cout, 2));
  l.aux = t.take(SSV_F16_AUX_BYTES);
  l.fb = t.take(AMAX_FB_BYTES);
  l.total = t.off;
  return l;
}
extern "C" size_t ssv_deconv1d_k2s2_bwd_workspace(int B, int Cin, int Cout) { return deconv_bwd_ws(B, Cin, Cout).total; }
extern "C" int ssv_deconv1d_k2s2_bwd(const float* dy, long dy_bs, const float* dy_amax, int dy_namax, const float* x, long x_bs, const float* w, float* dx, long dx_bs,
                                     float* dw, float* dbias, int B, int Cin, int Cout, int L, void* ws, size_t ws_bytes, ssv_stream_t stream) {
  SSV_CHECK(dy && x && w && dx && B > 0 && Cin > 0 && Cout > 0 && L > 0, SSV_BAD_SHAPE, "deconv1d_k2s2_bwd: bad argument");      // dw may be NULL: see the header
  const DeconvBwdWs l = deconv_bwd_ws(B, Cin, Cout);
  SSV_CHECK(ws && ws_bytes >= l.total, SSV_BAD_SHAPE, "deconv1d_k2s2_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int Z = l.Z;
  const long n = (long)Cin * Cout * 2;
  float* slabs = ws_f32(ws, l.slabs);
  float* rs = ws_f32(ws, l.rs);
  const bool bf3 = use_bf3(B, L, Cout, Cin);
  unsigned short* hi = ws_u16(ws, l.hi);
  unsigned short* lo = ws_u16(ws, l.lo);
  const int Kpad = pad32(Cout);
  const size_t tap = (size_t)((Cin + 15) / 16 * 16) * Kpad;
  const bool f16 = bf3 && use_f16();
  float* aux = ws_f32(ws, l.aux);
  AmaxList ya = {nullptr, 0};
  if (f16) {
    SSV_TRY(ssv_launch_pack_split_f16(w, (long)Cin * Cout * 2, hi, lo, Cin, Cout, Kpad, 2, (long)2 * Cout, 2, 1, aux, st));
    SSV_TRY(amax_of(dy, dy_bs, B, (long)Cout * 2 * L, dy_amax, dy_namax, ws_f32(ws, l.fb), &ya, st));
  } else if (bf3) SSV_TRY(ssv_launch_pack_split(w, hi, lo, Cin, Cout, Kpad, 2, (long)2 * Cout, 2, 1, 0, st));   // (m=c, k=o, tap j) = w[c][o][j]
  for (int j = 0; j < 2; ++j) {
    if (bf3) {                                 // dx(b,c,t) (+)= sum_o w[c,o,j] dy(b,o,2t+j)
      GemmNNB g;
      if (f16) { g.f16 = 1; g.a_inv = aux + 64; g.x_amax = ya.p; g.x_namax = ya.n; g.x_amax_bs = ya.n; }
      g.Ahi = hi + j * tap; g.Alo = lo + j * tap; g.Kpad = Kpad;
      g.X = dy + j; g.sxb = dy_bs; g.sxc = (long)2 * L; g.sxn = 2; g.Lx = L;
      g.C = dx; g.scb = dx_bs; g.scm = L;
      if (j == 1) { g.R = dx; g.srb = dx_bs; g.srm = L; }
      g.M = Cin; g.N = L; g.Kc = Cout; g.B = B;
      SSV_TRY(ssv_launch_gemm_nn_bf3(g, st));
    } else {
      GemmNN g;
      g.A = w + j; g.sam = (long)2 * Cout; g.sac = 2;
      g.X = dy + j; g.sxb = dy_bs; g.sxc = (long)2 * L; g.sxn = 2; g.Lx = L;
      g.C = dx; g.scb = dx_bs; g.scm = L;
      if (j == 1) { g.R = dx; g.srb = dx_bs; g.srm = L; }
      g.M = Cin; g.N = L; g.Kc = Cout; g.B = B;
      SSV_TRY(ssv_launch_gemm_nn(g, st));
    }
    if (!dw) continue;
    GemmNT t;                                  // dw[c,o,j] = sum_{b,t} x(b,c,t) dy(b,o,2t+j)
    t.A = x; t.sab = x_bs; t.sam = L; t.La = L;
    t.X = dy + j; t.sxb = dy_bs; t.sxc = (long)2 * L; t.sxn = 2; t.Lx = L;
    t.C = ((Z == 1) ? dw : slabs) + j; t.scz = n; t.scm = (long)2 * Cout; t.scc = 2;
    t.M = Cin; t.Nc = Cout; t.B = B; t.Z = Z; t.bstep = Z;
    SSV_TRY(ssv_launch_gemm_nt(t, st));
  }
  if (dw && Z > 1) SSV_TRY(ssv_launch_reduce_slabs(slabs, dw, n, Z, n, st));
  if (dbias) {
    SSV_TRY(ssv_rowsum(dy, dy_bs, rs, B, Cout, 2 * L, stream));
    SSV_TRY(ssv_launch_reduce_slabs(rs, dbias, Cout, B, Cout, st));
  }
  return 0;
}
