"""GE2E training on the HIP path against a float64 run of the oracle, in every arithmetic mode.

The LSTM backward (csrc/api_lstm_train.hip ssv_lstm_bwd: the reverse wavefront's merged data-gradient products, the cell backward, the weight gradients
over all frames) and the GE2E loss kernels (csrc/lstm.hip) are compared per tensor with ``oracle/ge2e_oracle.py`` run in float64 on the
GPU, at the embedder's real width (hidden 768, projection 256) and at the shapes where the kernels change form.  Each case runs the three
modes back to back against the same float64 result:

* "fp32": exact fp32 MFMA -- an absolute bar per metric;
* "f16x2" (the default): split-fp16 MFMA, promised fp32-grade -- a multiple of the fp32 mode's error on the same case and
  tensor (F16X2_FACTOR), plus a floor of 1e-7 for tensors the fp32 mode gets (almost) exactly right;
* "bf16x3": split-bf16 MFMA, ~2^-16 per product -- an absolute bar of its own.

Every backward runs twice per mode and must give bit-identical gradients (the kernels promise fixed reduction orders).
Run with ``-s`` to see the measured errors."""
import gc

import pytest
import torch

from _golden import rel_err, rel_l2
from oracle import ge2e_oracle as GO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("fp32", "f16x2", "bf16x3")

# (rel_l2, rel_err) bars against float64, over every tensor of every case below; the bias gradients (and the projection's) are sums over
# frames and utterances with cancellation and have bars of their own.  Measured worst over the cases (on the library before the split-fp16
# backward; the fp32 and bf16x3 paths are unchanged by it):
#   fp32    weights / embeddings 2.8e-6 / 4.0e-6 (inputs x 50, W_hh[0]),  biases 2.1e-5 / 4.1e-5 (config 5, layer 2 / projection)
#   bf16x3  1.1e-4 / 1.5e-4 (inputs x 50, layer 0)
FP32_BAR = {"weight": (1e-5, 1.5e-5), "bias": (7e-5, 1e-4)}
BF16X3_BAR = (3.5e-4, 5e-4)
# f16x2: at most F16X2_FACTOR x the fp32 mode's error on the same case and tensor, + F16X2_FLOOR.  With the backward in split-bf16 (before
# ssv_lstm_bwd took the split-fp16 products) the worst ratio per split case was 7.1 .. 32; with split-fp16 products it is 1.0 .. 3.5
# (ragged columns, layer 0's bias).  Config 5 has a bar of its own: there the f16x2 FORWARD is 10x the fp32 one on the embeddings (7.9e-7
# against 7.7e-8, the same before and after the backward's change), and that carries into every gradient (worst ratio 8.9 with the
# split-fp16 backward, 8.9 without) -- held where it is until the forward is looked into.
F16X2_FACTOR, F16X2_FLOOR = 4.0, 1e-7
F16X2_FACTOR_CONFIG5 = 10.0
# The GE2E loss's own w and b gradients are sums of N M N terms of order 1 whose exact value is far smaller than the terms (db ~ -1e-6 N M /
# sum exp S): they are held to an absolute error per embedding row, |err| / (N M), in every mode.
WB_BAR = 1e-6
_WB = ("w.grad", "b.grad")


def _model_sd(F, H, P, layers, seed, reseed_bias):
    from spoofsv_amd.ge2e import SpeechEmbedder
    torch.manual_seed(seed)
    m = SpeechEmbedder(nmels=F, hidden=H, num_layer=layers, proj=P)
    if reseed_bias:
        with torch.no_grad():
            for n, p in m.LSTM_stack.named_parameters():
                if "bias" in n:
                    p.uniform_(-0.2, 0.2)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _report(case, errs):
    names = list(errs["fp32"])
    print("\n%s: rel_l2 / rel_err against float64" % case)
    print("  %-28s %21s %21s %21s %8s" % ("tensor", "fp32", "f16x2", "bf16x3", "f16/fp32"))
    for n in names:
        a, b, c = (errs[m][n] for m in MODES)
        print("  %-28s %10.2e %10.2e %10.2e %10.2e %10.2e %10.2e %8.2f" % (n, a[0], a[1], b[0], b[1], c[0], c[1], b[0] / max(a[0], 1e-30)))


def _check(case, errs, f16x2_factor=F16X2_FACTOR):
    """All bars of one case; every violation is listed (not just the first)."""
    _report(case, errs)
    bad = []
    for n, (l2, mx) in errs["fp32"].items():
        if n in _WB:
            bad += [(m, n, errs[m][n][0]) for m in MODES if not errs[m][n][0] < WB_BAR]
            continue
        bar = FP32_BAR["bias" if "bias" in n else "weight"]
        if l2 > bar[0] or mx > bar[1]:
            bad.append(("fp32", n, l2, mx))
        f2, fm = errs["f16x2"][n]
        if f2 > f16x2_factor * l2 + F16X2_FLOOR or fm > f16x2_factor * mx + F16X2_FLOOR:
            bad.append(("f16x2 vs %g x fp32" % f16x2_factor, n, f2, fm, l2, mx))
        b2, bm = errs["bf16x3"][n]
        if b2 > BF16X3_BAR[0] or bm > BF16X3_BAR[1]:
            bad.append(("bf16x3", n, b2, bm))
    assert not bad, bad


def _errs(got, ref):
    return {n: (rel_l2(got[n], ref[n]), rel_err(got[n], ref[n])) for n in ref}


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _assert_same(a, b, what):
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, (what, "not bit-identical between two runs on the same input", diff)


# ---- embedder backward with a random upstream gradient on the embeddings --------------------------------------------------------

_REF = {}


def _embedder_case(Bn, T, F, H, P, layers, scale=1.0, seed=0):
    """float64 reference of (embeddings, every parameter gradient) for a random upstream gradient; computed once per shape (the graph is
    freed before any HIP run)."""
    key = (Bn, T, F, H, P, layers, scale, seed)
    if key not in _REF:
        sd = _model_sd(F, H, P, layers, 1000 + seed, reseed_bias=True)
        g = torch.Generator().manual_seed(2000 + seed)
        x = torch.randn(Bn, T, F, generator=g) * scale
        de = torch.randn(Bn, P, generator=g)
        p64 = {k: v.to(DEV, torch.float64).requires_grad_(True) for k, v in sd.items()}
        e = GO.speech_embedder(x.to(DEV), p64, num_layers=layers, dtype=torch.float64)
        e.backward(de.to(DEV, torch.float64))
        ref = {"embeddings": e.detach().cpu()}
        ref.update({k: p64[k].grad.cpu() for k in sd})
        del e, p64
        _free()
        _REF[key] = (sd, x, de, ref)
    return _REF[key]


def _run_embedder(sd, x, de, F, H, P, layers):
    import spoofsv_amd
    from spoofsv_amd.ge2e import SpeechEmbedder
    out = {}
    xg, deg = x.to(DEV), de.to(DEV)
    for mode in MODES:
        spoofsv_amd.set_precision(mode)
        m = SpeechEmbedder(nmels=F, hidden=H, num_layer=layers, proj=P)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        runs = []
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            e = m(xg)
            e.backward(deg)
            got = _grads(m)
            got["embeddings"] = e.detach().clone()
            runs.append(got)
        _assert_same(runs[0], runs[1], mode)
        out[mode] = {k: v.cpu() for k, v in runs[0].items()}
        del m, e, runs
        _free()
    return out


# (Bn, T, F, H, P, layers, input scale): what each reaches
EMBEDDER_CASES = {
    # lstm_cell_bwd_kernel<1> (Bn % 4 != 0), a ragged last 128-column tile, the wavefront's ramp-up and ramp-down
    "ragged_columns_scalar_cell": (701, 7, 40, 768, 256, 3, 1.0),
    # fewer frames than layers: reverse steps in which not every layer is active
    "frames_below_layers": (704, 2, 40, 768, 256, 3, 1.0),
    # one frame: dW_hh is exactly 0, only the top cell gets the projection's gradient
    "single_frame": (640, 1, 40, 768, 256, 3, 1.0),
    # lo / hi of the wavefront, g.B, skip_rows with a single layer, the forward's layers >= 2 pre-split rule
    "one_layer": (256, 9, 40, 768, 256, 1, 1.0),
    "two_layers": (256, 9, 40, 768, 256, 2, 1.0),
    "four_layers": (256, 9, 40, 768, 256, 4, 1.0),
    # W_ih[0]'s gradient with 130 input features; the inputs' scale moves the operand scales of the split modes
    "input_width_130_x50": (96, 11, 130, 256, 48, 3, 50.0),
    "input_width_130_x1e-3": (96, 11, 130, 256, 48, 3, 1e-3),
    # the smallest batch of the split kernels, and the exact-fp32 fallbacks of the split modes (Bn < 8, H % 32 != 0)
    "split_batch_8": (8, 5, 40, 64, 32, 3, 1.0),
    "split_batch_9": (9, 5, 40, 64, 32, 3, 1.0),
    "fallback_batch_7": (7, 5, 40, 64, 32, 3, 1.0),
    "fallback_hidden_48": (9, 5, 40, 48, 32, 3, 1.0),
}


@pytest.mark.parametrize("case", list(EMBEDDER_CASES))
def test_ge2e_embedder_backward_vs_float64(case):
    Bn, T, F, H, P, layers, scale = EMBEDDER_CASES[case]
    sd, x, de, ref = _embedder_case(Bn, T, F, H, P, layers, scale, seed=list(EMBEDDER_CASES).index(case))
    got = _run_embedder(sd, x, de, F, H, P, layers)
    if T == 1:                                  # no recurrent product: the weight_hh gradients are exactly zero in every mode
        for mode in MODES:
            for l in range(layers):
                assert not got[mode]["LSTM_stack.weight_hh_l%d" % l].any(), (mode, l)
        for l in range(layers):
            ref.pop("LSTM_stack.weight_hh_l%d" % l, None)
    errs = {mode: _errs(got[mode], ref) for mode in MODES}
    _check(case, errs)


# ---- config 5: the timed training iteration ----------------------------------------------------------------------------------

def test_ge2e_config5_training_iteration_vs_float64():
    """tools/ge2e_train_time.py's iteration (880 = 88 x 10 utterances of 120 frames, hidden 768, seed 0): loss, embeddings, every
    gradient including the loss's w and b, and the parameters after the reference's two clip_grad_norm_ calls and SGD."""
    import spoofsv_amd
    from spoofsv_amd.ge2e import GE2ELoss, SpeechEmbedder
    N, M, T, F, H, P, layers, lr = 88, 10, 120, 40, 768, 256, 3, 0.01
    torch.manual_seed(0)
    m0 = SpeechEmbedder()
    L0 = GE2ELoss("cpu")
    x = torch.randn(N * M, T, F)
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    w0, b0 = float(L0.w), float(L0.b)
    loss, grads, (dw, db), new_sd, (w1, b1), emb = GO.ge2e_train_step(x.to(DEV), sd, w0, b0, N, M, layers, lr=lr, dtype=torch.float64,
                                                                   return_emb=True)
    ref = {"loss": loss.cpu(), "embeddings": emb.cpu(), "w.grad": dw.cpu(), "b.grad": db.cpu()}
    ref.update({k: v.cpu() for k, v in grads.items()})
    ref.update({"new " + k: v.cpu() for k, v in new_sd.items()})
    ref.update({"new w": w1.cpu(), "new b": b1.cpu()})
    del loss, grads, dw, db, new_sd, w1, b1, emb
    _free()
    xg = x.to(DEV)
    errs = {}
    for mode in MODES:
        spoofsv_amd.set_precision(mode)
        runs = []
        for _ in range(2):
            m = SpeechEmbedder()
            m.load_state_dict(sd)
            m = m.to(DEV).train()
            L = GE2ELoss(DEV)
            opt = torch.optim.SGD([{"params": m.parameters()}, {"params": L.parameters()}], lr=lr)
            opt.zero_grad()
            e = m(xg)
            ls = L(e.reshape(N, M, -1))
            ls.backward()
            got = _grads(m)
            got.update({"loss": ls.detach().clone(), "embeddings": e.detach().clone(), "w.grad": L.w.grad.clone(), "b.grad": L.b.grad.clone()})
            torch.nn.utils.clip_grad_norm_(m.parameters(), 3.0)
            torch.nn.utils.clip_grad_norm_(L.parameters(), 1.0)
            opt.step()
            got.update({"new " + k: v.detach().clone() for k, v in m.state_dict().items()})
            got.update({"new w": L.w.detach().clone(), "new b": L.b.detach().clone()})
            runs.append({k: v.cpu() for k, v in got.items()})
            del m, L, opt, e, ls, got
            _free()
        _assert_same(runs[0], runs[1], mode)
        errs[mode] = _errs(runs[0], ref)
        for n in _WB:                           # absolute, per embedding row (see WB_BAR)
            e_ = float((runs[0][n].double() - ref[n]).abs()) / (N * M)
            errs[mode][n] = (e_, e_)
    _check("config5_iteration", errs, F16X2_FACTOR_CONFIG5)


# ---- GE2E loss kernels at ragged shapes ------------------------------------------------------------------------------------

# rel_l2 bar for the loss kernels (plain fp32 in every mode): measured worst 1.5e-6 (loss and per of N = 1, whose one term is the difference
# log(e^S + 1e-6) - S); dw and db are held to WB_BAR as above, scaled by the upstream gradient
LOSS_BAR = 1e-5


def _loss_inputs(N, M, D, seed):
    """Random embeddings whose row norms span 1e-3 .. 1e3: a speaker's rows within a factor of 4 of each other, the speakers spread over
    the six decades.  (Not six decades within one speaker: the leave-one-out centroid is (sum - e) / (M - 1), in the kernels as in the
    oracle's restatement, and a 1e-3 row beside a 1e3 row of its own speaker loses its digits to that subtraction in fp32 -- measured
    5e-3 on the cosines of the fp32 oracle itself.)"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(N, M, D, generator=g)
    scale = 10.0 ** torch.empty(N, 1, 1).uniform_(-3.0, 3.0, generator=g) * 2.0 ** torch.empty(N, M, 1).uniform_(-1.0, 1.0, generator=g)
    return e / e.norm(dim=2, keepdim=True) * scale


# (w, b, upstream gradient), clear of the reference's 10 / -5: with b = -14 the log's +1e-6 term is as large as the exponentials
LOSS_PARAMS = [(3.0, -14.0, 0.5), (0.5, 1.5, 3.0)]
LOSS_SHAPES = [(1, 2, 16), (5, 7, 48), (3, 17, 300), (13, 64, 256), (88, 10, 256), (1024, 2, 64)]
# (N = 1 with the second set is left out: its one loss term is log(e^S + 1e-6) - S ~ 1e-7, below fp32's resolution of the log)
LOSS_CASES = [(s, p) for s in LOSS_SHAPES for p in LOSS_PARAMS if not (s[0] == 1 and p[1] > 0)]


@pytest.mark.parametrize("shape,params", LOSS_CASES, ids=["%dx%dx%d-w%g" % (s + (p[0],)) for s, p in LOSS_CASES])
def test_ge2e_loss_kernels_vs_float64(shape, params):
    """GE2ELoss forward (loss, per-embedding losses) and backward (embeddings, w, b) against the float64 oracle: N not a multiple of
    the kernels' 4 waves, D > 256 (the d0 loop and the dok tail of ge2e_bwd_centroid_kernel), N = GE2E_MAXN; embeddings whose
    norms span 1e-3 .. 1e3 (the cosine is scale-invariant: a missing normalisation shows)."""
    from spoofsv_amd.ge2e import GE2ELoss
    N, M, D = shape
    w, b, up = params
    e = _loss_inputs(N, M, D, N * 1000 + M * 10 + D)
    er = e.double().requires_grad_(True)
    wr = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    br = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    lr_, per_r = GO.ge2e_loss(er, wr, br)
    (up * lr_).backward()
    L = GE2ELoss(DEV)
    with torch.no_grad():
        L.w.fill_(w); L.b.fill_(b)
    eg = e.to(DEV).requires_grad_(True)
    lg, per_g = L(eg, return_per_embedding=True)
    (up * lg).backward()
    res = {"loss": (lg, lr_), "per": (per_g, per_r), "d_emb": (eg.grad, er.grad), "dw": (L.w.grad, wr.grad), "db": (L.b.grad, br.grad)}
    errs = {n: rel_l2(a, r) for n, (a, r) in res.items() if n not in ("dw", "db")}
    errs.update({n: float((a.detach().double().cpu() - r).abs()) / (up * N * M) for n, (a, r) in res.items() if n in ("dw", "db")})
    print("\nGE2E loss %s w=%g b=%g x%g: " % (shape, w, b, up) + "  ".join("%s %.2e" % kv for kv in errs.items()))
    bad = {n: v for n, v in errs.items() if not v < (WB_BAR if n in ("dw", "db") else LOSS_BAR)}
    assert not bad, bad


def test_ge2e_loss_beyond_the_backward_speaker_limit():
    """N = 1025 > GE2E_MAXN: the forward is still right; the backward raises the library's error instead of returning gradients."""
    from spoofsv_amd.ge2e import GE2ELoss
    N, M, D = 1025, 2, 32
    e = _loss_inputs(N, M, D, 7)
    lr_, per_r = GO.ge2e_loss(e.double(), torch.tensor(10.0, dtype=torch.float64), torch.tensor(-5.0, dtype=torch.float64))
    L = GE2ELoss(DEV)
    eg = e.to(DEV).requires_grad_(True)
    lg, per_g = L(eg, return_per_embedding=True)
    assert rel_l2(lg, lr_) < LOSS_BAR and rel_l2(per_g, per_r) < LOSS_BAR, (rel_l2(lg, lr_), rel_l2(per_g, per_r))
    with pytest.raises(RuntimeError, match="ge2e_loss_bwd"):
        lg.backward()
    assert eg.grad is None
