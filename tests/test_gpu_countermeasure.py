"""The spoof countermeasure on the device against plain references (tests/_countermeasure_ref.py): the fused classifier head through the
raw ABI against the float64 value of its formulas, ssv_adam_ex_multi and FusedAdamEx per element against a float64 step from the
device's own state, the small whole classifiers against the float64 restatement in every arithmetic mode, and the trainer / scorer end
to end on a toy corpus.  Run with `-m gpu` on an MI355X."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _countermeasure_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -0x21524111                                # int32 pattern 0xDEADBEEF: a finite float, -6.26e18
GUARD = 8
MODES = ("f16x2", "bf16x3", "fp32")
_REF = {}
_WORST = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _report(part, what, err, bar):
    print("%-5s %-66s err %.3e  bar %.3e  fraction %.3f" % (part, what, err, bar, err / bar))
    if err / bar > _WORST.get(part, (0.0, ""))[0]:
        _WORST[part] = (err / bar, what)
    return err <= bar


@pytest.fixture(scope="module", autouse=True)
def _worst_fractions():
    yield
    print()
    for part, (f, what) in sorted(_WORST.items()):
        print("worst fraction of a bound, %-5s %.3f  (%s)" % (part, f, what))


@pytest.fixture
def precision(request):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(request.param)
    yield request.param
    spoofsv_amd.set_precision(prev)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ================================================================================================ a. the head through the raw ABI
class _Guarded:
    """Output tensors carved out of one poisoned device buffer with GUARD words before and after each; starts are whole 16-byte units."""

    def __init__(self, sizes):
        self.at, cur = {}, GUARD
        for name, n in sizes:
            cur = (cur + 3) // 4 * 4
            self.at[name] = (cur, n)
            cur += n + GUARD
        self.size = (cur + 3) // 4 * 4
        self.buf = torch.from_numpy(np.full(self.size, POISON, dtype=np.int32)).to(DEV).view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0

    def t(self, name):
        o, n = self.at[name]
        return self.buf[o:o + n]

    def host(self):
        return self.buf.view(torch.int32).cpu().numpy()

    def get(self, host, name):
        o, n = self.at[name]
        return host[o:o + n].view(np.float32).astype(np.float64)

    def guards_intact(self, host, written):
        mask = np.ones(self.size, dtype=bool)
        for name in written:
            o, n = self.at[name]
            mask[o:o + n] = False
        return bool(np.all(host[mask] == POISON))


def _head_inputs(B, C, T, kind, seed):
    """float32 (x, w, bias, labels or None).  x: unit normal with a tenth of its entries exactly zero (the `> 0` side of the slope).
    "sat+" / "sat-": the bias drives every logit to +-40 under mixed labels, so right and wrong labels both meet the saturated tail."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    x[rng.random((B, C, T)) < 0.1] = 0.0
    x.ravel()[0] = 0.0
    w = (0.5 * rng.standard_normal(C)).astype(np.float32)
    w[w == 0] = 0.25
    bias = np.array([{"sat+": 40.0, "sat-": -40.0}.get(kind, 0.1)], dtype=np.float32)
    labels = {"zeros": np.zeros(B), "ones": np.ones(B), "score": None}.get(kind, (np.arange(B) % 2 == 0).astype(np.float64))
    if kind in ("mixed", "sat+", "sat-") and B > 2:
        labels = rng.permutation(labels)
    return x, w, bias, None if labels is None else labels.astype(np.float32)


def _head_outputs(B, C, T):
    return _Guarded([("pred", B), ("amean", B * C), ("per", B), ("loss", 1), ("dx", B * C * T), ("dw", C), ("dbias", 1), ("dz", B)])


def _run_head(dev_in, B, C, T, gscale, backward=True, out=None):
    """One forward (and backward) through the raw ABI into poisoned buffers (fresh ones unless given); returns (_Guarded, names written)."""
    from spoofsv_amd import _lib
    x, w, bias, labels, gs = dev_in
    out = out if out is not None else _head_outputs(B, C, T)
    scoring = labels is None
    _lib.call("ssv_cm_head_fwd", _ptr(x), _ptr(w), _ptr(bias), _ptr(labels), R.SLOPE, _ptr(out.t("pred")), None if scoring else _ptr(out.t("amean")),
              None if scoring else _ptr(out.t("per")), None if scoring else _ptr(out.t("loss")), B, C, T, _stream())
    written = ["pred"] if scoring else ["pred", "amean", "per", "loss"]
    if backward and not scoring:
        _lib.call("ssv_cm_head_bwd", _ptr(x), _ptr(w), _ptr(bias), _ptr(labels), _ptr(out.t("amean")), _ptr(gs), R.SLOPE, _ptr(out.t("dx")),
                  _ptr(out.t("dw")), _ptr(out.t("dbias")), _ptr(out.t("dz")), B, C, T, _stream())
        written += ["dx", "dw", "dbias", "dz"]
    return out, written


# every value of each axis: B in {1, 3, 64, 130}, C in {1, 4, 8, 16}, T in {1, 2, 63, 64, 65, 257, 1031}
HEAD_SHAPES = [(1, 1, 1), (3, 4, 2), (64, 8, 63), (130, 16, 64), (3, 16, 65), (1, 8, 257), (3, 4, 1031), (64, 1, 65), (130, 8, 2)]
HEAD_KINDS = ("zeros", "ones", "mixed", "score", "sat+", "sat-")
HEAD_TOL = 2e-6          # 6e-8 x fewer than ten elementwise operations, plus a tree reduction of at most 1031 terms


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "B%d_C%d_T%d" % s)
def test_head_against_float64_in_guarded_buffers(shape):
    B, C, T = shape
    gscale = 0.37
    ok = True
    for kind in HEAD_KINDS:
        host_in = _head_inputs(B, C, T, kind, seed=B * 10000 + C * 100 + T)
        x, w, bias, labels = host_in
        dev_in = [None if a is None else torch.from_numpy(a.copy()).to(DEV) for a in host_in] + [torch.tensor([gscale], device=DEV)]
        out, written = _run_head(dev_in, B, C, T, gscale)
        torch.cuda.synchronize()
        host = out.host()
        what = "B=%d C=%d T=%d %s" % (B, C, T, kind)
        assert out.guards_intact(host, written), what + ": guard words or an output the call does not own were written"
        for a, d in zip(host_in, dev_in):
            assert a is None or np.array_equal(a.view(np.int32), d.view(torch.int32).cpu().numpy()), what + ": an input was written"
        ref = R.head_ref(x, w, bias, labels, R.SLOPE, gscale)
        if kind.startswith("sat"):
            assert np.all(np.abs(ref.z) > 30), what
        scal = lambda name, want: float(np.max(np.abs(out.get(host, name) - np.ravel(want)) / np.maximum(1.0, np.abs(np.ravel(want)))))
        ok &= _report("head", what + " pred", scal("pred", ref.pred), HEAD_TOL)
        if labels is None:
            continue
        for name, want in (("per", ref.per), ("loss", ref.loss), ("dw", ref.dw), ("dbias", ref.dbias)):
            ok &= _report("head", what + " " + name, scal(name, want), HEAD_TOL)
        dx = out.get(host, "dx").reshape(B, C, T)
        worst = max(float(np.linalg.norm(dx[b] - ref.dx[b]) / np.linalg.norm(ref.dx[b])) for b in range(B))
        ok &= _report("head", what + " dx, worst item rel_l2", worst, HEAD_TOL)
        again, _ = _run_head(dev_in, B, C, T, gscale)
        torch.cuda.synchronize()
        assert np.array_equal(again.host(), host), what + ": two runs differ"
    assert ok


def test_head_capture_and_two_replays_give_the_eager_values():
    from spoofsv_amd.train import _no_gc
    B, C, T = 5, 8, 65
    host_in = _head_inputs(B, C, T, "mixed", seed=77)
    dev_in = [torch.from_numpy(a.copy()).to(DEV) for a in host_in] + [torch.tensor([1.0], device=DEV)]
    eager, written = _run_head(dev_in, B, C, T, 1.0)
    torch.cuda.synchronize()
    want = eager.host()
    out = _head_outputs(B, C, T)                             # allocated and poisoned before the capture: an upload is not capturable
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc(), torch.cuda.graph(graph):
        _run_head(dev_in, B, C, T, 1.0, out=out)
    torch.cuda.synchronize()
    assert np.all(out.host() == POISON)                      # capturing runs nothing
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.host(), want), "replay %d differs from the eager run" % replay
        for name in written:
            out.t(name).view(torch.int32).fill_(POISON)


def test_cm_head_function_gradients_and_second_order_refusal():
    from spoofsv_amd import ops
    B, C, T = 3, 8, 9
    x, w, bias, labels = _head_inputs(B, C, T, "mixed", seed=5)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    wt = torch.from_numpy(w).view(1, C, 1).to(DEV).requires_grad_(True)
    bt = torch.from_numpy(bias).to(DEV).requires_grad_(True)
    loss, pred = ops.cm_head(xt, wt, bt, torch.from_numpy(labels).to(DEV))
    assert loss.shape == () and pred.shape == (B,) and not pred.requires_grad
    (3.0 * loss).backward()
    ref = R.head_ref(x, w, bias, labels, R.SLOPE, 3.0)
    rel = lambda got, want: float(np.abs(got.detach().cpu().numpy().astype(np.float64).ravel() - np.ravel(want)).max() / np.abs(want).max())
    assert wt.grad.shape == wt.shape and rel(xt.grad, ref.dx) < 1e-5 and rel(wt.grad, ref.dw) < 1e-5 and rel(bt.grad, ref.dbias) < 1e-5
    with torch.no_grad():
        scores = ops.cm_head(xt, wt, bt)
    assert torch.equal(scores, pred)
    loss2, _ = ops.cm_head(xt, wt, bt, torch.from_numpy(labels).to(DEV))
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(loss2, xt, create_graph=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.cm_head(torch.zeros(2, 4, 3), torch.zeros(1, 4, 1), torch.zeros(1))


# ================================================================================================ b. ssv_adam_ex_multi through the raw ABI
ROLES = 5                                           # p, g, m, v, vmax
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2049, 32768]
ALIGNS = [tuple((a >> r) & 1 for r in range(ROLES)) for a in range(1 << ROLES)]     # every combination of 0 / 1 float per pointer


class _Carved:
    """tests/test_gpu_optimizer_tail.py's carved table with a fifth role: one flat poisoned buffer per role, tensors behind guard words,
    the start of role r rounded up to 16 bytes and then moved by its 0 / 1 floats.  State for t > 1: vmax is v / 4 or 4 v element by
    element, so that both vmax < v' and vmax > v' occur in one table."""

    def __init__(self, specs, seed, t):
        self.specs = specs
        cur = [GUARD] * ROLES
        self.off = []
        for n, al in specs:
            o = []
            for r in range(ROLES):
                s = (cur[r] + GUARD + 3) // 4 * 4 + al[r]
                o.append(s)
                cur[r] = s + n
            self.off.append(o)
        self.size = (max(cur) + 2 * GUARD + 3) // 4 * 4
        rng = np.random.default_rng(seed)
        host = np.full((ROLES, self.size), POISON, dtype=np.int32).view(np.float32)
        self.mask = np.zeros((ROLES, self.size), dtype=bool)
        tot = sum(n for n, _ in specs)
        floor = lambda a: np.where(a == 0, 0.0, np.sign(a) * np.maximum(np.abs(a), 1e-15))
        scale = np.array([1e-12, 1e-6, 1.0, 1e4])[rng.integers(0, 4, tot)]
        p = floor(rng.standard_normal(tot))
        g = floor(rng.standard_normal(tot) * scale)
        g[rng.choice(tot, min(100, tot // 2), replace=False)] = 0.0
        if t > 1:
            m = floor(0.3 * rng.standard_normal(tot) * scale)
            v = np.maximum((rng.standard_normal(tot) * scale) ** 2, 1e-15)
            z = rng.choice(tot, min(50, tot // 2), replace=False)
            m[z] = 0.0
            v[z] = 0.0
            x = v * np.where(rng.random(tot) < 0.5, 0.25, 4.0)
        else:
            m, v, x = np.zeros(tot), np.zeros(tot), np.zeros(tot)
        at = 0
        for (n, _), o in zip(specs, self.off):
            for r, a in enumerate((p, g, m, v, x)):
                host[r, o[r]:o[r] + n] = a[at:at + n].astype(np.float32)
                self.mask[r, o[r]:o[r] + n] = True
            at += n
        self.before = host
        self.buf = torch.from_numpy(host.copy()).to(DEV)
        assert self.buf.data_ptr() % 16 == 0 and (self.size * 4) % 16 == 0

    def rows(self, null_vmax=False):
        base = [self.buf[r].data_ptr() for r in range(ROLES)]
        rows = [[base[r] + 4 * o[r] for r in range(ROLES)] + [n] for (n, _), o in zip(self.specs, self.off)]
        if null_vmax:
            for r in rows:
                r[4] = 0
        return rows

    def gather(self, host, r):
        return np.concatenate([host[r, o[r]:o[r] + n] for (n, _), o in zip(self.specs, self.off)])


def _launch_ex(rows, hp, wd, ams, step, step_dev):
    from spoofsv_amd import _lib
    assert ctypes.sizeof(_lib.AdamExChunk) == 48
    table = torch.from_numpy(np.array(rows, dtype=np.int64)).to(DEV)
    rc = _lib.lib().ssv_adam_ex_multi(_ptr(table), len(rows), *[float(v) for v in hp], float(wd), int(ams), step,
                                      None if step_dev is None else _ptr(step_dev), _stream())
    torch.cuda.synchronize()
    return rc


def _check_ex(c, before, hp, wd, ams, t, what, expect_both=False):
    """After a launch on ``c`` from the state ``before``: p, m, v, vmax inside their bounds; g, the guard words and (without amsgrad) vmax
    bitwise unchanged.  Returns the state after the launch."""
    after = c.buf.cpu().numpy()
    ref = R.adam_ex_step_ref(*[c.gather(before, r) for r in range(ROLES)], *hp, wd, ams, t)
    fr = R.adam_ex_fractions(c.gather(after, 0), c.gather(after, 2), c.gather(after, 3), c.gather(after, 4), ref, ams)
    ok = True
    for name, (f, i) in zip(("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"), fr):
        ok &= _report("adam", "%s %s (worst at element %d)" % (what, name, i), f, 1.0)
    assert ok
    a, b = after.view(np.int32), before.view(np.int32)
    assert np.array_equal(a[1], b[1]), what + ": the gradient buffer was written"
    if not ams:
        assert np.array_equal(a[4], b[4]), what + ": vmax was written without amsgrad"
    for r in (0, 2, 3, 4):
        assert np.array_equal(a[r][~c.mask[r]], b[r][~c.mask[r]]), "%s: guard words of role %d were written" % (what, r)
    if expect_both:
        x0 = c.gather(before, 4).astype(np.float64)
        assert np.any(x0 > ref.v) and np.any((x0 < ref.v) & (x0 > 0)), what + ": the table lacks vmax > v' or vmax < v'"
    return after


@pytest.mark.parametrize("ams", [True, False], ids=["amsgrad", "plain"])
@pytest.mark.parametrize("wd", [0.0, 1e-4], ids=["wd0", "wd1e-4"])
@pytest.mark.parametrize("hp", [R.REF_HP, R.TORCH_DEFAULT], ids=["reference", "torch_default"])
@pytest.mark.parametrize("t", [1, 2, 10, 100000])
def test_adam_ex_every_size_and_alignment_in_one_table(hp, t, wd, ams):
    """One chunk per (size, alignment of the five pointers): the sizes straddle the scalar tail, the single-vector loop and the
    two-in-flight loop; one misaligned pointer sends its chunk down the scalar path with the same result."""
    c = _Carved([(n, al) for n in SIZES for al in ALIGNS], seed=100 + t, t=t)
    rows = c.rows()
    assert len(rows) == len(SIZES) * 32
    assert _launch_ex(rows, hp, wd, ams, t, None) == 0
    _check_ex(c, c.before, hp, wd, ams, t, "lr=%g b2=%g t=%d wd=%g ams=%d" % (hp[0], hp[2], t, wd, ams), expect_both=ams and t > 1)


def test_adam_ex_plain_accepts_null_vmax_and_matches_adam_multi():
    """amsgrad = 0 never touches vmax: a table of NULL vmax pointers runs, and with weight_decay = 0 the result is ssv_adam_multi's, bit for bit."""
    from spoofsv_amd import _lib
    specs = [(n, al) for n in (5, 1025, 2049) for al in ((0, 0, 0, 0, 0), (0, 1, 0, 0, 0))]
    c = _Carved(specs, seed=9, t=7)
    assert _launch_ex(c.rows(null_vmax=True), R.REF_HP, 0.0, False, 7, None) == 0
    mine = _check_ex(c, c.before, R.REF_HP, 0.0, False, 7, "null vmax, plain")
    d = _Carved(specs, seed=9, t=7)
    table = torch.from_numpy(np.array([r[:4] + r[5:] for r in d.rows()], dtype=np.int64)).to(DEV)
    _lib.call("ssv_adam_multi", _ptr(table), len(specs), *[float(v) for v in R.REF_HP], 7, None, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d.buf.cpu().numpy().view(np.int32), mine.view(np.int32))


def test_adam_ex_step_source_and_captured_replay():
    """The device counter and the host step give the same bits; the counter advances once per call; a captured call replays as successive steps."""
    from spoofsv_amd.train import _no_gc
    specs = [(1025, (0, 0, 0, 0, 0)), (37, (1, 0, 0, 0, 1)), (2049, (0, 0, 0, 0, 0))]
    hp, wd = R.REF_HP, 1e-4
    a, b = _Carved(specs, seed=50, t=3), _Carved(specs, seed=50, t=3)
    step_dev = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    assert _launch_ex(a.rows(), hp, wd, True, 3, None) == 0
    assert _launch_ex(b.rows(), hp, wd, True, 1000, step_dev) == 0          # the host value is ignored
    assert int(step_dev.item()) == 3
    assert np.array_equal(a.buf.cpu().numpy().view(np.int32), b.buf.cpu().numpy().view(np.int32))
    state = _check_ex(b, b.before, hp, wd, True, 3, "step_dev, t=3")
    from spoofsv_amd import _lib
    table = torch.from_numpy(np.array(b.rows(), dtype=np.int64)).to(DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with _no_gc(), torch.cuda.graph(graph):
        _lib.call("ssv_adam_ex_multi", _ptr(table), len(specs), *[float(v) for v in hp], wd, 1, 0, _ptr(step_dev), _stream())
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 3
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert int(step_dev.item()) == 4 + replay
        state = _check_ex(b, state, hp, wd, True, 4 + replay, "captured, replay %d" % replay)
    c = _Carved(specs, seed=60, t=2)
    assert _launch_ex(c.rows(), hp, wd, True, 0, None) == -1               # no step at all
    assert np.array_equal(c.buf.cpu().numpy().view(np.int32), c.before.view(np.int32))


# ================================================================================================ c. FusedAdamEx
PARAM_SIZES = (33, 513, 32769, 40001)


def test_fused_adam_ex_six_steps_per_element():
    from spoofsv_amd.countermeasure import ADAM
    from spoofsv_amd.train import FusedAdamEx
    g = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in PARAM_SIZES]
    flat = torch.zeros(sum(PARAM_SIZES), device=DEV)
    at = 0
    for p in params:
        p.grad = flat[at:at + p.numel()].view_as(p)                    # consecutive unaligned views: the gradient arena's layout
        at += p.numel()
    opt = FusedAdamEx(params, **ADAM)
    hp = (ADAM["lr"],) + tuple(ADAM["betas"]) + (ADAM["eps"],)
    cat = lambda ts: np.concatenate([t.detach().cpu().numpy().ravel() for t in ts])
    n = flat.numel()
    state = [cat(params), np.zeros(n), np.zeros(n), np.zeros(n)]
    rng = np.random.default_rng(12)
    for t in range(1, 7):
        gr = rng.standard_normal(n) * np.array([1e-12, 1e-6, 1.0, 1e4])[rng.integers(0, 4, n)]
        gr[rng.choice(n, 100, replace=False)] = 0.0
        flat.copy_(torch.from_numpy(gr.astype(np.float32)))
        opt.step()
        ref = R.adam_ex_step_ref(state[0], flat.cpu().numpy(), state[1], state[2], state[3], *hp, ADAM["weight_decay"], True, t)
        state = [cat(params)] + [cat([opt.state[p][k] for p in params]) for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")]
        fr = R.adam_ex_fractions(*state, ref, True)
        ok = True
        for name, (f, i) in zip(("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"), fr):
            ok &= _report("fused", "FusedAdamEx step %d %s (worst at flat element %d)" % (t, name, i), f, 1.0)
        assert ok
    sd = opt.state_dict()
    assert [float(sd["state"][i]["step"]) for i in range(4)] == [6.0] * 4
    ta = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=0.1)
    ta.load_state_dict(sd)                                              # the reference's -R resume, the other way round
    assert ta.param_groups[0]["amsgrad"] is True and ta.param_groups[0]["weight_decay"] == 1e-4


# ================================================================================================ d. the small whole classifier
_ZERO_GRAD = ("conv1.bias", "conv2.bias", "conv3.bias", "conv4.bias", "hc.conv.bias")      # a bias feeding a LayerNorm: zero in exact arithmetic


@pytest.mark.parametrize("precision", MODES, indirect=True)
@pytest.mark.parametrize("train", [False, True], ids=["eval", "masks"])
@pytest.mark.parametrize("kind", ["mel", "lin"])
def test_small_whole_classifier_vs_float64(kind, train, precision):
    """CmMelDisc / CmLinDisc (24, 16) on (3, 24, 37): pred, loss and every parameter gradient against the float64 restatement, dropout off and
    with three injected masks.  The bars are those of test_small_whole_critic_vs_float64_oracle: max(2e-6, 16 e32) for the scalars and
    max(2e-5, 16 e32) for a gradient, e32 the error of the float32 stock-op run of the restatement (measured on that arm); bf16x3 1e-4 and
    2e-3.  The committed seeds keep every leaky-ReLU input of the float64 evaluation clear of its kink."""
    from spoofsv_amd import critic
    from spoofsv_amd.countermeasure import CmLinDisc, CmMelDisc
    sd, x, labels, masks = R.cm_case(kind)
    m = masks if train else False
    assert R.kink_margin(sd, kind, x, m) > R.KINK_MARGIN
    want, cpu32 = _cached((kind, train), lambda: (R.cm_reference(sd, kind, x, labels, m, torch.float64),
                                                 R.cm_reference(sd, kind, x, labels, m, torch.float32)))
    Fb, dim, B, T = R.CM_SHAPE
    disc = (CmLinDisc if kind == "lin" else CmMelDisc)(Fb, dim)
    disc.load_state_dict(sd)
    disc = disc.to(DEV).train(train)
    xd, yd = x.to(DEV), labels.to(DEV)
    if train:
        with critic.injected_dropout_masks([t.to(DEV) for t in masks]):
            loss, pred = disc.loss(xd, yd)
    else:
        loss, pred = disc.loss(xd, yd)
        with torch.no_grad():
            out = disc(xd)
        assert out.shape == (B, 1, 1) and torch.equal(out.view(-1), pred)        # the scoring form gives the training form's bits
    loss.backward()
    tag = "%s %s %s" % (kind, "masks" if train else "eval", precision)
    bf = precision == "bf16x3"
    ok = True
    e32 = float((cpu32[0] - want[0]).abs().max() / want[0].abs().max())
    err = float((pred.detach().double().cpu() - want[0]).abs().max() / want[0].abs().max())
    ok &= _report("whole", "%s pred (cpu32 %.2e)" % (tag, e32), err, 1e-4 if bf else max(2e-6, 16 * e32))
    e32 = abs(cpu32[1] - want[1]) / abs(want[1])
    ok &= _report("whole", "%s loss (cpu32 %.2e)" % (tag, e32), abs(float(loss) - want[1]) / abs(want[1]), 1e-4 if bf else max(2e-6, 16 * e32))
    rel_l2 = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())
    for n, p in disc.named_parameters():
        w = want[2][n]
        assert p.grad is not None and p.grad.shape == w.shape, n
        if n in _ZERO_GRAD:
            continue
        assert float(w.norm()) > 0, n
        e32 = rel_l2(cpu32[2][n], w)
        ok &= _report("whole", "%s grad %s (cpu32 %.2e)" % (tag, n, e32), rel_l2(p.grad.detach(), w), 2e-3 if bf else max(2e-5, 16 * e32))
    assert ok


# ================================================================================================ e. end to end
CFG = dict(json.load(open(os.path.join(ROOT, "config.json"))), DISC_DIM=16)
E2E_SEED, E2E_BATCH = 5, 8


def _check_score_file(path, source, model, feat_type, n):
    lines = open(path).read().splitlines()
    assert len(lines) == n
    idx = 0
    with torch.no_grad():
        for sp in source.batches(shuffle=False):
            feat = sp["data_0"] if feat_type == "mel" else sp["data_1"]
            pred = model(feat).view(-1).cpu().numpy()
            for k in range(pred.shape[0]):
                name, dash, gt, value = lines[idx].split(" ")
                assert name == "LA_D_%07d" % idx and dash == "-" and gt == ("bonafide" if sp["data_2"][k].item() == 1 else "spoof")
                assert np.float32(float(value)).view(np.int32) == pred[k].view(np.int32), (idx, value, pred[k])
                idx += 1
    assert idx == n


@pytest.mark.parametrize("case", ["lin_paths", "mel_spoof_device_22k"])
def test_train_resume_and_score_end_to_end(case, tmp_path):
    """24 one-second items at 16 kHz, two classes with disjoint spectra (bona fide 200..1400 Hz, spoof 4000..6400 Hz), B = 8.
    The float64 CPU restatement's trainer (tests/_countermeasure_ref.py: the same files, initial weights and batch order, dropout off)
    first reaches EER 0 after 5 iterations on the linear features of the wav files and after 9 on the mel features with the spoof class
    generated at 22.05 kHz and resampled (tests/test_countermeasure_cpu.py pins both counts); the device trainer takes twice as many
    optimizer steps, k = 10 and k = 18 (dropout active, half of them before a resume), and must then
    separate the classes: cm_eer == 0.  lin_paths: both classes from wav files; mel_spoof_device_22k: the spoof class as device
    waveforms at 22.05 kHz, the entry synthesized speech takes."""
    from spoofsv_amd import countermeasure as C
    feat, k = ("lin", 10) if case == "lin_paths" else ("mel", 18)
    bona, spoof_paths = R.write_toy_corpus(str(tmp_path))
    if case == "lin_paths":
        spoof = spoof_paths
    else:
        waves = np.stack([R.toy_wave(i, 0, 22050) for i in range(len(spoof_paths))])
        spoof = (torch.from_numpy(waves).to(DEV), torch.full((len(waves),), waves.shape[1], dtype=torch.int32, device=DEV), 22050)
    source = C.CmSource(CFG, bona, spoof, batch_size=E2E_BATCH, seed=0)
    assert len(source) == 24 and source.n_batches() == 3
    sp = next(iter(source.batches()))
    assert sp["data_0"].shape[:2] == (8, 80) and sp["data_1"].shape[:2] == (8, 513) and sp["data_1"].shape[2] == 4 * sp["data_0"].shape[2]
    assert sp["data_2"].tolist() == [1.0] * 8 and sp["data_0"].is_cuda
    save_dir = str(tmp_path / "ckpt")
    half = k // 2
    torch.manual_seed(E2E_SEED)
    first = C.train(CFG, source, feat, save_dir=save_dir, save_interval=half - 1, max_iterations=half, log=lambda *a: None)
    # saved when global_iteration % save_interval == 0 and > 0: at global_iteration = half - 1, after the half-th step
    path = os.path.join(save_dir, "%d_iteration.tar.pth" % half)
    assert first["checkpoints"] == [path] and first["global_iteration"] == half and len(first["losses"]) == half
    ckpt = torch.load(path, map_location="cpu")
    assert set(ckpt) == {"epoch", "global_iteration", "model_state_dict", "optimizer_state_dict"}
    assert ckpt["global_iteration"] == half - 1 and ckpt["epoch"] == first["epoch"] + 1
    assert ckpt["optimizer_state_dict"]["param_groups"][0]["amsgrad"] is True
    assert "max_exp_avg_sq" in ckpt["optimizer_state_dict"]["state"][0]
    # the reference resumes AT the stored global_iteration (it saves before incrementing): k - half more steps make k in all and end at
    # global_iteration = k - 1, the last of them (index k - 2) being the one that saves
    second = C.train(CFG, source, feat, save_dir=save_dir, resume=path, save_interval=k - 2, max_iterations=k - half, log=lambda *a: None)
    assert second["global_iteration"] == k - 1
    final = os.path.join(save_dir, "%d_iteration.tar.pth" % (k - 1))
    assert second["checkpoints"] == [final]
    assert int(second["optimizer"].state_dict()["state"][0]["step"]) == k
    out = str(tmp_path / "cm_scores" / "scores_t.txt")
    eer = C.score(CFG, source, final, out, feat)
    model = C.load_model(CFG, final, feat, DEV)
    assert not model.training
    _check_score_file(out, source, model, feat, 24)
    print("%s: losses %s ... %s, EER %.3f" % (case, ["%.3f" % v for v in first["losses"][:3]], ["%.3f" % v for v in second["losses"][-3:]], eer))
    assert eer == 0.0
