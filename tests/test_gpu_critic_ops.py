"""The twice-differentiable operators of the WGAN-GP critics against float64, per operator, at the smallest shapes that reach each
kernel variant (references and case tables: tests/_critic_ref.py, pinned by tests/test_critic_ref_cpu.py):

  A  ops.conv1d_dd to second order on the split-MFMA kernels, with the operand scale lists routed between its three Functions;
  B  ops.channel_ln_dd / ops.highway_gate_dd to second order: low variance, batch-strided operands, one cotangent, input_grads_only;
  C  the glue kernels of csrc/critic.hip: the dropout mask bit for bit, the gradient penalty across its chunk and round boundaries,
     the pools and their adjoints, and a convolution fed from a scale list that act_dropout passed on;
  D  one small whole critic (penalty, Wasserstein term, every parameter gradient), eval and with injected masks.

No bar is measured on the code under test: the convolution bars are the ones tests/test_gpu_accuracy.py holds the same kernels to, the
LayerNorm / gate and whole-critic bars are multiples of what torch's float32 CPU autograd loses on the same inputs (computed here), the
glue bars follow from float32 rounding.  Every case prints its error next to its bar; the worst per part and mode are printed at the end
(recorded in profiles/critic_ops_accuracy.txt).  Run with `-m gpu -s` on an MI355X."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _critic_ref as R
from test_gpu_parity import TOLS, _CRITIC_ZERO_GRAD, _critic_d_loss_hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = R.U32
CONV_BAR = 2e-6                 # fp32 and f16x2, relative L2 (tests/test_gpu_accuracy.py: the same kernels at larger shapes)
LN_BAR = 3e-6                   # LayerNorm / gate, forward and first order (tests/test_gpu_accuracy.py)
_WORST = {}


def _report(part, mode, what, err, bar):
    print("%-4s %-6s %-58s err %.3e  bar %.3e" % (part, mode, what, err, bar))
    key = (part, mode)
    if err / bar > _WORST.get(key, (0.0, 0.0, 0.0, ""))[0]:
        _WORST[key] = (err / bar, err, bar, what)
    return err <= bar


@pytest.fixture(scope="module", autouse=True)
def _worst_per_part_and_mode():
    yield
    print()
    for (part, mode), (_, err, bar, what) in sorted(_WORST.items()):
        print("WORST %-4s %-6s err %.3e  bar %.3e  (%s)" % (part, mode, err, bar, what))


def _set_mode(mode):
    import spoofsv_amd
    return spoofsv_amd.set_precision(mode)


@pytest.fixture(params=["fp32", "f16x2", "bf16x3"])
def precision(request):
    prev = _set_mode(request.param)
    yield request.param
    _set_mode(prev)


@pytest.fixture(params=["fp32", "f16x2"])
def ln_precision(request):
    prev = _set_mode(request.param)
    yield request.param
    _set_mode(prev)


_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ------------------------------------------------------------------------------------------- A
def _conv_case_on_device(shape, kind):
    """(float64 reference, HIP result) of the second-order functional for one row of the table."""
    from spoofsv_amd import ops
    k, d, causal = shape[4:]
    operands = R.conv_operands(shape, kind)
    want = _cached(("conv", shape, kind), lambda: R.conv_second_order(R.conv64, [t.double() for t in operands], k, d, causal))
    got = R.conv_second_order(ops.conv1d_dd, [t.to(DEV) for t in operands], k, d, causal)
    torch.cuda.synchronize()
    return want, got


@pytest.mark.parametrize("shape,kind", R.CONV_CASES, ids=["%s-%s" % ("x".join(str(int(v)) for v in s), k) for s, k in R.CONV_CASES])
def test_conv1d_dd_to_second_order_vs_float64(shape, kind, precision):
    """y, the three first-order gradients and the three gradients of <vx, gx> + <vw, gw>: single products or sums of two, no
    cancellation, so each is held to the bar of one product.  Between them they take every branch of the backwards of ConvFwdDD,
    ConvBwdDataDD and ConvBwdWeightDD, each of which hands a saved or a fresh scale list to the other two."""
    want, got = _conv_case_on_device(shape, kind)
    fwd_bar, bwd_bar = (CONV_BAR, CONV_BAR) if precision != "bf16x3" else TOLS["bf16x3"]
    ok = True
    for n in R.CONV_NAMES:
        assert got[n].shape == want[n].shape and bool(torch.isfinite(got[n]).all()), n
        err = R.worst_rel_l2(got[n], want[n], n in R.CONV_PER_ITEM)
        ok &= _report("A", precision, "%s %s %s" % (shape, kind, n), err, fwd_bar if n == "y" else bwd_bar)
    assert ok


# ------------------------------------------------------------------------------------------- B
def _leaves(ts, strided=()):
    """float32 device leaves of the float64 CPU tensors ``ts``; those indexed by ``strided`` as channel slices of a tensor twice as wide
    (stride(0) = 2 C L, rows contiguous: ops._act3 passes them on without a copy)."""
    out = []
    for i, t in enumerate(ts):
        if t is None:
            out.append(None)
            continue
        t = t.detach().float().to(DEV)
        if i in strided:
            wide = torch.randn(t.shape[0], 2 * t.shape[1], t.shape[2], device=DEV)
            wide[:, t.shape[1]:] = t
            t = wide[:, t.shape[1]:].detach()
            assert t.stride(0) == 2 * t.shape[1] * t.shape[2] and t.stride(1) == t.shape[2]
        out.append(t.requires_grad_(True))
    return out


def _cpu_pair(run, ts):
    """``run`` on the float64 operands and on their float32 roundings (torch's CPU autograd): (float64 results, float32 results)."""
    as_leaves = lambda dt: [None if t is None else t.to(dt).requires_grad_(True) for t in ts]
    return run(*as_leaves(torch.float64)), run(*as_leaves(torch.float32))


def _check_b(part, mode, tag, names1, names2, want, cpu32, got):
    ok = True
    for n, w, g in zip(names1, want[0], got[0]):
        ok &= _report(part, mode, "%s %s" % (tag, n), R.rel_l2(g, w), LN_BAR)
    for n, w, c, g in zip(names2, want[1], cpu32[1], got[1]):
        if w is None:          # the contraction does not depend on this argument: every term of the kernel's sum is a product with an exact 0
            assert c is None and g is not None and int(torch.count_nonzero(g)) == 0, (tag, n)
            continue
        e32 = R.rel_l2(c, w)
        ok &= _report(part, mode, "%s %s (cpu32 %.2e)" % (tag, n, e32), R.rel_l2(g, w), max(LN_BAR, 8 * e32))
    assert ok, tag


@pytest.mark.parametrize("kind", list(R.LN_KINDS))
@pytest.mark.parametrize("B,C,L", R.LN_SHAPES)
def test_channel_ln_dd_to_second_order_vs_float64(B, C, L, kind, ln_precision):
    from spoofsv_amd import ops
    ts = [t.float().double() for t in R.ln_operands((B, C, L), kind)]        # the reference sees exactly the float32 values the kernel gets
    run = lambda ln: (lambda x, g, b, gy, v: R.ln_second_order(ln, x, g, b, gy, v))
    want, cpu32 = _cached(("ln", B, C, L, kind), lambda: _cpu_pair(run(R.ln_ref), ts))
    got = run(ops.channel_ln_dd)(*_leaves(ts, strided=(0, 3, 4) if kind == "strided" else ()))
    torch.cuda.synchronize()
    _check_b("B-ln", ln_precision, "(%d, %d, %d) %s" % (B, C, L, kind), ("y", "gx", "ggamma", "gbeta"), ("d_gy", "d_x", "d_gamma"), want, cpu32, got)


@pytest.mark.parametrize("kind", list(R.LN_KINDS) + ["vh_only", "vx_only"])
@pytest.mark.parametrize("B,C,L", R.GATE_SHAPES)
def test_highway_gate_dd_to_second_order_vs_float64(B, C, L, kind, ln_precision):
    from spoofsv_amd import ops
    ts = [t.float().double() for t in R.gate_operands((B, C, L), kind if kind in R.LN_KINDS else "unit")]
    if kind == "vh_only":
        ts[8] = None
    if kind == "vx_only":
        ts[7] = None
    run = lambda gate: (lambda *a: R.gate_second_order(gate, *a))
    want, cpu32 = _cached(("gate", B, C, L, kind), lambda: _cpu_pair(run(R.gate_ref), ts))
    got = run(ops.highway_gate_dd)(*_leaves(ts, strided=(1, 6, 8) if kind == "strided" else ()))
    torch.cuda.synchronize()
    _check_b("B-gate", ln_precision, "(%d, %d, %d) %s" % (B, C, L, kind), ("y", "gh", "gx", "gg1", "gb1", "gg2", "gb2"),
             ("d_h", "d_x", "d_g1", "d_b1", "d_g2", "d_b2", "d_gy"), want, cpu32, got)


class _GateParams(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.ln1, self.ln2 = torch.nn.LayerNorm(C), torch.nn.LayerNorm(C)


def _randomise(mod, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=gen))
    return mod.to(DEV)


@pytest.mark.parametrize("B,C,L", [(2, 64, 41), (2, 33, 17)])
def test_first_pass_inside_input_grads_only_gives_bitwise_equal_second_order_results(B, C, L, ln_precision):
    """The penalty's first pass runs inside ops.input_grads_only(critic): the first-order backward then skips its parameter-gradient
    reductions.  The second pass must not notice: bitwise-equal results, parameter gradients included."""
    from spoofsv_amd import ops
    x, _, _, gy, v = [t.float().to(DEV) for t in R.ln_operands((B, C, L), "unit")]
    ln = _randomise(torch.nn.LayerNorm(C), 3)

    def ln_pass(inside):
        xs, gys = x.clone().requires_grad_(True), gy.clone().requires_grad_(True)
        with (ops.input_grads_only(ln) if inside else contextlib.nullcontext()):
            (gx,) = torch.autograd.grad(ops.channel_ln_dd(xs, ln.weight, ln.bias), xs, gys, create_graph=True)
        return (gx.detach(),) + torch.autograd.grad(gx, (gys, xs, ln.weight), v)
    for a, b in zip(ln_pass(True), ln_pass(False)):
        assert a is not None and b is not None and torch.equal(a, b)

    h, xg, _, _, _, _, gyg, vh, vx = [t.float().to(DEV) for t in R.gate_operands((B, C, L), "unit")]
    gate = _randomise(_GateParams(C), 4)
    params = (gate.ln1.weight, gate.ln1.bias, gate.ln2.weight, gate.ln2.bias)

    def gate_pass(inside):
        hs, xs, gys = [t.clone().requires_grad_(True) for t in (h, xg, gyg)]
        with (ops.input_grads_only(gate) if inside else contextlib.nullcontext()):
            gh, gx = torch.autograd.grad(ops.highway_gate_dd(hs, xs, *params), (hs, xs), gys, create_graph=True)
        return (gh.detach(), gx.detach()) + torch.autograd.grad((gh, gx), (gys, hs, xs) + params, (vh, vx))
    for a, b in zip(gate_pass(True), gate_pass(False)):
        assert a is not None and b is not None and torch.equal(a, b)
    # and the block really changes the first pass: outside it the skipped gradients exist, inside they are not produced
    xs = x.clone().requires_grad_(True)
    with ops.input_grads_only(ln):
        inside = torch.autograd.grad(ops.channel_ln_dd(xs, ln.weight, ln.bias), (xs, ln.weight), gy, allow_unused=True)
    outside = torch.autograd.grad(ops.channel_ln_dd(xs, ln.weight, ln.bias), (xs, ln.weight), gy, allow_unused=True)
    assert inside[1] is None and outside[1] is not None and torch.equal(inside[0], outside[0])


def test_second_order_over_257_channels_raises_and_leaves_the_device_usable():
    """The second-order kernels stop at 256 channels.  C = 257 runs forward and first-order backward (the generator's kernels); its
    second-order backward raises the library's error as a Python exception, and the next call works."""
    from spoofsv_amd import ops
    B, C, L = 2, 257, 19
    ts = [t.float() for t in R.ln_operands((B, C, L), "unit")]
    x, g, b, gy, v = _leaves(ts)
    y = ops.channel_ln_dd(x, g, b)
    gx, gg, gb = torch.autograd.grad(y, (x, g, b), gy, create_graph=True)
    want = R.ln_second_order(R.ln_ref, *[t.double().requires_grad_(True) for t in ts])[0]
    for n, w, a in zip(("y", "gx", "ggamma", "gbeta"), want, (y, gx, gg, gb)):
        assert R.rel_l2(a, w) <= LN_BAR, n
    with pytest.raises(RuntimeError, match=r"not supported \(max 256\)"):
        torch.autograd.grad(gx, (gy, x, g), v)
    tg = [t.float() for t in R.gate_operands((B, C, L), "unit")]
    h, xg, g1, b1, g2, b2, gyg, vh, vx = _leaves(tg)
    gh, gxg = torch.autograd.grad(ops.highway_gate_dd(h, xg, g1, b1, g2, b2), (h, xg), gyg, create_graph=True)
    with pytest.raises(RuntimeError, match=r"not supported \(max 256\)"):
        torch.autograd.grad((gh, gxg), (gyg, h, xg), (vh, vx))
    torch.cuda.synchronize()
    ts = [t.float().double() for t in R.ln_operands((2, 16, 20), "unit")]
    want = R.ln_second_order(R.ln_ref, *[t.requires_grad_(True) for t in ts])
    got = R.ln_second_order(ops.channel_ln_dd, *_leaves(ts))
    torch.cuda.synchronize()
    for w, a in zip(want[0] + want[1], got[0] + got[1]):
        assert R.rel_l2(a, w) <= 1e-5


# ------------------------------------------------------------------------------------------- C: dropout
def _act_dropout(x, y, d, n, slope, p, ctr, seed):
    from spoofsv_amd import _lib, ops
    _lib.call("ssv_act_dropout_fwd", x.data_ptr(), y.data_ptr(), d.data_ptr(), n, float(slope), float(p), None if ctr is None else ctr.data_ptr(),
              seed, ops._stream())


SEED = 0x9E3779B1


@pytest.mark.parametrize("slope", [1.0, 0.05])
@pytest.mark.parametrize("p", [0.05, 0.25])
def test_dropout_mask_is_the_predicted_philox_stream_bit_for_bit(p, slope):
    """d and y of ssv_act_dropout_fwd against the numpy Philox4x32-10 of tests/_critic_ref.py: whole groups of four and every ragged tail,
    16-byte aligned pointers (one 16-byte access per group) and pointers offset by one float (the scalar path), more than one workgroup,
    and a call counter with a non-zero high word.  Sentinels around the outputs stay untouched."""
    gen = torch.Generator().manual_seed(1)
    for n in (4100, 4101, 4102, 4103, 3):
        for off in (0, 1):
            for call in (0, (1 << 32) + 5):
                xb = torch.randn(n + off + 4, generator=gen).to(DEV)
                yb, db = torch.full_like(xb, 7.0), torch.full_like(xb, 7.0)
                ctr = torch.tensor([call], dtype=torch.int64, device=DEV)
                x, y, d = xb[off:], yb[off:], db[off:]
                assert x.data_ptr() % 16 == 4 * off
                _act_dropout(x, y, d, n, slope, p, ctr, SEED)
                want_d, want_y = R.act_dropout_ref(xb[off:off + n].cpu().numpy(), slope, p, SEED, call)
                assert np.array_equal(db[off:off + n].cpu().numpy(), want_d), (n, off, call)
                assert np.array_equal(yb[off:off + n].cpu().numpy(), want_y), (n, off, call)
                assert bool((yb[:off] == 7).all() and (yb[off + n:] == 7).all() and (db[:off] == 7).all() and (db[off + n:] == 7).all())
                assert int(ctr) == call + 1                                  # exactly one step per call with p > 0
                assert 0 < int((want_d == 0).sum()) < n or n == 3


def test_dropout_counter_steps_once_per_call_and_per_graph_replay_and_not_at_all_without_dropout():
    n = 4101
    x = torch.randn(n, generator=torch.Generator().manual_seed(2)).to(DEV)
    y, d = torch.empty_like(x), torch.empty_like(x)
    ctr = torch.tensor([41], dtype=torch.int64, device=DEV)
    _act_dropout(x, y, d, n, 0.05, 0.0, ctr, SEED)
    assert int(ctr) == 41                                                    # p = 0: no mask drawn, the counter does not move
    want_d, want_y = R.act_dropout_ref(x.cpu().numpy(), 0.05, 0.0, SEED, 41)
    assert np.array_equal(d.cpu().numpy(), want_d) and np.array_equal(y.cpu().numpy(), want_y)
    _act_dropout(x, y, d, n, 0.05, 0.0, None, SEED)                          # ... and none is needed
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _act_dropout(x, y, d, n, 0.05, 0.25, ctr, SEED)
    torch.cuda.current_stream().wait_stream(s)
    assert int(ctr) == 42
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _act_dropout(x, y, d, n, 0.05, 0.25, ctr, SEED)
    assert int(ctr) == 42                                                    # capturing runs nothing
    for call in (42, 43, 44):
        g.replay()
        torch.cuda.synchronize()
        want_d, want_y = R.act_dropout_ref(x.cpu().numpy(), 0.05, 0.25, SEED, call)
        assert int(ctr) == call + 1
        assert np.array_equal(d.cpu().numpy(), want_d) and np.array_equal(y.cpu().numpy(), want_y), call


@pytest.mark.parametrize("p", [0.05, 0.25])
def test_dropout_fraction_over_a_million_elements_is_within_four_standard_deviations(p):
    """The number of drops among n = 10^6 elements is binomial(n, q), q = uint32(p 2^32) / 2^32: within 4 sqrt(n q (1 - q)) of n q (a
    fair generator misses that once in 16,000 seeds; the seed is fixed).  The ops-level call draws from the process-wide counter."""
    from spoofsv_amd import ops
    n = 1000000
    q = R.dropout_threshold(p) / 2.0 ** 32
    x = torch.ones(n, device=DEV)
    y, d = torch.empty_like(x), torch.empty_like(x)
    ctr = torch.tensor([7], dtype=torch.int64, device=DEV)
    _act_dropout(x, y, d, n, 1.0, p, ctr, SEED)
    drops = int((d == 0).sum())
    bar = 4 * (n * q * (1 - q)) ** 0.5
    print("C-dropout p %.2f: %d drops of %d, expected %.0f +- %.0f" % (p, drops, n, n * q, bar))
    assert abs(drops - n * q) <= bar
    assert drops == int(R.dropout_drops(n, p, SEED, 7).sum()) and torch.equal(y, d)
    key = (x.device.type, x.device.index)
    y1 = ops.act_dropout(x, 1.0, p)
    c1 = int(ops._DROP_CTR[key])
    y2 = ops.act_dropout(x, 1.0, p)
    assert int(ops._DROP_CTR[key]) == c1 + 1 and not torch.equal(y1, y2)
    for t in (y1, y2):
        assert abs(int((t == 0).sum()) - n * q) <= bar


# ------------------------------------------------------------------------------------------- C: penalty, pool
@pytest.mark.parametrize("B,n", R.GP_SHAPES)
def test_grad_penalty_value_and_gradient_vs_float64(B, n):
    from spoofsv_amd import ops
    g = R.gp_operand(B, n)
    want_loss, want_dg = R.gp_ref(g, 10.0)
    bar = R.gp_bound(g, n)
    runs = []
    for _ in range(2):
        gd = g.to(DEV).requires_grad_(True)
        loss = ops.grad_penalty(gd, 10.0)
        (dg,) = torch.autograd.grad(loss, gd)
        runs.append((loss.detach().clone(), dg))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])        # fixed summation order
    loss, dg = runs[0]
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dg).all())
    ok = _report("C-gp", "-", "(%d, %d) loss" % (B, n), abs(float(loss) - float(want_loss)) / float(want_loss), bar)
    for b in range(B):
        if float(want_dg[b].abs().max()) == 0.0:          # the all-zero item and the item of norm exactly 1
            assert int(torch.count_nonzero(dg[b])) == 0, b
        else:
            ok &= _report("C-gp", "-", "(%d, %d) gradient of item %d" % (B, n, b), R.rel_l2(dg[b], want_dg[b]), bar)
    if B >= 3 and n >= 8:          # item 0: gradient exactly zero, loss term lam; item 1: norm exactly 1, loss term 0
        rest = g[2:].to(DEV)
        alone = float(ops.grad_penalty(rest, 10.0).detach()) * (B - 2)
        assert abs(float(loss) * B - (10.0 + alone)) <= 24 * U32 * float(loss) * B          # (two wave reductions and divisions of a few roundings each)
    assert ok


@pytest.mark.parametrize("B,C,L,k", R.POOL_SHAPES)
def test_avg_pool_its_adjoint_and_the_adjoints_adjoint_vs_float64(B, C, L, k):
    """Element-wise against float64 within the float32 rounding of the kernel's own arithmetic: k - 1 additions in sequence and one
    division for the pool, one division for its adjoint; the columns of a dropped tail get exactly 0."""
    from spoofsv_amd import ops
    gen = torch.Generator().manual_seed(L * 10 + k)
    x, v, w = torch.randn(B, C, L, generator=gen), torch.randn(B, C, L // k, generator=gen), torch.randn(B, C, L, generator=gen)
    xd, vd = x.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    y = ops.avg_pool1d(xd, k)
    (gx,) = torch.autograd.grad(y, xd, vd, create_graph=True)
    (gv,) = torch.autograd.grad(gx, vd, w.to(DEV))
    torch.cuda.synchronize()

    def pool_ok(got, src, what):
        want = F.avg_pool1d(src.double(), k)
        bound = 1.01 * ((k - 1) * U32 * F.avg_pool1d(src.double().abs(), k) + U32 * want.abs()) + 1e-38
        err = (got.detach().double().cpu() - want).abs()
        _report("C-pool", "-", "(%d, %d, %d, %d) %s, worst element's share of its bound" % (B, C, L, k, what), float((err / bound).max()), 1.0)
        return got.shape == want.shape and bool((err <= bound).all())
    assert pool_ok(y, x, "forward")
    want = torch.zeros(B, C, L, dtype=torch.float64)
    want[:, :, :L // k * k] = (v.double() / k).repeat_interleave(k, dim=2)
    err = (gx.detach().double().cpu() - want).abs()
    assert gx.shape == want.shape and bool((err <= 1.01 * U32 * want.abs()).all()) and int(torch.count_nonzero(gx[:, :, L // k * k:])) == 0
    assert pool_ok(gv, w, "adjoint's adjoint")


def test_convolution_fed_from_a_scale_list_inherited_through_act_dropout():
    """ops.act_dropout passes its input's split-fp16 scale list on to its output: the keep factor 1 / (1 - p) <= 4/3 must fit the headroom
    of the scale.  The worst case for that argument: a LayerNorm output (gamma = 1, beta = 0) whose entries ALL sit at the item's maximum
    magnitude, so every kept entry of the dropout output exceeds the maximum the inherited list states by 4/3."""
    import spoofsv_amd
    from spoofsv_amd import ops
    B, C, L, Cout = 2, 128, 131, 64
    prev = spoofsv_amd.set_precision("f16x2")
    try:
        gen = torch.Generator().manual_seed(21)
        order = torch.rand(B, C, L, generator=gen).argsort(dim=1)
        x0 = torch.where(order < C // 2, 1.0, -1.0)                              # per column: half the channels +1, half -1
        x = ops.channel_ln_dd(x0.to(DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV))
        assert float(x.abs().min()) > 0.999 * float(x.abs().max())
        y = ops.act_dropout(x, 1.0, 0.25)
        tag = getattr(x, "_ssv_amax", None)
        assert tag is not None and y._ssv_amax[0] is tag[0] and ops.amax_of(y) is tag[0]      # else this test does not test what it says
        assert float(y.abs().max()) > 1.33 * float(tag[0].max())
        w = torch.randn(Cout, C, 1, generator=gen) * 0.05
        z = ops.conv1d_dd(y, w.to(DEV))
        fresh = y.clone()
        assert getattr(fresh, "_ssv_amax", None) is None
        z_fresh = ops.conv1d_dd(fresh, w.to(DEV))
        torch.cuda.synchronize()
        want = F.conv1d(y.double().cpu(), w.double())
        e, e_fresh = R.rel_l2(z, want), R.rel_l2(z_fresh, want)
        ok = _report("C-inh", "f16x2", "inherited list, worst item (whole: inherited %.2e, fresh %.2e)" % (e, e_fresh), R.worst_rel_l2(z, want, True), CONV_BAR)
        ok &= _report("C-inh", "f16x2", "fresh list, worst item", R.worst_rel_l2(z_fresh, want, True), CONV_BAR)
        assert ok and bool(torch.isfinite(z).all())
        assert e <= 2 * e_fresh and e_fresh <= 2 * e, (e, e_fresh)
    finally:
        spoofsv_amd.set_precision(prev)


# ------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("kind", ["mel", "lin"])
def test_small_whole_critic_vs_float64_oracle(kind, train, precision):
    """melDisc(80, 32) on (4, 80, 40) and linDisc(65, 32) on (3, 65, 64): penalty, Wasserstein term and every parameter gradient of one
    critic iteration against oracle/critic_oracle.critic_losses evaluated in float64 (with the same nine masks in train mode).  The bars
    are multiples of what the float32 oracle loses on the same inputs; no element is excluded: the committed seeds keep every
    leaky-ReLU input of the float64 evaluation clear of its kink."""
    from spoofsv_amd.critic import linDisc, melDisc
    sd, real, fake, eps, masks = R.critic_case(kind)
    m = masks if train else False
    assert R.critic_kink_margins(sd, kind, real, fake, eps, m) > R.KINK_MARGIN
    want, cpu32 = _cached(("critic", kind, train), lambda: (R.critic_reference(sd, kind, real, fake, eps, m, torch.float64),
                                                           R.critic_reference(sd, kind, real, fake, eps, m, torch.float32)))
    Fb, dim, _ = R.CRITIC_CASES[kind]
    disc = (linDisc if kind == "lin" else melDisc)(Fb, dim)
    disc.load_state_dict(sd)
    disc = disc.to(DEV).train(train)
    got = _critic_d_loss_hip(disc, real, fake, eps, masks=masks if train else None)
    tag = "%s %s" % (kind, "train" if train else "eval")
    ok = True
    for i, n in enumerate(("penalty", "wasserstein")):
        e32 = abs(cpu32[i] - want[i]) / abs(want[i])
        bar = max(2e-6, 16 * e32) if precision != "bf16x3" else 1e-4 * max(1.0, abs(want[i])) / abs(want[i])
        ok &= _report("D", precision, "%s %s (cpu32 %.2e)" % (tag, n, e32), abs(got[i] - want[i]) / abs(want[i]), bar)
    for n, w in want[2].items():
        if n in _CRITIC_ZERO_GRAD:          # a bias in front of a LayerNorm: exactly zero in exact arithmetic
            continue
        if float(w.norm()) == 0.0:
            # exactly zero in float64 (conv5.bias: the penalty does not depend on it and the two halves of the Wasserstein term are
            # +1 and -1; ln4.bias when real and fake take the same sides of the last kink): no relative error exists, so the bar
            # applies to the absolute error, against halves of magnitude 1 or less
            ok &= _report("D", precision, "%s %s (zero in float64; absolute)" % (tag, n), float(got[2][n].double().norm()), 2e-5 if precision != "bf16x3" else 2e-3)
            continue
        e32 = R.rel_l2(cpu32[2][n], w)
        bar = max(2e-5, 16 * e32) if precision != "bf16x3" else 2e-3
        ok &= _report("D", precision, "%s %s (cpu32 %.2e)" % (tag, n, e32), R.rel_l2(got[2][n], w), bar)
    assert ok
