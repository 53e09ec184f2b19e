"""The three narrow column-step kernels that only one single-shape test reached -- column_matvec_kernel, column_ln_act_kernel,
column_gate_kernel (csrc/synth.hip) -- called alone through the C ABI and held to tests/_column_step_ref.py in float64, at every edge
of their index rules: K = C k around the lane stride of 8 quads and around the 192 prefetched quads (K = 768 exactly, one quad into
the tail loop, the cap 1536), M around the row group of 4, B around the item group of 8, every NULL / given combination of the two
bias terms, padded batch strides, k = 3 stepped over every frame at dilations 1, 3, 9, and 1 .. 4 live channels per thread in the
LayerNorm and the gate.  The rows and why each is there: MATVEC_CASES, LN_CASES of the reference module.

Bars.  matvec: |got - want| <= (K + 4) 2^-24 S per element, S the sum of the absolute terms -- the rounding bound of a length-K float32
dot product in any order with fused multiply-adds plus two bias additions, derived and not tuned; a position probe (one-hot inputs,
distinct integer weights) holds every index to the bit.  LayerNorm / gate: 1e-5 in rel_err, the bar of the earlier test, and the same
1e-5 per item against the item's own maximum; inputs of mean 100 are held to the larger of 1e-5 and four times what torch's float32
layer_norm loses on them.  Figures: profiles/column_step_accuracy.txt (`pytest -m gpu -s`)."""
import ctypes

import numpy as np
import pytest
import torch

import _column_step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0                  # what the tests fill outputs, histories, stride padding and guard zones with: finite, and no kernel writes it
PAD = 64                     # floats of guard zone on either side of a guarded buffer


def P(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def _st():
    from spoofsv_amd import ops
    return ops._stream()


def _call(name, *args):
    from spoofsv_amd import _lib
    _lib.call(name, *args)


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _guarded(shape, fill=SENT):
    """A float tensor of ``shape`` inside a larger allocation the test owns, everything filled with ``fill``: (whole allocation, view)."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * PAD,), fill, dtype=torch.float32, device=DEV)
    return big, big[PAD:PAD + n].view(shape)


def _matvec(w, bias, bias_b, bb_bs, cur, cur_bs, hist, hist_bs, Tmax, tdev, dil, out, out_bs, B, C, M, k):
    _call("ssv_column_matvec", P(w), P(bias), P(bias_b), bb_bs, P(cur), cur_bs, P(hist), hist_bs, Tmax, P(tdev), dil, P(out), out_bs,
          B, C, M, k, _st())


def _check_bound(got, want, S, K, what):
    """Element by element against the rounding bound; returns the worst fraction of it."""
    err, bound = np.abs(got.astype(np.float64) - want), R.matvec_bound(K, S)
    assert (bound > 0).all()
    frac = err / bound
    assert (err <= bound).all(), (what, "worst fraction of the bound %.3f at %s" % (float(frac.max()), np.unravel_index(frac.argmax(), frac.shape)))
    return float(frac.max())


# ---- ssv_column_matvec ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.MATVEC_CASES, ids=lambda c: c.name)
def test_matvec_vs_float64_per_element_and_neighbours_untouched(case):
    """One row of MATVEC_CASES, every frame of it (k = 1: one call).  Per call: out within the rounding bound element by element; the
    stride padding of out and the guard zones around it bitwise the sentinel they were filled with; the history, its stride padding
    and guard zones included, bitwise what it was except column t, which holds cur; after the last frame the history is the inputs."""
    B, C, M, k, Tmax, K = case.B, case.C, case.M, case.k, case.Tmax, case.C * case.k
    cur_bs, out_bs, bb_bs, hist_bs = R.matvec_strides(case)
    w, bias, bias_b, x = R.matvec_inputs(case)
    want, S = R.matvec_reference(case, w, bias, bias_b, x)
    wd, biasd, X = _dev(w), _dev(bias), _dev(x.transpose(1, 0, 2))              # X (Tmax, B, C)
    bbd = None
    if bias_b is not None:
        bbd = torch.full((B, bb_bs), SENT, device=DEV)
        bbd[:, :M] = _dev(bias_b)
    cur = torch.full((B, cur_bs), SENT, device=DEV)
    big_out, out = _guarded((B, out_bs))
    want_out_pad = torch.full((B, out_bs - M), SENT)
    hist = tdev = big_hist = None
    if k == 3:
        big_hist, hist = _guarded((B, hist_bs))
        big_want, hist_want = _guarded((B, hist_bs))
        tdev = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for t in range(Tmax):
        cur[:, :C] = X[t]
        big_out.fill_(SENT)
        if k == 3:
            tdev.fill_(t)
        _matvec(wd, biasd, bbd, bb_bs, cur, cur_bs, hist, hist_bs if k == 3 else 0, Tmax, tdev, case.dil if k == 3 else 1, out, out_bs,
                B, C, M, k)
        got = out.cpu()
        assert bool((big_out[:PAD] == SENT).all()) and bool((big_out[-PAD:] == SENT).all()), ("out: written outside the buffer", t)
        assert torch.equal(got[:, M:], want_out_pad), ("out: stride padding written", t)
        if k == 3:
            hist_want[:, t * C:(t + 1) * C] = X[t]
            assert torch.equal(big_hist, big_want), ("history: something other than column %d changed, or column %d is not cur" % (t, t))
        worst = max(worst, _check_bound(got[:, :M].numpy(), want[t], S[t], K, (case.name, t)))
    if k == 3:
        assert torch.equal(hist[:, :Tmax * C].reshape(B, Tmax, C).cpu(), torch.from_numpy(x))
    print("MATVEC %-34s K=%4d frames=%2d worst fraction of the bound %.3f" % (case.name, K, Tmax, worst))


@pytest.mark.parametrize("C,k", R.PROBE_CASES)
def test_matvec_position_probe_is_bitwise(C, k):
    """Item b's staged input is one-hot at flat tap-major position p_b, the weights are distinct integers: out[b][m] == w[m][p_b] to the
    bit, for every m, every position of [0, K) once (64 items per launch, each with its own p).  t = 5 >= 2 dilation: all taps live."""
    K, M, Tmax, dil, t = C * k, R.PROBE_M, 6, 2, 5
    w = R.probe_weights(C, k)
    wd, flat = _dev(w), w.reshape(M, K)
    tdev = torch.full((1,), t, dtype=torch.int32, device=DEV) if k == 3 else None
    for ps in R.probe_plan(C, k):
        B = len(ps)
        cur, hist = np.zeros((B, C), dtype=np.float32), np.zeros((B, Tmax, C), dtype=np.float32)
        for b, p in enumerate(ps):
            j, c = divmod(int(p), C)
            if j == k - 1:
                cur[b, c] = 1.0
            else:
                hist[b, t - (k - 1 - j) * dil, c] = 1.0
        curd, histd = _dev(cur), _dev(hist) if k == 3 else None
        out = torch.full((B, M), SENT, device=DEV)
        _matvec(wd, None, None, 0, curd, C, histd, Tmax * C if k == 3 else 0, Tmax, tdev, dil, out, M, B, C, M, k)
        got = out.cpu().numpy()
        bad = np.argwhere(got != flat[:, ps].T)
        assert bad.size == 0, ("C=%d k=%d: item %d (position %d), row %d: got %r, want %r"
                               % (C, k, bad[0][0], ps[bad[0][0]], bad[0][1], got[tuple(bad[0])], flat[bad[0][1], ps[bad[0][0]]]))


@pytest.mark.parametrize("C,dil,M,B", [(12, 1, 5, 9), (36, 3, 3, 17), (256, 2, 4, 8)])
def test_matvec_frame_counter_outside_the_history(C, dil, M, B):
    """t = -1, Tmax, Tmax + dilation, Tmax + 2 dilation: a tap outside [0, Tmax) is zero and cur is not filed.  The history is the middle
    of a (B, G + Tmax + G, C) allocation with G = 2 dilation + 1 guard columns on either side, so no access of the kernel -- with or
    without its range checks -- leaves the allocation; guards and history are bitwise unchanged, out is the reference's."""
    Tmax, G, K = 7, 2 * dil + 1, 3 * C
    rng = np.random.default_rng(C + dil)
    w = rng.standard_normal((M, 3, C)).astype(np.float32)
    bias = rng.standard_normal(M).astype(np.float32)
    x = rng.standard_normal((B, Tmax, C)).astype(np.float32)
    cur = rng.standard_normal((B, C)).astype(np.float32)
    wd, biasd, curd = _dev(w), _dev(bias), _dev(cur)
    before = torch.full((B, G + Tmax + G, C), SENT, device=DEV)
    before[:, G:G + Tmax] = _dev(x)
    hist_bs = (Tmax + 2 * G) * C
    for t in (-1, Tmax, Tmax + dil, Tmax + 2 * dil):
        alloc = before.clone()
        first = ctypes.c_void_p(alloc.data_ptr() + 4 * G * C)                       # column 0 of item 0's history
        tdev = torch.full((1,), t, dtype=torch.int32, device=DEV)
        big_out, out = _guarded((B, M))
        _call("ssv_column_matvec", P(wd), P(biasd), None, 0, P(curd), C, first, hist_bs, Tmax, P(tdev), dil, P(out), M, B, C, M, 3, _st())
        got = out.cpu().numpy()
        assert torch.equal(alloc[:, G:G + Tmax], before[:, G:G + Tmax]), ("a column of the history was written at t = %d" % t)
        assert torch.equal(alloc, before), ("a guard column was written at t = %d" % t)
        assert bool((big_out[:PAD] == SENT).all()) and bool((big_out[-PAD:] == SENT).all())
        want, S = R.matvec(w, bias, None, cur, x, t, dil, Tmax)
        frac = _check_bound(got, want, S, K, ("t", t))
        print("MATVEC outside C=%d dilation=%d t=%d: worst fraction of the bound %.3f" % (C, dil, t, frac))


# ---- ssv_column_ln_act / ssv_column_gate -------------------------------------------------------------------------------------------------
BAR = 1e-5


def _ln32(x, g, b):
    return torch.nn.functional.layer_norm(torch.from_numpy(x), (x.shape[1],), torch.from_numpy(g), torch.from_numpy(b), 1e-5)


def _strided_in(x, pad):
    """x (B, C) as the first C floats of every row of a sentinel-filled (B, C + pad)."""
    full = torch.full((x.shape[0], x.shape[1] + pad), SENT, device=DEV)
    full[:, :x.shape[1]] = _dev(x)
    return full


def _held(case, got, want, e32, tag):
    """The bars of one LayerNorm / gate case; returns (rel_err, worst per-item error or None, bar)."""
    e = R.rel_err(got, want)
    if case.kind == "mean100":
        bar = max(BAR, 4 * e32)
        assert e <= bar, (tag, case, e, bar, e32)
        return e, None, bar
    rows = float(R.row_err(got, want).max())
    assert e < BAR and rows <= BAR, (tag, case, e, rows)
    return e, rows, BAR


@pytest.mark.parametrize("C", R.LN_CHANNELS)
def test_ln_act_vs_float64(C):
    """Every row of LN_CASES with this C.  Normal and constant columns: 1e-5 in rel_err and 1e-5 per item against the item's own maximum.
    Mean 100: the larger of 1e-5 and 4 x the error of torch's float32 layer_norm (CPU) on the same inputs; both numbers are printed.

    The constant column (2^(b-1) in every channel of item b) gives act(beta), and how exactly follows from the kernel's arithmetic: the sum
    2^e C is an exact float32 in any order; the mean is col_mean of it, fl(sum * fl(1 / C)) corrected once by the exact residual, which is
    2^e itself for every C (restated and checked in tests/test_column_step_ref_cpu.py); so every v - mu is 0 and n = 0 * r * gamma + beta
    = beta: EXACTLY beta for act 0 and max(beta, 0) for act 1, asserted bitwise.  (With the mean as plain sum * (1 / C) the compiler
    contracts v - mu into fma(-1 / C, sum, v), the rounded reciprocal's 2^-24 survives, and rsqrt(eps) = 316 turns it into gamma c 2e-5:
    this test measured 1.3e-4 at c = 8 on that kernel.)  act 2 is 1 / (1 + __expf(-beta)): the argument's scaling by log2(e) loses at
    most |beta| 2^-23 of e^-beta, the hardware exponential one ulp (2^-23), the addition and the division half an ulp each -- within
    (|beta| + 4) 2^-23 of sigmoid(beta), relative; asserted."""
    worst = {}
    for case in [c for c in R.LN_CASES if c.C == C]:
        x, g, b = R.ln_inputs(case)
        B = case.B
        want = R.ln_act(x, g, b, case.act)
        xd = _strided_in(x, R.LN_PAD_X if case.padded else 0)
        big_y, y = _guarded((B, C + (R.LN_PAD_Y if case.padded else 0)))
        gd, bd = _dev(g), _dev(b)
        _call("ssv_column_ln_act", P(xd), xd.stride(0), P(gd), P(bd), P(y), y.stride(0), B, C, case.act, _st())
        got = y[:, :C].cpu().numpy()
        assert bool((y[:, C:] == SENT).all()) and bool((big_y[:PAD] == SENT).all()) and bool((big_y[-PAD:] == SENT).all()), case
        e32 = None
        if case.kind == "mean100":
            n32 = _ln32(x, g, b)
            n32 = torch.relu(n32) if case.act == 1 else torch.sigmoid(n32) if case.act == 2 else n32
            e32 = R.rel_err(n32.numpy(), want)
        e, rows, bar = _held(case, got, want, e32, "ln_act")
        if case.kind == "mean100":
            print("LN mean100 C=%d B=%d act=%d %s: kernel %.2e, torch float32 %.2e, bar %.2e" % (C, B, case.act, "padded" if case.padded else "dense", e, e32, bar))
        if case.kind == "constant":
            if case.act == 0:
                assert np.array_equal(got, np.repeat(b[None], B, axis=0)), case
            elif case.act == 1:
                assert np.array_equal(got, np.repeat(np.maximum(b, np.float32(0))[None], B, axis=0)), case
            else:
                assert (np.abs(got - want) <= (np.abs(b.astype(np.float64))[None] + 4) * 2.0 ** -23 * want).all(), case
        key = case.kind
        worst[key] = max(worst.get(key, 0.0), e)
        if rows is not None:
            worst[key + "/item"] = max(worst.get(key + "/item", 0.0), rows)
    print("LN   C=%4d worst over B, act, strides: %s" % (C, "  ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("C", R.LN_CHANNELS)
def test_gate_vs_float64(C):
    """Every row of GATE_CASES with this C, the bars of test_ln_act_vs_float64 (both halves of h are of the row's kind; x is standard
    normal).  h is dense (B, 2C) by contract; x and y carry padded strides."""
    worst = {}
    for case in [c for c in R.GATE_CASES if c.C == C]:
        h, x, g1, b1, g2, b2 = R.gate_inputs(case)
        B = case.B
        want = R.gate(h, x, g1, b1, g2, b2)
        xd = _strided_in(x, R.LN_PAD_X if case.padded else 0)
        big_y, y = _guarded((B, C + (R.LN_PAD_Y if case.padded else 0)))
        hd, pars = _dev(h), [_dev(v) for v in (g1, b1, g2, b2)]
        _call("ssv_column_gate", P(hd), P(xd), xd.stride(0), *[P(v) for v in pars], P(y), y.stride(0), B, C, _st())
        got = y[:, :C].cpu().numpy()
        assert bool((y[:, C:] == SENT).all()) and bool((big_y[:PAD] == SENT).all()) and bool((big_y[-PAD:] == SENT).all()), case
        e32 = None
        if case.kind == "mean100":
            sg = torch.sigmoid(_ln32(h[:, :C], g1, b1))
            e32 = R.rel_err((sg * _ln32(h[:, C:], g2, b2) + (1 - sg) * torch.from_numpy(x)).numpy(), want)
        e, rows, bar = _held(case, got, want, e32, "gate")
        if case.kind == "mean100":
            print("GATE mean100 C=%d B=%d %s: kernel %.2e, torch float32 %.2e, bar %.2e" % (C, B, "padded" if case.padded else "dense", e, e32, bar))
        worst[case.kind] = max(worst.get(case.kind, 0.0), e)
        if rows is not None:
            worst[case.kind + "/item"] = max(worst.get(case.kind + "/item", 0.0), rows)
    print("GATE C=%4d worst over B, strides: %s" % (C, "  ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


# ---- replay ------------------------------------------------------------------------------------------------------------------------------
def test_captured_matvec_gate_advance_replays_bitwise_like_eager_calls():
    """One graph of ssv_column_matvec (k = 3, dilation 3) -> ssv_column_gate -> ssv_synth_column_advance (which moves t_dev), replayed Tmax
    times with a fresh input column per frame, against the same calls made eagerly: histories, every frame's output and the counter are
    bitwise equal.  B = 9, C = 36."""
    B, C, Tmax, dil = 9, 36, 12, 3
    rng = np.random.default_rng(11)
    f = lambda *s: _dev(rng.standard_normal(s).astype(np.float32))
    w, bias, X = f(2 * C, 3, C), f(2 * C), f(Tmax, B, C)
    g1, b1, g2, b2 = f(C), f(C), f(C), f(C)

    class Bufs:
        def __init__(self):
            z = lambda *s: torch.zeros(s, device=DEV)
            self.cur, self.hist, self.pre, self.y = z(B, C), z(B, Tmax, C), z(B, 2 * C), z(B, C)
            self.Y, self.mel_cur, self.t = z(B, C, Tmax), z(B, C), torch.zeros(1, dtype=torch.int32, device=DEV)

        def reset(self):
            for v in vars(self).values():
                v.zero_()

        def step(self):
            _matvec(w, bias, None, 0, self.cur, C, self.hist, Tmax * C, Tmax, self.t, dil, self.pre, 2 * C, B, C, 2 * C, 3)
            _call("ssv_column_gate", P(self.pre), P(self.cur), C, P(g1), P(b1), P(g2), P(b2), P(self.y), C, B, C, _st())
            _call("ssv_synth_column_advance", P(self.y), P(self.Y), P(self.mel_cur), P(self.t), B, C, Tmax, _st())

    eager, replayed = Bufs(), Bufs()
    for t in range(Tmax):
        eager.cur.copy_(X[t])
        eager.step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        replayed.step()                              # warm step, outside the capture: frame 0 on zero inputs
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.step()
    replayed.reset()
    for t in range(Tmax):
        replayed.cur.copy_(X[t])
        graph.replay()
    torch.cuda.synchronize()
    assert int(eager.t[0]) == Tmax and int(replayed.t[0]) == Tmax
    assert torch.equal(eager.hist, X.permute(1, 0, 2)) and torch.equal(replayed.hist, eager.hist)
    assert torch.equal(replayed.Y, eager.Y) and torch.equal(replayed.mel_cur, eager.mel_cur) and torch.equal(replayed.pre, eager.pre)
    assert bool(eager.Y.abs().sum() > 0) and torch.equal(eager.Y[:, :, Tmax - 1], eager.y)


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------
def test_unsupported_arguments_are_refused_before_any_launch():
    """Every check of the three entry points: a RuntimeError, and the output buffer still holds its sentinel."""
    B, C, M, Tmax = 3, 64, 8, 4
    w = torch.zeros(M * 1540, device=DEV)
    cur, hist = torch.zeros(B, 1544, device=DEV), torch.zeros(B, Tmax, 64, device=DEV)
    tdev = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((B, 1028), SENT, device=DEV)
    g = torch.ones(1028, device=DEV)
    mv = lambda C=C, k=1, B=B, cur_bs=1544, hist=None, hist_bs=0, tdev=None: _matvec(w, None, None, 0, cur, cur_bs, hist, hist_bs, Tmax, tdev, 1, out, 1028,
                                                                                    B, C, M, k)
    refused = [
        ("multiple of 4", lambda: mv(C=62)),                                              # C % 4 != 0
        ("at most 1536", lambda: mv(C=1540)),                                             # C k = 1540
        ("at most 1536", lambda: mv(C=516, k=3, hist=hist, hist_bs=Tmax * 516, tdev=tdev)),
        ("batch strides", lambda: mv(cur_bs=1542)),                                       # a stride that is not a multiple of 4
        ("batch strides", lambda: mv(k=3, hist=hist, hist_bs=Tmax * 64 + 2, tdev=tdev)),
        ("bad argument", lambda: mv(k=2)),
        ("needs a history", lambda: mv(k=3, hist=None, hist_bs=Tmax * 64, tdev=tdev)),
        ("needs a history", lambda: mv(k=3, hist=hist, hist_bs=Tmax * 64, tdev=None)),
        ("bad argument", lambda: mv(B=0)),
        ("column_ln_act: 1025 channels", lambda: _call("ssv_column_ln_act", P(cur), 1544, P(g), P(g), P(out), 1028, B, 1025, 0, _st())),
        ("column_gate: 1025 channels", lambda: _call("ssv_column_gate", P(hist), P(cur), 1544, P(g), P(g), P(g), P(g), P(out), 1028, B, 1025, _st())),
        ("bad argument", lambda: _call("ssv_column_ln_act", P(cur), 1544, P(g), P(g), P(out), 1028, 0, 64, 0, _st())),
        ("bad argument", lambda: _call("ssv_column_gate", P(hist), P(cur), 1544, P(g), P(g), P(g), P(g), P(out), 1028, 0, 64, _st())),
    ]
    for match, fn in refused:
        with pytest.raises(RuntimeError, match=match):
            fn()
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote its output"
    mv()                                                                                   # the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert bool((out[:, :M] == 0).all()) and bool((out[:, M:] == SENT).all())


# ---- the whole run -----------------------------------------------------------------------------------------------------------------------
def test_free_run_at_hidden_36_vs_float64_oracle():
    """free_run_incremental on a conditioned tiny melSyn of hidden 36 (every highway layer K = 108, nq = 27: three full trips of an item's
    8 lanes and three lanes of a fourth; 1x1 links with nq = 9, 18, 20), B = 9 (an item group of one), N = 11, 24 frames, against
    oracle.tts_oracle.synthesize_loop in float64 on the same state dict.  The rule of test_full_size_shared_texts_vs_cpu_oracle: attention
    indices exact on every frame, mel within 1e-3 relative per item, and every item decisive on every frame (oracle top-two margin > 1e-3;
    also asserted on the CPU by tests/test_column_step_ref_cpu.py), so the compared prefix is the whole run."""
    from spoofsv_amd import synth
    B, frames = R.RUN["B"], R.RUN["frames"]
    m, text, spk = R.run_case()
    Yo, Ao, pma_o, margins = R.run_oracle(m, text, spk)
    print("RUN  oracle top-2 margins per item (min over %d frames): %s" % (frames, ["%.2e" % float(v) for v in margins.min(1).values]))
    assert tuple(margins.shape) == (B, frames)
    assert float(margins.min()) > R.RUN_MARGIN, "the oracle is indecisive on a compared frame: the inputs of this test no longer serve"
    m = m.to(DEV).eval()
    with torch.no_grad():
        Y, A = synth.free_run_incremental(m, text.to(DEV), spk.to(DEV), frames)
    assert tuple(Y.shape) == (B, R.RUN["freq_bins"], frames) and tuple(A.shape) == (B, R.RUN["N"], frames)
    pma = A.argmax(1).t().cpu()                                      # (frames, B)
    for b in range(B):
        assert torch.equal(pma[:, b], pma_o[:, b]), (b, int((pma[:, b] != pma_o[:, b]).nonzero()[0]))
        e = R.rel_err(Y[b].cpu().numpy(), Yo[b].numpy())
        print("RUN  item %d: mel %.2e over %d frames" % (b, e, frames))
        assert e < 1e-3, (b, e)
