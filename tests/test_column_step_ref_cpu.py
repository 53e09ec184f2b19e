"""tests/_column_step_ref.py held to plain torch float64 expressions, and its case tables held to what they claim: the GPU tests of
tests/test_gpu_column_step.py are only as good as these references and these rows."""
import numpy as np
import pytest
import torch

import _column_step_ref as R

F = torch.nn.functional


def _t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


@pytest.mark.parametrize("C,k,M,B,dil,Tmax", [(12, 3, 5, 3, 1, 21), (12, 3, 5, 3, 3, 21), (8, 3, 7, 2, 9, 21), (20, 1, 6, 4, 0, 1)])
def test_matvec_is_a_causal_conv1d_column_by_column(C, k, M, B, dil, Tmax):
    """Every frame of the stepped reference against conv1d on the left-padded full sequence (the weight back in (M, C, k)), with and
    without the two bias terms; S against the same convolution of the absolute values."""
    rng = np.random.default_rng(C + k + dil)
    w = rng.standard_normal((M, k, C)).astype(np.float32)
    bias = rng.standard_normal(M).astype(np.float32)
    bias_b = rng.standard_normal((B, M)).astype(np.float32)
    x = rng.standard_normal((B, Tmax, C)).astype(np.float32)
    conv = lambda ww, xx: F.conv1d(F.pad(_t64(xx).permute(0, 2, 1), ((k - 1) * max(dil, 1), 0)), _t64(ww).permute(0, 2, 1).contiguous(),
                                   dilation=max(dil, 1))
    full, full_abs = conv(w, x), conv(np.abs(w), np.abs(x))                      # (B, M, Tmax)
    for t in range(Tmax):
        out, S = R.matvec(w, bias, bias_b, x[:, t], x, t, dil, Tmax)
        want = full[:, :, t] + _t64(bias)[None] + _t64(bias_b)
        want_s = full_abs[:, :, t] + _t64(bias).abs()[None] + _t64(bias_b).abs()
        assert float((_t64(out) - want).abs().max()) < 1e-12 and float((_t64(S) - want_s).abs().max()) < 1e-12, t
        out0, S0 = R.matvec(w, None, None, x[:, t], x, t, dil, Tmax)
        assert float((_t64(out0) - full[:, :, t]).abs().max()) < 1e-12 and float((_t64(S0) - full_abs[:, :, t]).abs().max()) < 1e-12, t
        assert (S >= np.abs(out) - 1e-12).all()


def test_matvec_taps_outside_the_history_are_zero():
    """A frame counter before or past the history: the taps that fall outside [0, Tmax) contribute nothing, the others do."""
    rng = np.random.default_rng(5)
    C, M, B, dil, Tmax = 8, 3, 2, 2, 6
    w = rng.standard_normal((M, 3, C))
    cur, hist = rng.standard_normal((B, C)), rng.standard_normal((B, Tmax, C))
    own = cur @ w[:, 2].T
    tap = lambda j, col: hist[:, col] @ w[:, j].T
    assert np.allclose(R.matvec(w, None, None, cur, hist, -1, dil, Tmax)[0], own, atol=1e-12)
    assert np.allclose(R.matvec(w, None, None, cur, hist, Tmax, dil, Tmax)[0], own + tap(1, Tmax - 2) + tap(0, Tmax - 4), atol=1e-12)
    assert np.allclose(R.matvec(w, None, None, cur, hist, Tmax + dil, dil, Tmax)[0], own + tap(0, Tmax - 2), atol=1e-12)
    assert np.allclose(R.matvec(w, None, None, cur, hist, Tmax + 2 * dil, dil, Tmax)[0], own, atol=1e-12)


@pytest.mark.parametrize("C", [1, 4, 63, 257, 1024])
def test_ln_act_and_gate_are_torch_layer_norm(C):
    rng = np.random.default_rng(C)
    B = 3
    x = rng.standard_normal((B, C)) * 3 + 1
    h = rng.standard_normal((B, 2 * C))
    g1, b1, g2, b2 = (rng.standard_normal(C) for _ in range(4))
    ln = lambda v, g, b: F.layer_norm(_t64(v), (C,), _t64(g), _t64(b), 1e-5)
    for act, fn in ((0, lambda v: v), (1, torch.relu), (2, torch.sigmoid)):
        assert float((_t64(R.ln_act(x, g1, b1, act)) - fn(ln(x, g1, b1))).abs().max()) < 1e-12
    sg = torch.sigmoid(ln(h[:, :C], g1, b1))
    want = sg * ln(h[:, C:], g2, b2) + (1 - sg) * _t64(x)
    assert float((_t64(R.gate(h, x, g1, b1, g2, b2)) - want).abs().max()) < 1e-12


def test_matvec_rows_have_the_properties_they_name():
    """Recomputed here from C, k, M, B alone: nq % 8, nq against the 192 prefetched quads, M % 4 and the row groups, B % 8 and the item
    groups, and that a padded row's strides are padded by multiples of 4 floats."""
    cdiv = lambda a, b: -(-a // b)
    for c in R.MATVEC_CASES:
        K = c.C * c.k
        assert c.C % 4 == 0 and K <= R.KMAX and c.k in (1, 3), c.name
        nq = K // 4
        e = c.edge
        assert e["nq"] == nq and e["nq%8"] == nq % R.LANES_PER_ITEM, c.name
        assert e["prefetch"] == ("below" if nq < R.PREFETCH_QUADS else "exact" if nq == R.PREFETCH_QUADS else "tail"), c.name
        assert e["M%4"] == c.M % R.ROWS_PER_GROUP and e["row_groups"] == cdiv(c.M, R.ROWS_PER_GROUP), c.name
        assert e["B%8"] == c.B % R.ITEMS_PER_GROUP and e["item_groups"] == cdiv(c.B, R.ITEMS_PER_GROUP), c.name
        cur_bs, out_bs, bb_bs, hist_bs = R.matvec_strides(c)
        dense = (c.C, c.M, c.M, c.Tmax * c.C)
        assert e["strides"] == ("padded" if c.padded else "dense"), c.name
        for got, d in zip((cur_bs, out_bs, bb_bs, hist_bs), dense):
            assert (got > d and (got - d) % 4 == 0) if c.padded else got == d, c.name
        assert cur_bs % 4 == 0 and hist_bs % 4 == 0, c.name
        assert (c.k == 3) == (c.dil in (1, 3, 9)) and c.Tmax == (R.STEP_TMAX if c.k == 3 else 1), c.name
        if c.k == 3:            # the stepping passes both sides of every zero-tap boundary
            assert {c.dil - 1, c.dil, 2 * c.dil - 1, 2 * c.dil} <= set(range(c.Tmax)), c.name


def test_matvec_table_holds_every_listed_value_with_two_values_of_every_other_axis():
    ck = {(4, 1), (4, 3), (28, 1), (12, 3), (36, 3), (80, 1), (764, 1), (768, 1), (256, 3), (772, 1), (260, 3), (1532, 1), (512, 3), (1536, 1)}
    axes = {"CK": lambda c: (c.C, c.k), "M": lambda c: c.M, "B": lambda c: c.B, "bias": lambda c: (c.bias, c.bias_b),
            "strides": lambda c: c.padded, "dil": lambda c: c.dil}
    want = {"CK": ck, "M": {1, 3, 4, 5, 80, 513}, "B": {1, 7, 8, 9, 17}, "bias": {(a, b) for a in (False, True) for b in (False, True)},
            "strides": {False, True}, "dil": {1, 3, 9}}
    rows = R.MATVEC_CASES
    assert len(set(c.name for c in rows)) == len(rows)
    for a, fa in axes.items():
        have = {fa(c) for c in rows} - ({0} if a == "dil" else set())
        assert have == want[a], (a, have ^ want[a])
        for v in want[a]:
            mine = [c for c in rows if fa(c) == v]
            for o, fo in axes.items():
                if o == a:
                    continue
                if o == "dil" and a == "CK" and v[1] == 1:
                    continue                                   # a k = 1 row has no dilation
                others = {fo(c) for c in mine} - ({0} if o == "dil" else set())
                assert len(others) >= 2, ("%s = %r meets only %r on axis %s" % (a, v, others, o))
    # K = 768 and K = 1536 on both kernel sizes
    assert {(768, 1), (256, 3), (512, 3), (1536, 1)} <= {(c.C, c.k) for c in rows}


def test_ln_tables_cover_what_they_list():
    for table, acts in ((R.LN_CASES, {0, 1, 2}), (R.GATE_CASES, {None})):
        assert {c.C for c in table} >= {1, 4, 63, 64, 65, 80, 255, 256, 257, 512, 1023, 1024}
        assert {c.B for c in table} == {1, 5} and {c.act for c in table} == acts
        assert {c.padded for c in table} == {False, True} and {c.kind for c in table} == set(R.LN_KINDS)
        assert len(set(table)) == len(table)
    assert max(R.LN_CHANNELS) == 1024 and {256 * i + 1 for i in range(4)} <= set(R.LN_CHANNELS)      # where a thread's next channel goes live
    for case in R.LN_CASES[:9] + R.LN_CASES[-9:]:
        x, g, b = R.ln_inputs(case)
        assert x.dtype == g.dtype == b.dtype == np.float32 and x.shape == (case.B, case.C)
        if case.kind == "mean100":
            assert abs(float(x.mean()) - 100) < 1.5
        if case.kind == "constant":
            assert all(len(set(row.tolist())) == 1 for row in x) and float(np.abs(x).min()) > 0


def test_constant_columns_have_an_exact_mean_in_float32():
    """What the GPU test's "exactly beta" rests on: for every C of the table and every item's constant 2^e, the sum 2^e C is an exact float32
    and the kernels' mean of it (a reciprocal and one exact-residual correction, restated as kernel_mean) is 2^e; that mean is the correctly
    rounded quotient for other sums too; float64 agrees that the result is act(beta)."""
    rng = np.random.default_rng(3)
    for C in (3, 41, 63, 769, 1023):            # 41: the first C whose plain float32 C * (1 / C) is not 1
        for total in (rng.standard_normal(200) * C).astype(np.float32):
            assert R.kernel_mean(total, C) == total / np.float32(C), (C, total)
    assert np.float32(41) * (np.float32(1) / np.float32(41)) != np.float32(1) and R.constant_mean_is_exact(41)
    for C in R.LN_CHANNELS:
        for b in range(5):
            v = float(R.constant_value(b))
            assert np.log2(v) == round(np.log2(v)) and R.constant_mean_is_exact(C, b), (C, b)
    case = [c for c in R.LN_CASES if c.kind == "constant" and c.C == 257 and c.B == 5 and c.act == 2][0]
    x, g, b = R.ln_inputs(case)
    assert np.array_equal(R.ln_act(x, g, b, 2), np.repeat((1.0 / (1.0 + np.exp(-b.astype(np.float64))))[None], 5, axis=0))


@pytest.mark.parametrize("C,k", R.PROBE_CASES)
def test_probe_plans_cover_every_position_once(C, k):
    K = C * k
    plan = R.probe_plan(C, k)
    assert len(plan) == -(-K // R.PROBE_ITEMS) and all(1 <= len(p) <= R.PROBE_ITEMS for p in plan)
    assert all(len(set(p.tolist())) == len(p) for p in plan)                  # every item of a launch has its own position
    assert sorted(np.concatenate(plan).tolist()) == list(range(K))
    w = R.probe_weights(C, k)
    assert w.dtype == np.float32 and len(set(w.reshape(-1).tolist())) == w.size
    # a one-hot input at p picks w[m][p]: the reference agrees, exactly
    p = int(plan[-1][-1])
    cur, hist = np.zeros((1, C), dtype=np.float32), np.zeros((1, 6, C), dtype=np.float32)
    j, c = divmod(p, C)
    if j == k - 1:
        cur[0, c] = 1
    else:
        hist[0, 5 - (k - 1 - j) * 2, c] = 1
    assert np.array_equal(R.matvec(w, None, None, cur, hist, 5, 2, 6)[0][0], w.reshape(-1, K)[:, p].astype(np.float64))


def test_probe_cases_are_the_listed_sizes_on_both_kernel_sizes():
    assert {C * k for C, k in R.PROBE_CASES} == {108, 768, 772, 1536}
    assert {k for C, k in R.PROBE_CASES if C * k in (768, 1536)} == {1, 3} and {k for C, k in R.PROBE_CASES} == {1, 3}


def test_whole_run_inputs_are_decisive_on_every_frame():
    """The float64 oracle on the whole-run case of tests/test_gpu_column_step.py: every item's top-two attention margin is above 1e-3 on
    every frame, so the GPU test compares the whole run.  If the inputs ever stop serving, this fails, not a vacuous GPU pass."""
    assert R.RUN["hidden"] % 4 == 0 and (3 * R.RUN["hidden"] // 4) % 8 != 0 and 3 * R.RUN["hidden"] == 108
    m, text, spk = R.run_case()
    Y, A, pma, margins = R.run_oracle(m, text, spk)
    B, N, frames = R.RUN["B"], R.RUN["N"], R.RUN["frames"]
    assert Y.dtype == torch.float64 and tuple(Y.shape) == (B, R.RUN["freq_bins"], frames) and tuple(A.shape) == (B, N, frames)
    assert tuple(pma.shape) == (frames, B) and tuple(margins.shape) == (B, frames)
    print("whole run: oracle top-2 margins per item (min over %d frames): %s" % (frames, ["%.2e" % float(v) for v in margins.min(1).values]))
    assert float(margins.min()) > R.RUN_MARGIN
    assert len(set(pma[-1].tolist())) > 1 and int(pma.max()) == N - 1           # the items do not all walk the same path
