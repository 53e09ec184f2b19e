"""The three kernels that restate one synthesis step of the attention (models/TTSModel.py:281-295) -- attention_step_kernel (csrc/attn.hip),
attention_column_kernel (csrc/synth.hip), attention_column_wide_kernel (csrc/synth_wide.hip) -- called alone through the C ABI and held
to tests/_attention_ref.py: step_attention in float64.  One test body, one thin adapter per kernel for its layout.

What the whole-run tests never reach and these do: N up to the 1024 the kernels accept (four trips of every strided loop), d = 1, 3, 5,
6, 37 and 130 (channel quarters c0 = wave d / 4 that are empty, of one channel, uneven), the window at N - 1, N - 2, N - 3 and either
side of position 64 (two waves) and 256 (two trips of one thread), and EXACT ties inside the window, where the lower index has to win
across lanes, waves and trips.  Bars: ten times what the float32 restatement loses against float64 on the same case, at least 4 float32
ulp of the peak; indices are compared integer for integer except where float64's own top-two probabilities are closer than 1e-4, and
at most one item in 64 may be left out that way (asserted).  Figures: profiles/attention_paths_accuracy.txt (`pytest -m gpu -s`)."""
import ctypes

import numpy as np
import pytest
import torch

import _attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0                  # what the tests fill A, rq and the guard zones with: no kernel writes it
PAD = 64                     # floats of guard zone on either side of a guarded buffer
A_T = 5
KERNELS = ["step_col", "step_coldev", "column", "wide"]
ULP4 = 4 * 2.0 ** -23
_REF, _OUT = {}, {}


def P(x):
    return ctypes.c_void_p(x.data_ptr())


def _st():
    from spoofsv_amd import ops
    return ops._stream()


def _call(name, *args):
    from spoofsv_amd import _lib
    _lib.call(name, *args)


def _guarded(shape, fill=SENT, dtype=torch.float32):
    """A tensor of ``shape`` inside a larger allocation the test owns, everything filled with ``fill``: (whole allocation, view)."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return big, big[PAD:PAD + n].view(shape)


def _guards_intact(big, fill=SENT):
    return bool((big[:PAD] == fill).all()) and bool((big[-PAD:] == fill).all())


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _launch(kernel, kv, q, pma, col, a_T=A_T, U=None, Bw=None):
    """One launch of ``kernel`` for frame ``col``.  kv (B, 2d, N) -- for the wide kernel (U, 2d, N), item b reading text b % U -- q (B, d),
    pma (B,).  Returns a dict: A (B, N, a_T) and its allocation, idx (B,), and where the kernel produces them r and the q half (B, d)."""
    B, d = q.shape
    N = kv.shape[2]
    kvd, pmad = _dev(kv), _dev(pma.astype(np.int64))
    bigA, A = _guarded((B, N, a_T))
    out = {"A": A, "bigA": bigA, "pma_in": pmad}
    if kernel in ("step_col", "step_coldev"):
        idx = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        if kernel == "step_col":           # q is the last column of Q (B, d, col + 1), the frame index is a host int
            Q = torch.full((B, d, col + 1), float("nan"), device=DEV)
            Q[:, :, col] = _dev(q)
            q_last = ctypes.c_void_p(Q.data_ptr() + 4 * col)
            _call("ssv_attention_step", P(kvd), 2 * d * N, q_last, d * (col + 1), col + 1, P(pmad), P(A), a_T, col, None, P(idx), B, d, N, _st())
        else:                              # the pointer is column 0 of Q (B, d, a_T); the kernel adds the device-side frame index
            Q = torch.full((B, d, a_T), float("nan"), device=DEV)
            Q[:, :, col] = _dev(q)
            col_dev = torch.tensor([col], dtype=torch.int32, device=DEV)
            _call("ssv_attention_step", P(kvd), 2 * d * N, P(Q), d * a_T, a_T, P(pmad), P(A), a_T, 0, P(col_dev), P(idx), B, d, N, _st())
        out["idx"] = idx
    else:
        t_dev = torch.tensor([col], dtype=torch.int32, device=DEV)
        idx = pmad.clone()                 # read, then replaced by the arg-max
        if kernel == "column":
            qd = _dev(q)
            bigrq, rq = _guarded((B, 2 * d))
            _call("ssv_attention_column", P(kvd), 2 * d * N, P(qd), P(idx), P(A), a_T, P(t_dev), P(rq), B, d, N, _st())
            out.update(r=rq[:, :d], qhalf=rq[:, d:])
        else:
            U = B if U is None else U
            Bw = B if Bw is None else Bw
            assert kv.shape[0] == U
            qw = torch.zeros((d, Bw), device=DEV)
            qw[:, :B] = _dev(q).t()
            bigrq, rq = _guarded((2 * d, Bw))
            _call("ssv_attention_column_wide", P(kvd), 2 * d * N, U, P(qw), P(idx), P(A), a_T, P(t_dev), P(rq), B, Bw, d, N, _st())
            out.update(r=rq[:d, :B].t(), qhalf=rq[d:, :B].t(), rq_wide=rq)
        out.update(idx=idx, bigrq=bigrq, t_dev=t_dev)
    torch.cuda.synchronize()
    return out


def _reference(key, kv, q, pma):
    """float64 and float32 restatements of a case, once: (a64, idx64, r64, err32 of a, err32 of r relative to the peak, left-out mask)."""
    if key not in _REF:
        a, idx, r = R.step_attention_batch(kv, q, pma)
        a32, _, r32 = R.step_attention_batch(kv, q, pma, np.float32)
        e_a = float(np.abs(a32.astype(np.float64) - a).max())
        e_r = float(np.abs(r32.astype(np.float64) - r).max() / np.abs(r).max())
        _REF[key] = (a, idx, r, e_a, e_r, R.top_two_gap(a) < R.GAP_MIN)
    return _REF[key]


def _check(tag, kernel, out, ref, q, pma, col, a_T=A_T, tied=None):
    """Everything one launch has to satisfy.  ``tied``: the tie cases' (B,) counts of tied positions -- there the index is pma itself and the
    tied probabilities are bit-equal; otherwise the index is float64's wherever float64 is not itself within 1e-4 of a tie."""
    a64, idx64, r64, e_a, e_r, left_out = ref
    B, N = a64.shape
    A = out["A"].cpu().numpy()
    got = A[:, :, col].astype(np.float64)
    assert _guards_intact(out["bigA"]), "A: written outside the buffer"
    others = np.delete(A, col, axis=2)
    assert np.all(others == np.float32(SENT)), "a column other than %d of A was written" % col
    assert np.isfinite(got).all()
    n = np.arange(N)[None, :]
    outside = (n < pma[:, None]) | (n >= pma[:, None] + 3)
    assert np.all(got[outside] == 0.0), "probability outside the window"
    assert float(np.abs(got.sum(axis=1) - 1).max()) < 1e-6
    err_a, bar_a = float(np.abs(got - a64).max()), max(10 * e_a, ULP4 * float(a64.max()))
    idx = out["idx"].cpu().numpy()
    assert bool(torch.equal(out["pma_in"].cpu(), torch.from_numpy(pma.astype(np.int64))))
    line = "STEP  %-11s %-22s a %.2e (bar %.2e, float32 %.2e)" % (kernel, tag, err_a, bar_a, e_a)
    err_r = bar_r = None
    if "r" in out:
        r = out["r"].cpu().numpy().astype(np.float64)
        err_r, bar_r = float(np.abs(r - r64).max() / np.abs(r64).max()), max(10 * e_r, ULP4)
        line += "  r %.2e (bar %.2e, float32 %.2e)" % (err_r, bar_r, e_r)
    print(line + "  left out %d of %d" % (0 if tied is not None else int(left_out.sum()), B))
    assert err_a <= bar_a, (err_a, bar_a)
    if "r" in out:
        assert err_r <= bar_r, (err_r, bar_r)
        assert bool(torch.equal(out["qhalf"].cpu(), torch.from_numpy(q))), "the q half of rq is a copy of q"
        assert _guards_intact(out["bigrq"]), "rq: written outside the buffer"
    if tied is None:
        assert int(left_out.sum()) <= B // 64, "more than one item in 64 is too close to a tie in float64 itself: choose another seed"
        keep = ~left_out
        assert np.array_equal(idx[keep], idx64[keep]), (np.nonzero(idx != idx64)[0], idx[idx != idx64], idx64[idx != idx64])
    else:
        assert np.array_equal(idx, pma), ("the lower index wins a tie", np.nonzero(idx != pma)[0], idx[idx != pma], pma[idx != pma])
        for b in range(B):
            p, k = int(pma[b]), int(tied[b])
            assert len(set(A[b, p:p + k, col].tolist())) == 1, ("tied probabilities differ", b, A[b, p:p + 3, col])
            assert A[b, p, col] == A[b, :, col].max()
    return got, idx


def _case_out(d, N, kernel, col):
    """The checked outputs of ``kernel`` on case (d, N) at frame ``col``, once per module (the agreement test reads them again)."""
    key = (d, N, kernel, col)
    if key not in _OUT:
        kv, q, pma = R.step_case(d, N)
        ref = _reference((d, N), kv, q, pma)
        out = _launch(kernel, kv, q, pma, col)
        a, idx = _check("d%d N%d col%d" % (d, N, col), kernel, out, ref, q, pma, col)
        _OUT[key] = (out["A"][:, :, col].cpu(), out["idx"].cpu(), out["r"].cpu().clone() if "r" in out else None)
    return _OUT[key]


@pytest.mark.parametrize("d,N", R.STEP_CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_step_kernels_vs_float64_windows_at_every_edge(kernel, d, N):
    """64 items per case; the first ones have their window at 0, N - 1, N - 2, N - 3 and around 64 and 256, the rest anywhere.  The first
    and the last frame of A (the step kernel with a device-side frame index has no range check: nothing past a_T - 1 is passed to it)."""
    fixed = R.fixed_windows(N)
    assert {0, N - 1} <= set(fixed) and (N <= 256 or {254, 255, 256} <= set(fixed)) and (N <= 64 or {62, 63, 64} <= set(fixed))
    for col in (0, A_T - 1):
        _case_out(d, N, kernel, col)


@pytest.mark.parametrize("d,N", R.STEP_CASES)
def test_step_kernels_agree_with_each_other(d, N):
    """The same index from all three kernels (both forms of the step kernel) wherever float64 is not near a tie, and -- the wide kernel claims
    the column kernel's arithmetic "operation for operation" -- bitwise the same a and r from those two."""
    col = A_T - 1
    outs = {k: _case_out(d, N, k, col) for k in KERNELS}
    keep = ~_REF[(d, N)][5]
    for k in KERNELS[1:]:
        assert np.array_equal(outs[k][1].numpy()[keep], outs[KERNELS[0]][1].numpy()[keep]), k
    assert bool(torch.equal(outs["step_col"][0], outs["step_coldev"][0]))
    assert bool(torch.equal(outs["column"][0], outs["wide"][0])) and bool(torch.equal(outs["column"][2], outs["wide"][2]))
    assert bool(torch.equal(outs["column"][1], outs["wide"][1]))


@pytest.mark.parametrize("d,N", R.TIE_CASES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_ties_go_to_the_lower_index(kernel, d, N):
    """Column p of K copied to p + 1 (and p + 2 for half of the items), p = 0, 62, 63, 254, 255, 256, 511, N - 2: the tied positions sit in
    neighbouring lanes, in two waves (63 | 64), in two trips (255 | 256, 511 | 512) -- every arm of the arg-max's tie-break."""
    kv, q, pma, ntied = R.tie_case(d, N)
    ref = _reference(("tie", d, N), kv, q, pma)
    out = _launch(kernel, kv, q, pma, 1)
    _check("ties d%d N%d" % (d, N), kernel, out, ref, q, pma, 1, tied=ntied)


@pytest.mark.parametrize("U", [1, 16, 64])
def test_wide_kernel_shared_texts_and_pad_columns(U):
    """U = 1, B / 4 and B texts for B = 64 items in Bw = 80 columns: item b reads text b % U; the pad columns of rq stay untouched; items
    with the same text, query and window give bitwise the same column."""
    d, N, B, Bw, col = 37, 257, 64, 80, 2
    kv, q, pma = R.step_case(d, N)
    period = min(2 * U, B)
    q, pma = q[np.arange(B) % period].copy(), pma[np.arange(B) % period].copy()
    kv_u = kv[:U].copy()
    kv_items = kv_u[np.arange(B) % U]
    ref = _reference(("wide", U), kv_items, q, pma)
    out = _launch("wide", kv_u, q, pma, col, U=U, Bw=Bw)
    _check("U%d Bw%d d%d N%d" % (U, Bw, d, N), "wide", out, ref, q, pma, col)
    rq = out["rq_wide"].cpu()
    assert bool((rq[:, B:] == SENT).all()), "pad columns of rq were written"
    A, idx = out["A"].cpu(), out["idx"].cpu()
    pairs = [(b, b + period) for b in range(B - period)]
    assert (len(pairs) > 0) == (U < B)
    for b, c in pairs:
        assert bool(torch.equal(A[b], A[c])) and bool(torch.equal(rq[:, b], rq[:, c])) and int(idx[b]) == int(idx[c]), (b, c)


@pytest.mark.parametrize("kernel", ["column", "wide"])
def test_column_kernels_past_the_last_frame_write_no_attention_but_still_step(kernel):
    """t = a_T: the column and wide kernels guard the write of A (col < a_T) and still produce pma and rq -- the free run's last iterations
    rely on it.  A lives inside a larger allocation of the test's; nothing in it changes."""
    d, N = 37, 257
    kv, q, pma = R.step_case(d, N)
    ref = _reference((d, N), kv, q, pma)
    last = _launch(kernel, kv, q, pma, A_T - 1)
    _check("t=a_T-1 d%d N%d" % (d, N), kernel, last, ref, q, pma, A_T - 1)
    past = _launch(kernel, kv, q, pma, A_T)
    assert bool((past["bigA"] == SENT).all()), "A (or its surroundings) written at t = a_T"
    assert bool(torch.equal(past["idx"], last["idx"])) and bool(torch.equal(past["r"], last["r"])) and bool(torch.equal(past["qhalf"], last["qhalf"]))
    assert _guards_intact(past["bigrq"]) and int(past["t_dev"][0]) == A_T


def test_limits_fail_loudly():
    """N = 1025 is refused by all three kernels, d = 1025 by the wide one (its query lives in LDS): RuntimeError, nothing launched."""
    kv, q, pma = R.step_case(2, 1025, 2)
    for kernel in KERNELS:
        with pytest.raises(RuntimeError, match="N=1025"):
            _launch(kernel, kv, q, pma, 0)
    kv, q, pma = R.step_case(1025, 3)
    with pytest.raises(RuntimeError, match="d=1025"):
        _launch("wide", kv, q, pma, 0)
    # the column kernel has no such limit (a thread per channel, strided): five trips of its channel loops
    _check("d1025 N3", "column", _launch("column", kv, q, pma, 0), _reference((1025, 3), kv, q, pma), q, pma, 0)


@pytest.mark.parametrize("form", ["advance", "column_advance", "column_advance_wide"])
def test_synth_advance_feeds_the_frame_back_where_documented(form):
    """ssv_synth_advance: mel_in[b][f][col + 1] = y[b][f][col]; ssv_synth_column_advance: Y[:, :, t] = y_cur and mel_cur = y_cur;
    ssv_synth_column_advance_wide: frame t of Y (T, F, Bw) = y_cur (F, Bw) and mel_cur = y_cur.  Each then adds one to the counter.  At the
    last frame (and, for the column forms, one past it) nothing lands outside the buffers: they are views into sentinel-filled allocations."""
    B, F, T = 5, 83, 6                          # 415 rows: two workgroups, the second partly idle
    gen = torch.Generator().manual_seed(9)
    for t in ((0, T - 2, T - 1) if form == "advance" else (0, T - 1, T)):
        cnt = torch.tensor([t], dtype=torch.int32, device=DEV)
        if form == "advance":
            y = torch.randn(B, F, T, generator=gen).to(DEV)
            big, mel_in = _guarded((B, F, T))
            _call("ssv_synth_advance", P(y), P(mel_in), P(cnt), B, F, T, _st())
            torch.cuda.synchronize()
            want = torch.full((B, F, T), SENT, device=DEV)
            if t + 1 < T:
                want[:, :, t + 1] = y[:, :, t]
            assert bool(torch.equal(mel_in, want)), t
        else:
            shape = (B, F) if form == "column_advance" else (F, B)
            y_cur = torch.randn(shape, generator=gen).to(DEV)
            big, Y = _guarded((B, F, T) if form == "column_advance" else (T, F, B))
            big2, mel_cur = _guarded(shape)
            if form == "column_advance":
                _call("ssv_synth_column_advance", P(y_cur), P(Y), P(mel_cur), P(cnt), B, F, T, _st())
            else:
                _call("ssv_synth_column_advance_wide", P(y_cur), P(Y), P(mel_cur), P(cnt), B, F, T, _st())
            torch.cuda.synchronize()
            want = torch.full_like(Y, SENT)
            if t < T:
                if form == "column_advance":
                    want[:, :, t] = y_cur
                else:
                    want[t] = y_cur
            assert bool(torch.equal(Y, want)), t
            assert bool(torch.equal(mel_cur, y_cur)) and _guards_intact(big2), t
        assert _guards_intact(big), t
        assert int(cnt[0]) == t + 1
