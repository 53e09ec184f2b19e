"""Text2Mel's text path against float64, operator by operator (references: tests/_attention_ref.py): ops.text_embed forward and backward
(embed_fwd_kernel; embed_bwd_kernel with its 128 private rows of vocabulary bins in LDS, its eight-positions-in-flight loop and the tail
of B N mod 1024 positions behind it) and ops.guided_att_loss value and gradient (one pass below 1024 x 256 elements, a grid-stride loop
above; a weight matrix wider than the attention).  So far only the model goldens ran them, at one vocabulary and the configured lengths.

Bars: ten times what the float32 restatement of the same formula loses against float64 on the same input, at least 4 float32 ulp of the
peak.  Figures: profiles/attention_paths_accuracy.txt (`pytest -m gpu -s` prints them)."""
import numpy as np
import pytest
import torch

import _attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP4 = 4 * 2.0 ** -23


def _err(got, want):
    """Largest absolute error as a share of the peak of ``want`` (absolute where the reference is all zero)."""
    want = np.asarray(want, dtype=np.float64)
    peak = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / (peak if peak > 0 else 1.0)


def _ids(kind, rng, B, N, V):
    if kind == "uniform":
        return rng.integers(0, V, size=(B, N))
    if kind == "all_equal":                    # one bin receives every position
        return np.full((B, N), V - 1)
    if kind == "some_unused":                  # only even ids (only id 0 when V = 1): the odd rows of dw are exactly 0
        return 2 * rng.integers(0, (V + 1) // 2, size=(B, N))
    assert kind == "out_of_range"              # -1 and V among them: bias only in the forward, absent from dw, present in dbias
    ids = rng.integers(-1, V + 1, size=(B, N))
    ids[0, 0] = -1
    ids[-1, -1] = V if B * N > 1 else -1
    return ids


def _bwd_loops(tot):
    """The two loops of embed_bwd_kernel, restated: 128 threads; eight positions (128 apart) per trip of the unrolled body, then one by one.
    Returns (some thread runs the body, some thread runs the tail)."""
    body = tail = False
    for tid in range(128):
        i = tid
        while i + 7 * 128 < tot:
            body, i = True, i + 8 * 128
        tail = tail or i < tot
    return body, tail


def _embed(ids, w, bias, dy):
    from spoofsv_amd import ops
    wg, bg = torch.from_numpy(w).to(DEV).requires_grad_(True), torch.from_numpy(bias).to(DEV).requires_grad_(True)
    y = ops.text_embed(torch.from_numpy(ids).to(DEV).unsqueeze(1), wg, bg)
    y.backward(torch.from_numpy(dy).to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), wg.grad.cpu(), bg.grad.cpu()


@pytest.mark.parametrize("kind", ["uniform", "all_equal", "some_unused", "out_of_range"])
@pytest.mark.parametrize("B,N,E,V,what", [(1, 1, 1, 1, "one-position"), (3, 17, 16, 34, "tail-only"), (8, 128, 130, 34, "BN=1024:unrolled-body-only"),
                                          (7, 147, 16, 64, "BN=1029:unrolled-body-and-tail,V-at-the-cap"), (2, 5, 3, 34, "fewer-positions-than-threads")])
def test_text_embed_forward_and_backward_vs_float64(B, N, E, V, what, kind):
    assert _bwd_loops(B * N) == {"one-position": (False, True), "tail-only": (False, True), "fewer-positions-than-threads": (False, True),
                                 "BN=1024:unrolled-body-only": (True, False), "BN=1029:unrolled-body-and-tail,V-at-the-cap": (True, True)}[what]
    rng = np.random.default_rng(100 * N + V)
    ids = _ids(kind, rng, B, N, V)
    w, bias = rng.standard_normal((E, V)).astype(np.float32), rng.standard_normal(E).astype(np.float32)
    dy = rng.standard_normal((B, E, N)).astype(np.float32)
    y, dw, db = _embed(ids, w, bias, dy)
    y2, dw2, db2 = _embed(ids, w, bias, dy)
    y64, (dw64, db64) = R.text_embed(ids, w, bias), R.text_embed_grads(ids, dy, V)
    y32, (dw32, db32) = R.text_embed(ids, w, bias, np.float32), R.text_embed_grads(ids, dy, V, np.float32)
    rows = []
    for name, got, want, stick in (("y", y, y64, y32), ("dw", dw, dw64, dw32), ("dbias", db, db64, db32)):
        err, bar = _err(got.numpy(), want), max(10 * _err(stick, want), ULP4)
        rows.append((name, err, bar))
        print("TEXT  embed %-13s (%d,%d,%d,%d) %-5s err %.2e (bar %.2e, float32 %.2e)" % (kind, B, N, E, V, name, err, bar, _err(stick, want)))
    for name, err, bar in rows:
        assert err <= bar, (name, err, bar)
    used = np.zeros(V, dtype=bool)
    used[ids[(ids >= 0) & (ids < V)]] = True
    assert bool((dw[:, torch.from_numpy(~used)] == 0).all()), "a vocabulary row nobody used has a gradient"
    if kind == "some_unused" and V > 1:
        assert not used[1::2].any()
    if kind == "out_of_range":
        out = torch.from_numpy((ids < 0) | (ids >= V))
        assert bool(out.any()) and bool(torch.equal(y.permute(0, 2, 1)[out], torch.from_numpy(bias).expand(int(out.sum()), E)))
    assert bool(torch.equal(y, y2)) and bool(torch.equal(dw, dw2)) and bool(torch.equal(db, db2)), "two runs differ"


def test_text_embed_backward_refuses_a_vocabulary_above_its_bins():
    from spoofsv_amd import ops
    rng = np.random.default_rng(0)
    w = torch.from_numpy(rng.standard_normal((4, 65)).astype(np.float32)).to(DEV).requires_grad_(True)
    bias = torch.zeros(4, device=DEV, requires_grad=True)
    ids = torch.from_numpy(rng.integers(0, 65, size=(2, 1, 9))).to(DEV)
    y = ops.text_embed(ids, w, bias)            # the forward has no such limit
    assert _err(y.detach().cpu().numpy(), R.text_embed(ids[:, 0].cpu().numpy(), w.detach().cpu().numpy(), np.zeros(4))) <= ULP4
    with pytest.raises(RuntimeError, match="vocabulary 65"):
        y.sum().backward()


@pytest.mark.parametrize("B,N,T,gaw_T,what", [(1, 1, 1, 1, "one-pass"), (3, 17, 33, 40, "one-pass,gaw_T>T"), (2, 186, 325, 325, "one-pass"),
                                               (5, 186, 325, 400, "grid-stride,gaw_T>T")])
def test_guided_att_loss_value_and_gradient_vs_float64(B, N, T, gaw_T, what):
    from spoofsv_amd import ops, train
    assert ("grid-stride" in what) == (B * N * T > 1024 * 256) and ("gaw_T>T" in what) == (gaw_T > T)
    rng = np.random.default_rng(N + T)
    A = rng.random((B, N, T)).astype(np.float32)
    A /= A.sum(axis=1, keepdims=True)           # columns that sum to 1, as an attention's do
    gaw = train.guided_attention_mat(N + 3, gaw_T).numpy().astype(np.float32) if gaw_T > 1 else np.full((4, 1), 0.75, dtype=np.float32)
    assert gaw.shape == (N + 3, gaw_T)
    gout = np.float32(1.7)
    got = []
    for _ in range(2):
        a = torch.from_numpy(A).to(DEV).requires_grad_(True)
        loss = ops.guided_att_loss(a, torch.from_numpy(gaw).to(DEV))
        (loss * float(gout)).backward()
        torch.cuda.synchronize()
        got.append((loss.detach().cpu(), a.grad.cpu()))
    l64, g64 = R.guided_att_loss(A, gaw)
    l32, g32 = R.guided_att_loss(A, gaw, np.float32)
    g64, g32 = g64 * float(gout), g32 * gout
    e_l, bar_l = abs(float(got[0][0]) - l64) / abs(l64), max(10 * abs(float(l32) - l64) / abs(l64), ULP4)
    e_g, bar_g = _err(got[0][1].numpy(), g64), max(10 * _err(g32, g64), ULP4)
    print("TEXT  guided_att_loss (%d,%d,%d,%d) %-20s loss %.2e (bar %.2e)  gradient %.2e (bar %.2e)" % (B, N, T, gaw_T, what, e_l, bar_l, e_g, bar_g))
    assert e_l <= bar_l, (e_l, bar_l)
    assert e_g <= bar_g, (e_g, bar_g)
    assert bool(torch.equal(got[0][0], got[1][0])) and bool(torch.equal(got[0][1], got[1][1])), "two runs differ"
