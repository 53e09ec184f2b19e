"""CPU checks of tests/_attention_ref.py, the references of the attention-path, synthesis-step and text-path GPU tests: every numpy
restatement against a plain torch float64 expression of the same formula, the inputs the step tests are built from (how many items the
index comparison leaves out, what the tie cases tie), and the branch that every row of the training-attention table claims."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _attention_ref as R


@pytest.mark.parametrize("B,d,N,T", [(2, 3, 5, 4), (3, 64, 17, 33), (1, 32, 300, 2), (2, 1, 1, 1)])
def test_train_attention_is_softmax_of_scaled_scores_then_v_a_over_q(B, d, N, T):
    rng = np.random.default_rng(7 + N)
    kv, q = rng.standard_normal((B, 2 * d, N)), rng.standard_normal((B, d, T))
    a, rq = R.train_attention(kv, q)
    kvt, qt = torch.from_numpy(kv), torch.from_numpy(q)
    a_t = torch.softmax(torch.matmul(kvt[:, :d].transpose(1, 2), qt) / d ** 0.5, dim=1)
    rq_t = torch.cat((torch.matmul(kvt[:, d:], a_t), qt), dim=1)
    assert a.shape == (B, N, T) and rq.shape == (B, 2 * d, T)
    assert np.abs(a - a_t.numpy()).max() < 1e-14 and np.abs(rq - rq_t.numpy()).max() < 1e-13
    assert np.abs(a.sum(axis=1) - 1).max() < 1e-14
    a32, rq32 = R.train_attention(kv, q, np.float32)
    assert a32.dtype == np.float32 and rq32.dtype == np.float32 and np.abs(a32 - a).max() < 1e-5


@pytest.mark.parametrize("d,N", [(1, 1), (3, 2), (6, 5), (37, 257), (64, 600)])
def test_step_attention_is_the_windowed_softmax_first_argmax_and_v_a(d, N):
    kv, q, pma = R.step_case(d, N, 16)
    assert list(pma[:len(R.fixed_windows(N))]) == R.fixed_windows(N) and pma.min() >= 0 and pma.max() < N
    for b in range(16):
        K, V = torch.from_numpy(kv[b, :d]).double(), torch.from_numpy(kv[b, d:]).double()
        s = (K.t() @ torch.from_numpy(q[b]).double()) / d ** 0.5
        for n in range(N):                                     # the window, position by position
            if not (pma[b] <= n <= pma[b] + 2):
                s[n] = -2.0 ** 32
        a_t = torch.softmax(s, dim=0)
        first = min(n for n in range(N) if a_t[n] == a_t.max())
        a, idx, r = R.step_attention(kv[b, :d], kv[b, d:], q[b], int(pma[b]))
        assert a.dtype == np.float64 and np.abs(a - a_t.numpy()).max() < 1e-14
        assert idx == first and pma[b] <= idx <= min(pma[b] + 2, N - 1)
        assert np.abs(r - (V @ a_t).numpy()).max() < 1e-12
        outside = np.array([not (pma[b] <= n <= pma[b] + 2) for n in range(N)])
        assert np.all(a[outside] == 0.0) and abs(a.sum() - 1) < 1e-14
        a32, idx32, r32 = R.step_attention(kv[b, :d], kv[b, d:], q[b], int(pma[b]), np.float32)
        assert a32.dtype == np.float32 and r32.dtype == np.float32 and np.all(a32[outside] == 0.0)
    ab, ib, rb = R.step_attention_batch(kv, q, pma)
    assert np.array_equal(ab[15], a) and ib[15] == idx and np.array_equal(rb[15], r)


@pytest.mark.parametrize("d,N", R.STEP_CASES)
def test_step_cases_leave_out_at_most_one_item_in_64_and_float32_is_a_usable_stick(d, N):
    """The GPU test drops an item from the index comparison when its float64 top-two gap is under 1e-4 and caps that at one item per case: the
    reference alone must keep to the cap with the seeds used.  The float32 restatement agrees on the index of every item kept, and its error
    is the size the tolerances assume (some 1e-7)."""
    kv, q, pma = R.step_case(d, N)
    a, idx, r = R.step_attention_batch(kv, q, pma)
    gap = R.top_two_gap(a)
    left_out = gap < R.GAP_MIN
    assert int(left_out.sum()) <= 1, (d, N, int(left_out.sum()))
    a32, idx32, r32 = R.step_attention_batch(kv, q, pma, np.float32)
    assert np.array_equal(idx32[~left_out], idx[~left_out])
    assert np.abs(a32 - a).max() < 2e-6 and np.abs(r32 - r).max() / np.abs(r).max() < 2e-6


def test_top_two_gap():
    a = np.array([[0.2, 0.5, 0.3], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0]])
    assert np.allclose(R.top_two_gap(a), [0.2, 0.0, 1.0]) and np.allclose(R.top_two_gap(np.array([[1.0]])), [1.0])


@pytest.mark.parametrize("d,N", R.TIE_CASES)
def test_tie_cases_tie_exactly_at_the_window_maximum_and_the_lower_index_wins(d, N):
    kv, q, pma, ntied = R.tie_case(d, N)
    want = sorted(N + p if p < 0 else p for p in R.TIE_POSITIONS)
    assert sorted(set(pma.tolist())) == want and set(ntied.tolist()) == {2, 3}
    for dtype in (np.float64, np.float32):
        a, idx, _ = R.step_attention_batch(kv, q, pma, dtype)
        for b in range(len(pma)):
            p, k = int(pma[b]), int(ntied[b])
            assert np.array_equal(kv[b, :d, p + 1], kv[b, :d, p])
            assert len(set(a[b, p:p + k].tolist())) == 1 and a[b, p] == a[b].max() and idx[b] == p
            if p + k < min(p + 3, N):
                assert a[b, p + k] < a[b, p]


@pytest.mark.parametrize("B,N,E,V", [(1, 1, 1, 1), (3, 17, 16, 34), (2, 5, 3, 34)])
def test_text_embed_is_one_hot_times_w_transposed_plus_bias(B, N, E, V):
    rng = np.random.default_rng(3)
    ids = rng.integers(-1, V + 1, size=(B, N))                       # -1 and V: no one-hot row
    w, bias, dy = rng.standard_normal((E, V)), rng.standard_normal(E), rng.standard_normal((B, E, N))
    wt, bt = torch.from_numpy(w).requires_grad_(True), torch.from_numpy(bias).requires_grad_(True)
    idt = torch.from_numpy(ids)
    inside = (idt >= 0) & (idt < V)
    onehot = F.one_hot(torch.where(inside, idt, torch.full_like(idt, V)), V + 1)[..., :V].double()      # (B, N, V)
    y_t = (onehot @ wt.t() + bt).transpose(1, 2)
    (y_t * torch.from_numpy(dy)).sum().backward()
    y = R.text_embed(ids, w, bias)
    dw, db = R.text_embed_grads(ids, dy, V)
    assert y.shape == (B, E, N) and np.abs(y - y_t.detach().numpy()).max() < 1e-15
    assert np.abs(dw - wt.grad.numpy()).max() < 1e-13 and np.abs(db - bt.grad.numpy()).max() < 1e-13
    unused = [v for v in range(V) if not (ids == v).any()]
    assert np.all(dw[:, unused] == 0.0)
    assert R.text_embed(ids, w, bias, np.float32).dtype == np.float32 and R.text_embed_grads(ids, dy, V, np.float32)[0].dtype == np.float32


@pytest.mark.parametrize("B,N,T,gaw_T", [(1, 1, 1, 1), (3, 17, 33, 40), (2, 20, 9, 9)])
def test_guided_att_loss_is_the_mean_of_a_times_the_weight_corner(B, N, T, gaw_T):
    rng = np.random.default_rng(5)
    A, gaw = rng.random((B, N, T)), rng.random((N + 2, gaw_T))
    At = torch.from_numpy(A).requires_grad_(True)
    loss_t = (At * torch.from_numpy(gaw)[:N, :T]).mean()
    loss_t.backward()
    loss, grad = R.guided_att_loss(A, gaw)
    assert abs(loss - float(loss_t.detach())) < 1e-15 and grad.shape == A.shape and np.abs(grad - At.grad.numpy()).max() < 1e-18
    l32, g32 = R.guided_att_loss(A, gaw, np.float32)
    assert l32.dtype == np.float32 and g32.dtype == np.float32


def test_training_cases_reach_the_branches_they_name_and_cover_what_was_untested():
    ids = [R.train_case_id(c) for c in R.TRAIN_CASES]
    assert len(set(ids)) == len(ids)
    for case in R.TRAIN_CASES:
        assert [R.check_train_case(case, m) == "fp32" for m in (0, 1, 2)] == [True] + [case[1] != "split"] * 2
    paths = {c[0] for c in R.TRAIN_CASES}
    assert {"fallback:tile8", "fallback:tile24", "fallback:tile32", "fallback:percol"} <= paths
    fused = {R.fused_instance(c[3], c[4]) for c in R.TRAIN_CASES if c[0].startswith("fused")}
    every = {(nb, db) for nb in (1, 2, 3) for db in (1, 2, 3, 4)}
    assert fused == every - R.FUSED_TESTED_BEFORE and len(fused) == 7
    for path in paths:                                              # each path meets both dK / dV branches of the split modes
        assert {c[1] == "split" for c in R.TRAIN_CASES if c[0].split("(")[0] == path.split("(")[0]} == {True, False}, path
    ts = {c[5] for c in R.TRAIN_CASES if c[0].startswith("fallback")}
    assert {1, 31, 32, 33, 65} <= ts
    for c in R.TRAIN_CASES:
        if c[0].startswith("fused"):
            assert (c[5] + 1) % R.AF_BN == 0 or (c[5] - 1) % R.AF_BN == 0
    assert {c[4] for c in R.TRAIN_CASES if c[0].startswith("fused")} >= {64, 65, 128, 129}     # the edges of NB
    # the thresholds themselves
    assert R.fused_ok(2, 256, 192, 5) and not R.fused_ok(2, 256, 193, 5) and not R.fused_ok(2, 320, 100, 5) and not R.fused_ok(2, 32, 17, 5)
    assert [R.softmax_branch(2, n, 3) for n in (64, 65, 192, 193, 256, 257)] == ["tile8", "tile24", "tile24", "tile32", "tile32", "percol"]
    assert [R.fused_instance(64, n)[0] for n in (1, 64, 65, 128, 129, 192)] == [1, 1, 2, 2, 3, 3]
