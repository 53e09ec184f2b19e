"""Training attention (ops.attention_train: ssv_attention_train_fwd_rq / _bwd, csrc/api_attn.hip) against float64 on EVERY branch of its
dispatch, in the three arithmetic modes -- tests/test_gpu_accuracy.py holds it to float64 only at shapes the fused kernels take, five of
their twelve instantiations:

  * the fallback chain (general product, column softmax, V A, row copy; backward likewise) with each of its softmax kernels:
    softmax_cols_tile_kernel<8 | 24 | 32> at both ends of their ranges of N, and the per-column kernels for N > 256;
  * the seven (NB, DB) instantiations of the fused kernels that nothing ran, at the edges of NB (N = 64, 65, 128, 129) and with T one
    column short of / past a whole number of their 64-column tiles;
  * dK and dV (nt_per_batch) on the exact fp32 kernel and on the split-MFMA kernel, by B T < 256 / >= 256 at one shape, and at a shape
    ssv_nt_bf3_fits rejects (rows of 7 frames);
  * q as a batch-strided view, which ops._act3 passes on without a copy (its rows are contiguous; only the batch stride is larger).

The table (tests/_attention_ref.py: TRAIN_CASES) names the branch of every row; the dispatch rules are restated there in Python and each
test first asserts that its row reaches what its id says.  Bars: those of the fused test (A 2e-5 of the peak, rq 2e-6 and gradients 5e-6
relative L2) in fp32 and f16x2; in bf16x3 dK | dV are held to the 2e-5 of the bf16x3 weight-gradient kernel, the rest to the fp32 bars.
Figures: profiles/attention_paths_accuracy.txt (`pytest -m gpu -s` prints them)."""
import numpy as np
import pytest
import torch

import _attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = {"fp32": 0, "bf16x3": 1, "f16x2": 2}
A_BAR, RQ_BAR, GRAD_BAR, BF3_BAR = 2e-5, 2e-6, 5e-6, 2e-5
_REF = {}


@pytest.fixture(params=["f16x2", "bf16x3", "fp32"])
def precision(request):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(request.param)
    yield request.param
    spoofsv_amd.set_precision(prev)


def _rl2(got, want):
    want = torch.as_tensor(want)
    return float((got.detach().double().cpu() - want).norm() / want.norm())


def _reference(case):
    """Inputs and the float64 forward (numpy restatement) and gradients (torch autograd over the same formula), once per case."""
    if case in _REF:
        return _REF[case]
    _, _, B, d, N, T, _ = case
    gen = torch.Generator().manual_seed(1000 * d + 7 * N + T)
    kv = torch.randn(B, 2 * d, N, generator=gen)
    q = torch.randn(B, d, T, generator=gen)
    g_rq = torch.randn(B, 2 * d, T, generator=gen)
    g_a = torch.randn(B, N, T, generator=gen) * 0.1
    a_ref, rq_ref = R.train_attention(kv.numpy(), q.numpy())
    kvr, qr = kv.double().requires_grad_(True), q.double().requires_grad_(True)
    a_t = torch.softmax(torch.matmul(kvr[:, :d].transpose(1, 2), qr) / d ** 0.5, dim=1)
    rq_t = torch.cat((torch.matmul(kvr[:, d:], a_t), qr), dim=1)
    (rq_t * g_rq.double()).sum().add((a_t * g_a.double()).sum()).backward()
    _REF[case] = (kv, q, g_rq, g_a, a_ref, rq_ref, kvr.grad, qr.grad)
    return _REF[case]


def _run(kv, q, g_rq, g_a, view):
    from spoofsv_amd import ops
    B, d, T = q.shape
    kvg = kv.to(DEV).requires_grad_(True)
    if view:          # rows of a larger (B, d + 3, T) tensor: every row contiguous, the batch stride (d + 3) T
        big = torch.full((B, d + 3, T), float("nan"), device=DEV)
        big[:, :d] = q.to(DEV)
        big.requires_grad_(True)
        qg = big[:, :d]
        assert not qg.is_contiguous() and ops._act3(qg)[0].data_ptr() == qg.data_ptr() and ops._act3(qg)[1] == (d + 3) * T
    else:
        big = qg = q.to(DEV).requires_grad_(True)
    rq, a = ops.attention_train(kvg, qg)
    ((rq * g_rq.to(DEV)).sum() + (a * g_a.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    dq = big.grad[:, :d] if view else big.grad
    return a.detach(), rq.detach(), kvg.grad, dq


@pytest.mark.parametrize("case", R.TRAIN_CASES, ids=R.train_case_id)
def test_attention_train_every_dispatch_branch_vs_float64(case, precision):
    from spoofsv_amd import _lib
    path, nt, B, d, N, T, view = case
    assert _lib.precision() == MODES[precision]
    dkdv = R.check_train_case(case, MODES[precision])            # the row reaches the branch its id names
    kv, q, g_rq, g_a, a_ref, rq_ref, dkv_ref, dq_ref = _reference(case)
    a, rq, dkv, dq = _run(kv, q, g_rq, g_a, view)
    a2, rq2, dkv2, dq2 = _run(kv, q, g_rq, g_a, view)
    a64 = a.double().cpu().numpy()
    err_a = float(np.abs(a64 - a_ref).max() / np.abs(a_ref).max())
    err_rq, err_dkv, err_dq = _rl2(rq, rq_ref), _rl2(dkv, dkv_ref), _rl2(dq, dq_ref)
    err_dk, err_dv = _rl2(dkv[:, :d], dkv_ref[:, :d]), _rl2(dkv[:, d:], dkv_ref[:, d:])
    kv_bar = BF3_BAR if precision == "bf16x3" else GRAD_BAR
    print("TRAIN %-6s %-58s dkdv %-6s  A %.2e  rq %.2e  dkv %.2e (dk %.2e dv %.2e; bar %.0e)  dq %.2e"
          % (precision, R.train_case_id(case), dkdv, err_a, err_rq, err_dkv, err_dk, err_dv, kv_bar, err_dq))
    assert np.isfinite(a64).all() and float(np.abs(a64.sum(axis=1) - 1).max()) < 1e-6, float(np.abs(a64.sum(axis=1) - 1).max())
    assert bool(torch.equal(rq[:, d:].cpu(), q)), "the Q half of cat(R, Q) is a copy"
    assert err_a < A_BAR, err_a
    assert err_rq < RQ_BAR, err_rq
    assert err_dkv < kv_bar, (err_dkv, err_dk, err_dv)
    assert err_dq < GRAD_BAR, err_dq
    for name, x, y in (("A", a, a2), ("rq", rq, rq2), ("dkv", dkv, dkv2), ("dq", dq, dq2)):
        assert bool(torch.equal(x, y)), name + " differs between two calls"
