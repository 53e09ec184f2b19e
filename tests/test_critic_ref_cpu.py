"""CPU checks of tests/_critic_ref.py, the references of tests/test_gpu_critic_ops.py: the Philox4x32-10 restatement against the
published Random123 known answers, the critic restatement against oracle/critic_oracle.py, the distance of the committed cases from
every leaky-ReLU kink, and the side of each kernel-choice threshold that the rows of the convolution shape table claim."""
import numpy as np
import pytest
import torch

import _critic_ref as R
from oracle import critic_oracle as CO


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want
    # and vectorised: the same answer in every lane of an array-valued counter
    lanes = R.philox4x32_10([np.full(5, v, dtype=np.uint32) for v in counter], key)
    assert all(np.array_equal(v, np.full(5, w, dtype=np.uint32)) for v, w in zip(lanes, want))


def test_dropout_reference_uses_counter_call_and_seed_as_the_kernel_does():
    """Element 4 * i4 + q reads word q of Philox((i4, 0, call lo, call hi), (seed, 0x5f3759df)); the threshold is uint32(p * 2^32) of the
    float32 p; kept values are scaled by the float32 1 / (1 - p)."""
    n, p, seed, call = 23, 0.25, 1234, (1 << 32) + 5
    drops = R.dropout_drops(n, p, seed, call)
    thr = R.dropout_threshold(p)
    assert thr == 1 << 30 and R.dropout_threshold(0.05) == int(float(np.float32(0.05)) * 2.0 ** 32) == 214748368
    for i in (0, 5, 22):
        words = R.philox4x32_10((i // 4, 0, 5, 1), (seed, 0x5F3759DF))
        assert bool(drops[i]) == (int(words[i % 4]) < thr)
    assert not np.array_equal(drops, R.dropout_drops(n, p, seed, 5)) and not np.array_equal(drops, R.dropout_drops(n, p, seed + 1, call))
    x = np.linspace(-2, 2, n).astype(np.float32)
    d, y = R.act_dropout_ref(x, 0.05, p, seed, call)
    assert d.dtype == np.float32 and y.dtype == np.float32
    inv = np.float32(1) / np.float32(0.75)
    assert set(np.unique(d).tolist()) <= {0.0, float(inv), float(np.float32(0.05) * inv)} and np.array_equal(y, x * d)
    d0, y0 = R.act_dropout_ref(x, 0.05, 0.0, seed, call)
    assert np.array_equal(y0, np.where(x > 0, x, x * np.float32(0.05)))


@pytest.mark.parametrize("kind", ["mel", "lin"])
def test_critic_restatement_equals_the_oracle_in_float64(kind):
    sd, real, fake, eps, masks = R.critic_case(kind)
    sd = {k: v.double() for k, v in sd.items()}
    assert len(masks) == 9 and sum(int((m == 0).sum()) for m in masks) > 0
    for x, m in ((real.double(), False), (fake.double(), [t.double() for t in masks[:3]])):
        got, kinks = R.critic_with_kink_inputs(x, sd, kind, m)
        want = CO.critic(x, sd, kind, masks=m)
        assert torch.equal(got, want)
        assert len(kinks) == 3 and got.shape == (x.shape[0], 1, 1)


@pytest.mark.parametrize("kind", ["mel", "lin"])
def test_committed_critic_seeds_keep_clear_of_every_leaky_relu_kink(kind):
    sd, real, fake, eps, masks = R.critic_case(kind)
    for m in (False, masks):
        margin = R.critic_kink_margins(sd, kind, real, fake, eps, m)
        print("%s %s: closest leaky-ReLU input at %.2e of its tensor's rms" % (kind, "eval" if m is False else "train", margin))
        assert margin > R.KINK_MARGIN, (kind, m is not False, margin)


def test_conv_shape_table_rows_sit_on_the_side_of_each_threshold_they_claim():
    """A later change of SSV_MIN_SPLIT_CHANNELS, of the B * L >= 128 rule or of the weight gradient's B * L >= 256 must not silently move a
    row of the table onto another kernel: ops._tiny_conv / ops._bf3_shape decide whether scale lists travel, the library's own predicate
    (ssv_conv1d_bwd_weight_multi_ok, the weight-gradient rule for dense operands) which weight-gradient kernel runs."""
    from spoofsv_amd import _lib, ops
    L_ = _lib.lib()
    prev = L_.ssv_set_precision(2)
    try:
        for (B, Cin, Cout, L, k, d, causal), split, wsplit, _ in R.CONV_SHAPES:
            x = torch.empty(B, Cin, L)
            assert (ops._bf3_shape(x) and not ops._tiny_conv(Cin, Cout)) == split, (B, Cin, Cout, L)
            assert bool(L_.ssv_conv1d_bwd_weight_multi_ok(B, Cin, Cout, L, k)) == wsplit, (B, Cin, Cout, L)
            assert wsplit == (split and B * L >= 256), (B, Cin, Cout, L)
        L_.ssv_set_precision(0)
        assert not any(L_.ssv_conv1d_bwd_weight_multi_ok(s[0], s[1], s[2], s[3], s[4]) for s, _, _, _ in R.CONV_SHAPES)
    finally:
        L_.ssv_set_precision(prev)
    shapes = {s: (a, b) for s, a, b, _ in R.CONV_SHAPES}
    # the rows that exist FOR a threshold sit exactly on it / one below it
    assert shapes[(2, 32, 32, 64, 3, 1, False)] == (True, False) and 2 * 64 == 128 and not ops._tiny_conv(32, 32) and ops._tiny_conv(31, 32)
    assert shapes[(2, 32, 32, 63, 3, 1, False)] == (False, False) and not ops._bf3_shape(torch.empty(2, 32, 63))
    assert shapes[(2, 64, 16, 131, 1, 1, False)] == (False, False) and ops._tiny_conv(64, 16) and ops._bf3_shape(torch.empty(2, 64, 131))
    assert 256 <= 2 * 131 < 256 + 8
    assert sorted(c for c in R.CONV_CASES if c[1] == "spread") == sorted((s, "spread") for s in list(shapes)[:2] + list(shapes)[3:4])


def test_gp_operand_has_the_two_special_items_exactly():
    g = R.gp_operand(3, 592)
    assert float(g[0].abs().max()) == 0.0 and float((g[1] * g[1]).sum()) == 1.0 and float(g[1].double().norm()) == 1.0
    loss, dg = R.gp_ref(g, 10.0)
    assert torch.isfinite(dg).all() and float(dg[0].abs().max()) == 0.0 and float(dg[1].abs().max()) == 0.0
    nrm2 = float(g[2].double().norm())
    assert float(loss) == pytest.approx((10.0 + 0.0 + 10.0 * (nrm2 - 1) ** 2) / 3, rel=1e-12)
