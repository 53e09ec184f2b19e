"""tests/_conv_tiles_ref.py pinned without a device: the float64 reference of the Conv1d forward and data gradient against
torch.nn.functional.conv1d and autograd, the tables of tests/test_gpu_conv_tiles.py against the restated dispatch (every row names the
instantiation it is listed under, all 27 forms occur, the natural rows are what the search over the box finds), and the constant the
per-element bars are derived from against the float32 numpy evaluation of every row."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_tiles_ref as R

SPLIT_MODES = ("f16x2", "bf16x3")


@pytest.mark.parametrize("k,d,causal", [(1, 1, 0)] + [(3, d, c) for d in (1, 8, 9, 27) for c in (0, 1)])
def test_reference_equals_torch_conv1d_and_autograd_in_float64(k, d, causal):
    """Every (k, dilation, causal) of the tables, at a length shorter than the widest halo (L = 31 < 54: taps leave the row at both ends)
    and a longer one."""
    for B, Cin, Cout, L in ((2, 5, 7, 31), (3, 4, 6, 70)):
        rng = np.random.default_rng([k, d, causal, L])
        x, w = rng.standard_normal((B, Cin, L)), rng.standard_normal((Cout, Cin, k))
        bias, bias_b = rng.standard_normal(Cout), rng.standard_normal((B, Cout))
        dy, dx_add = rng.standard_normal((B, Cout, L)), rng.standard_normal((B, Cin, L))
        sh = R.conv_shifts(k, d, causal)
        y, S = R.conv_fwd(x, w, bias, bias_b, sh)
        dx, Sdx = R.conv_dgrad(dy, w, dx_add, sh)
        xt = torch.from_numpy(x).requires_grad_(True)
        left = (k - 1) * d if causal else (k - 1) * d // 2
        yt = F.conv1d(F.pad(xt, (left, (k - 1) * d - left)), torch.from_numpy(w), torch.from_numpy(bias), dilation=d)
        yt.backward(torch.from_numpy(dy))
        want_y = yt.detach().numpy() + bias_b[:, :, None]
        want_dx = xt.grad.numpy() + dx_add
        assert np.abs(y - want_y).max() <= 1e-12 * np.abs(want_y).max()
        assert np.abs(dx - want_dx).max() <= 1e-12 * np.abs(want_dx).max()
        assert (S >= np.abs(y) * (1 - 1e-12)).all() and (Sdx >= np.abs(dx) * (1 - 1e-12)).all()
        # S is the same sum over absolute values
        Sw = R.conv_fwd(np.abs(x), np.abs(w), np.abs(bias), np.abs(bias_b), sh)[0]
        assert np.abs(S - Sw).max() <= 1e-14 * S.max()


def test_column_statistics_of_the_reference():
    y = np.random.default_rng(3).standard_normal((2, 128, 9))
    cs = R.colstats(y)
    assert cs.shape == (2, 2, 9, 2)
    assert np.allclose(cs[1, 1, 4, 0], y[1, 64:, 4].mean()) and np.allclose(cs[1, 1, 4, 1], y[1, 64:, 4].var() * 64)


def test_shift_table_is_conv_shifts():
    assert R.conv_shifts(1, 1, 0) == [0] and R.conv_shifts(3, 1, 0) == [-1, 0, 1]
    assert R.conv_shifts(3, 27, 1) == [-54, -27, 0] and R.conv_shifts(3, 9, 0) == [-9, 0, 9]


@pytest.mark.parametrize("row", R.TILE_CASES + R.WIDE_CASES, ids=R.row_id)
def test_every_row_names_the_instantiation_in_its_id(row):
    for mode in SPLIT_MODES:
        assert R.predicted(row, mode) == R.kernel_of(row.form, mode), (R.predicted(row, mode), R.kernel_of(row.form, mode))
    assert R.predicted(row, "fp32") is None
    if row.form[0] == "plain":
        _, kt, wm, nt, halo = row.form
        assert row.forced == (wm, nt) and row.kt == kt
        assert halo == (R.HALO_SMALL if (kt == 3 and R.span_of(kt, row.d) <= R.HALO_SMALL) else 54)
        assert row.colstats == (row.M == 128 * wm) and (not row.colstats or row.M % 64 == 0)
        if row.colstats:                                  # asking for the statistics does not move the row to another program
            assert R.pick_tile(kt, row.B, row.M, row.N, row.K, True, row.forced, R.span_of(kt, row.d)) == R.kernel_of(row.form, "f16x2")
    else:
        assert row.forced is None and row.kt == 1


def test_all_24_plain_and_3_wide_forms_occur_with_their_edges():
    assert len(R.PLAIN_FORMS) == 24 and len(R.WIDE_FORMS) == 3 and len(set(R.FORMS)) == 27
    assert {r.form for r in R.TILE_CASES} == set(R.PLAIN_FORMS) and {r.form for r in R.WIDE_CASES} == set(R.WIDE_FORMS)
    for form in R.PLAIN_FORMS:
        _, kt, wm, nt, halo = form
        rows = [r for r in R.TILE_CASES if r.form == form]
        BM, BN = 64 * wm, 16 * nt
        assert {r.M for r in rows} == {BM - 15, BM + 1, 2 * BM} and {r.N for r in rows} == {BN - 1, BN + 1, 2 * BN}
        assert {r.K for r in rows} == {40, 96} and all(r.B == max(2, -(-128 // r.N)) for r in rows)
        want = {(1, 0)} if kt == 1 else {(d, c) for d in ((1, 8) if halo == 16 else (9, 27)) for c in (0, 1)}
        assert {(r.d, r.causal) for r in rows} == want
        assert len(rows) == 18 * len(want) == len(set(rows))
    # the halo that leaves the row at both ends at once
    assert any(r.form == ("plain", 3, wm, 2, 54) and r.N == 31 and r.d == 27 for wm in (1, 2) for r in R.TILE_CASES)
    # the force key (kt, M, N) names one tile only: the rows of two forms never share it
    keys = {}
    for r in R.TILE_CASES:
        assert keys.setdefault((r.kt, r.M, r.N), r.forced) == r.forced


def test_wide_rows_are_the_smallest_the_wide_rule_admits():
    for r in [r for r in R.WIDE_CASES if r.N <= 1025]:              # (N = 1345 is there for the ragged 448-column tile: 8 x 192 columns)
        assert R.predicted(r._replace(B=r.B - 1), "f16x2").startswith("gemm_nn_bf3_kernel<"), r
    k1057 = [r for r in R.WIDE_CASES if r.K == 1057]
    assert len(k1057) == 1 and R.predicted(k1057[0], "f16x2") == "gemm_nn_bf3w_kernel<1, 2, 7, 4, 1>"
    assert R.predicted(k1057[0]._replace(K=1056), "f16x2") == "gemm_nn_bf3w_kernel<1, 2, 6, 2, 1, 1>"


def test_natural_rows_are_what_the_search_over_the_box_finds():
    found, forced_only = R.natural_search()
    assert found == R.NATURAL and forced_only == R.FORCED_ONLY
    assert set(R.NATURAL) | set(R.FORCED_ONLY) == set(R.TILES) and len(R.TILES) == 16 and not set(R.NATURAL) & set(R.FORCED_ONLY)
    assert len(R.NATURAL_CASES) == len(R.NATURAL)


@pytest.mark.parametrize("row", R.NATURAL_CASES, ids=R.row_id)
def test_every_natural_row_names_its_tile_unforced(row):
    assert row.forced is None
    for mode in SPLIT_MODES:
        assert R.predicted(row, mode) == R.kernel_of(row.form, mode)
    box = R.NATURAL_BOX
    assert row.B <= box["B"] and row.M <= box["M"] and row.N <= box["N"] and row.K == box["K"]


def test_half_group_rows_stay_on_64_row_tiles_when_they_ask_for_statistics():
    for r in R.HALF_GROUP_CASES:
        span = R.span_of(r.kt, r.d)
        assert r.M % 128 == 64 and r.colstats
        with_stats = R.pick_tile(r.kt, r.B, r.M, r.N, r.K, True, r.forced, span)
        plain = R.pick_tile(r.kt, r.B, r.M, r.N, r.K, False, r.forced, span)
        assert with_stats.startswith("gemm_nn_bf3_kernel<%d, 1, " % r.kt), with_stats
        assert plain.startswith("gemm_nn_bf3_kernel<%d, 2, " % r.kt), "without the statistics the row would run a 128-row tile"
        assert R.f32_error(r) <= R.BAR_F32 / 4


def test_every_row_runs_a_split_kernel():
    for r in R.TILE_CASES + R.WIDE_CASES + R.NATURAL_CASES + R.HALF_GROUP_CASES:
        assert r.B * r.N >= 128 and r.M >= 32 and r.K >= 32, r
    assert sorted(r for f in R.FORMS for r in R.rows_of(f)) == sorted(R.TILE_CASES + R.WIDE_CASES + R.NATURAL_CASES)


def test_the_bars_follow_from_the_float32_constant():
    assert R.BAR_F32 == 4 * R.F32_WORST and R.BAR_F16 == R.BAR_F32 + 2.0 ** -21 and R.BAR_BF3 == 15 * R.BAR_F16
    assert R.BARS == {"fp32": R.BAR_F32, "f16x2": R.BAR_F16, "bf16x3": R.BAR_BF3}
    assert R.L2_BARS == {"fp32": 2e-6, "f16x2": 2e-6, "bf16x3": 3e-5} and R.COLSTATS_BAR == 2e-5


@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
def test_float32_numpy_error_of_every_row_is_a_quarter_of_the_bar(form):
    worst = max(R.f32_error(r) for r in R.rows_of(form))
    print("%-18s float32 numpy worst |err|/S %.3e (BAR_F32 / 4 = %.3e)" % (R.form_id(form), worst, R.BAR_F32 / 4))
    assert 0 < worst <= R.BAR_F32 / 4
