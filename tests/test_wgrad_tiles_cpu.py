"""tests/_wgrad_tiles_ref.py pinned without a device: the float64 reference of the Conv1d weight gradient against float64 autograd of
torch.nn.functional.conv1d, the tables of tests/test_gpu_wgrad_tiles.py against the restated dispatch (every row names the program it is
listed under, every form keeps the edges it is there for), the range-slab partition, the spelling of the predicted shape-log lines, and
the constant the per-element bars are derived from against the float32 numpy evaluation of every row."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _wgrad_tiles_ref as R


def _rows(form):
    rows = R.rows_of(form)
    assert rows, form
    return rows


def test_shift_table_is_conv_shifts():
    assert R.conv_shifts(1, 1, 0) == [0] and R.conv_shifts(3, 3, 0) == [-3, 0, 3] and R.conv_shifts(3, 27, 1) == [-54, -27, 0]


SMALL = [r for r in R.all_rows() if r.Cin * r.Cout <= 130 * 130]


@pytest.mark.parametrize("row", SMALL, ids=R.row_id)
def test_reference_equals_float64_autograd_of_conv1d(row):
    dy, x = R.inputs(row)
    dw, S = R.reference(row)
    k, d = row.k, row.d
    left = (k - 1) * d if row.causal else (k - 1) * d // 2
    w = torch.zeros(row.Cout, row.Cin, k, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(F.pad(torch.from_numpy(x).double(), (left, (k - 1) * d - left)), w, dilation=d)
    y.backward(torch.from_numpy(dy).double())
    want = w.grad.numpy()
    assert dw.shape == want.shape == (row.Cout, row.Cin, k)
    assert np.abs(dw - want).max() <= 1e-12 * np.abs(want).max()
    assert (S > 0).all() and (S >= np.abs(dw) * (1 - 1e-12)).all()
    Sw = R.wgrad(np.abs(dy), np.abs(x), R.conv_shifts(k, d, row.causal))[0]
    assert np.abs(S - Sw).max() <= 1e-14 * S.max()


def test_inputs_do_not_depend_on_the_forced_slab_count_and_differ_between_jobs():
    a, b = R.Row("ring", 5, 64, 128, 200, 3, 3, 0, 1), R.Row("ring", 5, 64, 128, 200, 3, 3, 0, 5)
    assert all(np.array_equal(u, v) for u, v in zip(R.inputs(a), R.inputs(b)))
    j = R.JOB_TABLES[0].jobs
    assert not np.array_equal(R.inputs(j[0]._replace(d=1))[0], R.inputs(j[1]._replace(d=1))[0])


@pytest.mark.parametrize("row", [r for r in R.CASES], ids=R.row_id)
def test_every_row_names_the_program_it_is_listed_under(row):
    for mode in R.SPLIT_MODES:
        got = R.predicted(row, mode)
        if row.form in R.SPLIT_FORMS:
            assert got == R.kernel_of(row.form, mode), (got, R.kernel_of(row.form, mode))
            assert row.B * row.L >= 256 and min(row.Cin, row.Cout) >= 32 and row.L >= 8
        elif row.form == "len1":
            assert got == "linear_len1_wgrad_kernel" and row.L == 1 and row.k == 1
        else:
            assert got in R.FP32_FORMS
    want32 = "linear_len1_wgrad_kernel" if row.form == "len1" else R.fp32_kernel_name(row.k, row.Cin)
    assert R.predicted(row, "fp32") == want32
    if row.Z is not None:
        assert R.clamped_z(row) == row.Z, "a forced count the library would clamp names another plan than the row's id"


def test_every_form_occurs_and_the_fp32_forms_are_all_reached():
    assert {r.form for r in R.CASES} == set(R.FORMS) - {"k3_128x64"}
    assert {t.form for t in R.JOB_TABLES} >= {"k3_128x64", "ring", "k1_128x96_xrow"}
    assert {R.predicted(r, "f16x2") for r in _rows("fallback")} == set(R.FP32_FORMS)
    assert {R.predicted(r, "fp32") for r in R.CASES} == set(R.FP32_FORMS) | {"linear_len1_wgrad_kernel"}
    # the split forms are the eight of ssv_launch_gemm_nt_bf3, in both split modes
    names = {R.kernel_of(f, m) for f in R.SPLIT_FORMS for m in R.SPLIT_MODES}
    assert len(names) == 16


def test_the_64x64_form_keeps_its_edges():
    rows = _rows("k1_64x64")
    assert all(r.Cin > 48 and r.Cin * r.Cout < 1 << 18 for r in rows)
    short = [r for r in rows if (r.B, r.L) == (4, 64)]
    assert sorted(R.chunks_per_workgroup(r)[0] for r in short) == [1, 2, 4]               # the chunk loop's short cases: nfull < 1
    assert all(len(set(R.chunks_per_workgroup(r))) == 1 for r in short)
    assert any(r.Cout % 64 == 1 and r.Cin % 64 == 1 and r.L % 8 == 2 for r in rows)       # one-row row tile, one-channel column tile
    assert any(r.Cout % 16 != 0 and r.Cout < 64 and r.Cin < 64 for r in rows)                   # partly filled 16-row block
    assert any(r.L == 8 for r in rows)
    leaves = lambda r, row: row * r.L + 64 * R.cdiv(r.L, 64) > r.Cout * r.L            # the row's last chunk ends past its batch item
    assert any(r.L == 8 and leaves(r, r.Cout - 2) and (r.Cout - 2) // 16 != (r.Cout - 1) // 16 for r in rows), "rows of two waves leave the item"
    assert any(R.chunks_per_workgroup(r) == [3 * 4, 2 * 4] for r in rows if r.Z == 2 and r.L == 200)      # slabs of 3 and 2 items


def test_the_128_row_forms_keep_their_edges():
    assert all(r.Cin <= 48 for r in _rows("k1_128x32")) and {r.Cin for r in _rows("k1_128x32")} >= {32, 33, 48}
    rows = _rows("k1_128x96")
    assert all(r.Cin * r.Cout >= 1 << 18 and not R.nt_bf3_xrow(1, r.Cout, r.Cin) for r in rows)
    assert any(r.Cin % 96 == 1 and r.Cout % 128 == 2 for r in rows)
    grid = lambda r: int(np.prod(R.tiles_of(r.k, r.Cout, r.Cin)))
    assert any(grid(r) > 64 for r in rows) and any(grid(r) <= 64 for r in rows)           # both tile orders (ct_fast)
    assert sorted(grid(r) for r in _rows("k1_128x128")) == [129, 129]
    assert sorted(grid(r) for r in _rows("k1_256x128_w8")) == [64, 66]                     # the last plain order, the first fast one
    for form in ("k1_128x128", "k1_256x128_w8"):
        assert {r.L % 64 for r in _rows(form)} == {0, 26}                                   # whole chunks, and a ragged last chunk


def test_the_extra_row_form_keeps_its_range_slab_edges():
    rows = _rows("k1_128x96_xrow")
    assert all(r.Cout % 128 == 1 and r.Cout > 128 and R.range_slabs_run(r, "f16x2") and not R.range_slabs_run(r, "fp32") for r in rows)
    assert {R.tiles_of(1, r.Cout, r.Cin)[0] for r in rows} >= {1, 2, 4}
    a = [r for r in rows if (r.B, r.L) == (4, 70)]
    assert {r.Z for r in a} == {1, 3, 5, 8, None}
    assert R.empty_slabs(4, 70, 5) == [4] and R.empty_slabs(4, 70, 3) == [] and R.mid_item_starts(4, 70, 3) == [1]
    assert R.range_slabs(4, 70, 3)[1] == [(0, 3), (3, 3), (6, 2)]
    assert R.range_slabs(4, 70, 8) == (1, [(z, 1) for z in range(8)]) and R.mid_item_starts(4, 70, 8) == [1, 3, 5, 7]
    assert any(r.L < 64 and r.Cout * r.L < (r.Cout - 2) * r.L + 64 for r in rows), "a tile row (not the extra row) whose chunk leaves the item"
    b = [r for r in rows if (r.B, r.L) == (5, 64)]
    assert {r.Z for r in b} == {2, 4}
    assert R.range_slabs(5, 64, 2)[1] == [(0, 3), (3, 2)] and R.range_slabs(5, 64, 4)[1] == [(0, 2), (2, 2), (4, 1), (6, 0)]
    assert R.empty_slabs(5, 64, 4) == [3]


@pytest.mark.parametrize("B,L,Z", [(B, L, Z) for B in (1, 2, 3, 4, 5, 7) for L in (8, 64, 65, 70, 128, 200) for Z in range(1, 2 + B * -(-L // 64))])
def test_range_slabs_partition_the_chunks(B, L, Z):
    """Every chunk belongs to exactly one slab, the slabs follow each other, only trailing slabs are empty."""
    per, slabs = R.range_slabs(B, L, Z)
    allc = B * R.cdiv(L, 64)
    owner = np.zeros(allc, dtype=int)
    for start, total in slabs:
        assert 0 <= total <= per and (total == 0 or start + total <= allc)
        owner[start:start + total] += 1
    assert (owner == 1).all()
    totals = [t for _, t in slabs]
    first_empty = totals.index(0) if 0 in totals else Z
    assert all(t == 0 for t in totals[first_empty:]) and R.empty_slabs(B, L, Z) == list(range(first_empty, Z))


def test_the_ring_rows_keep_their_edges():
    rows = _rows("ring")
    tch = lambda r: R.ring_tchunks(r.L, R.ring_bound(3, R.conv_shifts(3, r.d, r.causal)))
    assert all(r.k == 3 and 0 <= R.ring_bound(3, R.conv_shifts(3, r.d, r.causal)) <= 64 for r in rows)
    edge = [r for r in rows if r.d == 27 and r.causal]
    assert sorted({(r.L + 54, tch(r)) for r in edge}) == [(128, 2), (129, 3)]              # tchunks 64 == L + max_shift, and one step past it
    # rows whose chunk count without max_shift would be smaller, with more than one item per slab (or the padding chunk is never missed)
    assert {(r.L, r.d) for r in rows if R.cdiv(r.L, 64) < tch(r) and r.Z == 1 and r.B > 1} == {(64, 1), (75, 27)}
    long = [r for r in rows if r.L == 200]
    assert {r.Z for r in long} == {1, 5} and [R.chunks_per_workgroup(r) for r in long if r.Z == 1] == [[20]]     # >= 5 chunks: the ring wraps
    assert any(r.L == 8 for r in rows) and any(r.Cin % 64 and r.Cout % 128 for r in rows)
    assert R.ring_bound(3, [-65, 0, 65]) == -1 and R.ring_bound(3, [-54, -27, 0], -1) == -1 and R.ring_bound(3, [-54, -27, 0], 70) == -1
    assert R.ring_bound(3, [-1, 0, 1], 64) == 64 and R.ring_bound(1, [0]) == -1


def test_the_fallback_and_length_one_rows_keep_their_reasons():
    why = set()
    for r in _rows("fallback"):
        why |= {n for n, c in (("B L < 256", r.B * r.L < 256), ("L < 8", r.L < 8), ("channels < 32", min(r.Cin, r.Cout) < 32)) if c}
        assert not any(R.wgrad_bf3_runs(r.B, r.Cin, r.Cout, r.L, m) for m in R.MODES)
    assert why == {"B L < 256", "L < 8", "channels < 32"}
    assert any(r.B * r.L == 255 for r in _rows("fallback")) and any(r.Cin == 31 for r in _rows("fallback"))
    assert sorted(r.B for r in _rows("len1")) == [1, 3, 4, 5, 9] and all((r.Cin, r.Cout) == (7, 5) for r in _rows("len1"))     # B % 4: the unrolled batch loop


def test_the_job_tables():
    by = {t.name: t for t in R.JOB_TABLES}
    for t in R.JOB_TABLES:
        assert len({(r.B, r.Cin, r.Cout, r.L, r.k) for r in t.jobs}) == 1 and len({r.seed for r in t.jobs}) == len(t.jobs) >= 2
        for m in R.SPLIT_MODES:
            for r in t.jobs:
                assert R.predicted(r, m, t.max_shift if r.k == 3 else None) == R.kernel_of(t.form, m)
        reach = [max(abs(s) for s in R.conv_shifts(r.k, r.d, r.causal)) for r in t.jobs]
        assert tuple(i for i, s in enumerate(reach) if t.form == "ring" and s > t.max_shift) == t.nan_jobs
        assert t.same_kernel == all(R.predicted(r, "f16x2") == R.kernel_of(t.form, "f16x2") for r in t.jobs)
    assert [(r.d, r.causal) for r in by["ring_ms54"].jobs] == [(1, 1), (3, 1), (9, 1), (27, 1)]
    assert by["ring_ms53"].nan_jobs == (3,) and by["general_ms-1"].form == "k3_128x64" and not by["general_ms-1"].nan_jobs
    assert R.PART_NBLK == (1, 9, 129) and R.PART_N2 % 32 != 0


def test_predicted_names_and_notes_have_the_shape_logs_spelling():
    ring, bf3 = re.compile(r"^gemm_nt3r_kernel<2, [01]>$"), re.compile(r"^gemm_nt_bf3_kernel<[13], [12], [2468], [01], [01], 4>$")
    w8 = re.compile(r"^gemm_nt_bf3_kernel<1, 2, 8, [01], 0, 8>$")
    for r in R.CASES:
        if r.form not in R.SPLIT_FORMS:
            continue
        for m in R.SPLIT_MODES:
            n = R.predicted(r, m)
            assert (ring if r.form == "ring" else w8 if r.form == "k1_256x128_w8" else bf3).match(n), n
            assert n.split(", ")[1 if r.form == "ring" else 3].rstrip(">") == ("1" if m == "f16x2" else "0")
    assert R.note_of(1, 4, 64, 64, 64, 1, 2) == "jobs=1 B=4 M=64 Nc=64 L=64 k=1 Z=2"
    assert R.note_of(4, 4, 129, 65, 75, 3) == "jobs=4 B=4 M=129 Nc=65 L=75 k=3 Z="
    assert R.force_key(R.Row("k1_64x64", 5, 64, 32, 200, 1, 1, 0, 2)) == "32:64:1=2"


def test_the_bars_follow_from_the_float32_constant():
    assert R.BAR_F32 == 4 * R.F32_WORST and R.BAR_F16 == R.BAR_F32 + 2.0 ** -21 and R.BAR_BF3 == 15 * R.BAR_F16
    assert R.BARS == {"fp32": R.BAR_F32, "f16x2": R.BAR_F16, "bf16x3": R.BAR_BF3}
    assert R.L2_BARS == {"fp32": 2e-6, "f16x2": 2e-6, "bf16x3": 3e-5} and R.PART_BAR == 1e-5


def test_float32_numpy_error_over_all_rows_is_the_constant():
    errs = {}
    for r in R.all_rows():
        errs.setdefault(r._replace(Z=None), R.f32_error(r._replace(Z=None)))
    worst = max(errs.values())
    for form in R.FORMS:
        e = [v for r, v in errs.items() if r.form == form]
        if e:
            print("%-16s float32 numpy worst |err|/S %.3e" % (form, max(e)))
    assert all(v > 0 for v in errs.values())
    # the constant is this maximum; a BLAS that sums in another order may come out below it, but not far (the bars must not go stale)
    assert 0.8 * R.F32_WORST <= worst <= R.F32_WORST, (worst, R.F32_WORST)
