"""Every instantiation of gemm_nn_bf3_kernel and gemm_nn_bf3w_kernel (csrc/conv_nn.hip) that a Conv1d forward or data gradient can run --
2 kernel sizes x 8 tiles, the k = 3 tiles with their 16- and 54-column halo, the two wide tiles and the extra-row kernel, each in
split-fp16 and split-bf16 -- called through the C ABI at the edges of its own tile and held to float64 per element.  The rows, and why
each is there, are TILE_CASES / WIDE_CASES / NATURAL_CASES of tests/_conv_tiles_ref.py: SSV_NNB_FORCE puts a plain tile on shapes of one
or two tiles (a partly filled last 16-row block, a second row tile of a single row, a ragged and a one-column last column tile, a ragged
last K chunk, an odd chunk count, the halo off either end of the row and off both at once); the wide rows are the smallest the wide rule
admits; the natural rows are the cheapest shapes on which the cost model picks the tile by itself.  The exact-fp32 kernel of gemm_nn.hip
runs the same rows as a control.

Per row, forward (bias and bias_b given) and data gradient (dx_add given), operands and results with a batch stride of C L + 37 floats,
the gaps of the inputs NaN and the outputs pre-filled with -12345:
  |got - float64| <= bar S for EVERY element, S = sum |w| |x| + |bias| + |bias_b| (sum |w| |dy| + |dx_add|); the bars and their derivation
  are in the reference module (BAR_F32 from the float32 numpy evaluation of the same sums, + 2^-21 for f16x2, x 15 for bf16x3);
  whole-tensor relative L2 <= 2e-6 (fp32, f16x2) / 3e-5 (bf16x3); every result finite; gaps and guard zones bitwise untouched; a second
  call and a call on resident planes bitwise equal to the first; the forward's column statistics within 2e-5 of their largest entry.
The reach test asks the library's own shape log (a child process) for the kernel name and note tests/_conv_tiles_ref.pick_tile predicts
for every row, in both split modes.  Figures: profiles/conv_tiles_accuracy.txt (`pytest -m gpu -s`)."""
import contextlib
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _conv_tiles_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = -12345.0              # what outputs, their gaps and guard zones are filled with before a call
GAP = 37                     # floats between two batch items of x, dy, y, dx (and dx_add, which shares dx's stride)
PAD = 64                     # floats of guard zone on either side of a strided buffer
MODES = ("f16x2", "bf16x3", "fp32")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    from spoofsv_amd import ops
    return ops._stream()


@contextlib.contextmanager
def _forced(row):
    """SSV_NNB_FORCE names the row's tile (no force for a wide or natural row) while the block runs; the environment and the library's
    copy of it are put back afterwards."""
    from spoofsv_amd import _lib
    old = os.environ.get("SSV_NNB_FORCE")
    if row.forced:
        os.environ["SSV_NNB_FORCE"] = "%d:%d:%d=%d,%d" % (row.kt, row.M, row.N, row.forced[0], row.forced[1])
    else:
        os.environ.pop("SSV_NNB_FORCE", None)
    _lib.lib().ssv_reload_tuning()
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SSV_NNB_FORCE", None)
        else:
            os.environ["SSV_NNB_FORCE"] = old
        _lib.lib().ssv_reload_tuning()


@contextlib.contextmanager
def _mode(mode):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(mode)
    try:
        yield
    finally:
        spoofsv_amd.set_precision(prev)


def _strided(B, C, L, fill, src=None):
    """(whole allocation, (B, C, L) view with batch stride C L + GAP inside it): guard zones and gaps hold ``fill``, the view ``src``."""
    bs = C * L + GAP
    flat = torch.full((2 * PAD + B * bs,), fill, dtype=torch.float32, device=DEV)
    view = flat.as_strided((B, C, L), (bs, L, 1), PAD)
    if src is not None:
        view.copy_(src)
    return flat, view, bs


# ---- operands and references, per form ---------------------------------------------------------------------------------------------------
class _RowData:
    """Operands of one row on the device (inputs strided, gaps NaN) and its float64 references: numpy on the CPU for the small rows, torch
    float64 on the device (a checker, as tests/test_gpu_bench_shapes._ref64 is) for the wide ones."""

    def __init__(self, row):
        self.row = row
        inp = R.inputs(row)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        nan = float("nan")
        self.x = _strided(row.B, row.K, row.N, nan, dev(inp.x))
        self.dy = _strided(row.B, row.K, row.N, nan, dev(inp.dy))
        self.dx_add = _strided(row.B, row.M, row.N, nan, dev(inp.dx_add))
        self.w, self.wd, self.bias, self.bias_b = dev(inp.w), dev(inp.wd), dev(inp.bias), dev(inp.bias_b)
        if row.form is None or row.form[0] == "plain":
            (y, Sy), (dx, Sdx) = R.reference(row, inp)
            self.y, self.Sy, self.dx, self.Sdx = dev(y), dev(Sy), dev(dx), dev(Sdx)
        else:
            assert row.kt == 1
            mm = lambda a, b: torch.matmul(a, b)
            x, w, dy, wd = self.x[1].double(), self.w[:, :, 0].double(), self.dy[1].double(), self.wd[:, :, 0].double().t()
            add = self.bias.double().view(1, -1, 1) + self.bias_b.double().unsqueeze(2)
            self.y, self.Sy = mm(w, x) + add, mm(w.abs(), x.abs()) + self.bias.double().abs().view(1, -1, 1) + self.bias_b.double().abs().unsqueeze(2)
            self.dx, self.Sdx = mm(wd, dy) + self.dx_add[1].double(), mm(wd.abs(), dy.abs()) + self.dx_add[1].double().abs()
        self.cs = dev(R.colstats(self.y.cpu().numpy())) if row.colstats else None
        assert bool((self.Sy > 0).all()) and bool((self.Sdx > 0).all())


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_operands():
    yield
    _CACHE.clear()


def _data(form):
    """The rows of one form with their operands and references: computed once, shared by the three modes (one form is kept at a time)."""
    if form not in _CACHE:
        _CACHE.clear()
        _CACHE[form] = [_RowData(r) for r in R.rows_of(form)]
    return _CACHE[form]


# ---- the two entry points ------------------------------------------------------------------------------------------------------------------
def _ws(name, *dims):
    from spoofsv_amd import _lib
    nb = _lib.query(name, *dims)
    return torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV), nb


def _fwd(row, x, x_bs, xa, w, planes, bias, bias_b, y, y_bs, cs):
    from spoofsv_amd import _lib
    ws, nb = _ws("ssv_conv1d_fwd_workspace", row.K, row.M, row.kt)
    _lib.call("ssv_conv1d_fwd", P(x), x_bs, P(xa), xa.shape[1], P(w), planes, P(bias), P(bias_b), P(y), y_bs, P(cs),
              row.B, row.K, row.M, row.N, row.kt, row.d, row.causal, P(ws), nb, _st())


def _dgrad(row, dy, dy_bs, dya, wd, planes, dx_add, dx, dx_bs):
    from spoofsv_amd import _lib
    ws, nb = _ws("ssv_conv1d_bwd_data_workspace", row.M, row.K, row.kt)
    _lib.call("ssv_conv1d_bwd_data", P(dy), dy_bs, P(dya), dya.shape[1], P(wd), planes, P(dx_add), P(dx), dx_bs,
              row.B, row.M, row.K, row.N, row.kt, row.d, row.causal, P(ws), nb, _st())


def _three_calls(launch, row, fails, what):
    """launch(planes kind, y view, y batch stride) three times into a fresh strided, pre-filled output: per-call planes, the same again, resident
    planes.  Returns the first result; records a written gap / guard zone and any bitwise difference between the three."""
    got = []
    for kind in ("per call", "again", "resident"):
        flat, view, bs = _strided(row.B, row.M, row.N, FILL)
        launch(kind == "resident", view, bs)
        got.append(view.clone())
        view.fill_(FILL)
        if not bool((flat == FILL).all()):
            fails.append((what, kind, "wrote outside the live part of its output", int((flat != FILL).sum())))
    if not torch.equal(got[0], got[1]):
        fails.append((what, "a second call differs", int((got[0] != got[1]).sum())))
    if not torch.equal(got[0], got[2]):
        fails.append((what, "resident planes differ from per-call planes", int((got[0] != got[2]).sum())))
    return got[0]


def _held(got, want, S, mode, fails, what, fig, key):
    """Per element against bar S, whole tensor in relative L2; the figures go into ``fig`` before anything is judged."""
    if not bool(torch.isfinite(got).all()):
        fails.append((what, "non-finite results", int((~torch.isfinite(got)).sum())))
        return
    err = (got.double() - want).abs()
    frac = err / S
    e, l2 = float(frac.max()), float((got.double() - want).norm() / want.norm())
    fig[key] = max(fig.get(key, 0.0), e)
    fig[key + " L2"] = max(fig.get(key + " L2", 0.0), l2)
    if e > R.BARS[mode]:
        at = np.unravel_index(int(frac.argmax()), tuple(frac.shape))
        fails.append((what, "|err|/S %.3e > %.3e at (b, m, t) = %s, %d elements over" % (e, R.BARS[mode], at, int((frac > R.BARS[mode]).sum()))))
    if l2 > R.L2_BARS[mode]:
        fails.append((what, "relative L2 %.3e > %.1e" % (l2, R.L2_BARS[mode])))


def _run_row(d, mode, fails, fig):
    from spoofsv_amd import ops, resident
    row = d.row
    what = R.row_id(row) + " " + mode
    rw = resident.ResidentWeights([d.w, d.wd])
    rw.refresh(_st())
    try:
        with _forced(row):
            xa, dya = ops.amax_of(d.x[1]), ops.amax_of(d.dy[1])
            planes = lambda w, res: resident.lookup(w) if res else None
            assert resident.lookup(d.w) is not None and resident.lookup(d.wd) is not None
            y = _three_calls(lambda res, v, bs: _fwd(row, d.x[1], d.x[2], xa, d.w, planes(d.w, res), d.bias, d.bias_b, v, bs, None), row, fails, what + " fwd")
            _held(y, d.y, d.Sy, mode, fails, what + " fwd", fig, "fwd")
            dx = _three_calls(lambda res, v, bs: _dgrad(row, d.dy[1], d.dy[2], dya, d.wd, planes(d.wd, res), d.dx_add[1], v, bs), row, fails, what + " dgrad")
            _held(dx, d.dx, d.Sdx, mode, fails, what + " dgrad", fig, "dgrad")
            if row.form[0] == "xrow":                                   # the row beside the tiles, on its own
                m = row.M - 1
                _held(y[:, m:], d.y[:, m:], d.Sy[:, m:], mode, fails, what + " fwd row M-1", fig, "fwd row M-1")
                _held(dx[:, m:], d.dx[:, m:], d.Sdx[:, m:], mode, fails, what + " dgrad row M-1", fig, "dgrad row M-1")
            if row.colstats and mode != "fp32":                         # (the statistics come from the split-MFMA epilogue, into a dense output)
                yd = torch.full((row.B, row.M, row.N), FILL, device=DEV)
                cs = torch.full((row.B, row.M // 64, row.N, 2), float("nan"), device=DEV)
                _fwd(row, d.x[1], d.x[2], xa, d.w, None, d.bias, d.bias_b, yd, row.M * row.N, cs)
                _held(yd, d.y, d.Sy, mode, fails, what + " fwd +colstats", fig, "fwd")
                if not bool(torch.isfinite(cs).all()):
                    fails.append((what, "column statistics not finite or not written", int((~torch.isfinite(cs)).sum())))
                else:
                    for i, name in enumerate(("colstats mean", "colstats M2")):
                        e = float((cs[..., i].double() - d.cs[..., i]).abs().max() / d.cs[..., i].abs().max())
                        fig[name] = max(fig.get(name, 0.0), e)
                        if e > R.COLSTATS_BAR:
                            fails.append((what, name, e))
            torch.cuda.synchronize()
    finally:
        resident.invalidate([d.w, d.wd])


CASES = [(form, mode) for form in R.FORMS for mode in MODES]


@pytest.mark.parametrize("form,mode", CASES, ids=["%s-%s" % (R.form_id(f), m) for f, m in CASES])
def test_every_row_of_one_instantiation_vs_float64_per_element(form, mode):
    """All rows of one instantiation in one arithmetic mode (fp32: the same shapes on the exact kernel; the force has no effect there).
    Every row runs and its figures are printed before the first failure is raised."""
    fails, fig = [], {}
    rows = _data(form)
    with _mode(mode):
        for d in rows:
            _run_row(d, mode, fails, fig)
    kernel = R.kernel_of(form, mode) if mode != "fp32" else "gemm_nn_kernel (exact fp32)"
    print("CONVTILE %-18s %-6s %-44s rows %2d  bar %.3e  %s" % (R.form_id(form), mode, kernel, len(rows), R.BARS[mode],
                                                                "  ".join("%s %.3e" % kv for kv in sorted(fig.items()))))
    assert not fails, fails[:8]


@pytest.mark.parametrize("mode", ("f16x2", "bf16x3"))
def test_column_statistics_of_a_product_whose_last_row_tile_is_half_a_tile(mode):
    """HALF_GROUP_CASES: M = 192 with the statistics asked for, the 128 x 112 tile named by force or chosen by the cost model's own rule for
    k = 1.  On that tile the second 64-row group of the last row tile would be written into the next item's first group and, for the last
    item, past the buffer; pick_nnb keeps such a product on 64-row tiles.  The statistics of every group against float64, the guard zones
    around their buffer bitwise untouched, the output per element."""
    fails, fig = [], {}
    with _mode(mode):
        for row in R.HALF_GROUP_CASES:
            from spoofsv_amd import ops
            d, what = _RowData(row), R.row_id(row) + " " + mode
            n = row.B * (row.M // 64) * row.N * 2
            flat = torch.full((n + 2 * PAD,), FILL, device=DEV)
            cs = flat[PAD:PAD + n].view(row.B, row.M // 64, row.N, 2)
            yd = torch.full((row.B, row.M, row.N), FILL, device=DEV)
            with _forced(row):
                _fwd(row, d.x[1], d.x[2], ops.amax_of(d.x[1]), d.w, None, d.bias, d.bias_b, yd, row.M * row.N, cs)
            torch.cuda.synchronize()
            _held(yd, d.y, d.Sy, mode, fails, what, fig, "fwd")
            assert bool((flat[:PAD] == FILL).all()) and bool((flat[-PAD:] == FILL).all()), (what, "statistics written outside their buffer")
            for i, name in enumerate(("colstats mean", "colstats M2")):
                e = float((cs[..., i].double() - d.cs[..., i]).abs().max() / d.cs[..., i].abs().max())
                fig[name] = max(fig.get(name, 0.0), e)
                assert e <= R.COLSTATS_BAR, (what, name, e)
    print("CONVTILE %-18s %-6s rows %2d  bar %.3e  %s" % ("half group M=192", mode, len(R.HALF_GROUP_CASES), R.BARS[mode],
                                                        "  ".join("%s %.3e" % kv for kv in sorted(fig.items()))))
    assert not fails, fails


# ---- reach -----------------------------------------------------------------------------------------------------------------------------------
def _probe_main():
    """Child process (SSV_SHAPE_LOG set): the forward launch of every row in both split modes, on zero operands."""
    from spoofsv_amd import resident
    z = lambda *s: torch.zeros(s, device=DEV)
    for mode in ("f16x2", "bf16x3"):
        with _mode(mode):
            for row in R.TILE_CASES + R.WIDE_CASES + R.NATURAL_CASES + R.HALF_GROUP_CASES:
                with _forced(row):
                    x, w, bias, bias_b, xa = z(row.B, row.K, row.N), z(row.M, row.K, row.kt), z(row.M), z(row.B, row.M), z(row.B, 8)
                    y = z(row.B, row.M, row.N)
                    _fwd(row, x, row.K * row.N, xa, w, None, bias, bias_b, y, row.M * row.N, None)
                    if row.colstats:
                        _fwd(row, x, row.K * row.N, xa, w, None, bias, bias_b, y, row.M * row.N, z(row.B, row.M // 64, row.N, 2))
            torch.cuda.synchronize()
    resident.invalidate()


@pytest.fixture(scope="module")
def shape_log():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "shapes.tsv")
        env = dict(os.environ, SSV_SHAPE_LOG=path, SSV_PRECISION="f16x2")
        env.pop("SSV_NNB_FORCE", None)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_conv_tiles as t; t._probe_main()" % (root, os.path.join(root, "tests"))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return {(f[0], f[4]) for f in rows if len(f) >= 5}


REACH = [(form, mode) for form in R.FORMS for mode in ("f16x2", "bf16x3")]


@pytest.mark.parametrize("form,mode", REACH, ids=["%s-%s" % (R.form_id(f), m) for f, m in REACH])
def test_every_row_reaches_the_instantiation_pick_tile_predicts(shape_log, form, mode):
    """The library's own shape log holds, for every forced, wide and natural row of the form, the kernel name and the note pick_tile predicted
    -- which ties the Python restatement of the dispatch to pick_nnb, and keeps a later retune from emptying a case above unnoticed."""
    rows = R.rows_of(form)
    assert rows
    for row in rows:
        kernel = R.predicted(row, mode)
        assert kernel == R.kernel_of(form, mode)
        notes = [R.note_of(row.kt, row.B, row.M, row.N, row.K, xrow=form[0] == "xrow")]
        if row.colstats:
            notes.append(R.note_of(row.kt, row.B, row.M, row.N, row.K, colstats=True))
        for note in notes:
            assert (kernel, note) in shape_log, (R.row_id(row), kernel, note, sorted(k for k, n in shape_log if n == note))


@pytest.mark.parametrize("mode", ("f16x2", "bf16x3"))
def test_half_group_rows_with_statistics_run_64_row_tiles(shape_log, mode):
    """The same shape runs the forced 128-row tile without the statistics and a 64-row tile with them (HALF_GROUP_CASES)."""
    for row in R.HALF_GROUP_CASES:
        span = R.span_of(row.kt, row.d)
        for colstats in (False, True):
            kernel = R.pick_tile(row.kt, row.B, row.M, row.N, row.K, colstats, row.forced, span, mode)
            assert kernel.startswith("gemm_nn_bf3_kernel<%d, %d, " % (row.kt, 1 if colstats else 2))
            note = R.note_of(row.kt, row.B, row.M, row.N, row.K, colstats=colstats)
            assert (kernel, note) in shape_log, (R.row_id(row), kernel, note, sorted(k for k, n in shape_log if n == note))
