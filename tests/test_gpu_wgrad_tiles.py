"""Every program a Conv1d weight gradient can run -- the ring kernel gemm_nt3r_kernel<2, F>, the seven gemm_nt_bf3_kernel instantiations
(csrc/wgrad_nt.hip: <3, 2, 4>, <1, 1, 4>, <1, 2, 2>, <1, 2, 6>, the extra-row form on range slabs, <1, 2, 8> on 4 and on 8 waves), each
in split-fp16 and split-bf16, the three exact-fp32 gemm_nt_kernel forms and linear_len1_wgrad_kernel, with the slab reductions of
csrc/misc.hip behind them -- called through the C ABI at the edges of its own tile and slab plan and held to float64 per element.  The
rows, and why each is there, are CASES / JOB_TABLES of tests/_wgrad_tiles_ref.py (SSV_NT_FORCE sets a row's slab count): workgroups that
reduce over 1, 2 and 4 chunks, range slabs that start inside an item and slabs that own no chunk at all, both tile orders, lengths of 8,
of 8 j + 2 and of 64 j, the ring at tchunks 64 == L + max_shift and wrapped five times over, both paths of the slab reduction.

Per row, operands with a batch stride of C L + 37 floats, every gap and guard zone NaN; dw inside a buffer pre-filled with -12345, once
16-byte aligned and once one float later; the workspace exactly as large as the query says, between guard zones:
  |got - float64| <= bar S for EVERY element, S = sum |dy| |x|; the bars and their derivation are in the reference module (BAR_F32 from
  the float32 numpy evaluation of the same sums, + 2^-21 for f16x2, x 15 for bf16x3); relative L2 per tap <= 2e-6 (fp32, f16x2) / 3e-5
  (bf16x3); every result finite; operands, gaps and guard zones bitwise untouched; a second call, a call without the caller's scale lists
  and the call into the misaligned dw bitwise equal to the first.
Job tables (ssv_conv1d_bwd_weight_multi): the same per job, each job bitwise equal to the one-layer entry forced to the table's slab
count, a job whose shifts exceed the stated bound all NaN, the partial rows of a job summed to 1e-5.  The reach test asks the library's
own shape log (a child process) for the kernel name and note tests/_wgrad_tiles_ref.predicted gives for every row, in both split modes.
Figures: profiles/wgrad_tiles_accuracy.txt (`pytest -m gpu -s`)."""
import contextlib
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _wgrad_tiles_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = -12345.0              # what dw and its guard zones are filled with before a call
GAP = 37                     # floats between two batch items of x and dy
PAD = 64                     # floats of guard zone on either side of a buffer
WS_GUARD = 256               # bytes of guard zone on either side of the workspace
WS_BYTE = 0xFF               # the workspace and its guard zones before a call: a slab that is read without having been written is NaN
NAN = float("nan")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    from spoofsv_amd import ops
    return ops._stream()


@contextlib.contextmanager
def _forced(key):
    """SSV_NT_FORCE = ``key`` ("M:Nc:k=Z", or None for the library's own count) while the block runs; the environment and the library's
    copy of it are put back afterwards."""
    from spoofsv_amd import _lib
    old = os.environ.get("SSV_NT_FORCE")
    if key:
        os.environ["SSV_NT_FORCE"] = key
    else:
        os.environ.pop("SSV_NT_FORCE", None)
    _lib.lib().ssv_reload_tuning()
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SSV_NT_FORCE", None)
        else:
            os.environ["SSV_NT_FORCE"] = old
        _lib.lib().ssv_reload_tuning()


@contextlib.contextmanager
def _mode(mode):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(mode)
    try:
        yield
    finally:
        spoofsv_amd.set_precision(prev)


def _bits(t):
    return t.view(torch.int32)


class _Strided:
    """A (B, C, L) view with batch stride C L + GAP inside an allocation whose guard zones and gaps hold NaN, and a snapshot of the whole
    allocation to hold it to afterwards."""

    def __init__(self, src):
        B, C, L = src.shape
        self.bs = C * L + GAP
        self.flat = torch.full((2 * PAD + B * self.bs,), NAN, dtype=torch.float32, device=DEV)
        self.view = self.flat.as_strided((B, C, L), (self.bs, L, 1), PAD)
        self.view.copy_(src)
        self.snap = self.flat.clone()

    def untouched(self):
        return torch.equal(_bits(self.flat), _bits(self.snap))


class _Out:
    """n floats at 16-byte alignment (+ ``off`` floats) inside an allocation pre-filled with FILL."""

    def __init__(self, shape, off):
        n = int(np.prod(shape))
        self.flat = torch.full((2 * PAD + n + 4,), FILL, dtype=torch.float32, device=DEV)
        self.t = self.flat[PAD + off:PAD + off + n].view(shape)
        assert self.t.data_ptr() % 16 == 4 * off

    def take(self):
        """The result; the allocation must hold FILL everywhere else."""
        got = self.t.clone()
        self.t.fill_(FILL)
        return got, bool((self.flat == FILL).all())


class _Ws:
    """Exactly ``nb`` bytes of workspace between two guard zones."""

    def __init__(self, nb):
        self.nb = nb
        self.buf = torch.full((2 * WS_GUARD + nb,), WS_BYTE, dtype=torch.uint8, device=DEV)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + WS_GUARD)
        assert (self.buf.data_ptr() + WS_GUARD) % 256 == 0

    def untouched(self):
        return bool((self.buf[:WS_GUARD] == WS_BYTE).all()) and bool((self.buf[WS_GUARD + self.nb:] == WS_BYTE).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- operands and references, per form ---------------------------------------------------------------------------------------------------
class _RowData:
    """Operands of one row on the device and its float64 reference: numpy on the CPU for the small rows, torch float64 on the device (a
    checker, as tests/test_gpu_bench_shapes._ref64 is) for R.WIDE_ROWS.  Rows that differ in the forced Z only share everything."""

    def __init__(self, row):
        self.row = row
        dy, x = R.inputs(row)
        self.dy, self.x = _Strided(_dev(dy)), _Strided(_dev(x))
        if row in R.WIDE_ROWS:
            assert row.k == 1
            d64, x64 = self.dy.view.double(), self.x.view.double()
            self.dw = torch.einsum("bot,bct->oc", d64, x64).unsqueeze(2)
            self.S = torch.einsum("bot,bct->oc", d64.abs(), x64.abs()).unsqueeze(2)
        else:
            dw, S = R.reference(row)
            self.dw, self.S = _dev(dw), _dev(S)
        assert bool((self.S > 0).all())


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_operands():
    yield
    _CACHE.clear()


def _data(form):
    """The rows of one form with their operands and references: computed once, shared by the three modes (one form is kept at a time)."""
    if form not in _CACHE:
        _CACHE.clear()
        made, out = {}, []
        for r in R.rows_of(form):
            key = r._replace(Z=None)
            if key not in made:
                made[key] = _RowData(key)
            out.append((r, made[key]))
        _CACHE[form] = out
    return _CACHE[form]


# ---- the entry point ---------------------------------------------------------------------------------------------------------------------
def _wgrad(row, dy, dya, x, xa, dw):
    """ssv_conv1d_bwd_weight into ``dw`` with a workspace of exactly the queried size; False when its guard zones were written."""
    from spoofsv_amd import _lib
    ws = _Ws(_lib.query("ssv_conv1d_bwd_weight_workspace", row.B, row.Cin, row.Cout, row.L, row.k))
    an = lambda a: (None, 0) if a is None else (P(a), a.shape[1])
    _lib.call("ssv_conv1d_bwd_weight", P(dy.view), dy.bs, *an(dya), P(x.view), x.bs, *an(xa), P(dw), row.B, row.Cin, row.Cout, row.L, row.k, row.d,
              row.causal, ws.ptr, ws.nb, _st())
    torch.cuda.synchronize()
    return ws.untouched()


def _held(got, want, S, mode, fails, what, fig):
    """Per element against bar S, per tap in relative L2; the figures go into ``fig`` before anything is judged."""
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).nonzero()
        fails.append((what, "non-finite results", len(bad), "first at (o, c, j) = %s" % (tuple(int(v) for v in bad[0]),)))
        return
    diff = got.double() - want
    frac = diff.abs() / S
    e = float(frac.max())
    l2 = max(float(diff[:, :, j].norm() / want[:, :, j].norm()) for j in range(want.shape[2]))
    fig["err"] = max(fig.get("err", 0.0), e)
    fig["L2"] = max(fig.get("L2", 0.0), l2)
    if e > R.BARS[mode]:
        at = np.unravel_index(int(frac.argmax()), tuple(frac.shape))
        fails.append((what, "|err|/S %.3e > %.3e at (o, c, j) = %s, %d elements over" % (e, R.BARS[mode], at, int((frac > R.BARS[mode]).sum()))))
    if l2 > R.L2_BARS[mode]:
        fails.append((what, "relative L2 of a tap %.3e > %.1e" % (l2, R.L2_BARS[mode])))


def _run_row(row, d, mode, fails, fig):
    from spoofsv_amd import ops
    what = R.row_id(row) + " " + mode
    shape = (row.Cout, row.Cin, row.k)
    with _forced(R.force_key(row) if row.Z else None):
        lists = (ops.amax_of(d.dy.view), ops.amax_of(d.x.view)) if mode != "fp32" else (None, None)
        calls = [("aligned", 0, lists), ("again", 0, lists), ("one float later", 1, lists)]
        if mode != "fp32":
            calls.append(("without scale lists", 0, (None, None)))
        got = []
        for name, off, (dya, xa) in calls:
            out = _Out(shape, off)
            ws_ok = _wgrad(row, d.dy, dya, d.x, xa, out.t)
            g, clean = out.take()
            got.append(g)
            if not clean:
                fails.append((what, name, "wrote outside dw", int((out.flat != FILL).sum())))
            if not ws_ok:
                fails.append((what, name, "wrote outside its workspace"))
            if not (d.dy.untouched() and d.x.untouched()):
                fails.append((what, name, "an operand, a gap or a guard zone of an operand changed"))
    for (name, _, _), g in zip(calls[1:], got[1:]):
        if not torch.equal(_bits(got[0]), _bits(g)):
            fails.append((what, "%s: differs bitwise from the first call" % name, int((_bits(got[0]) != _bits(g)).sum())))
    _held(got[0], d.dw, d.S, mode, fails, what, fig)


ROW_FORMS = [f for f in R.FORMS if R.rows_of(f)]
CASES = [(form, mode) for form in ROW_FORMS for mode in R.MODES]


def _program(form, mode, rows):
    if form in R.SPLIT_FORMS and mode != "fp32":
        return R.kernel_of(form, mode)
    return " / ".join(sorted({R.predicted(r, mode) for r in rows}))


@pytest.mark.parametrize("form,mode", CASES, ids=["%s-%s" % c for c in CASES])
def test_every_row_of_one_program_vs_float64_per_element(form, mode):
    """All rows of one form in one arithmetic mode (fp32: the same shapes on the exact kernels; a forced Z holds there too, up to B).  Every
    row runs and its figures are printed before the first failure is raised."""
    fails, fig = [], {}
    rows = _data(form)
    with _mode(mode):
        for row, d in rows:
            _run_row(row, d, mode, fails, fig)
    print("WGRADTILE %-15s %-6s %-44s rows %2d  bar %.3e  %s" % (form, mode, _program(form, mode, [r for r, _ in rows]), len(rows), R.BARS[mode],
                                                                "  ".join("%s %.3e" % kv for kv in sorted(fig.items()))))
    assert not fails, fails[:8]


# ---- job tables ------------------------------------------------------------------------------------------------------------------------------
class _Table:
    """The device side of one ssv_conv1d_bwd_weight_multi call: the jobs' operands (strided, NaN gaps), their dw buffers (even jobs 16-byte
    aligned, odd jobs one float later), scale lists, optional partial rows, the table itself and a workspace of the queried size."""

    def __init__(self, jobs, zeros=False, n2=0, nblk=0):
        from spoofsv_amd import _lib, ops
        r0 = jobs[0]
        self.jobs, self.n2, self.nblk = jobs, n2, nblk
        self.data, self.outs, self.parts, self.pgs, self.lists = [], [], [], [], []
        table = (_lib.WgradJob * len(jobs))()
        for i, (r, t) in enumerate(zip(jobs, table)):
            d = _RowData(r) if not zeros else None
            if zeros:
                dy, x = _Strided(torch.zeros(r.B, r.Cout, r.L, device=DEV)), _Strided(torch.zeros(r.B, r.Cin, r.L, device=DEV))
            else:
                dy, x = d.dy, d.x
            out = _Out((r.Cout, r.Cin, r.k), i % 2)
            dya, xa = ops.amax_of(dy.view), ops.amax_of(x.view)
            t.dy, t.x, t.dw = dy.view.data_ptr(), x.view.data_ptr(), out.t.data_ptr()
            if n2:
                part = torch.randn(nblk, n2, generator=torch.Generator().manual_seed(100 * nblk + i)).to(DEV)
                pg = _Out((n2,), i % 2)
                t.part, t.pgrads = part.data_ptr(), pg.t.data_ptr()
                self.parts.append(part)
                self.pgs.append(pg)
            sh = R.conv_shifts(r.k, r.d, r.causal)
            for j in range(3):
                t.shift[j] = sh[j] if j < len(sh) else 0
            t.dy_amax, t.x_amax, t.dy_namax, t.x_namax = dya.data_ptr(), xa.data_ptr(), dya.numel(), xa.numel()
            self.data.append((dy, x, d))
            self.outs.append(out)
            self.lists.append((dya, xa))
        self.tdev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
        self.dy_bs, self.x_bs = self.data[0][0].bs, self.data[0][1].bs
        self.Z = int(_lib.lib().ssv_conv1d_bwd_weight_multi_splits(len(jobs), r0.B, r0.Cin, r0.Cout, r0.L, r0.k))
        self.ws = _Ws(_lib.query("ssv_conv1d_bwd_weight_multi_workspace", len(jobs), r0.B, r0.Cin, r0.Cout, r0.L, r0.k))

    def run(self, max_shift):
        from spoofsv_amd import _lib
        r = self.jobs[0]
        _lib.call("ssv_conv1d_bwd_weight_multi", P(self.tdev), len(self.jobs), self.dy_bs, self.x_bs, r.B, r.Cin, r.Cout, r.L, r.k, max_shift,
                  self.n2, self.nblk, self.ws.ptr, self.ws.nb, _st())
        torch.cuda.synchronize()


TABLE_CASES = [(t, m) for t in R.JOB_TABLES for m in R.SPLIT_MODES]


@pytest.mark.parametrize("table,mode", TABLE_CASES, ids=["%s-%s" % (t.name, m) for t, m in TABLE_CASES])
def test_job_table_vs_float64_per_element_and_vs_the_one_layer_entry_bitwise(table, mode):
    fails, fig = [], {}
    with _mode(mode):
        assert not os.environ.get("SSV_NT_FORCE")
        T = _Table(table.jobs)
        both = []
        for call in ("first", "again"):
            T.run(table.max_shift)
            res = []
            for i, out in enumerate(T.outs):
                g, clean = out.take()
                res.append(g)
                if not clean:
                    fails.append((table.name, call, "job %d wrote outside dw" % i))
            both.append(res)
            if not T.ws.untouched():
                fails.append((table.name, call, "wrote outside its workspace"))
            if not all(dy.untouched() and x.untouched() for dy, x, _ in T.data):
                fails.append((table.name, call, "an operand, a gap or a guard zone of an operand changed"))
        for i, (r, (dy, x, d)) in enumerate(zip(table.jobs, T.data)):
            what = "%s job %d %s" % (table.name, i, mode)
            if not torch.equal(_bits(both[0][i]), _bits(both[1][i])):
                fails.append((what, "a second call differs"))
            if i in table.nan_jobs:
                if not bool(torch.isnan(both[0][i]).all()):
                    fails.append((what, "shifts past the stated bound must give NaN gradients", int((~torch.isnan(both[0][i])).sum())))
                continue
            _held(both[0][i], d.dw, d.S, mode, fails, what, fig)
            if table.same_kernel:
                with _forced(R.force_key(r._replace(Z=T.Z))):
                    out = _Out((r.Cout, r.Cin, r.k), i % 2)
                    _wgrad(r, dy, T.lists[i][0], x, T.lists[i][1], out.t)
                    one = out.take()[0]
                if not torch.equal(_bits(one), _bits(both[0][i])):
                    fails.append((what, "differs bitwise from the one-layer entry at Z = %d" % T.Z, int((_bits(one) != _bits(both[0][i])).sum())))
    print("WGRADTILE %-15s %-6s %-44s jobs %2d  bar %.3e  Z %d  max_shift %d  %s" % (
        table.name, mode, R.kernel_of(table.form, mode), len(table.jobs), R.BARS[mode], T.Z, table.max_shift,
        "  ".join("%s %.3e" % kv for kv in sorted(fig.items()))))
    assert not fails, fails[:8]


@pytest.mark.parametrize("nblk", R.PART_NBLK)
def test_job_table_sums_each_jobs_partial_rows(nblk):
    """part (nblk, n2) -> pgrads (n2) in the reduction launch of the table: 1 row, 9 rows (one per row group and one more), 129 rows (one
    trip of 16 loads per row group and one more), n2 = 70 (the last workgroup owns 6 outputs).  The weight gradients ride along."""
    table = [t for t in R.JOB_TABLES if t.name == "k1_64x64"][0]
    with _mode("f16x2"):
        T = _Table(table.jobs, n2=R.PART_N2, nblk=nblk)
        T.run(table.max_shift)
        for i, (part, pg, out, (_, _, d)) in enumerate(zip(T.parts, T.pgs, T.outs, T.data)):
            got, clean = pg.take()
            assert clean, ("job", i, "wrote outside pgrads")
            want = part.double().sum(0)
            e = float((got.double() - want).abs().max() / want.abs().max())
            print("WGRADTILE partial rows nblk %3d job %d: %.3e of the largest sum (bar %.0e)" % (nblk, i, e, R.PART_BAR))
            assert e <= R.PART_BAR, (nblk, i, e)
            fails, fig = [], {}
            g, clean = out.take()
            _held(g, d.dw, d.S, "f16x2", fails, "job %d" % i, fig)
            assert clean and not fails, fails
        assert T.ws.untouched()


# ---- the gap between the items of dy, through autograd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d,causal", [(1, 1, 0), (3, 3, 1)], ids=["k1", "k3_ring"])
@pytest.mark.parametrize("large", (0, 1), ids=["first_half_large", "second_half_large"])
def test_weight_gradients_of_two_convolutions_whose_outputs_are_concatenated(large, k, d, causal):
    """y = cat((conv_a(x), conv_b(x)), 1), as models/TTSModel.py:270 builds (R, Q): autograd hands each convolution a narrow view of y's
    gradient, passed through uncopied, so what lies between two batch items of one convolution's dy is the OTHER convolution's gradient.
    Here that one is 2^10 times larger -- beyond what the view's own split-fp16 scale leaves representable -- and L = 90 ends inside a
    chunk, so the windows of the last row of dy run on into it.  Both weight gradients per element against float64."""
    import spoofsv_amd
    from spoofsv_amd import ops
    assert spoofsv_amd.get_precision() == "f16x2"
    B, Cin, Cout, L = 3, 64, 64, 90
    gen = torch.Generator().manual_seed(10 * k + large)
    x = torch.randn(B, Cin, L, generator=gen).to(DEV)
    ws = [(torch.randn(Cout, Cin, k, generator=gen) * (2.0 / (Cin * k)) ** 0.5).to(DEV).requires_grad_(True) for _ in range(2)]
    g = torch.randn(B, 2 * Cout, L, generator=gen)
    g[:, large * Cout:(large + 1) * Cout] *= 2.0 ** 10
    g = g.to(DEV)
    y = torch.cat([ops.conv1d(x, w, None, k, d, bool(causal)) for w in ws], 1)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    fails, fig = [], {}
    for i, w in enumerate(ws):
        dw, S = R.wgrad(g[:, i * Cout:(i + 1) * Cout].cpu().numpy(), x.cpu().numpy(), R.conv_shifts(k, d, causal))
        _held(w.grad, _dev(dw), _dev(S), "f16x2", fails, "half %d (the %s one)" % (i, "large" if i == large else "small"), fig)
    print("WGRADTILE cat halves k=%d large=%d: %s" % (k, large, "  ".join("%s %.3e" % kv for kv in sorted(fig.items()))))
    assert not fails, fails


# ---- reach -----------------------------------------------------------------------------------------------------------------------------------
def _probe_main():
    """Child process (SSV_SHAPE_LOG set): every row and every job table in both split modes, on zero operands."""
    for mode in R.SPLIT_MODES:
        with _mode(mode):
            for row in R.CASES:
                with _forced(R.force_key(row) if row.Z else None):
                    dy, x = _Strided(torch.zeros(row.B, row.Cout, row.L, device=DEV)), _Strided(torch.zeros(row.B, row.Cin, row.L, device=DEV))
                    _wgrad(row, dy, None, x, None, _Out((row.Cout, row.Cin, row.k), 0).t)
            for table in R.JOB_TABLES:
                _Table(table.jobs, zeros=True).run(table.max_shift)
            torch.cuda.synchronize()


@pytest.fixture(scope="module")
def shape_log():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "shapes.tsv")
        env = dict(os.environ, SSV_SHAPE_LOG=path, SSV_PRECISION="f16x2")
        env.pop("SSV_NT_FORCE", None)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_wgrad_tiles as t; t._probe_main()" % (root, os.path.join(root, "tests"))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return {(f[0], f[4]) for f in rows if len(f) >= 5}


REACH = [(form, mode) for form in R.SPLIT_FORMS for mode in R.SPLIT_MODES]


@pytest.mark.parametrize("form,mode", REACH, ids=["%s-%s" % c for c in REACH])
def test_every_row_reaches_the_program_the_restated_dispatch_predicts(shape_log, form, mode):
    """The library's own shape log holds, for every row and job table of the form, the kernel name and the note predicted for it -- with
    the forced slab count where the row forces one.  That ties the Python restatement to the dispatch, and keeps a later retune from
    emptying a case above unnoticed."""
    kernel = R.kernel_of(form, mode)
    rows, tables = R.rows_of(form), [t for t in R.JOB_TABLES if t.form == form]
    assert rows or tables
    seen = lambda note: [n for k_, n in shape_log if k_ == kernel and n.startswith(note) and (note.endswith("=") or n == note)]
    for row in rows:
        assert R.predicted(row, mode) == kernel
        note = R.note_of(1, row.B, row.Cout, row.Cin, row.L, row.k, R.clamped_z(row, mode))
        assert seen(note), (R.row_id(row), kernel, note, sorted(kn for kn in shape_log if kn[1].startswith(R.note_of(1, row.B, row.Cout, row.Cin, row.L, row.k))))
    for t in tables:
        r = t.jobs[0]
        note = R.note_of(len(t.jobs), r.B, r.Cout, r.Cin, r.L, r.k)
        assert seen(note), (t.name, kernel, note, sorted(kn for kn in shape_log if kn[1].startswith(note)))


def test_fallback_and_length_one_rows_run_no_split_kernel(shape_log):
    for row in R.rows_of("fallback") + R.rows_of("len1"):
        key = " B=%d M=%d Nc=%d L=%d k=%d " % (row.B, row.Cout, row.Cin, row.L, row.k)
        assert not [kn for kn in shape_log if key in " " + kn[1]], (R.row_id(row), "ran a split kernel")
    names = {k_ for k_, n in shape_log if k_.startswith("gemm_nt")}
    assert names == {R.kernel_of(f, m) for f in R.SPLIT_FORMS for m in R.SPLIT_MODES}, sorted(names)
