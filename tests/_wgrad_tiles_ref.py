"""The Conv1d weight-gradient dispatch of csrc/api_conv.hip / csrc/wgrad_nt.hip restated in Python, the range-slab partition of the extra-row
kernel, a plain numpy float64 reference of the product, and the case tables of tests/test_gpu_wgrad_tiles.py (pinned on the CPU by
tests/test_wgrad_tiles_cpu.py).  No device, no library.

  dw(o, c, j) = sum_{b, t} dy(b, o, t) x(b, c, t + shift_j),  x zero outside [0, L);  S(o, c, j) = sum |dy| |x|
for dy (B, Cout, L), x (B, Cin, L) and the shifts of (k, dilation, causal) as ssv_conv_shifts gives them.  The kernels call Cout "M" and Cin
"Nc"; a row of the tables is (B, Cin, Cout, L, k, dilation, causal, forced Z or None).

predicted() says which program a row runs, as ssv_launch_gemm_nt_bf3 logs it: wgrad_bf3_runs (api_conv.hip), ssv_nt_bf3_tile and
ssv_nt_bf3_xrow (wgrad_nt.hip), the ring rule (k = 3 and every |shift| <= 64; with a job table, the caller's bound), else the exact-fp32
kernel gemm_nt.hip chooses, or the L = 1 kernel of misc.hip.  The slab count Z is NOT modelled (nt_slabs is a cost model that a retune may
change): a row either forces it (SSV_NT_FORCE="M:Nc:k=Z", clamped by dw_splits as clamped_z does) or leaves it to the library, and the tests
take it from the shape log or from ssv_conv1d_bwd_weight_multi_splits."""
import collections

import numpy as np

from _conv_tiles_ref import cdiv, conv_shifts, rel_l2, shifted  # noqa: F401  (the same shift table and helpers as the other two products)

MIN_SPLIT_CHANNELS = 32      # SSV_MIN_SPLIT_CHANNELS (csrc/ssv_host.h)
KB = 64                      # time steps per chunk of both split kernels
SPLIT_MODES = ("f16x2", "bf16x3")
MODES = SPLIT_MODES + ("fp32",)


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------------
def wgrad_bf3_runs(B, Cin, Cout, L, mode):
    """wgrad_bf3_runs of api_conv.hip for operands whose spans stay below 2^30 elements (ssv_nt_bf3_fits: and L >= 8)."""
    return mode != "fp32" and B * L >= 256 and Cin >= MIN_SPLIT_CHANNELS and Cout >= MIN_SPLIT_CHANNELS and L >= 8


def nt_bf3_tile(kt, M, Nc):
    """ssv_nt_bf3_tile: (wm, ntc); wm = 4 stands for 8 waves x 32 rows."""
    if kt == 3:
        return 2, 4
    if Nc <= 48:
        return 2, 2
    if M % 256 == 0 and Nc % 128 == 0 and M * Nc >= 1 << 21:
        return 4, 8
    if M % 128 == 0 and Nc % 128 == 0 and M * Nc >= 1 << 21:
        return 2, 8
    if M * Nc >= 1 << 18:
        return 2, 6
    return 1, 4


def nt_bf3_xrow(kt, M, Nc):
    """ssv_nt_bf3_xrow: the last of 128 j + 1 output rows beside the tiles, range slabs."""
    return kt == 1 and nt_bf3_tile(kt, M, Nc) == (2, 6) and M > 128 and M % 128 == 1


def tiles_of(kt, M, Nc):
    """(row tiles, column tiles) of the launch: gridDim.x is their product."""
    wm, ntc = nt_bf3_tile(kt, M, Nc)
    return cdiv(M - 1 if nt_bf3_xrow(kt, M, Nc) else M, 64 * wm), cdiv(Nc, 16 * ntc)


def ring_bound(kt, shifts, max_shift=None):
    """The largest |shift| the ring kernel is planned for, or -1 where gemm_nt_bf3_kernel<3, 2, 4> runs.  max_shift: a job table's stated
    bound (the shifts are on the device), None for the one-layer entry, which looks at its own shifts."""
    if kt != 3:
        return -1
    ms = max(abs(s) for s in shifts) if max_shift is None else max_shift
    return ms if 0 <= ms <= 64 else -1


def ring_tchunks(L, ms):
    """Chunks per item on the ring's virtual time line: tchunks 64 >= L + the largest |shift|."""
    return cdiv(L + ms, KB)


def split_kernel_name(kt, M, Nc, mode, ring_ms=-1):
    f16 = 1 if mode == "f16x2" else 0
    wm, ntc = nt_bf3_tile(kt, M, Nc)
    if ring_ms >= 0:
        return "gemm_nt3r_kernel<%d, %d>" % (wm, f16)
    if wm == 4:
        return "gemm_nt_bf3_kernel<%d, 2, %d, %d, 0, 8>" % (kt, ntc, f16)
    return "gemm_nt_bf3_kernel<%d, %d, %d, %d, %d, 4>" % (kt, wm, ntc, f16, 1 if nt_bf3_xrow(kt, M, Nc) else 0)


def fp32_kernel_name(kt, Nc):
    """ssv_launch_gemm_nt's choice (the exact kernels write no shape-log line; the name is for the printed figures)."""
    return "gemm_nt_kernel<3, 2, 2>" if kt == 3 else ("gemm_nt_kernel<1, 2, 6>" if Nc > 48 else "gemm_nt_kernel<1, 2, 2>")


def predicted(row, mode, max_shift=None):
    """The program a row runs: the split kernel's name as the shape log spells it, or the unlogged exact kernels' names."""
    if wgrad_bf3_runs(row.B, row.Cin, row.Cout, row.L, mode):
        ms = ring_bound(row.k, conv_shifts(row.k, row.d, row.causal), max_shift)
        return split_kernel_name(row.k, row.Cout, row.Cin, mode, ms)
    if row.L == 1 and row.k == 1:
        return "linear_len1_wgrad_kernel"
    return fp32_kernel_name(row.k, row.Cin)


def note_of(njobs, B, M, Nc, L, k, Z=None):
    """The note ssv_launch_gemm_nt_bf3 logs; Z = None: up to and including "Z=" (the count is the library's to choose)."""
    head = "jobs=%d B=%d M=%d Nc=%d L=%d k=%d Z=" % (njobs, B, M, Nc, L, k)
    return head if Z is None else head + "%d" % Z


def range_slabs_run(row, mode):
    return row.k == 1 and nt_bf3_xrow(1, row.Cout, row.Cin) and wgrad_bf3_runs(row.B, row.Cin, row.Cout, row.L, mode)


def clamped_z(row, mode="f16x2"):
    """What dw_splits makes of a forced Z: at most B, or at most B ceil(L / 64) for range slabs."""
    if row.Z is None:
        return None
    top = row.B * cdiv(row.L, KB) if range_slabs_run(row, mode) else row.B
    return max(1, min(row.Z, top))


def force_key(row):
    return "%d:%d:%d=%d" % (row.Cout, row.Cin, row.k, row.Z)


# ---- range slabs ---------------------------------------------------------------------------------------------------------------------------
def range_slabs(B, L, Z):
    """(per, [(start, total)] for z < Z): slab z owns `total` chunks from `start` of the item-major sequence of all B ceil(L / 64) chunks."""
    tch = cdiv(L, KB)
    allc = B * tch
    per = cdiv(allc, Z)
    return per, [(z * per, max(min(per, allc - z * per), 0)) for z in range(Z)]


def empty_slabs(B, L, Z):
    return [z for z, (_, total) in enumerate(range_slabs(B, L, Z)[1]) if total == 0]


def mid_item_starts(B, L, Z):
    """Non-empty slabs that begin inside a batch item."""
    tch = cdiv(L, KB)
    return [z for z, (start, total) in enumerate(range_slabs(B, L, Z)[1]) if total > 0 and start % tch != 0]


def chunks_per_workgroup(row, mode="f16x2"):
    """Whole-item slabs: the chunk counts the Z slabs of a forced row reduce over (the ring counts its own tchunks)."""
    Z = clamped_z(row, mode)
    sh = conv_shifts(row.k, row.d, row.causal)
    ms = ring_bound(row.k, sh)
    tch = ring_tchunks(row.L, ms) if ms >= 0 else cdiv(row.L, KB)
    return [cdiv(row.B - z, Z) * tch for z in range(Z)]


# ---- reference -----------------------------------------------------------------------------------------------------------------------------
def wgrad(dy, x, shifts, dtype=np.float64):
    """dw (Cout, Cin, k); float64: (dw, S).  Another dtype: dw alone, both operands and the product (one GEMM over B L per tap) in it."""
    dy, x = np.asarray(dy, dtype=dtype), np.asarray(x, dtype=dtype)
    taps = [np.tensordot(dy, shifted(x, s), axes=([0, 2], [0, 2])) for s in shifts]
    dw = np.stack(taps, axis=-1)
    assert dw.dtype == dtype
    if dtype != np.float64:
        return dw
    ady, ax = np.abs(dy), np.abs(x)
    S = np.stack([np.tensordot(ady, shifted(ax, s), axes=([0, 2], [0, 2])) for s in shifts], axis=-1)
    return dw, S


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
# Z: the slab count the row forces, None for the library's own; seed: tells the jobs of one table apart
Row = collections.namedtuple("Row", "form B Cin Cout L k d causal Z seed")
Row.__new__.__defaults__ = (None, 0)

# form -> (kt, wm, ntc, extra row) of the split kernel, None for the ring
SPLIT_FORMS = collections.OrderedDict([
    ("k1_64x64", (1, 1, 4, 0)), ("k1_128x32", (1, 2, 2, 0)), ("k1_128x96", (1, 2, 6, 0)), ("k1_128x96_xrow", (1, 2, 6, 1)),
    ("k1_128x128", (1, 2, 8, 0)), ("k1_256x128_w8", (1, 4, 8, 0)), ("ring", None), ("k3_128x64", (3, 2, 4, 0)),
])
FP32_FORMS = ("gemm_nt_kernel<3, 2, 2>", "gemm_nt_kernel<1, 2, 6>", "gemm_nt_kernel<1, 2, 2>")
FORMS = list(SPLIT_FORMS) + ["fallback", "len1"]


def kernel_of(form, mode):
    """The shape log's name of a split form."""
    f16 = 1 if mode == "f16x2" else 0
    if form == "ring":
        return "gemm_nt3r_kernel<2, %d>" % f16
    kt, wm, ntc, xr = SPLIT_FORMS[form]
    if wm == 4:
        return "gemm_nt_bf3_kernel<%d, 2, %d, %d, 0, 8>" % (kt, ntc, f16)
    return "gemm_nt_bf3_kernel<%d, %d, %d, %d, %d, 4>" % (kt, wm, ntc, f16, xr)


def _rows(form, k, d, causal, table):
    out = []
    for B, Cin, Cout, L, zs in table:
        for Z in (zs if isinstance(zs, tuple) else (zs,)):
            out.append(Row(form, B, Cin, Cout, L, k, d, causal, Z))
    return out


# Every row runs a split kernel only from B L >= 256 on; the rows keep that with the smallest B.
CASES = (
    # gemm_nt_bf3_kernel<1, 1, 4>: Cin > 48, Cin Cout < 2^18
    _rows("k1_64x64", 1, 1, 0, [
        (4, 64, 64, 64, (1, 2, 4)),        # a workgroup reduces over 4, 2, 1 chunks: the prologue and the tested tail of the chunk loop alone
        (3, 65, 65, 90, None),             # a second row tile of one row, a second column tile of one channel, L % 8 = 2
        (2, 49, 33, 135, None),            # a partly filled 16-row block
        (32, 64, 128, 8, None),            # the shortest length: one 8-step window per row
        (32, 65, 129, 8, None),            # ... where the 64-step chunk of rows 121 .. 128 leaves the item from two waves of two row tiles
        (5, 64, 64, 200, 2),               # slabs of 3 and 2 items
    ]) +
    # <1, 2, 2>: Cin <= 48
    _rows("k1_128x32", 1, 1, 0, [(3, 33, 129, 90, None), (2, 48, 128, 128, None), (5, 32, 32, 52, None)]) +
    # <1, 2, 6> without the extra row
    _rows("k1_128x96", 1, 1, 0, [
        (2, 512, 512, 130, None),
        (3, 2017, 130, 90, None),          # the last column tile holds one channel; the second row tile two rows
        (2, 3169, 130, 130, None),         # 2 x 34 = 68 tiles: the ct_fast order
    ]) +
    # <1, 2, 6, ., 1>: 128 j + 1 rows, range slabs
    _rows("k1_128x96_xrow", 1, 1, 0, [
        (4, 1021, 257, 70, (1, 3, 5, 8, None)),   # 8 chunks.  Z = 3: 3 + 3 + 2, two slabs starting mid-item; Z = 5: the fifth slab empty; Z = 8: one chunk each
        (3, 2033, 129, 90, None),          # one row tile
        (16, 1021, 257, 24, None),         # rows shorter than a chunk: MFMA row 255 runs through row 256 and out of the item
        (5, 512, 513, 64, (2, 4)),         # ranges of 3 + 2 chunks, and of 2 + 2 + 1 + 0
    ]) +
    # <1, 2, 8>, 4 waves
    _rows("k1_128x128", 1, 1, 0, [(2, 5504, 384, 128, None), (3, 5504, 384, 90, None)]) +           # 3 x 43 = 129 tiles
    # <1, 2, 8, ., 0, 8>, 8 waves
    _rows("k1_256x128_w8", 1, 1, 0, [(2, 8192, 256, 128, None), (3, 4224, 512, 90, None)]) +        # 64 tiles (the last plain order), 66 tiles
    # the ring, k = 3
    # (Z = 1: the items follow each other on one slab's time line, so a tap that leaves an item lands in its neighbour unless the padding chunks
    # are there -- left to itself the library gives these small rows one slab per item, which hides a chunk count computed without max_shift)
    _rows("ring", 3, 1, 0, [(4, 64, 128, 64, (None, 1)), (32, 64, 128, 8, None)]) +                  # L + 1 = 65: a second chunk for one row of padding
    _rows("ring", 3, 27, 1, [(4, 65, 129, 74, (None, 1)), (4, 65, 129, 75, (None, 1))]) +            # L + 54 = 128: two chunks exactly; three chunks
    _rows("ring", 3, 3, 0, [(5, 64, 128, 200, (1, 5))]) +              # Z = 1: 20 chunks in one slab -- the ring wraps, the mirror rows are read
    _rows("ring", 3, 13, 0, [(2, 100, 70, 193, None)]) +
    # the exact-fp32 kernels in the split modes, and linear_len1_wgrad_kernel
    _rows("fallback", 1, 1, 0, [(3, 64, 64, 85, (None, 3)), (37, 64, 64, 7, None), (4, 31, 64, 64, None)]) +       # B L = 255; L < 8; Cin < 32
    _rows("fallback", 3, 2, 0, [(8, 16, 24, 40, None)]) +
    _rows("len1", 1, 1, 0, [(B, 7, 5, 1, None) for B in (1, 3, 4, 5, 9)])
)
WIDE_ROWS = [r for r in CASES if r.form in ("k1_128x128", "k1_256x128_w8")]        # their float64 reference is computed on the device

# Job tables (ssv_conv1d_bwd_weight_multi): jobs of one shape, their own seeds.  max_shift: the caller's bound; nan_jobs: the jobs whose shifts
# exceed it and must come back all NaN; same_kernel: the one-layer entry runs the same program, so each job must equal it bitwise at the same Z.
JobTable = collections.namedtuple("JobTable", "name form jobs max_shift nan_jobs same_kernel")


def _ring_jobs():
    return [Row("ring", 4, 65, 129, 75, 3, d, 1, None, i + 1) for i, d in enumerate((1, 3, 9, 27))]


def _k1_jobs(form, B, Cin, Cout, L):
    return [Row(form, B, Cin, Cout, L, 1, 1, 0, None, i + 1) for i in range(2)]


JOB_TABLES = [
    JobTable("ring_ms54", "ring", _ring_jobs(), 54, (), True),
    JobTable("ring_ms64", "ring", _ring_jobs(), 64, (), True),
    JobTable("general_ms-1", "k3_128x64", _ring_jobs(), -1, (), False),      # the only way into <3, 2, 4>; the head-of-tensor clamp of its windows
    JobTable("ring_ms53", "ring", _ring_jobs(), 53, (3,), True),              # the dilation-27 causal job reaches 54 > 53
    JobTable("k1_64x64", "k1_64x64", _k1_jobs("k1_64x64", 3, 65, 65, 90), 0, (), True),
    JobTable("k1_xrow", "k1_128x96_xrow", _k1_jobs("k1_128x96_xrow", 4, 1021, 257, 70), 0, (), True),
]
PART_NBLK = (1, 9, 129)      # partial rows of a job (ssv_fold_rows: 8 row groups, 16 loads in flight per trip from 121 rows on)
PART_N2 = 70                 # not a multiple of the 32 outputs a workgroup owns


def all_rows():
    return list(CASES) + [r for t in JOB_TABLES[:1] + JOB_TABLES[4:] for r in t.jobs]      # (the four ring tables share their jobs)


def rows_of(form):
    return [r for r in CASES if r.form == form]


def row_id(r):
    return "%s-B%d_%dto%d_L%d_k%d_d%d%s_%s%s" % (r.form, r.B, r.Cin, r.Cout, r.L, r.k, r.d, "c" if r.causal else "",
                                                "Z%d" % r.Z if r.Z else "free", "_s%d" % r.seed if r.seed else "")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def inputs(row):
    """(dy (B, Cout, L), x (B, Cin, L)) float32, seeded standard normals (so S > 0 everywhere); the forced Z does not enter the seed."""
    rng = np.random.default_rng([row.B, row.Cin, row.Cout, row.L, row.k, row.d, row.causal, row.seed])
    return rng.standard_normal((row.B, row.Cout, row.L), dtype=np.float32), rng.standard_normal((row.B, row.Cin, row.L), dtype=np.float32)


def reference(row, dtype=np.float64):
    dy, x = inputs(row)
    out = wgrad(dy, x, conv_shifts(row.k, row.d, row.causal), dtype)
    if dtype == np.float64:
        assert (out[1] > 0).all(), row
    return out


def f32_error(row):
    """The largest |err| / S of the row's product evaluated in numpy float32."""
    dw, S = reference(row)
    return float((np.abs(reference(row, np.float32) - dw) / S).max())


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------
# Per element, |got - float64| <= bar S.  F32_WORST is the largest f32_error over all_rows() (computed on the CPU from the tables' own inputs;
# tests/test_wgrad_tiles_cpu.py recomputes it row by row and holds it to this constant).
#   exact fp32  4 x F32_WORST: the factor covers the difference in summation order between numpy's one GEMM over B L and the kernels' chunks
#               of 32 / 64 time steps, batch items and Z slabs
#   f16x2       + 2^-21: each operand keeps 22 significand bits, so a product is off by at most 2^-21 of |dy| |x|
#   bf16x3      15 x the f16x2 bar: the ratio of the two whole-tensor bars the suite already holds (3e-5 and 2e-6)
F32_WORST = 3.8433032871087677e-07        # at (2, 512, 512, 130); the wide rows reach 3.7e-7, the ring rows 2.9e-7, the L = 1 rows 1.1e-7
BAR_F32 = 4.0 * F32_WORST
BAR_F16 = BAR_F32 + 2.0 ** -21
BAR_BF3 = 15.0 * BAR_F16
BARS = {"fp32": BAR_F32, "f16x2": BAR_F16, "bf16x3": BAR_BF3}
L2_BARS = {"fp32": 2e-6, "f16x2": 2e-6, "bf16x3": 3e-5}           # relative L2 per tap (tests/test_gpu_accuracy.py)
PART_BAR = 1e-5                                                    # summed partial rows, of their largest (tests/test_gpu_bench_shapes.py)
