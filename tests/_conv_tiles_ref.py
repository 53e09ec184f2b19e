"""The Conv1d forward / data-gradient dispatch of csrc/conv_nn.hip restated in Python, a plain numpy float64 reference of the two products,
and the case tables of tests/test_gpu_conv_tiles.py (pinned on the CPU by tests/test_conv_tiles_cpu.py).  No device, no library.

Both products are one implicit GEMM: out(b, m, t) = add(b, m, t) + sum_j sum_c A_j[m][c] in(b, c, t + s_j), zero outside [0, N).
  forward        rows m = output channels, reduction c = input channels, A_j = w[:, :, j], s_j = shift_j, add = bias + bias_b
  data gradient  rows m = input channels, reduction c = output channels, A_j = w[:, :, j]^T, s_j = -shift_j, add = dx_add
A table row names (B, M, N, K) of that GEMM, so the same row runs the forward of a (Cin = K, Cout = M) layer and the data gradient of a
(Cin = M, Cout = K) layer on one instantiation: M rows, N columns per batch item, K reduction channels.

pick_tile says which of the 54 programs a shape runs: use_bf3 (ssv_host.h), the halo rule and launcher names (launch_nnb*), the extra-row
condition (api_conv.hip conv_nn) and pick_nnb -- the wide rule, the SSV_NNB_FORCE knob, then the cost model in its own tie order."""
import collections
import math

import numpy as np

HALO_SMALL = 16              # SSV_NN_HALO_SMALL (csrc/bf3_tuning.h)
MIN_SPLIT_CHANNELS = 32      # SSV_MIN_SPLIT_CHANNELS (csrc/ssv_host.h)
NTS = (7, 6, 4, 2)           # the order pick_nnb tries the column counts in
XROW_KPAD_MAX = 1056


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------------
def conv_shifts(k, d, causal):
    """conv_shifts of csrc/api_conv.hip: the column offset of tap j."""
    assert k in (1, 3) and d >= 1 and d * (k - 1) <= 54
    j0 = k - 1 if causal else (k - 1) // 2
    return [(j - j0) * d for j in range(k)]


def span_of(k, d):
    return (k - 1) * d


def cdiv(a, b):
    return -(-a // b)


def pad32(n):
    return (n + 31) & ~31


def use_bf3(B, L, Cin, Cout, mode):
    """mode: "fp32", "bf16x3" or "f16x2" (ssv_precision 0, 1, 2)."""
    return mode != "fp32" and B * L >= 128 and Cin >= MIN_SPLIT_CHANNELS and Cout >= MIN_SPLIT_CHANNELS


def plain_name(kt, wm, nt, f16, span):
    return "gemm_nn_bf3_kernel<%d, %d, %d, 0, %d, %d>" % (kt, wm, nt, f16, HALO_SMALL if (kt == 3 and span <= HALO_SMALL) else 54)


def wide_name(nt, nwn, f16, xrow=False):
    return "gemm_nn_bf3w_kernel<1, 2, %d, %d, %d%s>" % (nt, nwn, f16, ", 1" if xrow else "")


def cost_model(kt, B, M, N, a_max=2):
    """The (wm, nt) pick_nnb's cost model chooses: first strict minimum over a = a_min .. a_max, c in NTS."""
    a_min = 2 if (kt == 1 and B > 1 and M > 64 and a_max == 2) else 1
    best, pick = 1e30, (2, 7)
    for a in range(a_min, a_max + 1):
        for c in NTS:
            tiles = cdiv(M, 64 * a) * cdiv(N, 16 * c) * B
            per_tile = float(a) * c + 0.9 * a + 0.25 * c + 1.0
            n = (tiles + 255) // 256
            overlap = (1.8 if n >= 3 else (1.5 if n == 2 else 1.0)) if kt == 1 else 1.0
            lonely = 1.35 if tiles <= 256 else 1.0
            cost = float(n) * per_tile * lonely / overlap
            if cost < best:
                best, pick = cost, (a, c)
    return pick


def pick_tile(kt, B, M, N, K, colstats=False, forced=None, span=0, mode="f16x2"):
    """The instantiation a Conv1d product of M rows, N columns, K reduction channels and B items runs, as the shape log prints it; None where
    the exact-fp32 kernel of gemm_nn.hip runs instead.  forced: the (wm, nt) SSV_NNB_FORCE names for this (kt, M, N), or None.  span: the
    columns between the outermost taps, (k - 1) dilation."""
    if not use_bf3(B, N, K, M, mode):
        return None
    f16 = 1 if mode == "f16x2" else 0
    if kt == 1 and not colstats and N >= 1024 and M >= 256 and K >= 256 and cdiv(M, 128) * cdiv(N, 192) * B >= 256:
        if M > 128 and M % 128 == 1 and pad32(K) <= XROW_KPAD_MAX:              # (M > 128: the xrow_w condition of conv_nn)
            return wide_name(6, 2, f16, xrow=True)
        return wide_name(6, 2, f16) if M % 128 == 0 else wide_name(7, 4, f16)
    # column statistics go by whole 64-row groups of a row tile: M % 128 == 64 takes 64-row tiles, whatever the model or a force says
    a_max = 1 if (colstats and M % 128 != 0) else 2
    if forced is not None and forced[0] in (1, 2) and forced[0] <= a_max and forced[1] in NTS:
        wm, nt = forced
    else:
        wm, nt = cost_model(kt, B, M, N, a_max)
    return plain_name(kt, wm, nt, f16, span)


def note_of(kt, B, M, N, K, colstats=False, xrow=False):
    """The note the launchers put beside the kernel name in the shape log."""
    return "B=%d M=%d N=%d K=%d k=%d%s" % (B, M, N, K, kt, " (last row beside the tiles)" if xrow else (" +colstats" if colstats else ""))


# ---- reference -----------------------------------------------------------------------------------------------------------------------------
def shifted(a, s):
    """a(..., t + s), zero outside [0, N)."""
    if s == 0:
        return a
    out = np.zeros_like(a)
    n = a.shape[-1]
    if abs(s) < n:
        if s > 0:
            out[..., :n - s] = a[..., s:]
        else:
            out[..., -s:] = a[..., :n + s]
    return out


def _sum_taps(a, mats, shifts, adds, dtype):
    a = np.asarray(a, dtype=dtype)
    out = None
    for m, s in zip(mats, shifts):
        term = np.matmul(np.asarray(m, dtype=dtype), shifted(a, s))           # (M, K) x (B, K, N) -> (B, M, N), one matmul per tap
        out = term if out is None else out + term
    for t in adds:
        out = out + np.asarray(t, dtype=dtype)
    assert out.dtype == dtype
    return out


def _fwd_terms(x, w, bias, bias_b, shifts):
    mats = [w[:, :, j] for j in range(w.shape[2])]
    return x, mats, list(shifts), [bias[None, :, None], bias_b[:, :, None]]


def _dgrad_terms(dy, w, dx_add, shifts):
    mats = [w[:, :, j].T for j in range(w.shape[2])]
    return dy, mats, [-s for s in shifts], [dx_add]


def _with_scale(terms, dtype):
    a, mats, shifts, adds = terms
    out = _sum_taps(a, mats, shifts, adds, dtype)
    if dtype != np.float64:
        return out
    S = _sum_taps(np.abs(np.asarray(a, dtype=np.float64)), [np.abs(np.asarray(m, dtype=np.float64)) for m in mats], shifts,
                  [np.abs(np.asarray(t, dtype=np.float64)) for t in adds], np.float64)
    return out, S


def conv_fwd(x, w, bias, bias_b, shifts, dtype=np.float64):
    """y(b, o, t) = bias[o] + bias_b[b, o] + sum_{j, c} w[o, c, j] x(b, c, t + shift_j) for x (B, Cin, L), w (Cout, Cin, k).  float64:
    (y, S) with S = sum |w| |x| + |bias| + |bias_b| per element; another dtype: y alone, every operand and every matmul in that dtype."""
    return _with_scale(_fwd_terms(x, w, bias, bias_b, shifts), dtype)


def conv_dgrad(dy, w, dx_add, shifts, dtype=np.float64):
    """dx(b, c, t) = dx_add(b, c, t) + sum_{j, o} w[o, c, j] dy(b, o, t - shift_j) for dy (B, Cout, L), w (Cout, Cin, k); (dx, S) as conv_fwd."""
    return _with_scale(_dgrad_terms(dy, w, dx_add, shifts), dtype)


def colstats(y):
    """(B, M / 64, N, 2): per 64-row group and column, the mean of y and the sum of its squared deviations from that mean."""
    B, M, N = y.shape
    g = np.asarray(y, dtype=np.float64).reshape(B, M // 64, 64, N)
    mean = g.mean(axis=2)
    return np.stack([mean, ((g - mean[:, :, None]) ** 2).sum(axis=2)], axis=-1)


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel()))


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
# form: ("plain", kt, wm, nt, halo) | ("wide", nt, nwn) | ("xrow",)
Row = collections.namedtuple("Row", "form kt B M N K d causal colstats forced")


def form_id(form):
    if form is None:
        return "half_group"
    if form[0] == "plain":
        return "k%d_%dx%d_h%d" % (form[1], 64 * form[2], 16 * form[3], form[4])
    return "wide_128x192_xrow" if form[0] == "xrow" else "wide_128x%d" % (16 * form[1] * form[2])


def kernel_of(form, mode):
    """The launcher's name of the instantiation, for the split mode ``mode``."""
    f16 = 1 if mode == "f16x2" else 0
    if form[0] == "plain":
        return "gemm_nn_bf3_kernel<%d, %d, %d, 0, %d, %d>" % (form[1], form[2], form[3], f16, form[4])
    return wide_name(6, 2, f16, xrow=True) if form[0] == "xrow" else wide_name(form[1], form[2], f16)


def predicted(row, mode):
    return pick_tile(row.kt, row.B, row.M, row.N, row.K, False, row.forced, span_of(row.kt, row.d), mode)


def row_id(r):
    return "%s-B%d_M%d_N%d_K%d_d%d%s%s" % (form_id(r.form), r.B, r.M, r.N, r.K, r.d, "c" if r.causal else "", "" if r.forced else "_free")


PLAIN_FORMS = [("plain", kt, wm, nt, halo) for kt in (1, 3) for wm in (2, 1) for nt in NTS for halo in ((54,) if kt == 1 else (HALO_SMALL, 54))]
WIDE_FORMS = [("wide", 6, 2), ("wide", 7, 4), ("xrow",)]
FORMS = PLAIN_FORMS + WIDE_FORMS
TILES = [(kt, wm, nt) for kt in (1, 3) for wm in (2, 1) for nt in NTS]


def _tile_cases():
    rows = []
    for form in PLAIN_FORMS:
        _, kt, wm, nt, halo = form
        BM, BN = 64 * wm, 16 * nt
        variants = [(1, 0)] if kt == 1 else [(d, c) for d in ((1, 8) if halo == HALO_SMALL else (9, 27)) for c in (0, 1)]
        for M in (BM - 15, BM + 1, 2 * BM):              # a partly filled last 16-row block; a second row tile of one row; whole tiles
            for N in (BN - 1, BN + 1, 2 * BN):           # a ragged only column tile; a second column tile of one column; whole tiles
                for K in (40, 96):                       # a ragged last chunk (two chunks); three chunks through the two LDS images
                    for d, causal in variants:
                        rows.append(Row(form, kt, max(2, cdiv(128, N)), M, N, K, d, causal, M == 2 * BM, (wm, nt)))
    return rows


TILE_CASES = _tile_cases()

# The smallest shapes the wide rule of pick_nnb admits (N >= 1024, M >= 256, K >= 256, ceil(M / 128) ceil(N / 192) B >= 256): B = 22 is the
# first with 2 x 6 x B >= 256, B = 15 the first with 3 x 6 x B >= 256.  N = 1025 / 1345: one column into a 192- / 448-column tile.  K = 264: a
# ragged last chunk; K = 1056: the last K the extra-row rule admits (Kpad <= 1056); K = 1057: the same shape on the 128 x 448 tile instead.
WIDE_CASES = [
    Row(("wide", 6, 2), 1, 22, 256, 1024, 256, 1, 0, False, None),
    Row(("wide", 6, 2), 1, 22, 256, 1025, 256, 1, 0, False, None),
    Row(("wide", 7, 4), 1, 15, 300, 1024, 264, 1, 0, False, None),
    Row(("wide", 7, 4), 1, 15, 300, 1345, 264, 1, 0, False, None),
    Row(("wide", 7, 4), 1, 15, 257, 1025, 1057, 1, 0, False, None),
    Row(("xrow",), 1, 15, 257, 1025, 264, 1, 0, False, None),
    Row(("xrow",), 1, 15, 257, 1025, 1056, 1, 0, False, None),
]

# The cheapest shape (least B M N; K = 32 -- K enters neither the cost model nor, below 256, the wide rule) of the box B <= 8, 32 <= M <= 512,
# N <= 2048, B N >= 128 on which pick_nnb's cost model chooses each plain tile by itself, ties to the smallest (B, M, N): natural_search() below,
# re-run by tests/test_conv_tiles_cpu.py.  (kt, wm, nt): (B, M, N)
NATURAL = {
    (1, 1, 2): (1, 32, 128), (1, 2, 2): (2, 65, 64), (1, 2, 4): (7, 129, 1729), (1, 2, 7): (7, 385, 1729),
    (3, 1, 2): (1, 32, 128), (3, 1, 4): (7, 65, 1729), (3, 1, 6): (6, 65, 1345), (3, 1, 7): (7, 193, 1729),
    (3, 2, 2): (5, 193, 1601), (3, 2, 4): (7, 193, 2017), (3, 2, 6): (8, 385, 1457), (3, 2, 7): (7, 385, 1729),
}
FORCED_ONLY = [(1, 2, 6), (1, 1, 7), (1, 1, 6), (1, 1, 4)]
NATURAL_BOX = dict(B=8, M=512, N=2048, K=32)


def natural_search(box=NATURAL_BOX):
    """({(kt, wm, nt): (B, M, N)}, [tiles no shape of the box selects]): the cost model over the whole box, vectorised (cost_model is the scalar
    form; the CPU test holds every found row to it through pick_tile)."""
    found = {}
    Ms = np.arange(MIN_SPLIT_CHANNELS, box["M"] + 1)[:, None]
    Ns = np.arange(1, box["N"] + 1)[None, :]
    for kt in (1, 3):
        for B in range(1, box["B"] + 1):
            costs = []
            for a in (1, 2):
                for c in NTS:
                    tiles = (-(-Ms // (64 * a))) * (-(-Ns // (16 * c))) * B
                    per_tile = float(a) * c + 0.9 * a + 0.25 * c + 1.0
                    n = (tiles + 255) // 256
                    overlap = np.where(n >= 3, 1.8, np.where(n == 2, 1.5, 1.0)) if kt == 1 else 1.0
                    lonely = np.where(tiles <= 256, 1.35, 1.0)
                    cost = n.astype(np.float64) * per_tile * lonely / overlap
                    if a == 1 and kt == 1 and B > 1:
                        cost = np.where(Ms > 64, np.inf, cost)
                    costs.append(cost)
            pick = np.argmin(np.stack(costs), axis=0)                           # the first minimum: pick_nnb's strict "<"
            size = np.where(B * Ns >= 128, B * Ms * Ns, np.iinfo(np.int64).max)
            for i, (a, c) in enumerate((a, c) for a in (1, 2) for c in NTS):
                s = np.where(pick == i, size, np.iinfo(np.int64).max)
                at = np.unravel_index(np.argmin(s), s.shape)
                if s[at] == np.iinfo(np.int64).max:
                    continue
                cand = (B, int(Ms[at[0], 0]), int(Ns[0, at[1]]))
                old = found.get((kt, a, c))
                if old is None or cand[0] * cand[1] * cand[2] < old[0] * old[1] * old[2]:
                    found[(kt, a, c)] = cand
    return found, [t for t in TILES if t not in found]


def _natural_cases():
    rows = []
    for (kt, wm, nt), (B, M, N) in sorted(NATURAL.items()):
        rows.append(Row(("plain", kt, wm, nt, HALO_SMALL if kt == 3 else 54), kt, B, M, N, NATURAL_BOX["K"], 1, 0, False, None))
    return rows


NATURAL_CASES = _natural_cases()

# Column statistics of a product whose last 64 rows would be the FIRST half of a 128-row tile (M = 192): the second group of that tile is the next
# batch item's first group, and past the buffer for the last item.  pick_nnb keeps such a product on 64-row tiles; these rows ask for the
# 128 x 112 tile by force, and (k = 1, B > 1, M > 64) by the cost model's own a_min = 2.  The plain forward of the same shape (no statistics)
# does run the forced tile, so the rows are in no form's list: tests/test_gpu_conv_tiles.py runs them on their own.
HALF_GROUP_CASES = [
    Row(None, 1, 3, 192, 70, 40, 1, 0, True, (2, 7)),
    Row(None, 3, 3, 192, 70, 40, 1, 1, True, (2, 7)),
    Row(None, 1, 3, 192, 70, 40, 1, 0, True, None),
]


def rows_of(form):
    return [r for r in TILE_CASES + WIDE_CASES + NATURAL_CASES if r.form == form]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "x w bias bias_b dy wd dx_add")


def inputs(row):
    """float32 operands of a row: the forward of a (Cin = K, Cout = M) layer -- x (B, K, N), w (M, K, kt), bias (M,), bias_b (B, M) -- and the
    data gradient of a (Cin = M, Cout = K) layer -- dy (B, K, N), wd (K, M, kt), dx_add (B, M, N).  Standard normal activations, weights of
    the variance a layer of that fan-in is initialised with."""
    rng = np.random.default_rng([row.kt, row.B, row.M, row.N, row.K, row.d, row.causal])
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    sc = np.float32(math.sqrt(2.0 / (row.K * row.kt)))
    return Inputs(f(row.B, row.K, row.N), f(row.M, row.K, row.kt) * sc, f(row.M), f(row.B, row.M),
                  f(row.B, row.K, row.N), f(row.K, row.M, row.kt) * sc, f(row.B, row.M, row.N))


def reference(row, inp, dtype=np.float64):
    """((y, Sy), (dx, Sdx)) in float64, (y, dx) in another dtype."""
    sh = conv_shifts(row.kt, row.d, row.causal)
    return conv_fwd(inp.x, inp.w, inp.bias, inp.bias_b, sh, dtype), conv_dgrad(inp.dy, inp.wd, inp.dx_add, sh, dtype)


def f32_error(row):
    """The largest |err| / S of the row's two products evaluated in numpy float32."""
    inp = inputs(row)
    (y, Sy), (dx, Sdx) = reference(row, inp)
    y32, dx32 = reference(row, inp, np.float32)
    return max(float((np.abs(y32 - y) / Sy).max()), float((np.abs(dx32 - dx) / Sdx).max()))


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------
# Per element, |got - float64| <= bar S.  F32_WORST is the largest f32_error over every row of TILE_CASES, WIDE_CASES and NATURAL_CASES (computed
# on the CPU from the tables' own inputs; tests/test_conv_tiles_cpu.py recomputes it row by row and holds it to this constant).
#   exact fp32  4 x F32_WORST: the factor covers the difference in summation order between numpy's matmul and the kernels' 32-wide chunks
#   f16x2       + 2^-21: each operand keeps 22 significand bits, so a product is off by at most 2^-21 of |w| |x|
#   bf16x3      15 x the f16x2 bar: the ratio of the two whole-tensor bars the suite already holds (3e-5 and 2e-6)
F32_WORST = 4.151875321046948e-07         # at a k = 3 row of TILE_CASES; the wide rows reach 3.9e-7, the natural ones 3.1e-7
BAR_F32 = 4.0 * F32_WORST
BAR_F16 = BAR_F32 + 2.0 ** -21
BAR_BF3 = 15.0 * BAR_F16
BARS = {"fp32": BAR_F32, "f16x2": BAR_F16, "bf16x3": BAR_BF3}
L2_BARS = {"fp32": 2e-6, "f16x2": 2e-6, "bf16x3": 3e-5}           # whole-tensor relative L2 (tests/test_gpu_accuracy.py)
COLSTATS_BAR = 2e-5                                                # of the largest mean / M2 (tests/test_gpu_bench_shapes.py)
