"""Plain numpy float64 restatements of the three narrow column-step kernels of csrc/synth.hip -- ssv_column_matvec, ssv_column_ln_act,
ssv_column_gate -- with the case tables of tests/test_gpu_column_step.py (pinned on the CPU by tests/test_column_step_ref_cpu.py).
No device, no library.

The tables are built around the index rules of column_matvec_kernel, restated here so that a row can say which of them it is there for:
a workgroup takes 4 output rows (one per wave; a wave with m >= M leaves after the barrier, its weight pointer clamped to row M - 1) and
8 batch items (dead items staged as zeros); the 8 lanes of an item take every 8th quad (float4) of the K = C k inputs, the first 24 quads
per lane (K <= 768, nq = K / 4 <= 192) prefetched with the index clamped to quad 0 past the end, the rest in a tail loop."""
import collections

import numpy as np

LANES_PER_ITEM = 8           # quads ks, ks + 8, ... of a row go to lane ks of the item's 8
PREFETCH_QUADS = 192         # 24 per lane: K = 768
ROWS_PER_GROUP = 4
ITEMS_PER_GROUP = 8
KMAX = 1536
EPS = 1e-5
STEP_TMAX = 21               # history length of every k = 3 row of MATVEC_CASES, stepped over t = 0 .. 20


# ---- references ------------------------------------------------------------------------------------------------------------------------
def matvec(w_tap_major, bias, bias_b, cur, hist, t, dil, Tmax):
    """out[b][m] = bias[m] + bias_b[b][m] + sum_{j, c} w[m][j][c] x_j[b][c] for w (M, k, C) tap-major, cur (B, C), hist (B, Tmax, C) (k = 1:
    ignored).  x_{k-1} = cur, x_j = hist[:, t - (k - 1 - j) dil]; a tap outside [0, Tmax) is zero.  bias (M,) and bias_b (B, M) may be None.
    Returns (out, S) with S[b][m] = sum |w x| + |bias[m]| + |bias_b[b][m]|, the quantity a float32 rounding bound is taken against."""
    w = np.asarray(w_tap_major, dtype=np.float64)
    cur = np.asarray(cur, dtype=np.float64)
    M, k, C = w.shape
    B = cur.shape[0]
    x = np.zeros((B, k, C))
    x[:, k - 1] = cur
    for j in range(k - 1):
        col = t - (k - 1 - j) * dil
        if 0 <= col < Tmax:
            x[:, j] = np.asarray(hist, dtype=np.float64)[:, col]
    x, w = x.reshape(B, k * C), w.reshape(M, k * C)
    out, S = x @ w.T, np.abs(x) @ np.abs(w).T
    if bias is not None:
        out, S = out + np.asarray(bias, dtype=np.float64)[None], S + np.abs(np.asarray(bias, dtype=np.float64))[None]
    if bias_b is not None:
        out, S = out + np.asarray(bias_b, dtype=np.float64), S + np.abs(np.asarray(bias_b, dtype=np.float64))
    return out, S


def _activate(n, act):
    if act == 1:
        return np.maximum(n, 0.0)
    if act == 2:
        return 1.0 / (1.0 + np.exp(-n))
    assert act == 0
    return n


def _ln(x, g, b):
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)                 # two passes, biased
    return (x - mu) / np.sqrt(var + EPS) * np.asarray(g, dtype=np.float64)[None] + np.asarray(b, dtype=np.float64)[None]


def ln_act(x, g, b, act):
    """act(LayerNorm over the channels of x (B, C)): eps 1e-5, two-pass biased variance; act 0 none, 1 relu, 2 sigmoid."""
    return _activate(_ln(x, g, b), act)


def gate(h, x, g1, b1, g2, b2):
    """The highway gate on one column: h (B, 2C) = H1 | H2, x (B, C): sigmoid(LN1(H1)) * LN2(H2) + (1 - sigmoid(LN1(H1))) * x."""
    C = np.asarray(x).shape[1]
    h = np.asarray(h, dtype=np.float64)
    sg = _activate(_ln(h[:, :C], g1, b1), 2)
    return sg * _ln(h[:, C:], g2, b2) + (1.0 - sg) * np.asarray(x, dtype=np.float64)


def matvec_bound(K, S):
    """|fl(sum) - sum| for a length-K float32 dot product in any order of summation, fused multiply-adds or not, plus two bias additions:
    gamma_{K+2} sum |terms| with u = 2^-24, which (K + 4) u covers for every K <= 1536."""
    return (K + 4) * 2.0 ** -24 * S


# ---- ssv_column_matvec: the case table -----------------------------------------------------------------------------------------------
MatvecCase = collections.namedtuple("MatvecCase", "name C k M B bias bias_b padded dil Tmax edge")

# (C, k) and what its K = C k is there for: nq against the lane stride of 8 quads, and against the 192 prefetched quads
_CK = [
    (4, 1, {"nq": 1, "nq%8": 1, "prefetch": "below"}),            # one quad: lane 0 of an item works alone
    (4, 3, {"nq": 3, "nq%8": 3, "prefetch": "below"}),
    (28, 1, {"nq": 7, "nq%8": 7, "prefetch": "below"}),           # one lane short of a full stride
    (12, 3, {"nq": 9, "nq%8": 1, "prefetch": "below"}),           # one quad into the second trip
    (36, 3, {"nq": 27, "nq%8": 3, "prefetch": "below"}),
    (80, 1, {"nq": 20, "nq%8": 4, "prefetch": "below"}),          # the mel input
    (764, 1, {"nq": 191, "nq%8": 7, "prefetch": "below"}),        # one quad short of the prefetch
    (768, 1, {"nq": 192, "nq%8": 0, "prefetch": "exact"}),        # the prefetch exactly exhausted
    (256, 3, {"nq": 192, "nq%8": 0, "prefetch": "exact"}),        # ... as production runs it (hidden 256, k = 3)
    (772, 1, {"nq": 193, "nq%8": 1, "prefetch": "tail"}),         # one quad in the tail loop
    (260, 3, {"nq": 195, "nq%8": 3, "prefetch": "tail"}),
    (1532, 1, {"nq": 383, "nq%8": 7, "prefetch": "tail"}),        # one quad short of the cap
    (512, 3, {"nq": 384, "nq%8": 0, "prefetch": "tail"}),         # the cap
    (1536, 1, {"nq": 384, "nq%8": 0, "prefetch": "tail"}),
]
# M: waves of the last row group that take the m >= M exit (and read the clamped row M - 1)
_M = [(1, {"M%4": 1, "row_groups": 1}), (3, {"M%4": 3, "row_groups": 1}), (4, {"M%4": 0, "row_groups": 1}), (5, {"M%4": 1, "row_groups": 2}),
      (80, {"M%4": 0, "row_groups": 20}), (513, {"M%4": 1, "row_groups": 129})]
# B: dead items of the last item group
_B = [(1, {"B%8": 1, "item_groups": 1}), (7, {"B%8": 7, "item_groups": 1}), (8, {"B%8": 0, "item_groups": 1}), (9, {"B%8": 1, "item_groups": 2}),
      (17, {"B%8": 1, "item_groups": 3})]
_BIAS = [(False, False), (True, False), (False, True), (True, True)]         # (bias, bias_b)
_DIL = (1, 3, 9)
PAD_CUR, PAD_OUT, PAD_BB, PAD_HIST = 8, 4, 12, 4         # floats added to the dense batch stride of a padded row (multiples of 4)


def _build_matvec_cases():
    """42 rows: every (C, k) three times, the other axes cycling at periods that are coprime enough for every value of an axis to meet at least
    two values of every other axis (tests/test_column_step_ref_cpu.py counts them)."""
    rows, n3 = [], 0
    for i in range(3 * len(_CK)):
        C, k, e = _CK[i % len(_CK)]
        (M, em), (B, eb) = _M[i % len(_M)], _B[i % len(_B)]
        bias, bias_b = _BIAS[i % len(_BIAS)]
        padded = bool((i // len(_CK) + i) % 2)
        dil = 0
        if k == 3:
            dil = _DIL[(n3 + 2 * (n3 // 6)) % 3]
            n3 += 1
        edge = dict(e, **em, **eb, strides="padded" if padded else "dense")
        name = "C%d-k%d-M%d-B%d-%s%s-%s%s" % (C, k, M, B, "b" if bias else "_", "s" if bias_b else "_", "pad" if padded else "dense",
                                             "-d%d" % dil if k == 3 else "")
        rows.append(MatvecCase(name, C, k, M, B, bias, bias_b, padded, dil, STEP_TMAX if k == 3 else 1, edge))
    return rows


MATVEC_CASES = _build_matvec_cases()


def matvec_strides(case):
    """(cur_bs, out_bs, bb_bs, hist_bs) in floats."""
    p = 1 if case.padded else 0
    return (case.C + p * PAD_CUR, case.M + p * PAD_OUT, case.M + p * PAD_BB, case.Tmax * case.C + p * PAD_HIST)


def matvec_inputs(case, seed=None):
    """float32 inputs of a row: w (M, k, C) tap-major, bias (M,) or None, bias_b (B, M) or None, x (B, Tmax, C): the input column of every
    frame (k = 1: one frame)."""
    rng = np.random.default_rng(MATVEC_CASES.index(case) if seed is None else seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = f(case.M, case.k, case.C)
    bias = f(case.M) if case.bias else None
    bias_b = f(case.B, case.M) if case.bias_b else None
    return w, bias, bias_b, f(case.B, case.Tmax, case.C)


def matvec_reference(case, w, bias, bias_b, x):
    """(out, S) of every frame of a row, (Tmax, B, M) each; the history of frame t holds the input columns of the frames before it."""
    outs = [matvec(w, bias, bias_b, x[:, t], x, t, case.dil, case.Tmax) for t in range(case.Tmax)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# ---- the position probe ------------------------------------------------------------------------------------------------------------
PROBE_CASES = [(36, 3), (256, 3), (768, 1), (772, 1), (512, 3), (1536, 1)]      # K = 108, 768 (both k), 772, 1536 (both k)
PROBE_ITEMS = 64
PROBE_M = 5


def probe_plan(C, k, B=PROBE_ITEMS):
    """One launch per entry: the flat tap-major positions p = j C + c of its items' one-hot inputs, B per launch (the last launch: what is
    left), every position of [0, C k) once."""
    K = C * k
    return [np.arange(p0, min(p0 + B, K), dtype=np.int64) for p0 in range(0, K, B)]


def probe_weights(C, k, M=PROBE_M):
    """(M, k, C) of distinct integers, all exact in float32."""
    assert M * C * k < 2 ** 24
    return (1 + np.arange(M * k * C, dtype=np.float32)).reshape(M, k, C)


# ---- ssv_column_ln_act / ssv_column_gate: the case tables ------------------------------------------------------------------------------
LN_CHANNELS = [1, 4, 63, 64, 65, 80, 255, 256, 257, 512, 513, 768, 769, 1023, 1024]     # a thread holds channels tid, tid + 256, ...: the
#                                                                 first thread's second, third and fourth channel go live at 257, 513, 769
LN_KINDS = ("normal", "mean100", "constant")
LN_PAD_X, LN_PAD_Y = 12, 4
LnCase = collections.namedtuple("LnCase", "C B act padded kind")
LN_CASES = [LnCase(C, B, act, padded, kind) for C in LN_CHANNELS for B in (1, 5) for act in (0, 1, 2) for padded in (False, True)
            for kind in LN_KINDS]
GATE_CASES = [LnCase(C, B, None, padded, kind) for C in LN_CHANNELS for B in (1, 5) for padded in (False, True) for kind in LN_KINDS]


def constant_value(b):
    """The constant column of item b: a power of two, so that the column's sum 2^e C is exact in float32 in any order."""
    return np.float32(2.0 ** (b - 1))


def ln_column(kind, B, C, rng):
    """x (B, C) float32 of the given kind: standard normal; mean 100, deviation 1; one constant per item."""
    if kind == "normal":
        return rng.standard_normal((B, C)).astype(np.float32)
    if kind == "mean100":
        return (100.0 + rng.standard_normal((B, C))).astype(np.float32)
    assert kind == "constant"
    return np.repeat(np.array([constant_value(b) for b in range(B)], dtype=np.float32)[:, None], C, axis=1)


def ln_inputs(case):
    """x (B, C), gamma, beta (C,) float32."""
    rng = np.random.default_rng(7919 * case.C + 31 * case.B + LN_KINDS.index(case.kind))
    x = ln_column(case.kind, case.B, case.C, rng)
    return x, rng.standard_normal(case.C).astype(np.float32), rng.standard_normal(case.C).astype(np.float32)


def gate_inputs(case):
    """h (B, 2C) = H1 | H2 (both of the row's kind), x (B, C) standard normal, g1, b1, g2, b2 (C,) float32."""
    rng = np.random.default_rng(104729 * case.C + 17 * case.B + LN_KINDS.index(case.kind))
    h = np.concatenate((ln_column(case.kind, case.B, case.C, rng), ln_column(case.kind, case.B, case.C, rng)), axis=1)
    x = rng.standard_normal((case.B, case.C)).astype(np.float32)
    return (h, x) + tuple(rng.standard_normal(case.C).astype(np.float32) for _ in range(4))


def _fma32(a, b, c):
    """float32 fma of float32 operands: the product is exact in float64 (48 bits)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def kernel_mean(total, C):
    """col_mean of csrc/synth.hip in its own arithmetic: q = fl(total * fl(1 / C)), then one correction by the exact residual
    total - C q -- the last step of a float32 division, which gives total / C correctly rounded."""
    fC = np.float32(C)
    inv = np.float32(1.0) / fC
    q = np.float32(total) * inv
    return _fma32(_fma32(-q, fC, total), inv, q)


def constant_mean_is_exact(C, b=0):
    """The kernels' mean of item b's constant column 2^e: the sum 2^e C is an exact float32 in any order, and kernel_mean of it is 2^e
    itself -- so every v - mu is 0 and the LayerNorm gives beta exactly."""
    c = constant_value(b)
    total = np.float32(c) * np.float32(C)
    return float(total) == float(c) * C and kernel_mean(total, C) == c


def rel_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (np.abs(want).max() + 1e-30))


def row_err(got, want):
    """Per item: max |got - want| over the item's row, relative to that row's own maximum."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want).max(axis=1)
    return d / (np.abs(want).max(axis=1) + 1e-30)


# ---- the whole run ---------------------------------------------------------------------------------------------------------------------
RUN = dict(B=9, N=11, frames=24, freq_bins=80, hidden=36, textemb=16, seed=36)        # hidden 36: every highway layer runs K = 108, nq = 27
RUN_MARGIN = 1e-3


def run_case(seed=None):
    """The conditioned tiny melSyn of the whole-run test with its inputs, on the CPU: (model, text (B, 1, N), spk (B, 200, 1))."""
    import torch
    from spoofsv_amd import train
    from spoofsv_amd.tts import melSyn
    seed = RUN["seed"] if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = melSyn(34, True, 200, textemb_dim=RUN["textemb"], freq_bins=RUN["freq_bins"], hidden_dim=RUN["hidden"])
    m.apply(train.init_weights)
    text = torch.randint(2, 33, (RUN["B"], 1, RUN["N"]), generator=gen)
    text[:, :, -1] = 1
    spk = 0.04 + 0.05 * torch.rand(RUN["B"], 200, 1, generator=gen)
    return m.eval(), text, spk


def run_oracle(m, text, spk):
    """oracle.tts_oracle.synthesize_loop in float64 on the model's state dict: Y (B, F, frames), A (B, N, frames), pma (frames, B) and
    the top-two margins of A (B, frames).  The oracle's functions take a double state dict as they are; its loop builds the first, all-zero
    frame with torch.zeros, i.e. in the default dtype, which is float64 for the duration of the call."""
    import torch
    from oracle import tts_oracle as TO
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            Y, A, pma = TO.synthesize_loop(text, spk.double(), sd, RUN["frames"] - 1, RUN["freq_bins"])
    finally:
        torch.set_default_dtype(prev)
    top = torch.topk(A, 2, dim=1).values
    return Y, A, pma, top[:, 0] - top[:, 1]
