"""Plain numpy restatements of Text2Mel's attention block and text path, the references of tests/test_gpu_attention_paths.py,
tests/test_gpu_attention_step.py and tests/test_gpu_text_path.py (pinned on the CPU by tests/test_attention_ref_cpu.py).  Everything
is float64 unless a ``dtype`` says otherwise; with ``dtype=numpy.float32`` the same lines are the measuring stick for a tolerance: what
float32 arithmetic loses on that input, in numpy's order of summation.

Also here, as plain Python, the dispatch rules of csrc/api_attn.hip: which kernels a training-attention shape reaches.  The GPU tests
name the branch in their ids and assert it against these functions, so a later change of a threshold there makes an id visibly wrong."""
import numpy as np

MASKED = -2.0 ** 32          # models/TTSModel.py:282-286: the logit of a position outside the forced window


def _softmax0(s):
    """Softmax over axis 0 of ``s`` in its own dtype."""
    e = np.exp(s - s.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True, dtype=s.dtype)


# ---- training attention, models/TTSModel.py:266-270 ----------------------------------------------------------------------------------
def train_attention(kv, q, dtype=np.float64):
    """kv (B, 2d, N) = K | V, q (B, d, T).  Returns A (B, N, T) = softmax over the text axis of K^T Q / sqrt(d) and rq (B, 2d, T) = [V A ; Q]."""
    kv, q = np.asarray(kv, dtype=dtype), np.asarray(q, dtype=dtype)
    d = q.shape[1]
    assert kv.shape[1] == 2 * d and kv.shape[0] == q.shape[0]
    k, v = kv[:, :d], kv[:, d:]
    s = np.einsum("bcn,bct->bnt", k, q) / dtype(np.sqrt(dtype(d)))
    a = np.stack([_softmax0(s[b]) for b in range(s.shape[0])])
    r = np.einsum("bcn,bnt->bct", v, a)
    return a, np.concatenate((r, q), axis=1)


# ---- one synthesis step, models/TTSModel.py:281-295 ----------------------------------------------------------------------------------
def step_attention(K, V, q, pma, dtype=np.float64):
    """K, V (d, N), q (d,), pma: the previous arg-max.  Logits K^T q / sqrt(d); every position outside [pma, pma + 2] is set to -2^32;
    softmax over n; the FIRST maximum; r = V a.  Returns (a (N,), idx, r (d,))."""
    K, V, q = np.asarray(K, dtype=dtype), np.asarray(V, dtype=dtype), np.asarray(q, dtype=dtype)
    d, N = K.shape
    # channel by channel, the same order for every position: two identical columns of K get bit-identical logits (a BLAS product may not)
    s = (np.ascontiguousarray(K) * q[:, None]).sum(axis=0, dtype=dtype) / dtype(np.sqrt(dtype(d)))
    n = np.arange(N)
    s = np.where((n < pma) | (n >= pma + 3), dtype(MASKED), s).astype(dtype)
    a = _softmax0(s)
    return a, int(np.argmax(a)), V @ a


def step_attention_batch(kv, q, pma, dtype=np.float64):
    """step_attention over items: kv (B, 2d, N), q (B, d), pma (B,).  Returns (a (B, N), idx (B,) int64, r (B, d))."""
    B, d = q.shape
    out = [step_attention(kv[b, :d], kv[b, d:], q[b], int(pma[b]), dtype) for b in range(B)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int64), np.stack([o[2] for o in out])


def top_two_gap(a):
    """Largest minus second-largest entry of every row of a (B, N) (N = 1: the gap to 0)."""
    if a.shape[1] == 1:
        return a[:, 0].copy()
    top = np.sort(a, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0]


# ---- text embedding, models/TTSModel.py:25-35 ------------------------------------------------------------------------------------------
def text_embed(ids, w, bias, dtype=np.float64):
    """ids (B, N) integers, w (E, V), bias (E,).  y (B, E, N) = one_hot(ids) W^T + bias; an id outside [0, V) has an all-zero one-hot row
    and contributes the bias only."""
    ids = np.asarray(ids)
    w, bias = np.asarray(w, dtype=dtype), np.asarray(bias, dtype=dtype)
    E, V = w.shape
    ok = (ids >= 0) & (ids < V)
    y = np.where(ok[:, None, :], w[:, np.where(ok, ids, 0)].transpose(1, 0, 2), dtype(0))
    return (y + bias[None, :, None]).astype(dtype)


def text_embed_grads(ids, dy, V, dtype=np.float64):
    """Gradients of sum(dy * text_embed(ids, w, bias)): dw (E, V) sums dy over the positions that hold each id (an id outside [0, V): none),
    dbias (E,) over all positions."""
    ids, dy = np.asarray(ids), np.asarray(dy, dtype=dtype)
    B, E, N = dy.shape
    dw = np.zeros((E, V), dtype=dtype)
    flat, g = ids.reshape(-1), dy.transpose(1, 0, 2).reshape(E, B * N)
    for v in range(V):
        sel = flat == v
        if sel.any():
            dw[:, v] = g[:, sel].sum(axis=1, dtype=dtype)
    return dw, g.sum(axis=1, dtype=dtype)


# ---- guided attention loss, train/ordinary.py:232-234 -------------------------------------------------------------------------------
def guided_att_loss(A, gaw, dtype=np.float64):
    """mean(A * gaw[:N, :T]) for A (B, N, T) and its gradient with respect to A, gaw[:N, :T] / (B N T) for every item."""
    A, gaw = np.asarray(A, dtype=dtype), np.asarray(gaw, dtype=dtype)
    B, N, T = A.shape
    w = gaw[:N, :T]
    loss = (A * w[None]).mean(dtype=dtype)
    return loss, np.broadcast_to(w / dtype(B * N * T), A.shape).astype(dtype)


# ---- the dispatch of csrc/api_attn.hip, restated ------------------------------------------------------------------------------------
AF_BN = 64                   # frame columns per workgroup of the fused kernels (csrc/attn_fused.hip)


def fused_ok(B, d, N, T):
    """ssv_attn_fused_ok: scores, softmax and V A (backward: dA, dS, dQ) in one launch."""
    return d % 64 == 0 and d <= 256 and 1 <= N <= 192 and T >= 1 and B <= 65535 and N * T < 2 ** 31 and 2 * d * T < 2 ** 31


def fused_instance(d, N):
    """(NB, DB) of AF_CASE: text rows in groups of 4 x 16, channels in groups of 64."""
    cdiv = lambda a, b: (a + b - 1) // b
    return cdiv(cdiv(N, 16), 4), d // 64


def softmax_branch(B, N, T):
    """ssv_launch_softmax_cols / _bwd: which column softmax the fallback chain runs."""
    if N <= 256 and B <= 65535 and N * T < 2 ** 31:
        return "tile8" if N <= 64 else "tile24" if N <= 192 else "tile32"
    return "percol"


def attention_path(B, d, N, T):
    if fused_ok(B, d, N, T):
        return "fused(%d,%d)" % fused_instance(d, N)
    return "fallback:" + softmax_branch(B, N, T)


def nt_bf3_fits(B, M, Nc, T, a_bs, x_bs):
    """ssv_nt_bf3_fits for the two reductions over time (rows of T contiguous frames): 32-bit operand offsets, rows of at least 8."""
    lim = 1 << 30
    return ((B - 1) * a_bs + (M - 1) * T + T < lim and (B - 1) * x_bs + (Nc - 1) * T + T < lim and B * a_bs < lim and B * x_bs < lim
            and T >= 8)


def dkdv_branch(mode, B, d, N, T):
    """nt_per_batch: the arithmetic of dK and dV.  ``mode``: 0 fp32, 1 bf16x3, 2 f16x2.  dV reads dR out of d(rq) (batch stride 2 d T) and A;
    dK reads Q (dense here, or any larger batch stride) and dS (N T)."""
    if mode >= 1 and B * T >= 256 and nt_bf3_fits(B, d, N, T, 2 * d * T, N * T):
        return {1: "bf16x3", 2: "f16x2"}[mode]
    return "fp32"


# ---- inputs of the synthesis-step tests -----------------------------------------------------------------------------------------------
STEP_CASES = [(1, 1), (3, 2), (5, 3), (6, 5), (64, 64), (32, 255), (64, 256), (37, 257), (64, 600), (130, 1023), (256, 1024)]    # (d, N)
STEP_ITEMS = 64
GAP_MIN = 1e-4               # an item whose float64 top-two probabilities are closer than this is left out of the index comparison
TIE_CASES = [(64, 600), (37, 1024)]
TIE_POSITIONS = (0, 62, 63, 254, 255, 256, 511, -2)      # -2: N - 2, a window of two positions


def fixed_windows(N):
    """The window starts every case places on purpose: both ends of the text, and either side of a wave's (64) and a trip's (256) boundary."""
    fixed = [0, N - 1, N - 2, N - 3]
    if N > 256:
        fixed += [254, 255, 256]
    if N > 64:
        fixed += [62, 63, 64]
    out = []
    for p in fixed:
        if 0 <= p < N and p not in out:
            out.append(p)
    return out


def step_case(d, N, B=STEP_ITEMS):
    """Standard normal K | V (B, 2d, N) and q (B, d) in float32, and pma (B,): the fixed windows first, then uniform in [0, N)."""
    rng = np.random.default_rng(1000 * d + N)
    kv = rng.standard_normal((B, 2 * d, N)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    fixed = fixed_windows(N)[:B]
    pma = rng.integers(0, N, size=B).astype(np.int64)
    pma[:len(fixed)] = fixed
    return kv, q, pma


def tie_case(d, N, B=STEP_ITEMS):
    """Exact ties inside the window.  Item b takes p = TIE_POSITIONS[b % 8] as its window start; column p of K is copied into column p + 1
    and, for every item of the upper half, into column p + 2 as well; q is flipped where needed so that the copied logit is positive, and a
    third column that is not a copy is half of column p (half the logit: below the tie).  Returns kv, q, pma and the number of tied positions
    (B,).  The copies are bit-identical, so their logits are in any arithmetic that treats every position alike."""
    kv, q, _ = step_case(d, N, B)
    pma = np.zeros(B, dtype=np.int64)
    ntied = np.zeros(B, dtype=np.int64)
    for b in range(B):
        p = TIE_POSITIONS[b % len(TIE_POSITIONS)]
        p = N + p if p < 0 else p
        assert p + 1 < N
        K = kv[b, :d]
        if float(K[:, p].astype(np.float64) @ q[b].astype(np.float64)) < 0:
            q[b] = -q[b]
        K[:, p + 1] = K[:, p]
        ntied[b] = 2
        if p + 2 < N:
            if b >= B // 2:
                K[:, p + 2] = K[:, p]
                ntied[b] = 3
            else:
                K[:, p + 2] = np.float32(0.5) * K[:, p]
        pma[b] = p
    return kv, q, pma, ntied


# ---- shapes of the training-attention test: (claimed path, claimed dK / dV arithmetic in the split modes, B, d, N, T, q is a strided view) --
# T covers {1, 31, 32, 33, 65} on the fallback chain (its softmax tiles are 32 columns wide) and AF_BN -+ 1 / 2 AF_BN -+ 1 on the fused kernels.
# "split": B T >= 256 and the operands fit -> the split-MFMA weight-gradient kernel in bf16x3 / f16x2; "exact:...": the fp32 kernel, and why.
TRAIN_CASES = [
    ("fallback:tile8", "exact:BT<256", 2, 32, 17, 33, False),
    ("fallback:tile8", "exact:BT<256", 2, 32, 17, 33, True),
    ("fallback:tile8", "split", 3, 32, 17, 97, False),
    ("fallback:tile8", "exact:T<8", 37, 32, 17, 7, False),             # 259 columns, but rows of 7 frames: ssv_nt_bf3_fits says no
    ("fallback:tile24", "exact:BT<256", 3, 96, 65, 31, False),
    ("fallback:tile24", "split", 2, 96, 65, 129, False),
    ("fallback:tile24", "exact:BT<256", 2, 96, 192, 65, False),
    ("fallback:tile24", "exact:BT<256", 2, 320, 100, 31, False),       # d a multiple of 64, but above 256
    ("fallback:tile32", "exact:BT<256", 2, 64, 193, 32, False),
    ("fallback:tile32", "exact:BT<256", 3, 64, 256, 1, False),
    ("fallback:tile32", "split", 3, 64, 256, 97, False),
    ("fallback:percol", "exact:BT<256", 3, 64, 257, 33, False),
    ("fallback:percol", "split", 2, 64, 257, 129, False),
    ("fallback:percol", "exact:BT<256", 2, 48, 300, 65, False),
    ("fused(2,4)", "exact:BT<256", 3, 256, 100, 63, False),
    ("fused(2,4)", "exact:BT<256", 3, 256, 100, 65, False),
    ("fused(1,2)", "exact:BT<256", 2, 128, 40, 127, False),
    ("fused(1,2)", "split", 2, 128, 40, 129, False),
    ("fused(2,2)", "exact:BT<256", 3, 128, 128, 63, False),
    ("fused(2,2)", "exact:BT<256", 3, 128, 128, 65, False),
    ("fused(3,1)", "exact:BT<256", 2, 64, 150, 127, False),
    ("fused(3,1)", "split", 2, 64, 150, 129, False),
    ("fused(2,1)", "exact:BT<256", 3, 64, 65, 63, False),
    ("fused(2,1)", "exact:BT<256", 3, 64, 65, 65, False),
    ("fused(3,3)", "exact:BT<256", 2, 192, 129, 127, False),
    ("fused(3,3)", "split", 2, 192, 129, 129, False),
    ("fused(1,3)", "exact:BT<256", 3, 192, 64, 63, False),
    ("fused(1,3)", "split", 3, 192, 64, 129, False),
]
FUSED_TESTED_BEFORE = {(3, 4), (1, 4), (3, 2), (1, 1), (2, 3)}      # test_fused_attention_forward_and_backward_vs_float64


def train_case_id(case):
    path, nt, B, d, N, T, view = case
    return "%s-dkdv_%s-B%d-d%d-N%d-T%d%s" % (path, nt.replace("<", "lt"), B, d, N, T, "-qview" if view else "")


def check_train_case(case, mode):
    """The path and the dK / dV arithmetic that ``case`` claims, against the restated dispatch; returns the dK / dV branch in ``mode``."""
    path, nt, B, d, N, T, view = case
    assert attention_path(B, d, N, T) == path, (case, attention_path(B, d, N, T))
    q_bs = (d + 3) * T if view else d * T
    fits = nt_bf3_fits(B, d, N, T, 2 * d * T, N * T) and nt_bf3_fits(B, d, N, T, q_bs, N * T)
    if nt == "split":
        assert B * T >= 256 and fits, case
    elif nt == "exact:BT<256":
        assert B * T < 256, case
    else:
        assert nt == "exact:T<8" and B * T >= 256 and T < 8 and not fits, case
    got = dkdv_branch(mode, B, d, N, T)
    assert got == ({1: "bf16x3", 2: "f16x2"}[mode] if (nt == "split" and mode >= 1) else "fp32"), (case, mode, got)
    return got
