"""The i-vector extractor restated in float64 numpy (include/ssv_hip.h, "I-vector extractor"): planes, centring, the E-step, the M-step with
the starved rule and the minimum-divergence step, cosine trials -- the yardstick of tests/test_gpu_ivector_tv.py -- with the same
mathematics as float32 arithmetic does it (the bars), the case generators and the recorded figures.

The float32 form: the planes and the centred statistics rounded to float32, the four big products as numpy's float32 ``matmul`` (a blocked
BLAS product), the factorisation in float64 on those rounded products, w and M rounded to float32.  A bar is FACTOR x the error of that
form on the very inputs a test uses, relative to the magnitude of the terms; the figures below were measured by ``python
tests/_ivector_tv_ref.py`` and test_ivector_tv_cpu.py holds a fresh measurement within a factor 4 of each."""
import numpy as np

FACTOR = 4.0
# products: worst |float32 matmul - float64| / sum |a| |b| per (m, n, K) of PRODUCT_SHAPES (plain) and PRODUCT_TN_SHAPES (transposed)
MEASURED_PRODUCT = {(64, 64, 1): 5.849e-08, (65, 63, 32): 2.045e-07, (1, 130, 33): 8.845e-08, (63, 65, 256): 2.454e-07, (70, 17, 257): 1.568e-07, (33, 129, 700): 1.124e-07}
MEASURED_PRODUCT_TN = {(64, 64, 1): 5.849e-08, (65, 63, 32): 2.045e-07, (1, 130, 33): 8.845e-08, (63, 65, 256): 2.454e-07, (70, 1, 257): 3.273e-08, (129, 33, 700): 1.018e-07}
# E-step per rank of ESTEP_RANKS, from T: w and M against the utterance's largest entry, obj against |1/2 log|L|| + |1/2 b.w|
MEASURED_ESTEP_W = {1: 7.775e-08, 16: 2.177e-04, 17: 2.806e-05, 33: 2.441e-04, 64: 3.910e-04, 65: 7.890e-04, 192: 2.059e-03}
MEASURED_ESTEP_M = {1: 1.430e-07, 16: 1.938e-04, 17: 5.301e-05, 33: 2.454e-04, 64: 1.845e-04, 65: 4.261e-04, 192: 8.125e-04}
MEASURED_ESTEP_OBJ = {1: 1.078e-07, 16: 9.044e-08, 17: 8.468e-08, 33: 6.016e-08, 64: 3.857e-08, 65: 4.766e-08, 192: 1.051e-08}
# EM at EM_SHAPE: worst |history32 - history64| / mean objective scale, worst |T32 - T64| / max |T64|
MEASURED_EM_HISTORY = 2.779e-07
MEASURED_EM_T = 3.326e-06
MEASURED_COSINE = 3.253e-08             # worst |float32 scores - float64 scores| (scores lie in [-1, 1])
# the E-step against float64 from the device's OWN float32 Lp and b: w and M are that value rounded once (2^-24 of an entry, at most of the
# utterance's largest), the factorisation's own error in double (R 2^-53 cond(L), cond(L) < 1e5 here) is far below; FACTOR x 2^-24.  obj
# leaves as float64: 1e-9 of its scale covers R 2^-53 cond(L) with room.
BAR_ESTEP_OWN = FACTOR * 2.0 ** -24
BAR_ESTEP_OWN_OBJ = 1e-9
# the M-step is float64 throughout, against numpy.linalg.solve in float64: both carry about 2^-53 cond(A_c) (cond < 1e6 here)
BAR_UPDATE = 1e-8

RUN, TILE = 256, 64                 # ssv_ivec_product_run(), ssv_ivec_product_tile()
# (m, n, K): a tile edge and one beyond in m and n, K = 1, K at a staged step's edge, one run, one run + 1, several runs and a ragged tail
PRODUCT_SHAPES = ((64, 64, 1), (65, 63, 32), (1, 130, 33), (63, 65, 256), (70, 17, 257), (33, 129, 700))
PRODUCT_TN_SHAPES = ((64, 64, 1), (65, 63, 32), (1, 130, 33), (63, 65, 256), (70, 1, 257), (129, 33, 700))
ESTEP_RANKS = (1, 16, 17, 33, 64, 65, 192)
EM_SHAPE = dict(C=16, D=12, R=17, U=60, iters=5, min_count=10.0, seed=11)
MONOTONE_SHAPE = dict(C=16, D=12, R=17, U=60, iters=6, min_count=10.0, seed=11)


def bar(measured):
    return FACTOR * measured


# ------------------------------------------------------------------------------------------------------------ the packed triangle
def tri_pack(S):
    i, j = np.tril_indices(S.shape[-1])
    return np.ascontiguousarray(S[..., i, j])


def tri_unpack(p):
    n = int(round((np.sqrt(8.0 * p.shape[-1] + 1.0) - 1.0) / 2.0))
    assert n * (n + 1) // 2 == p.shape[-1]
    i, j = np.tril_indices(n)
    S = np.zeros(p.shape[:-1] + (n, n), dtype=p.dtype)
    S[..., i, j] = p
    S[..., j, i] = p
    return S


# ------------------------------------------------------------------------------------------------------------ cases
def ubm_case(C, D, rng):
    return rng.dirichlet(np.full(C, 5.0)), rng.normal(0, 2, (C, D)), rng.uniform(0.5, 2.0, (C, D))


def stats_case(C, D, R, U, seed=0, starved=None, empty=None, big=None, t_scale=0.3, w_true=None):
    """Statistics drawn from the model: T_true, w_u ~ N(0, I), N_u = frames x a Dirichlet draw over a few Gaussians, F_uc = N_uc (mu_c +
    T_c w_u) + sqrt(N_uc var_c) z.  ``starved``: a Gaussian nobody visits (N = 0 everywhere); ``empty``: an utterance without frames;
    ``big``: an utterance of about 5,000 frames.  Returns float32 N (U, C), F (U, C, D) and the float64 w, mu, var, T_true, w_true."""
    rng = np.random.default_rng(seed)
    w, mu, var = ubm_case(C, D, rng)
    T_true = t_scale * np.sqrt(var)[:, :, None] * rng.standard_normal((C, D, R))
    w_true = rng.standard_normal((U, R)) if w_true is None else w_true
    frames = rng.integers(80, 400, U).astype(np.float64)
    if big is not None:
        frames[big] = 5000.0
    N = frames[:, None] * rng.dirichlet(np.full(C, 0.7), U)
    if starved is not None:
        N[:, starved] = 0.0
    if empty is not None:
        N[empty] = 0.0
    mean = mu[None] + np.einsum("cdr,ur->ucd", T_true, w_true)
    F = N[:, :, None] * mean + np.sqrt(N[:, :, None] * var[None]) * rng.standard_normal((U, C, D))
    return N.astype(np.float32), F.astype(np.float32), w, mu, var, T_true, w_true


def init_T(var, R, seed=0):
    """TotalVariability.from_ubm's start: 0.1 sqrt(var) z."""
    return 0.1 * np.sqrt(var)[:, :, None] * np.random.default_rng(seed).standard_normal(var.shape + (R,))


def product_case(m, n, K, seed=0):
    rng = np.random.default_rng(seed + 7 * m + 11 * n + 13 * K)
    return rng.normal(0, 1, (m, K)).astype(np.float32), rng.normal(0, 1, (K, n)).astype(np.float32)


def product_tn_case(m, n, K, seed=0):
    """A (K, m) and B (K, n) of the transposed form A^T B."""
    a, b = product_case(m, n, K, seed)
    return np.ascontiguousarray(a.T), b


def speaker_case(S, per_spk, R, seed=0, within=0.35):
    """Synthetic i-vectors of S speakers, ``per_spk`` each: a speaker's direction plus within-speaker noise.  (S * per_spk, R) float64."""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((S, R))
    return (centre[:, None, :] + within * rng.standard_normal((S, per_spk, R))).reshape(S * per_spk, R)


# ------------------------------------------------------------------------------------------------------------ the model
def planes(T, var):
    """G (C D, R) and packed Pk (C, P), float64."""
    C, D, R = T.shape
    G = T / var[:, :, None]
    return G.reshape(C * D, R), tri_pack(np.einsum("cdi,cdj->cij", T, G))


def centre(N, F, mu, dtype=np.float64):
    """Ft = F - N mu; float32: mu rounded once, then one rounding per element (a fused multiply-add is the float64 value rounded once)."""
    if dtype == np.float32:
        return (F.astype(np.float64) - N.astype(np.float64)[:, :, None] * mu.astype(np.float32).astype(np.float64)[None]).astype(np.float32)
    return F.astype(np.float64) - N.astype(np.float64)[:, :, None] * mu[None]


def estep_from(Lp, b, want_M=True):
    """The E-step in float64 from given Lp (U, P) and b (U, R): w, obj, packed M, and the two terms of obj's scale."""
    Lp, b = np.asarray(Lp, dtype=np.float64), np.asarray(b, dtype=np.float64)
    L = tri_unpack(Lp) + np.eye(b.shape[1])
    Linv = np.linalg.inv(L)
    w = np.einsum("uij,uj->ui", Linv, b)
    half_logdet = 0.5 * np.linalg.slogdet(L)[1]
    half_bw = 0.5 * (b * w).sum(1)
    M = tri_pack(Linv + w[:, :, None] * w[:, None, :]) if want_M else None
    return w, -half_logdet + half_bw, M, np.abs(half_logdet) + np.abs(half_bw)


def estep(N, Ft, T, var, float32=False):
    """From T: (w, obj, M, obj_scale, Lp, b).  ``float32``: the float32 form of the module docstring (w and M rounded to float32)."""
    G, Pk = planes(T, var)
    U = N.shape[0]
    if float32:
        Lp = (N.astype(np.float32) @ Pk.astype(np.float32)).astype(np.float64)
        b = (Ft.reshape(U, -1).astype(np.float32) @ G.astype(np.float32)).astype(np.float64)
    else:
        Lp, b = N.astype(np.float64) @ Pk, Ft.reshape(U, -1).astype(np.float64) @ G
    w, obj, M, scale = estep_from(Lp, b)
    if float32:
        w, M = w.astype(np.float32).astype(np.float64), M.astype(np.float32).astype(np.float64)
    return w, obj, M, scale, Lp, b


def accumulate(N, Ft, w, M, float32=False):
    """A (C, P), Cm (C D, R), Nc (C), sum M (P), float64; ``float32``: the two products as float32 matmul."""
    U = N.shape[0]
    F2 = Ft.reshape(U, -1)
    if float32:
        A = (N.astype(np.float32).T @ M.astype(np.float32)).astype(np.float64)
        Cm = (F2.astype(np.float32).T @ w.astype(np.float32)).astype(np.float64)
    else:
        A, Cm = N.astype(np.float64).T @ M, F2.astype(np.float64).T @ w
    return A, Cm, N.astype(np.float64).sum(0), M.sum(0)


def min_div_factor(Msum, U):
    return np.linalg.cholesky(tri_unpack(Msum / U))


def mstep(A, Cm, Nc, T, J=None, min_count=10.0):
    """T_c <- Cm_c A_c^-1 (then T_c J); a Gaussian with Nc < min_count (or not > 0) keeps its T_c."""
    C, D, R = T.shape
    out = T.copy()
    Cm = Cm.reshape(C, D, R)
    for c in range(C):
        if Nc[c] < min_count or not Nc[c] > 0:
            continue
        Tc = np.linalg.solve(tri_unpack(A[c]), Cm[c].T).T
        out[c] = Tc @ J if J is not None else Tc
    return out


def em_step(N, Ft, T, var, min_div=True, min_count=10.0, float32=False):
    """(mean objective under T, new T)."""
    w, obj, M, _, _, _ = estep(N, Ft, T, var, float32)
    A, Cm, Nc, Msum = accumulate(N, Ft, w, M, float32)
    J = min_div_factor(Msum, N.shape[0]) if min_div else None
    return obj.mean(), mstep(A, Cm, Nc, T, J, min_count)


def em_fit(N, Ft, T, var, iters, min_div=True, min_count=10.0, float32=False):
    hist = []
    for _ in range(iters):
        h, T = em_step(N, Ft, T, var, min_div, min_count, float32)
        hist.append(h)
    return np.asarray(hist), T


# ---- literal loops (test_ivector_tv_cpu.py holds the restatement above against them)
def estep_loop(N, Ft, T, var):
    U, C = N.shape
    _, D, R = T.shape
    ws, objs, Ms = [], [], []
    for u in range(U):
        L, b = np.eye(R), np.zeros(R)
        for c in range(C):
            for d in range(D):
                L += float(N[u, c]) * np.outer(T[c, d], T[c, d]) / var[c, d]
                b += T[c, d] * float(Ft[u, c, d]) / var[c, d]
        w = np.linalg.solve(L, b)
        ws.append(w)
        objs.append(-0.5 * np.log(np.linalg.det(L)) + 0.5 * b @ w)
        Ms.append(np.linalg.inv(L) + np.outer(w, w))
    return np.array(ws), np.array(objs), np.array(Ms)


def mstep_loop(N, Ft, w, Mfull, T, J, min_count):
    U, C = N.shape
    _, D, R = T.shape
    out = T.copy()
    for c in range(C):
        n = sum(float(N[u, c]) for u in range(U))
        if n < min_count or not n > 0:
            continue
        A, Cm = np.zeros((R, R)), np.zeros((D, R))
        for u in range(U):
            A += float(N[u, c]) * Mfull[u]
            Cm += np.outer(Ft[u, c].astype(np.float64), w[u])
        out[c] = Cm @ np.linalg.inv(A)
        if J is not None:
            out[c] = out[c] @ J
    return out


# ------------------------------------------------------------------------------------------------------------ trials
def normalise(v):
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return np.where(n > 0, v / np.where(n > 0, n, 1.0), 0.0)


def speaker_models(enroll, spk_off):
    models = np.zeros((len(spk_off) - 1, enroll.shape[1]))
    for s in range(len(spk_off) - 1):
        a, b = spk_off[s], spk_off[s + 1]
        if b > a:
            models[s] = normalise(normalise(enroll[a:b].astype(np.float64)).sum(0) / (b - a))
    return models


def cosine_trials(enroll, spk_off, evalv, float32=False):
    """scores (E, S) in float64; ``float32``: every step in float32 arithmetic."""
    if float32:
        e32, v32 = enroll.astype(np.float32), evalv.astype(np.float32)
        n = lambda x: np.where((x * x).sum(-1, keepdims=True) > 0, x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True, dtype=np.float32)), np.float32(1e-30)), np.float32(0))
        models = np.zeros((len(spk_off) - 1, enroll.shape[1]), dtype=np.float32)
        for s in range(len(spk_off) - 1):
            a, b = spk_off[s], spk_off[s + 1]
            if b > a:
                models[s] = n(n(e32[a:b]).sum(0, dtype=np.float32) / np.float32(b - a))
        return (n(v32) @ models.T).astype(np.float64)
    return normalise(evalv.astype(np.float64)) @ speaker_models(enroll, spk_off).T


def cosine_case(seed=3):
    """Ragged enrolment (1, 3, 0 and 5 vectors), a zero enrolment vector, a zero eval vector; R = 70 (two lanes' strides, ragged)."""
    rng = np.random.default_rng(seed)
    off = np.array([0, 1, 4, 4, 9], dtype=np.int64)
    enroll = rng.normal(0, 1, (9, 70)).astype(np.float32)
    enroll[2] = 0.0
    evalv = rng.normal(0, 3, (11, 70)).astype(np.float32)
    evalv[5] = 0.0
    return enroll, off, evalv


E2E_SHAPE = dict(S=4, per=9, C=8, D=6, R=5, iters=3, seed=5)


def e2e_case():
    """Synthetic speakers drawn from the model for the whole chain: S speakers x 9 utterances named <spk>_001 .. _006 (3 enrol, 3 real
    eval) and _024 .. _026 (the parser's spoofing trials: numbers above enrol + eval = 23), speaker-major.  Returns (N, F float32, w, mu, var,
    T0, utt2spk lines)."""
    s = E2E_SHAPE
    w_true = speaker_case(s["S"], s["per"], s["R"], seed=s["seed"])
    N, F, w, mu, var, _, _ = stats_case(s["C"], s["D"], s["R"], s["S"] * s["per"], seed=s["seed"], w_true=w_true, t_scale=0.5)
    lines = ["S%02d_%03d S%02d" % (k + 1, n, k + 1) for k in range(s["S"]) for n in (1, 2, 3, 4, 5, 6, 24, 25, 26)]
    return N, F, w, mu, var, init_T(var, s["R"], seed=s["seed"]), lines


def e2e_reference():
    """The chain in float64: train, extract, score.  Returns (scores (E, S), target mask (E, S)) in split_enroll_eval / trial_list order."""
    s = E2E_SHAPE
    N, F, _, mu, var, T0, _ = e2e_case()
    Ft = centre(N, F, mu, np.float32)
    _, T = em_fit(N, Ft, T0, var, s["iters"], True, 10.0)
    w = estep(N, Ft, T, var)[0].reshape(s["S"], s["per"], s["R"])
    enroll, ev = w[:, :3].reshape(-1, s["R"]), w[:, 3:].reshape(-1, s["R"])
    scores = cosine_trials(enroll, np.arange(0, 3 * s["S"] + 1, 3), ev)
    target = np.repeat(np.eye(s["S"], dtype=bool), s["per"] - 3, axis=0)
    return scores, target


# ------------------------------------------------------------------------------------------------------------ measurement of the bars
def product_error(got, a64, b64):
    """worst |got - a b| / sum |a| |b| against the float64 product of the (float32-valued) operands."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - a64 @ b64) / (np.abs(a64) @ np.abs(b64))).max())


def measure_product(m, n, K, tn=False):
    if tn:
        a, b = product_tn_case(m, n, K)
        return product_error(a.T @ b, a.T.astype(np.float64), b.astype(np.float64))
    a, b = product_case(m, n, K)
    return product_error(a @ b, a.astype(np.float64), b.astype(np.float64))


def estep_case(R):
    """The E-step case of rank R: C D small, an utterance without frames (0) and one of about 5,000 frames (1); R = 192 has 3 utterances."""
    U = 3 if R == 192 else 6
    C, D = (4, 3)
    N, F, _, mu, var, T_true, _ = stats_case(C, D, R, U, seed=100 + R, empty=0, big=1)
    return N, centre(N, F, mu, np.float32), T_true, var


def estep_errors(w, obj, M, ref):
    """(w, M, obj) errors of float64-valued arrays against ref = (w64, obj64, M64, scale): per utterance against its largest entry."""
    w64, obj64, M64, scale = ref
    ew = float((np.abs(w - w64).max(1) / np.maximum(np.abs(w64).max(1), 1e-300)).max())
    eM = float((np.abs(M - M64).max(1) / np.abs(M64).max(1)).max())
    eo = float((np.abs(obj - obj64) / np.maximum(scale, 1e-300)).max())
    return ew, eM, eo


def measure_estep(R):
    N, Ft, T, var = estep_case(R)
    w64, obj64, M64, scale, _, _ = estep(N, Ft, T, var)
    w32, obj32, M32, _, _, _ = estep(N, Ft, T, var, float32=True)
    return estep_errors(w32, obj32, M32, (w64, obj64, M64, scale))


def em_case(shape=None):
    """(N, Ft float32, T0, var): one starved Gaussian (C - 1), an empty utterance, a long one."""
    s = shape or EM_SHAPE
    N, F, _, mu, var, _, _ = stats_case(s["C"], s["D"], s["R"], s["U"], seed=s["seed"], starved=s["C"] - 1, empty=3, big=5)
    return N, centre(N, F, mu, np.float32), init_T(var, s["R"], seed=s["seed"]), var


def em_scales(N, Ft, T, var):
    """What the EM figures are relative to: the mean objective scale at the start, and max |T|."""
    return float(estep(N, Ft, T, var)[3].mean())


def measure_em():
    s = EM_SHAPE
    N, Ft, T0, var = em_case()
    h64, T64 = em_fit(N, Ft, T0, var, s["iters"], True, s["min_count"])
    h32, T32 = em_fit(N, Ft, T0, var, s["iters"], True, s["min_count"], float32=True)
    return float(np.abs(h32 - h64).max() / em_scales(N, Ft, T0, var)), float(np.abs(T32 - T64).max() / np.abs(T64).max())


def measure_cosine():
    enroll, off, evalv = cosine_case()
    return float(np.abs(cosine_trials(enroll, off, evalv, float32=True) - cosine_trials(enroll, off, evalv)).max())


if __name__ == "__main__":
    print("MEASURED_PRODUCT = {%s}" % ", ".join("%r: %.3e" % (sh, measure_product(*sh)) for sh in PRODUCT_SHAPES))
    print("MEASURED_PRODUCT_TN = {%s}" % ", ".join("%r: %.3e" % (sh, measure_product(*sh, tn=True)) for sh in PRODUCT_TN_SHAPES))
    es = {R: measure_estep(R) for R in ESTEP_RANKS}
    for i, name in enumerate(("W", "M", "OBJ")):
        print("MEASURED_ESTEP_%s = {%s}" % (name, ", ".join("%d: %.3e" % (R, es[R][i]) for R in ESTEP_RANKS)))
    print("MEASURED_EM_HISTORY, MEASURED_EM_T = %.3e, %.3e" % measure_em())
    print("MEASURED_COSINE = %.3e" % measure_cosine())
