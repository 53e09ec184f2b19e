"""The PLDA back end restated in float64 numpy (include/ssv_hip.h, "I-vector back end: PLDA"): length normalisation, class statistics, EM by the
formulas as the header writes them (every inverse and determinant taken directly, no inversion lemma), the objective, finalisation, the
transform, speaker models and the score in its DIRECT form -- the yardstick of tests/test_gpu_plda.py -- with the same mathematics as
float32 arithmetic does it (the bars), the case generators and the recorded figures.

The float32 form: residuals, centred rows and planes rounded to float32, the three big products (scatter, transform, score) as numpy's
float32 ``matmul``, EM in float64.  A bar is FACTOR x the error of that form on the very inputs a test uses, relative to the magnitude of the
terms; the figures below were measured by ``python tests/_plda_ref.py`` and test_plda_cpu.py holds a fresh measurement within a factor 4 of
each."""
import numpy as np

FACTOR = 4.0
# score, product form in float32 against the direct form in float64, per rank of SCORE_RANKS: worst |s32 - s64| / (sum |[t^2, t]| |H| + |k|)
MEASURED_SCORE = {1: 1.019e-07, 16: 2.568e-07, 17: 2.344e-07, 64: 3.327e-07, 65: 3.550e-07, 128: 4.311e-07, 129: 4.142e-07, 192: 5.134e-07}
# transform per rank of TRANSFORM_RANKS: worst over rows |u32 - u64| / max |u64| of the row, (length-normalised, not normalised)
MEASURED_TRANSFORM = {1: (3.003e-08, 2.165e-08), 17: (2.206e-07, 1.957e-07), 65: (3.665e-07, 4.123e-07), 128: (4.938e-07, 5.497e-07), 129: (6.998e-07, 5.396e-07), 192: (8.794e-07, 6.763e-07)}
# scatter of the float32 residuals per rank of STATS_RANKS: worst |float32 chains of 256 (scatter_chain) - float64| / sum |d| |d|
MEASURED_SCATTER = {1: 1.160e-06, 17: 1.832e-07, 64: 3.554e-07, 192: 5.219e-07}
# the scoring chain at CHAIN_SHAPE from a given model: worst |s32 - s64| / term scale
MEASURED_CHAIN = 2.394e-07

# The float64-only stages (mixed inverse, EM classes, wsyrk, update, objective) against numpy in float64.  Both sides carry about
# 2^-53 R cond: a Cholesky inverse of a matrix of condition cond loses log2(cond) of its 53 bits, R terms meet in every entry, and the
# device's E-step goes through the inversion lemma (w = n Mx W^-1 c, quad = n t.r), which stacks two such inverses and one subtraction of
# comparable magnitudes.  The generators keep cond(W), cond(B) < 1e3, the mixed matrices B^-1 + n W^-1 inherit at most their product's
# order, so 2^-53 x 192 x 1e3 x 1e3 ~ 2e-8 is the far corner and the typical entry sits orders below: 1e-9 of the largest entry holds
# with room at the shapes tested (cond(B^-1 + n W^-1) < 1e3 there: it is measured and asserted in test_plda_cpu.py).
BAR_F64 = 1e-9
BAR_MEAN = 1e-12                    # the class means: a sum of n float64 terms in a fixed order, against numpy's; n 2^-53 of the largest entry
BAR_ROUND = 2.0 ** -24              # a value rounded once to float32

SCORE_RANKS = (1, 16, 17, 64, 65, 128, 129, 192)
TRANSFORM_RANKS = (1, 17, 65, 128, 129, 192)
STATS_RANKS = (1, 17, 64, 192)
STATS_COUNTS = (1, 2, 64, 0, 65, 300)                # one speaker without rows in the middle
INVERSE_RANKS = (1, 16, 17, 33, 64, 65, 192)
EM_SHAPES = ((17, 40), (192, 24))
MONOTONE_SHAPES = ((17, 40), (64, 120))
CHAIN_SHAPE = dict(R=17, S_train=40, S_test=8, enroll=3, real=5, spoof=5, iters=10, seed=7)


def bar(measured):
    return FACTOR * measured


# ------------------------------------------------------------------------------------------------------------ cases
def spd(R, lo, hi, rng):
    """A symmetric positive definite matrix with eigenvalues spread geometrically over [lo, hi] in a random basis."""
    q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    lam = np.exp(np.linspace(np.log(lo), np.log(hi), R)) if R > 1 else np.array([np.sqrt(lo * hi)])
    M = (q * lam) @ q.T
    return 0.5 * (M + M.T)


def model_case(R, seed=0):
    """(mu, W, B) of a two-covariance model: cond(W) = 20, cond(B) = 30."""
    rng = np.random.default_rng(1000 + 31 * R + seed)
    return rng.normal(0, 0.5, R), spd(R, 0.1, 2.0, rng), spd(R, 0.3, 9.0, rng)


def counts_case(S, seed=0):
    """Mixed counts 1 ... 9."""
    return np.random.default_rng(50 + seed).integers(1, 10, S)


def draw(mu, W, B, counts, seed=0):
    """float32 rows x = mu + y_s + e drawn from the model, speaker-major, and the offsets (S + 1) int64."""
    rng = np.random.default_rng(77 + seed)
    R = mu.size
    cw, cb = np.linalg.cholesky(W), np.linalg.cholesky(B)
    rows = []
    for n in counts:
        y = cb @ rng.standard_normal(R)
        rows.append(mu + y + rng.standard_normal((int(n), R)) @ cw.T)
    X = np.concatenate(rows) if rows else np.zeros((0, R))
    return X.astype(np.float32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def train_case(R, S, seed=0):
    mu, W, B = model_case(R, seed)
    X, off = draw(mu, W, B, counts_case(S, seed), seed)
    return X, off


def stats_case(R, seed=0):
    """Speakers of STATS_COUNTS rows, one zero row (the second row of the 64-row speaker)."""
    mu, W, B = model_case(R, seed)
    X, off = draw(mu, W, B, np.array(STATS_COUNTS), seed + 1)
    X[off[2] + 1] = 0.0
    return X, off


def psi_case(R, seed=0):
    return np.sort(np.random.default_rng(5 + R + seed).uniform(0.0, 12.0, R))[::-1].copy()


def score_case(E, S, R, seed=0):
    """Transformed-looking float32 vectors t (E, R), y (S, R), counts n (S) mixed 0 ... 9 (speaker 2 has none when there is one), psi."""
    rng = np.random.default_rng(900 + 7 * E + 11 * S + 13 * R + seed)
    psi = psi_case(R, seed)
    n = rng.integers(1, 10, S).astype(np.int32)
    if S > 2:
        n[2] = 0
    y = (rng.standard_normal((S, R)) * np.sqrt(psi + 0.3)).astype(np.float32)
    t = (y[rng.integers(0, S, E)] * 0.7 + rng.standard_normal((E, R))).astype(np.float32)
    return t, y, n, psi


def transform_case(n, R, seed=0):
    """(X float32 (n, R), mu, A, psi, nex int32 mixed 1 ... 9); row n // 2 is mu itself, whose entries are float32 values here, so that
    the centred row is zero in every form and its factor 1."""
    rng = np.random.default_rng(300 + 3 * n + 5 * R + seed)
    mu, W, B = model_case(R, seed)
    mu = mu.astype(np.float32).astype(np.float64)
    A, psi = finalize(W, B)
    X, _ = draw(mu, W, B, np.full(n, 1), seed)
    X[n // 2] = mu.astype(np.float32)
    return X, mu, A, psi, rng.integers(1, 10, n).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ the model
def normalise(x):
    """x sqrt(R) / |x|; a zero vector stays zero."""
    x = np.asarray(x, dtype=np.float64)
    ss = (x * x).sum(-1, keepdims=True)
    return x * np.where(ss > 0, np.sqrt(x.shape[-1] / np.where(ss > 0, ss, 1.0)), 0.0)


def class_stats(X, off, length_norm=True):
    """(Xd (n, R) float64 residual rows -- zero where no speaker owns the row --, means (S, R), mu, counts)."""
    xh = normalise(X) if length_norm else np.asarray(X, dtype=np.float64)
    S = len(off) - 1
    means, Xd, counts = np.zeros((S, xh.shape[1])), np.zeros_like(xh), np.diff(off)
    for k in range(S):
        if counts[k] > 0:
            means[k] = xh[off[k]:off[k + 1]].sum(0) / counts[k]
            Xd[off[k]:off[k + 1]] = xh[off[k]:off[k + 1]] - means[k]
    return Xd, means, means[counts > 0].mean(0), counts


def scatter(Xd, float32=False):
    if float32:
        d = Xd.astype(np.float32)
        return (d.T @ d).astype(np.float64)
    d = Xd.astype(np.float32).astype(np.float64)
    return d.T @ d


def scatter_chain(Xd, run=256):
    """The scatter as ssv_ivec_product_tn's documented arithmetic does it: over each run of 256 rows one float32 chain per element from a zero
    accumulator, a fused multiply-add per row in ascending order (the float64 value rounded once), the runs added in double.  numpy's float32
    ``matmul`` is no model of this at small R: length-normalised vectors of R = 1 are +-1, a speaker's residuals take two values, the chain
    adds the same positive square again and again and its rounding is systematic, while BLAS's dot splits the sum over several accumulators."""
    d = Xd.astype(np.float32).astype(np.float64)
    total = np.zeros((d.shape[1], d.shape[1]))
    for r0 in range(0, d.shape[0], run):
        acc = np.zeros_like(total, dtype=np.float32)
        for row in d[r0:r0 + run]:
            acc = (acc.astype(np.float64) + np.outer(row, row)).astype(np.float32)
        total += acc
    return total


def speaker_terms(means, mu, counts, W, B):
    """Per speaker with rows: (Mx, w, r, log|B + W/n|, quadratic form), by the header's formulas, every inverse taken directly."""
    Winv, Binv = np.linalg.inv(W), np.linalg.inv(B)
    cache, out = {}, []
    for k in np.nonzero(counts > 0)[0]:
        n = int(counts[k])
        if n not in cache:
            G = B + W / n
            cache[n] = (np.linalg.inv(Binv + n * Winv), np.linalg.slogdet(G)[1], np.linalg.inv(G))
        Mx, ld, Ginv = cache[n]
        c = means[k] - mu
        w = n * Mx @ (Winv @ c)
        out.append((k, n, Mx, w, c - w, ld, float(c @ Ginv @ c)))
    return out


def objective(Sigma, means, mu, counts, W, B, terms=None):
    terms = terms if terms is not None else speaker_terms(means, mu, counts, W, B)
    N, S = float(counts.sum()), float((counts > 0).sum())
    obj = -0.5 * ((N - S) * np.linalg.slogdet(W)[1] + np.trace(np.linalg.inv(W) @ Sigma))
    return (obj - 0.5 * sum(ld + q for _, _, _, _, _, ld, q in terms)) / N


def em_step(Sigma, means, mu, counts, W, B):
    """(objective under W and B, new W, new B)."""
    terms = speaker_terms(means, mu, counts, W, B)
    N, S = float(counts.sum()), float((counts > 0).sum())
    Bn, Wn = np.zeros_like(B), Sigma.copy()
    for _, n, Mx, w, r, _, _ in terms:
        Bn += Mx + np.outer(w, w)
        Wn += n * (Mx + np.outer(r, r))
    return objective(Sigma, means, mu, counts, W, B, terms), Wn / N, Bn / S


def em_fit(Sigma, means, mu, counts, iters=10):
    """From W = B = I: (history of iters + 1 objectives, W, B)."""
    R = mu.size
    W, B, hist = np.eye(R), np.eye(R), []
    for _ in range(iters):
        h, W, B = em_step(Sigma, means, mu, counts, W, B)
        hist.append(h)
    hist.append(objective(Sigma, means, mu, counts, W, B))
    return np.asarray(hist), W, B


def finalize(W, B):
    """(A, psi): W = C C^T, C^-1 B C^-T = U diag(psi) U^T, psi floored at 0 and descending, A = U^T C^-1, the largest entry of a row positive."""
    Ci = np.linalg.inv(np.linalg.cholesky(W))
    M = Ci @ B @ Ci.T
    psi, U = np.linalg.eigh(0.5 * (M + M.T))
    order = np.argsort(-psi, kind="stable")
    psi, A = np.maximum(psi[order], 0.0), U[:, order].T @ Ci
    sign = np.where(A[np.arange(A.shape[0]), np.abs(A).argmax(1)] < 0, -1.0, 1.0)
    return A * sign[:, None], psi


def train(X, off, iters=10, length_norm=True, float32=False):
    """(mu, A, psi, history) from float32 rows; ``float32``: the scatter as float32 matmul."""
    Xd, means, mu, counts = class_stats(X, off, length_norm)
    hist, W, B = em_fit(scatter(Xd, float32), means, mu, counts, iters)
    A, psi = finalize(W, B)
    return mu, A, psi, hist


def transform(X, mu, A, psi, nex=1, length_norm=True, float32=False):
    """u (n, R) float64.  ``float32``: the factor and mu rounded once, the centring one rounding per element (a fused multiply-add is the
    float64 value rounded once), the product as float32 matmul against the plane A^T rounded once, the result rounded once."""
    X = np.asarray(X, dtype=np.float32)
    R = X.shape[1]
    nex = np.broadcast_to(np.asarray(nex, dtype=np.float64), (X.shape[0],))
    if float32:
        x64 = X.astype(np.float64)
        ss = (x64 * x64).sum(1, keepdims=True)
        f = np.where(ss > 0, np.sqrt(R / np.where(ss > 0, ss, 1.0)), 0.0).astype(np.float32) if length_norm else np.ones((X.shape[0], 1), np.float32)
        xc = (x64 * f.astype(np.float64) - mu.astype(np.float32).astype(np.float64)).astype(np.float32)
        u = (xc @ np.ascontiguousarray(A.T).astype(np.float32)).astype(np.float64)
    else:
        u = ((normalise(X) if length_norm else X.astype(np.float64)) - mu) @ A.T
    s = (u * u / (psi + 1.0 / nex[:, None])).sum(1, keepdims=True)
    u = u * np.where(s > 0, np.sqrt(R / np.where(s > 0, s, 1.0)), 1.0)
    return u.astype(np.float32).astype(np.float64) if float32 else u


def model_rows(enroll, off):
    """(S, R) float64: the mean of a speaker's normalised rows, normalised again; zero for a speaker without rows."""
    out = np.zeros((len(off) - 1, enroll.shape[1]))
    for s in range(len(off) - 1):
        if off[s + 1] > off[s]:
            out[s] = normalise(normalise(enroll[off[s]:off[s + 1]]).sum(0) / (off[s + 1] - off[s]))
    return out


def speaker_models(enroll, off, mu, A, psi, float32=False):
    """(y (S, R), n (S)).  The model rows are float32 by the model's definition (rounded once), in both forms; ``float32``: their transform in
    the float32 form."""
    n = np.diff(off).astype(np.int64)
    return transform(model_rows(enroll, off).astype(np.float32), mu, A, psi, np.maximum(n, 1), False, float32), n


def score_direct(t, y, n, psi):
    """LLR (E, S) float64 by the direct form; a speaker with n = 0 scores exactly 0."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.zeros((t.shape[0], y.shape[0]))
    for s in range(y.shape[0]):
        if n[s] <= 0:
            continue
        den = n[s] * psi + 1.0
        c, v = n[s] * psi / den, 1.0 + psi / den
        out[:, s] = -0.5 * (np.log(v) + (t - c * y[s]) ** 2 / v).sum(1) + 0.5 * (np.log(psi + 1.0) + t * t / (psi + 1.0)).sum(1)
    return out


def planes(y, n, psi):
    """H (S, 2R) and k (S) float64."""
    y = np.asarray(y, dtype=np.float64)
    nn = np.asarray(n, dtype=np.float64)[:, None]
    den = nn * psi + 1.0
    c, v = nn * psi / den, 1.0 + psi / den
    a = 1.0 / v
    live = (nn > 0).astype(np.float64)
    H = np.concatenate([-0.5 * (a - 1.0 / (psi + 1.0)), a * c * y], axis=1) * live
    k = (-0.5 * (a * c * c * y * y).sum(1) - 0.5 * (np.log(v) - np.log(psi + 1.0)).sum(1)) * live[:, 0]
    return H, k


def score_product(t, H, k, float32=False):
    """[t^2, t] H^T + k.  ``float32``: t^2 one float32 product, H rounded once, the product as float32 matmul, k added in double."""
    if float32:
        t = np.asarray(t, dtype=np.float32)
        return (np.concatenate([t * t, t], axis=1) @ H.astype(np.float32).T).astype(np.float64) + k
    t = np.asarray(t, dtype=np.float64)
    return np.concatenate([t * t, t], axis=1) @ H.T + k


def term_scale(t, H, k):
    t = np.asarray(t, dtype=np.float64)
    return np.abs(np.concatenate([t * t, t], axis=1)) @ np.abs(H).T + np.abs(k)


def trials(enroll, off, evalv, mu, A, psi, float32=False):
    """(scores (E, S), term scale): the whole scoring chain."""
    y, n = speaker_models(enroll, off, mu, A, psi, float32)
    t = transform(evalv, mu, A, psi, 1, True, float32)
    H, k = planes(y, n, psi)
    if float32:
        return score_product(t, H, k, True), term_scale(t, H, k)
    return score_direct(t, y, n, psi), term_scale(t, H, k)


def compute_eer(target, nontarget):
    """The walk of compute-eer, restated: returns (eer, threshold)."""
    t, non = sorted(float(v) for v in target), sorted(float(v) for v in nontarget)
    if not t or not non:
        raise ValueError("empty list")
    p = 0
    while p + 1 < len(t):
        q = len(non) - 1 - int(np.floor(len(non) * p / len(t)))
        if non[max(q, 0)] < t[p]:
            break
        p += 1
    return p / len(t), t[p]


# ------------------------------------------------------------------------------------------------------------ the chain
def chain_case():
    """Data drawn from one model at CHAIN_SHAPE: (Xtrain, off_train, enroll, enroll lines, evalv, eval lines).  Test speakers are named
    T01 ...; utterances <spk>_001 .. _003 enrol, _004 .. _008 are real eval, _024 .. _028 the parser's spoofing trials (numbers above enrol +
    eval = 23): the same speaker's vectors moved a little towards the global mean."""
    s = CHAIN_SHAPE
    mu, W, B = model_case(s["R"], s["seed"])
    Xtr, off = draw(mu, W, B, counts_case(s["S_train"], s["seed"]), s["seed"])
    per = s["enroll"] + s["real"] + s["spoof"]
    Xte, _ = draw(mu, W, B, np.full(s["S_test"], per), s["seed"] + 1)
    Xte = Xte.reshape(s["S_test"], per, s["R"])
    Xte[:, s["enroll"] + s["real"]:] = (0.8 * Xte[:, s["enroll"] + s["real"]:] + 0.2 * mu).astype(np.float32)
    names = lambda k, nums: ["T%02d_%03d T%02d" % (k + 1, i, k + 1) for i in nums]
    en_lines = [l for k in range(s["S_test"]) for l in names(k, range(1, s["enroll"] + 1))]
    ev_nums = list(range(s["enroll"] + 1, s["enroll"] + s["real"] + 1)) + list(range(24, 24 + s["spoof"]))
    ev_lines = [l for k in range(s["S_test"]) for l in names(k, ev_nums)]
    enroll = np.ascontiguousarray(Xte[:, :s["enroll"]].reshape(-1, s["R"]))
    evalv = np.ascontiguousarray(Xte[:, s["enroll"]:].reshape(-1, s["R"]))
    return Xtr, off, enroll, en_lines, evalv, ev_lines


# ------------------------------------------------------------------------------------------------------------ measurement of the bars
SCORE_SHAPE = (130, 65)             # E, S of the score measurements


def measure_score(R, E=SCORE_SHAPE[0], S=SCORE_SHAPE[1]):
    t, y, n, psi = score_case(E, S, R)
    H, k = planes(y, n, psi)
    return float((np.abs(score_product(t, H, k, True) - score_direct(t, y, n, psi)) / np.maximum(term_scale(t, H, k), 1e-300)).max())


def transform_error(u, u64):
    return float((np.abs(u - u64).max(1) / np.maximum(np.abs(u64).max(1), 1e-300)).max())


def measure_transform(R, n=130):
    X, mu, A, psi, nex = transform_case(n, R)
    X2 = X.copy()
    X2[n // 2] = X[0]               # (normalised, the row equal to mu is as any other: keep the factor-1 case to the plain form)
    return (transform_error(transform(X2, mu, A, psi, nex, True, True), transform(X2, mu, A, psi, nex, True)),
            transform_error(transform(X, mu, A, psi, 3, False, True), transform(X, mu, A, psi, 3, False)))


def measure_scatter(R):
    X, off = stats_case(R)
    Xd = class_stats(X, off)[0]
    d = np.abs(Xd.astype(np.float32).astype(np.float64))
    return float((np.abs(scatter_chain(Xd) - scatter(Xd)) / np.maximum(d.T @ d, 1e-300)).max())


def measure_chain():
    Xtr, off, enroll, _, evalv, _ = chain_case()
    s = CHAIN_SHAPE
    mu, A, psi, _ = train(Xtr, off, s["iters"])
    eoff = np.arange(0, enroll.shape[0] + 1, s["enroll"])
    s32, scale = trials(enroll, eoff, evalv, mu, A, psi, True)
    s64, _ = trials(enroll, eoff, evalv, mu, A, psi)
    return float((np.abs(s32 - s64) / scale).max())


if __name__ == "__main__":
    print("MEASURED_SCORE = {%s}" % ", ".join("%d: %.3e" % (R, measure_score(R)) for R in SCORE_RANKS))
    print("MEASURED_TRANSFORM = {%s}" % ", ".join("%d: (%.3e, %.3e)" % ((R,) + measure_transform(R)) for R in TRANSFORM_RANKS))
    print("MEASURED_SCATTER = {%s}" % ", ".join("%d: %.3e" % (R, measure_scatter(R)) for R in STATS_RANKS))
    print("MEASURED_CHAIN = %.3e" % measure_chain())
