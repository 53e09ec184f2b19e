"""Float64 numpy restatement of the i-vector groundwork (include/ssv_hip.h, "I-vector groundwork"), written from the definitions there:
cepstral features, Gaussian selection and posteriors of a diagonal GMM, sufficient statistics, the M-step, exact EM.  Kaldi is not the
yardstick (its binaries and the recipe's conf/ are not available); this file is.

The log-likelihood is in the DIRECT form  -1/2 sum((x - mu)^2 / var + log 2 pi var) + log w,  not the expanded product the kernel
computes, so that the reference and the kernel do not share the cancellation.  Functions that take ``dtype`` run every operation in
that type: with float32 they are the "float32 numpy direct form" the error bars are measured from (the ``measure_*`` functions), never a
reference.

Error bars.  Each bar is 4 x the worst error of the float32 numpy form against float64 on the TEST'S OWN inputs, relative to the sum of
the magnitudes of the terms (4 x: the MFMA's k order differs from numpy's blocking, and the planes are rounded once more).  Both numbers
are recorded below; ``python tests/_ivector_ref.py`` prints them again, and tests/test_ivector_cpu.py holds the recorded ones against a
fresh measurement.
"""
import numpy as np

# ------------------------------------------------------------------------------------------------------------ recorded bars
# shape (D, C, nsel) -> worst |L32 - L64| / (sum_d |A x| + |B x^2| + |g|) of the float32 numpy expanded product on the shape's inputs
MEASURED_LOGLIK = {(60, 1024, 20): 3.721e-07, (13, 50, 5): 2.347e-07, (128, 2048, 32): 3.955e-07, (13, 21, 21): 1.327e-07}
# statistics: worst |S32 - S64| / sum |gamma v| of a sequential float32 sum over ONE segment of all 2000 frames (the longest chain of the
# layouts tested), order 2, per (D, C, nsel)
MEASURED_STATS = {(13, 50, 5): 7.830e-07, (60, 1000, 20): 3.150e-07}
# features: worst |out32 - out64| / (|v| + mean |v|, from the magnitudes of the terms) of the float32 direct form
MEASURED_FEATURES = 5.998e-07
# exact EM, C = 16, D = 5, 4000 frames, 5 iterations: float64 against an E-step in float32 (expanded product, soft max in float32)
MEASURED_EM_HISTORY = 3.337e-07     # worst |history32 - history64|
MEASURED_EM_MEANS = 8.567e-07      # worst |mu32 - mu64| after the last iteration
FACTOR = 4.0
BAR_LOGLIK = {k: FACTOR * v for k, v in MEASURED_LOGLIK.items()}
BAR_STATS = {k: FACTOR * v for k, v in MEASURED_STATS.items()}
BAR_FEATURES = FACTOR * MEASURED_FEATURES
BAR_EM_HISTORY = FACTOR * MEASURED_EM_HISTORY
BAR_EM_MEANS = FACTOR * MEASURED_EM_MEANS

LOG_SHAPES = ((60, 1024, 20, 2000), (13, 50, 5, 2000), (128, 2048, 32, 64), (13, 21, 21, 70))      # (D, C, nsel, F); the last: every Gaussian selected
STATS_SHAPES = ((13, 50, 5, 2000), (60, 1000, 20, 2000))
FEATURE_LENGTHS = (0, 1, 5, 299, 300, 301, 1000)
EM_SHAPE = dict(D=5, C=16, F=4000, iters=5, var_floor=1e-3, min_count=10.0, min_weight=1e-5)


# ------------------------------------------------------------------------------------------------------------ test inputs
def clustered(D, n, rng):
    """n frames: 128 centres drawn from N(0, 3^2) plus unit noise."""
    cent = rng.normal(0, 3, (128, D))
    return (cent[rng.integers(0, 128, n)] + rng.normal(0, 1, (n, D))).astype(np.float32)


def gmm_case(D, C, F, seed=0):
    """Frames X (F, D) float32 and float64 parameters (w, mu, var): the means are C distinct frames of the same population plus
    N(0, 0.3^2), the variances uniform in [0.5, 2], the weights a Dirichlet(5) draw."""
    rng = np.random.default_rng(seed)
    pool = clustered(D, max(F, C), rng)
    mu = pool[rng.choice(len(pool), C, replace=False)].astype(np.float64) + rng.normal(0, .3, (C, D))
    var = rng.uniform(.5, 2, (C, D))
    w = rng.dirichlet(np.ones(C) * 5)
    return pool[:F].copy(), w, mu, var


def feature_case(M=40, seed=3):
    """Log-mel-like frames for ragged utterances of FEATURE_LENGTHS (in a shuffled order, the empty one in the middle), 3 frames in
    front of the first utterance and 5 behind the last that belong to none: (mel (G, M) float32, utt_off (U + 1) int64)."""
    rng = np.random.default_rng(seed)
    lens = [299, 1, 0, 1000, 5, 301, 300]
    assert sorted(lens) == sorted(FEATURE_LENGTHS)
    off = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G = int(off[-1]) + 5
    t = np.arange(G)[:, None]
    mel = (-6.0 + 2.0 * np.sin(t / 37.0 + np.arange(M)[None, :] / 5.0) + rng.normal(0, 1.5, (G, M))).astype(np.float32)
    return mel, off


def em_case(seed=5):
    s = EM_SHAPE
    rng = np.random.default_rng(seed)
    cent = rng.normal(0, 3, (s["C"], s["D"]))
    X = (cent[rng.integers(0, s["C"], s["F"])] + rng.normal(0, 1, (s["F"], s["D"]))).astype(np.float32)
    rows = np.sort(rng.choice(s["F"], s["C"], replace=False))
    mu = X[rows].astype(np.float64)
    var = np.tile(X.astype(np.float64).var(axis=0), (s["C"], 1))
    w = np.full(s["C"], 1.0 / s["C"])
    return X, w, mu, var


# ------------------------------------------------------------------------------------------------------------ features
def dct_table(n_ceps, n_mels, lifter):
    """Closed form: row k of the orthonormal DCT-II, sqrt(1/M) for k = 0 and sqrt(2/M) cos(pi k (2m + 1) / 2M) otherwise, times the
    lifter 1 + (Q/2) sin(pi k / Q).  float64."""
    t = np.empty((n_ceps, n_mels))
    for k in range(n_ceps):
        for m in range(n_mels):
            t[k, m] = (np.sqrt(1.0 / n_mels) if k == 0 else np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (2 * m + 1) / (2.0 * n_mels)))
        if lifter:
            t[k] *= 1.0 + 0.5 * lifter * np.sin(np.pi * k / lifter)
    return t


def delta_coeffs(w):
    """(first order, second order): c_j = j / (2 sum_{i=1..w} i^2), j in [-w, w], and c (*) c of length 4 w + 1."""
    c = np.arange(-w, w + 1, dtype=np.float64) / (2.0 * sum(i * i for i in range(1, w + 1)))
    return c, np.convolve(c, c)


def cmn_window(t, T, W):
    lo = t - W // 2
    hi = lo + W
    if lo < 0:
        lo, hi = 0, min(T, W)
    if hi > T:
        hi, lo = T, max(0, T - W)
    return lo, hi


def _utt_rows(s, w, order, absolute, dtype):
    """[s, d, dd] of one utterance's statics s (T, Cc), indices clamped to [0, T - 1]; every operation in ``dtype``."""
    T = s.shape[0]
    rows = [s]
    for o, c in zip((1, 2), delta_coeffs(w) if order else ()):
        if o > order:
            break
        c = (np.abs(c) if absolute else c).astype(dtype)
        h = (len(c) - 1) // 2
        d = np.zeros_like(s)
        for j in range(-h, h + 1):
            d = d + c[j + h] * s[np.clip(np.arange(T) + j, 0, T - 1)]
        rows.append(d)
    return np.concatenate(rows, axis=1)


def features(mel, utt_off, dct=None, w=3, order=2, W=300, dtype=np.float64, absolute=False):
    """(G, Cc (order + 1)); rows of frames in no utterance are NaN.  ``absolute``: the same pipeline on the magnitudes of the terms
    (|dct| |mel|, |c_j|, |v| + mean |v|) -- the scale the error bars are relative to."""
    mel = np.asarray(mel).astype(dtype)
    if absolute:
        mel = np.abs(mel)
    tab = None if dct is None else (np.abs(dct) if absolute else np.asarray(dct)).astype(dtype)
    Cc = mel.shape[1] if tab is None else tab.shape[0]
    out = np.full((mel.shape[0], Cc * (order + 1)), np.nan, dtype=dtype)
    for u in range(len(utt_off) - 1):
        a, b = int(utt_off[u]), int(utt_off[u + 1])
        T = b - a
        if T == 0:
            continue
        s = mel[a:b] if tab is None else (mel[a:b] @ tab.T).astype(dtype)
        v = _utt_rows(s, w, order, absolute, dtype)
        for t in range(T):
            lo, hi = cmn_window(t, T, W)
            m = v[lo:hi].sum(axis=0, dtype=dtype) / dtype(hi - lo)
            out[a + t] = v[t] + m if absolute else v[t] - m
    return out


def features_loop(mel, utt_off, dct, w, order, W):
    """The same by literal loops over frames, columns and taps (tiny inputs only)."""
    mel = np.asarray(mel, dtype=np.float64)
    Cc = mel.shape[1] if dct is None else len(dct)
    c1, c2 = delta_coeffs(w) if order else (None, None)
    out = np.full((mel.shape[0], Cc * (order + 1)), np.nan)
    for u in range(len(utt_off) - 1):
        a, T = int(utt_off[u]), int(utt_off[u + 1] - utt_off[u])
        s = [[sum(dct[c][m] * mel[a + t][m] for m in range(mel.shape[1])) if dct is not None else mel[a + t][c] for c in range(Cc)] for t in range(T)]
        v = np.zeros((T, Cc * (order + 1)))
        for t in range(T):
            for c in range(Cc):
                v[t][c] = s[t][c]
                if order >= 1:
                    v[t][Cc + c] = sum(c1[j + w] * s[min(max(t + j, 0), T - 1)][c] for j in range(-w, w + 1))
                if order >= 2:
                    v[t][2 * Cc + c] = sum(c2[j + 2 * w] * s[min(max(t + j, 0), T - 1)][c] for j in range(-2 * w, 2 * w + 1))
        for t in range(T):
            lo = t - W // 2
            hi = lo + W
            if lo < 0:
                lo, hi = 0, min(T, W)
            if hi > T:
                hi, lo = T, max(0, T - W)
            for c in range(v.shape[1]):
                out[a + t][c] = v[t][c] - sum(v[k][c] for k in range(lo, hi)) / (hi - lo)
    return out


# ------------------------------------------------------------------------------------------------------------ the mixture
def planes(w, mu, var):
    """float64 (A, B, g): A = mu / var, B = -1/2 / var, g = log w - 1/2 sum (log 2 pi var + mu^2 / var)."""
    return mu / var, -0.5 / var, np.log(w) - 0.5 * (np.log(2 * np.pi * var) + mu * mu / var).sum(1)


def loglik_direct(X, w, mu, var, chunk=64):
    """(F, C) float64, the direct form."""
    X = np.asarray(X, dtype=np.float64)
    cst = np.log(w) - 0.5 * np.log(2 * np.pi * var).sum(1)
    out = np.empty((X.shape[0], len(w)))
    for f in range(0, X.shape[0], chunk):
        d = X[f:f + chunk, None, :] - mu[None]
        out[f:f + chunk] = cst[None] - 0.5 * (d * d / var[None]).sum(2)
    return out


def loglik_expanded_f32(X, w, mu, var):
    """The kernel's expanded product evaluated by float32 numpy (measurement of the bar only)."""
    A, B, g = (p.astype(np.float32) for p in planes(w, mu, var))
    X = np.asarray(X, dtype=np.float32)
    return np.concatenate([X, X * X], 1) @ np.concatenate([A, B], 1).T + g


def loglik_scale(X, w, mu, var):
    """(F, C): sum_d |A x| + |B x^2| + |g|."""
    A, B, g = planes(w, mu, var)
    X = np.asarray(X, dtype=np.float64)
    return np.abs(X) @ np.abs(A).T + (X * X) @ np.abs(B).T + np.abs(g)[None]


def select(L, nsel):
    """Indices of the nsel largest per row, by descending value and, among equal values, ascending index."""
    return np.argsort(-L, axis=1, kind="stable")[:, :nsel].astype(np.int32)


def posteriors_on(Lsel, min_post=0.0, keep=None):
    """log-sum-exp and soft max over the given values per row (F, nsel), float64; entries below ``min_post`` zeroed -- or, with
    ``keep`` (a boolean mask), exactly the entries outside it -- and the rest renormalised.  Returns (post before pruning, post, loglik)."""
    mx = Lsel.max(1, keepdims=True)
    e = np.exp(Lsel - mx)
    s = e.sum(1, keepdims=True)
    p0 = e / s
    p = p0.copy()
    if keep is None and min_post > 0:
        keep = p0 >= min_post
        keep[np.arange(len(p0)), p0.argmax(1)] = True
    if keep is not None:
        p = np.where(keep, p0, 0.0)
        p /= p.sum(1, keepdims=True)
    return p0, p, (mx + np.log(s))[:, 0]


def stats(X, idx, post, seg_off, C, order, dtype=np.float64, absolute=False):
    """slab (S, C, 1 + order D): sum over the segment's frames of gamma [1, x, x^2]; an idx outside [0, C) is skipped, a repeated one
    adds.  float64: a dense product per segment.  Another ``dtype``: a strictly SEQUENTIAL sum over the frames in that type (the direct
    form the bar is measured from).  ``absolute``: sum |gamma v|."""
    X = np.asarray(X).astype(dtype)
    V = np.concatenate([np.ones((len(X), 1), dtype), X] + ([X * X] if order == 2 else []), axis=1)
    if absolute:
        V = np.abs(V)
    S = len(seg_off) - 1
    out = np.zeros((S, C, V.shape[1]), dtype=dtype)
    for s in range(S):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        if b <= a:
            continue
        G = np.zeros((b - a, C), dtype=dtype)
        ii, pp = np.asarray(idx[a:b]), np.asarray(post[a:b]).astype(dtype)
        ok = (ii >= 0) & (ii < C)
        rows = np.broadcast_to(np.arange(b - a)[:, None], ii.shape)
        np.add.at(G, (rows[ok], ii[ok]), np.abs(pp[ok]) if absolute else pp[ok])
        if dtype == np.float64:
            out[s] = G.T @ V[a:b]
        else:
            for c0 in range(0, C, 64):      # (T, 64, NV) terms, added frame by frame
                out[s, c0:c0 + 64] = np.cumsum(G[:, c0:c0 + 64, None] * V[a:b, None, :], axis=0, dtype=dtype)[-1]
    return out


def update(acc, w, mu, var, var_floor, min_count, min_weight):
    """The M-step from (C, 1 + 2 D) float64 statistics: new (w, mu, var)."""
    D = mu.shape[1]
    N, Fs, Ss = acc[:, 0], acc[:, 1:1 + D], acc[:, 1 + D:]
    starved = (N < min_count) | ~(N > 0)
    wn = N / N.sum()
    wn = np.where(starved, np.maximum(wn, min_weight), wn)
    wn = wn / wn.sum()
    Nn = np.where(starved, 1.0, N)[:, None]
    m = np.where(starved[:, None], mu, Fs / Nn)
    v = np.where(starved[:, None], var, np.maximum(Ss / Nn - m * m, var_floor))
    return wn, m, v


def em_fit(X, w, mu, var, iters, var_floor, min_count, min_weight, float32_estep=False):
    """Exact EM (every Gaussian selected).  Returns (history of mean log-likelihoods per frame, each under the parameters its
    iteration started from; final w, mu, var).  ``float32_estep``: the E-step as float32 arithmetic does it -- the expanded product,
    log-sum-exp and soft max all in float32 -- with the sums and the M-step still in float64 (measurement of the bar only)."""
    X64 = np.asarray(X, dtype=np.float64)
    V = np.concatenate([np.ones((len(X64), 1)), X64, X64 * X64], axis=1)
    hist = []
    for _ in range(iters):
        if float32_estep:
            L = loglik_expanded_f32(X, w, mu, var)
            mx = L.max(1, keepdims=True)
            e = np.exp(L - mx, dtype=np.float32)
            s = e.sum(1, keepdims=True, dtype=np.float32)
            p, ll = (e / s).astype(np.float64), (mx + np.log(s, dtype=np.float32))[:, 0].astype(np.float64)
        else:
            _, p, ll = posteriors_on(loglik_direct(X, w, mu, var))
        hist.append(ll.sum() / len(X64))
        w, mu, var = update(p.T @ V, w, mu, var, var_floor, min_count, min_weight)
    return np.asarray(hist), w, mu, var


# ------------------------------------------------------------------------------------------------------------ measurement of the bars
def measure_loglik(D, C, nsel, F):
    X, w, mu, var = gmm_case(D, C, F)
    return float((np.abs(loglik_expanded_f32(X, w, mu, var).astype(np.float64) - loglik_direct(X, w, mu, var)) / loglik_scale(X, w, mu, var)).max())


def stats_segments(F):
    return np.array([0, F], dtype=np.int64)


def measure_stats(D, C, nsel, F):
    X, w, mu, var = gmm_case(D, C, F)
    L = loglik_direct(X, w, mu, var)
    idx = select(L, nsel)
    post = posteriors_on(np.take_along_axis(L, idx, 1))[1].astype(np.float32)
    seg = stats_segments(F)
    s64 = stats(X, idx, post, seg, C, 2)
    s32 = stats(X, idx, post, seg, C, 2, dtype=np.float32).astype(np.float64)
    scale = stats(X, idx, post, seg, C, 2, absolute=True)
    return float((np.abs(s32 - s64)[scale > 0] / scale[scale > 0]).max())


def measure_features():
    mel, off = feature_case()
    worst = 0.0
    for dct in (None, dct_table(20, mel.shape[1], 22)):
        d32 = None if dct is None else dct.astype(np.float32)
        o64 = features(mel, off, d32, 3, 2, 300)
        o32 = features(mel, off, d32, 3, 2, 300, dtype=np.float32).astype(np.float64)
        scale = features(mel, off, d32, 3, 2, 300, absolute=True)
        live = ~np.isnan(o64[:, 0])
        worst = max(worst, float((np.abs(o32 - o64)[live] / scale[live]).max()))
    return worst


def measure_em():
    s = EM_SHAPE
    X, w, mu, var = em_case()
    h64, _, m64, _ = em_fit(X, w, mu, var, s["iters"], s["var_floor"], s["min_count"], s["min_weight"])
    h32, _, m32, _ = em_fit(X, w, mu, var, s["iters"], s["var_floor"], s["min_count"], s["min_weight"], float32_estep=True)
    return float(np.abs(h32 - h64).max()), float(np.abs(m32 - m64).max())


if __name__ == "__main__":
    for sh in LOG_SHAPES:
        print("loglik", sh[:3], "%.3e" % measure_loglik(*sh))
    for sh in STATS_SHAPES:
        print("stats", sh[:3], "%.3e" % measure_stats(*sh))
    print("features %.3e" % measure_features())
    print("em history %.3e means %.3e" % measure_em())
