"""Float64 numpy restatement of the full-covariance UBM (include/ssv_hip.h, "I-vector groundwork: full-covariance UBM"), written from the
definitions there: planes, posteriors over a given selection, the centred statistics over the Gaussian-major lists, the M-step with the
kept rule, EM on a fixed selection, and the extractor's planes under full covariances.  Kaldi is not the yardstick; this file is.

The log-likelihood is in the DIRECT form -- numpy.linalg.solve and slogdet on Sigma itself -- not the whitened product the kernel
computes, so that the reference and the kernel do not share a factorisation.  Functions with ``float32=True`` are the "float32 numpy
form" the error bars are measured from (the ``measure_*`` functions), never a reference.

Error bars, by _ivector_ref.py's convention.  float32 paths: FACTOR x the worst error of the float32 numpy form against float64 on the
TEST'S OWN inputs, relative to the magnitudes of the terms; both numbers are recorded below, ``python tests/_fgmm_ref.py`` prints them
again, and tests/test_fgmm_cpu.py holds the recorded ones against a fresh measurement.  float64-only entries: BAR_F64, derived beside it.
"""
import numpy as np

import _ivector_ref as R
from _ivector_tv_ref import tri_pack, tri_unpack

FACTOR = R.FACTOR
# log-likelihood on the selected pairs, per (D, C, nsel) of POST_SHAPES and for ILL_SHAPE: worst |L32 - L64| / scale of the float32
# WHITENED form, scale = |g| + 1/2 sum_i (sum_j |W_ij| |x_j - mu_j|)^2
MEASURED_LOGLIK = {(13, 50, 5): 1.759e-07, (60, 64, 20): 9.603e-08, (128, 16, 8): 8.267e-08, (13, 21, 21): 1.701e-07}
MEASURED_LOGLIK_ILL = 1.666e-07          # the whitened form at cond(Sigma) = 1e3 ...
MEASURED_EXPANDED_ILL = 6.306e-06        # ... and the EXPANDED form x^T P x - 2 x^T P mu + mu^T P mu there, on the same scale: why it was not chosen
# statistics per (D, C, nsel) of STATS_SHAPES: worst |S32 - S64| / scale of a SEQUENTIAL float32 sum along each list of float32-centred
# rows; scale = sum gamma [1, a, a a^T], a = |x| + |mu| (the terms of the centring)
MEASURED_STATS = {(13, 50, 5): 4.399e-07, (60, 64, 20): 2.707e-07}
MEASURED_STATS_HAND = 4.394e-07         # the same on hand_case (the list and run edges)
# EM per (D, C, nsel, F, iters) of EM_SHAPES: float64 against an E-step in float32 (whitened product, soft max and centring in float32)
MEASURED_EM_HISTORY = {(5, 16, 16, 4000, 5): 1.080e-07, (13, 24, 5, 4000, 4): 3.544e-07}      # worst |history32 - history64|
MEASURED_EM_MEANS = {(5, 16, 16, 4000, 5): 1.309e-06, (13, 24, 5, 4000, 4): 2.170e-06}        # worst |mu32 - mu64| after the last iteration
MEASURED_EM_COVS = {(5, 16, 16, 4000, 5): 4.219e-06, (13, 24, 5, 4000, 4): 7.546e-06}         # worst |cov32 - cov64| after the last iteration
# The float64-only entries (planes, M-step, the extractor's planes before their final rounding) against numpy in float64.  Both sides
# carry about 2^-53 D cond(Sigma): a Cholesky inverse of a matrix of condition cond loses log2(cond) of its 53 bits and D terms meet in
# every entry.  The generators keep cond(Sigma) <= 1e3 (the ill-conditioned case; 4 elsewhere) and D <= 128, and the covariances the
# M-step tests produce stay below 1e4 (asserted in test_fgmm_cpu.py), so 2^-53 x 128 x 1e4 ~ 1.4e-10 is the far corner: 1e-9 of the
# largest entry holds with room, as _plda_ref.BAR_F64 does for the same functions.
BAR_F64 = 1e-9
BAR_ROUND = 2.0 ** -24              # a value rounded once to float32


def bar(measured):
    return FACTOR * measured


POST_SHAPES = ((13, 50, 5, 2000), (60, 64, 20, 600), (128, 16, 8, 64), (13, 21, 21, 70))      # (D, C, nsel, F); the last: every Gaussian selected
ILL_SHAPE = (13, 50, 5, 500)
ILL_COND = 1e3
STATS_SHAPES = ((13, 50, 5, 2000), (60, 64, 20, 600))
PLANES_SHAPES = ((1, 3), (13, 50), (60, 8), (128, 4))                                           # (D, C)
EM_SHAPES = ((5, 16, 16, 4000, 5), (13, 24, 5, 4000, 4))                                        # (D, C, nsel, F, iters); the first: exact EM
EM_RULES = dict(var_floor=1e-3, min_count=10.0, min_weight=1e-5)
KEPT_RULES = dict(var_floor=1e-3, min_count=10.0, min_weight=1e-2)                            # kept_case: a floor the starved Gaussian's weight lies below
TV_SHAPES = ((6, 13, 20), (4, 60, 192), (3, 1, 1))                                              # (C, D, R)
LOG2PI = float(np.log(2 * np.pi))


# ------------------------------------------------------------------------------------------------------------ test inputs
def rotations(C, D, rng):
    return np.stack([np.linalg.qr(rng.standard_normal((D, D)))[0] for _ in range(C)])


def full_case(D, C, F, seed=0, cond=None):
    """``_ivector_ref.gmm_case``'s frames, weights and means, with covariances Q diag(lambda) Q^T in random rotations: lambda uniform in
    [0.5, 2], or (``cond``) spread geometrically over [cond^-1/2, cond^1/2].  Returns X float32, w, mu float64, cov (C, Pd) packed, and
    the diagonal variances of gmm_case (the selector's)."""
    X, w, mu, var = R.gmm_case(D, C, F, seed)
    rng = np.random.default_rng(seed + 1000)
    Q = rotations(C, D, rng)
    if cond is None:
        lam = rng.uniform(0.5, 2, (C, D))
    else:
        lam = np.tile(np.geomspace(cond ** -0.5, cond ** 0.5, D) if D > 1 else np.ones(1), (C, 1))
    S = np.einsum("cij,cj,ckj->cik", Q, lam, Q)
    return X, w, mu, tri_pack((S + S.transpose(0, 2, 1)) / 2), var


def from_diag(var):
    """cov (C, Pd) with the given diagonals."""
    C, D = var.shape
    S = np.zeros((C, D, D))
    S[:, np.arange(D), np.arange(D)] = var
    return tri_pack(S)


def hand_idx(tile, C=9, seed=0):
    """A hand-made selection for the list and run edges: Gaussians 1 .. 6 get lists of length 0, 1, tile - 1, tile, tile + 1 and
    3 tile + 5, Gaussian 0 is selected by EVERY frame (column 0), column 1 holds the lists above spread over the frames in a shuffled
    order, the rest of it Gaussian 7 and, in 11 frames, indices outside [0, C); column 2 holds Gaussian 8 or an index outside.  Returns
    idx (F, 3) int32 and the wanted lengths of Gaussians 1 .. 6."""
    rng = np.random.default_rng(seed)
    want = [0, 1, tile - 1, tile, tile + 1, 3 * tile + 5]
    F = sum(want) + 150
    col1 = np.concatenate([np.full(n, c + 1) for c, n in enumerate(want)] + [np.full(139, 7), np.array([-1, C, C + 5, -7, 1 << 20] + [-3] * 6)])
    assert len(col1) == F
    rng.shuffle(col1)
    col2 = np.where(rng.random(F) < 0.5, 8, np.where(rng.random(F) < 0.5, -1, C))
    return np.stack([np.zeros(F, np.int64), col1, col2], 1).astype(np.int32), want


def group(idx, C):
    """(start (C + 1), pairs): numpy's stable argsort of the slots by Gaussian, the slots outside [0, C) left out."""
    flat = np.asarray(idx).reshape(-1).astype(np.int64)
    ok = (flat >= 0) & (flat < C)
    order = np.argsort(np.where(ok, flat, C), kind="stable")
    n = int(ok.sum())
    start = np.concatenate([[0], np.cumsum(np.bincount(flat[ok], minlength=C))]).astype(np.int32)
    return start, order[:n].astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ the mixture
def unpack(cov):
    return tri_unpack(cov)


def planes(w, mu, cov):
    """float64 (W (C, D, D) lower triangular, g (C), icov (C, Pd), cond (C))."""
    S = unpack(cov)
    Lc = np.linalg.cholesky(S)
    W = np.linalg.inv(Lc)
    logdet = 2 * np.log(np.einsum("cii->ci", Lc)).sum(1)
    g = np.log(w) - 0.5 * (mu.shape[1] * LOG2PI + logdet)
    return np.tril(W), g, tri_pack(np.linalg.inv(S)), np.linalg.cond(S)


def loglik_direct(X, w, mu, cov):
    """(F, C) float64, the direct form: solve and slogdet on Sigma."""
    X = np.asarray(X, dtype=np.float64)
    S = unpack(cov)
    out = np.empty((X.shape[0], len(w)))
    for c in range(len(w)):
        d = X - mu[c]
        out[:, c] = np.log(w[c]) - 0.5 * (X.shape[1] * LOG2PI + np.linalg.slogdet(S[c])[1]) - 0.5 * (d * np.linalg.solve(S[c], d.T).T).sum(1)
    return out


def loglik_whitened_f32(X, w, mu, cov):
    """The kernel's form evaluated by float32 numpy: centre on the rounded mean, multiply by the rounded W, square and add."""
    W, g, _, _ = planes(w, mu, cov)
    W32, g32, mu32, X32 = W.astype(np.float32), g.astype(np.float32), mu.astype(np.float32), np.asarray(X, dtype=np.float32)
    out = np.empty((X32.shape[0], len(w)), dtype=np.float32)
    for c in range(len(w)):
        z = (X32 - mu32[c]) @ W32[c].T
        out[:, c] = g32[c] - np.float32(0.5) * (z * z).sum(1, dtype=np.float32)
    return out


def loglik_expanded_f32(X, w, mu, cov):
    """The form NOT chosen, in float32: x^T P x - 2 x^T (P mu) + mu^T P mu with P = Sigma^-1 (measurement only)."""
    _, g, icov, _ = planes(w, mu, cov)
    P = unpack(icov)
    X32 = np.asarray(X, dtype=np.float32)
    out = np.empty((X32.shape[0], len(w)), dtype=np.float32)
    for c in range(len(w)):
        P32, b32 = P[c].astype(np.float32), (P[c] @ mu[c]).astype(np.float32)
        k32 = np.float32(g[c] - 0.5 * mu[c] @ P[c] @ mu[c])
        out[:, c] = k32 + X32 @ b32 - np.float32(0.5) * ((X32 @ P32) * X32).sum(1, dtype=np.float32)
    return out


def loglik_scale(X, w, mu, cov):
    """(F, C): |g| + 1/2 sum_i (sum_j |W_ij| |x_j - mu_j|)^2, the magnitudes of the whitened form's terms."""
    W, g, _, _ = planes(w, mu, cov)
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((X.shape[0], len(w)))
    for c in range(len(w)):
        a = np.abs(X - mu[c]) @ np.abs(W[c]).T
        out[:, c] = np.abs(g[c]) + 0.5 * (a * a).sum(1)
    return out


def select(X, w, mu, var, nsel):
    """The selector: the nsel likeliest Gaussians of the DIAGONAL mixture (w, mu, var)."""
    return R.select(R.loglik_direct(X, w, mu, var), nsel)


def posteriors(X, w, mu, cov, idx, min_post=0.0, C=None):
    """On a given selection: (L on the slots (NaN where idx lies outside), post before pruning, post, loglik); a slot outside takes no part."""
    C = len(w) if C is None else C
    L = loglik_direct(X, w, mu, cov)
    ok = (idx >= 0) & (idx < C)
    Ls = np.where(ok, np.take_along_axis(L, np.clip(idx, 0, C - 1).astype(np.int64), 1), -np.inf)
    p0, p, ll = R.posteriors_on(Ls, min_post)
    return np.where(ok, Ls, np.nan), p0, p, ll


# ------------------------------------------------------------------------------------------------------------ statistics and the M-step
def full_stats(X, mu, idx, post, C, float32=False, absolute=False):
    """(C, 1 + D + Pd): N, S1, S2 (packed) centred on mu over each Gaussian's list.  ``float32``: rows centred in float32 on the rounded
    mean and summed SEQUENTIALLY in float32 along the list; ``absolute``: the scale, sum gamma [1, a, a a^T] with a = |x| + |mu|."""
    D = X.shape[1]
    start, pairs = group(idx, C)
    nsel = idx.shape[1]
    dt = np.float32 if float32 else np.float64
    out = np.zeros((C, 1 + D + D * (D + 1) // 2), dtype=np.float64)
    gam_all = np.asarray(post).reshape(-1)
    for c in range(C):
        sl = pairs[start[c]:start[c + 1]].astype(np.int64)
        if not len(sl):
            continue
        f, gam = sl // nsel, gam_all[sl].astype(dt)
        if absolute:
            xc = np.abs(X[f].astype(np.float64)) + np.abs(mu[c])
        elif float32:
            xc = X[f].astype(np.float32) - mu[c].astype(np.float32)
        else:
            xc = X[f].astype(np.float64) - mu[c]
        terms = np.concatenate([np.ones((len(sl), 1), dt), xc, tri_pack(xc[:, :, None] * xc[:, None, :])], 1) * gam[:, None]
        out[c] = np.cumsum(terms, axis=0, dtype=dt)[-1] if float32 else terms.sum(0)
    return out


def pivots(S):
    """L_ii^2 of the Cholesky factor, the conditional variance of dimension i given those before it; a matrix that has none (not positive
    definite) gives zeros from the failing pivot on."""
    D = S.shape[0]
    A = S.copy()
    out = np.zeros(D)
    for j in range(D):
        if not A[j, j] > 0:
            break
        out[j] = A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j]) / A[j, j]
    return out


def update(acc, w, mu, cov, var_floor, min_count, min_weight):
    """The M-step from (C, 1 + D + Pd) float64 statistics: (w, mu, cov, kept, smallest pivot per Gaussian (inf where starved))."""
    C, D = mu.shape
    N, S1, S2 = acc[:, 0], acc[:, 1:1 + D], acc[:, 1 + D:]
    kept = (N < min_count) | ~(N > 0)
    mu2, cov2, piv = mu.copy(), cov.copy(), np.full(C, np.inf)
    for c in range(C):
        if kept[c]:
            continue
        dl = S1[c] / N[c]
        Sn = tri_unpack(S2[c]) / N[c] - np.outer(dl, dl)
        piv[c] = pivots(Sn).min()
        if piv[c] < var_floor:
            kept[c] = True
            continue
        mu2[c], cov2[c] = mu[c] + dl, tri_pack(Sn)
    wn = N / N.sum()
    wn = np.where(kept, np.maximum(wn, min_weight), wn)
    return wn / wn.sum(), mu2, cov2, kept, piv


def em_fit(X, w, mu, cov, idx, iters, var_floor, min_count, min_weight, float32=False):
    """EM on the fixed selection ``idx``.  Returns (history of mean log-likelihoods over the selected, each under the parameters its
    iteration started from; w, mu, cov; any Gaussian kept; smallest occupancy; smallest pivot).  ``float32``: the E-step as float32
    arithmetic does it (whitened product, soft max, centring), the sums and the M-step in float64 (measurement of the bar only)."""
    C = len(w)
    hist, any_kept, min_n, min_piv = [], False, np.inf, np.inf
    for _ in range(iters):
        if float32:
            L = np.take_along_axis(loglik_whitened_f32(X, w, mu, cov), idx.astype(np.int64), 1)
            mx = L.max(1, keepdims=True)
            e = np.exp(L - mx, dtype=np.float32)
            s = e.sum(1, keepdims=True, dtype=np.float32)
            p, ll = (e / s), (mx + np.log(s, dtype=np.float32))[:, 0].astype(np.float64)
            acc = full_stats(X, mu.astype(np.float32).astype(np.float64), idx, p, C)      # (the rounded mean; the subtraction's own rounding is below it)
        else:
            _, _, p, ll = posteriors(X, w, mu, cov, idx)
            acc = full_stats(X, mu, idx, p, C)
        hist.append(ll.sum() / len(X))
        w, mu, cov, kept, piv = update(acc, w, mu, cov, var_floor, min_count, min_weight)
        any_kept, min_n, min_piv = any_kept or bool(kept.any()), min(min_n, acc[:, 0].min()), min(min_piv, piv.min())
    return np.asarray(hist), w, mu, cov, any_kept, float(min_n), float(min_piv)


def em_case(D, C, nsel, F):
    """gmm_case's frames and mixture, the covariances its diagonals (FullUbm.from_diag), the selection by the diagonal mixture."""
    X, w, mu, var = R.gmm_case(D, C, F)
    return X, w, mu, from_diag(var), select(X, w, mu, var, nsel)


def kept_case(D=6, C=5, seed=3):
    """Float64 statistics for the kept rule: Gaussian 1 is starved (N = 3), the frames of Gaussian 3 lie in a subspace up to noise of
    1e-3 in the last dimension (conditional variance ~ 1e-6); the others are healthy.  Returns (acc, w, mu, cov)."""
    rng = np.random.default_rng(seed)
    w, mu = rng.dirichlet(np.full(C, 5.0)), rng.normal(0, 2, (C, D))
    cov = tri_pack(np.stack([np.eye(D)] * C))
    acc = np.zeros((C, 1 + D + D * (D + 1) // 2))
    for c in range(C):
        n = 3 if c == 1 else 400
        x = rng.normal(0, 1, (n, D)) @ rng.normal(0, 0.7, (D, D)) + rng.normal(0, 0.3, D)
        if c == 3:
            x[:, -1] = x[:, :-1] @ rng.normal(0, 1, D - 1) + rng.normal(0, 1e-3, n)
        gam = rng.uniform(0.2, 1.0, n)
        acc[c] = np.concatenate([[gam.sum()], gam @ x, tri_pack(np.einsum("n,ni,nj->ij", gam, x, x))])
    return acc, w, mu, cov


# ------------------------------------------------------------------------------------------------------------ the extractor's planes
def tv_case(C, D, Rk, seed=0):
    rng = np.random.default_rng(seed + 31 * C + 7 * D + Rk)
    """T (C, D, R) float64 and packed covariances (C, Pd) in random rotations, eigenvalues in [0.5, 2]."""
    Q = rotations(C, D, rng)
    S = np.einsum("cij,cj,ckj->cik", Q, rng.uniform(0.5, 2, (C, D)), Q)
    return rng.normal(0, 1, (C, D, Rk)), tri_pack((S + S.transpose(0, 2, 1)) / 2)


def tv_planes_full(T, icov):
    """G (C D, R) = Sigma^-1 T and packed Pk (C, P) = T^T G, float64, from the packed inverses."""
    C, D, Rk = T.shape
    G = np.einsum("cde,cer->cdr", unpack(icov), T)
    return G.reshape(C * D, Rk), tri_pack(np.einsum("cdi,cdj->cij", T, G))


def tv_em_fit(N, Ft, T, icov, iters, min_div=True, min_count=10.0, float32=False):
    """_ivector_tv_ref.em_fit with the planes of the full covariances: (objective history, its scale at the start, final T).
    ``float32``: the planes rounded and the two products as float32 matmul, w and M rounded (measurement of a bar only)."""
    import _ivector_tv_ref as TV
    U = N.shape[0]
    hist, scale0 = [], None
    for _ in range(iters):
        G, Pk = tv_planes_full(T, icov)
        if float32:
            Lp = (N.astype(np.float32) @ Pk.astype(np.float32)).astype(np.float64)
            b = (Ft.reshape(U, -1).astype(np.float32) @ G.astype(np.float32)).astype(np.float64)
        else:
            Lp, b = N.astype(np.float64) @ Pk, Ft.reshape(U, -1).astype(np.float64) @ G
        w, obj, M, scale = TV.estep_from(Lp, b)
        if float32:
            w, M = w.astype(np.float32).astype(np.float64), M.astype(np.float32).astype(np.float64)
        scale0 = float(scale.mean()) if scale0 is None else scale0
        A, Cm, Nc, Msum = TV.accumulate(N, Ft, w, M, float32)
        hist.append(obj.mean())
        T = TV.mstep(A, Cm, Nc, T, TV.min_div_factor(Msum, U) if min_div else None, min_count)
    return np.asarray(hist), scale0, T


# ------------------------------------------------------------------------------------------------------------ measurement of the bars
def _on_selection(A, idx):
    return np.take_along_axis(A, idx.astype(np.int64), 1)


def measure_loglik(D, C, nsel, F, cond=None, expanded=False):
    X, w, mu, cov, var = full_case(D, C, F, cond=cond)
    idx = select(X, w, mu, var, nsel)
    f32 = (loglik_expanded_f32 if expanded else loglik_whitened_f32)(X, w, mu, cov).astype(np.float64)
    err = np.abs(f32 - loglik_direct(X, w, mu, cov)) / loglik_scale(X, w, mu, cov)
    return float(_on_selection(err, idx).max())


def stats_case(D, C, nsel, F):
    X, w, mu, cov, var = full_case(D, C, F)
    idx = select(X, w, mu, var, nsel)
    post = posteriors(X, w, mu, cov, idx)[2].astype(np.float32)
    return X, w, mu, cov, idx, post


def measure_stats(D, C, nsel, F):
    X, w, mu, cov, idx, post = stats_case(D, C, nsel, F)
    s64, s32, scale = full_stats(X, mu, idx, post, C), full_stats(X, mu, idx, post, C, float32=True), full_stats(X, mu, idx, post, C, absolute=True)
    return float((np.abs(s32 - s64)[scale > 0] / scale[scale > 0]).max())


def hand_case(tile, D=7, C=9, seed=4):
    """Frames, means and posteriors (a fifth of them exactly 0: pruned pairs) on ``hand_idx``: (X, mu, idx, post, wanted lengths)."""
    idx, want = hand_idx(tile, C)
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 2, (len(idx), D)).astype(np.float32)
    post = np.where(rng.random(idx.shape) < 0.2, 0.0, rng.uniform(0.01, 1.0, idx.shape)).astype(np.float32)
    return X, rng.normal(0, 2, (C, D)), idx, post, want


def measure_stats_hand(tile=64):
    X, mu, idx, post, _ = hand_case(tile)
    s64, s32, scale = full_stats(X, mu, idx, post, 9), full_stats(X, mu, idx, post, 9, float32=True), full_stats(X, mu, idx, post, 9, absolute=True)
    return float((np.abs(s32 - s64)[scale > 0] / scale[scale > 0]).max())


def measure_em(D, C, nsel, F, iters):
    X, w, mu, cov, idx = em_case(D, C, nsel, F)
    a = em_fit(X, w, mu, cov, idx, iters, **EM_RULES)
    b = em_fit(X, w, mu, cov, idx, iters, float32=True, **EM_RULES)
    return float(np.abs(a[0] - b[0]).max()), float(np.abs(a[2] - b[2]).max()), float(np.abs(a[3] - b[3]).max())


if __name__ == "__main__":
    for sh in POST_SHAPES:
        print("loglik", sh[:3], "%.3e" % measure_loglik(*sh))
    print("loglik ill whitened %.3e expanded %.3e" % (measure_loglik(*ILL_SHAPE, cond=ILL_COND), measure_loglik(*ILL_SHAPE, cond=ILL_COND, expanded=True)))
    for sh in STATS_SHAPES:
        print("stats", sh[:3], "%.3e" % measure_stats(*sh))
    print("stats hand %.3e" % measure_stats_hand())
    for sh in EM_SHAPES:
        print("em", sh, "history %.3e means %.3e covs %.3e" % measure_em(*sh))
