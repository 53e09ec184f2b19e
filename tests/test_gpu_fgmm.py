"""The full-covariance UBM on the device against the float64 restatement (tests/_fgmm_ref.py): planes, the Gaussian-major selection lists,
posteriors over a selection, the centred statistics, the M-step with the kept rule, EM on a fixed selection, and the extractor on the
full planes.  Every float32 bar is one recorded in _fgmm_ref.py (FACTOR x the error of the float32 numpy form on these very inputs,
relative to the magnitudes of the terms); the float64 entries are held to BAR_F64.  Every output buffer is poisoned before the call."""
import functools

import numpy as np
import pytest
import torch

import _fgmm_ref as G
import _ivector_ref as R
import _ivector_tv_ref as TV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float32).eps)
NAN = float("nan")


def _iv():
    from spoofsv_amd import ivector
    return ivector


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)              # (a copy: the shared cases are read-only)


def _call(name, *args):
    from spoofsv_amd import _lib
    _lib.call(name, *args)


def _p(t):
    from spoofsv_amd import ops
    return ops._p(t)


def _st():
    from spoofsv_amd import ops
    return ops._stream()


def _ws(name, *args):
    from spoofsv_amd import _lib, ops
    return ops._ws(_lib.query(name, *args), DEV)


def _tile():
    from spoofsv_amd import _lib
    return _lib.lib().ssv_fgmm_pair_tile()


# ================================================================================================ shared cases (computed once)
@functools.lru_cache(maxsize=None)
def _case(D, C, nsel, F, cond=None):
    """Inputs, the device mixture, the reference's selection, L and its scale for one shape; nothing in it is modified afterwards."""
    X, w, mu, cov, var = G.full_case(D, C, F, cond=cond)
    ubm = _iv().FullUbm(_dev(w), _dev(mu), _dev(cov))
    case = dict(X=X, w=w, mu=mu, cov=cov, var=var, ubm=ubm, Xd=_dev(X), idx=G.select(X, w, mu, var, nsel), L=G.loglik_direct(X, w, mu, cov),
                scale=G.loglik_scale(X, w, mu, cov))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _planes(w, mu, cov):
    """ssv_fgmm_planes on poisoned outputs: (Wt, muf, g, icov) as numpy."""
    C, D = mu.shape
    Wt = torch.full((C, D, D), NAN, dtype=torch.float32, device=DEV)
    muf = torch.full((C, D), NAN, dtype=torch.float32, device=DEV)
    g = torch.full((C,), NAN, dtype=torch.float32, device=DEV)
    icov = torch.full((C, cov.shape[1]), NAN, dtype=torch.float64, device=DEV)
    wd, md, cd = _dev(w), _dev(mu), _dev(cov)
    _call("ssv_fgmm_planes", _p(wd), _p(md), _p(cd), _p(Wt), _p(muf), _p(g), _p(icov), C, D, _st())
    return Wt.cpu().numpy(), muf.cpu().numpy(), g.cpu().numpy(), icov.cpu().numpy()


def _group(idx, C):
    """ssv_fgmm_group_selection on poisoned outputs: device tensors (start, pairs)."""
    F, nsel = idx.shape
    start = torch.full((C + 1,), -7, dtype=torch.int32, device=DEV)
    pairs = torch.full((F * nsel,), -7, dtype=torch.int32, device=DEV)
    ws = _ws("ssv_fgmm_group_workspace", F, nsel, C)
    idx_d = _dev(idx)
    _call("ssv_fgmm_group_selection", _p(idx_d), _p(start), _p(pairs), F, nsel, C, _p(ws), ws.numel(), _st())
    return start, pairs


def _check_group(idx, C, start, pairs):
    want_start, want_pairs = G.group(idx, C)
    start, pairs = start.cpu().numpy(), pairs.cpu().numpy()
    assert np.array_equal(start, want_start) and np.array_equal(pairs[:len(want_pairs)], want_pairs)
    assert np.all(pairs[len(want_pairs):] == -7), "pairs beyond start[C] were written"


def _post(ubm, Xd, idx, min_post, C=None):
    """The two entries on poisoned outputs for the frames of Xd on the selection idx (numpy): (post, loglik) as numpy."""
    C = ubm.C if C is None else C
    F, nsel = idx.shape
    start, pairs = _group(idx, C)
    _check_group(idx, C, start, pairs)
    post = torch.full((F, nsel), NAN, dtype=torch.float32, device=DEV)
    ll = torch.full((F,), NAN, dtype=torch.float32, device=DEV)
    ws = _ws("ssv_fgmm_post_workspace", F, nsel)
    ws.fill_(0xFF)                                        # (NaN as float32)
    Wt, muf, g, _ = ubm.planes()
    idx_d = _dev(idx)
    _call("ssv_fgmm_select_post", _p(Xd), _p(Wt), _p(muf), _p(g), _p(idx_d), _p(start), _p(pairs), _p(post), _p(ll), F, ubm.D, C, nsel, float(min_post),
          _p(ws), ws.numel(), _st())
    return post.cpu().numpy(), ll.cpu().numpy()


def _check_posteriors(post, ll, Lsel, tol, nsel, min_post, what):
    """Agreement of post / loglik with the reference on the given selection (the logic of test_gpu_ivector._check_posteriors; the slots
    are in the selector's order, not the full mixture's, so the largest entry is wherever it is).  Lsel (F, nsel) float64, tol (F)."""
    assert np.isfinite(post).all() and np.isfinite(ll).all()
    kept = post > 0
    top = post.argmax(axis=1)
    assert kept[np.arange(len(post)), top].all(), "the largest entry was pruned"
    p0 = R.posteriors_on(Lsel)[0]
    # every L is off by at most tol_f: |d log p| <= 2 tol_f, once more for the renormalised sum; 16 eps for exp, the sums and the divisions
    # in float32.  The log-likelihood: tol_f in the maximum, 2 tol_f in the log-sum, 4 eps of its own magnitude for logf and the final sum.
    ptol = p0 * 4 * tol[:, None] + 16 * EPS
    if min_post > 0:
        assert 1.0 / nsel > min_post
        assert np.all(post[~kept] == 0.0) and np.all(p0[kept] >= min_post - ptol[kept]) and np.all(p0[~kept] <= min_post + ptol[~kept])
    _, p_ref, ll_ref = R.posteriors_on(Lsel, keep=kept if min_post > 0 else None)
    err_p = float((np.abs(post - p_ref) / ptol).max())
    err_ll = float((np.abs(ll - ll_ref) / (3 * tol + 4 * EPS * np.maximum(1.0, np.abs(ll_ref)))).max())
    rows = float(np.abs(post.astype(np.float64).sum(axis=1) - 1.0).max())
    print("%s min_post=%g: tol_f max %.3e, post err / bar %.3f, loglik err / bar %.3f, |row sum - 1| %.2e (bar %.2e)"
          % (what, min_post, tol.max(), err_p, err_ll, rows, 4 * EPS * nsel))
    assert err_p <= 1.0 and err_ll <= 1.0 and rows <= 4 * EPS * nsel


def _on(case, name, idx):
    return np.take_along_axis(case[name], idx.astype(np.int64), 1)


# ================================================================================================ planes
@pytest.mark.parametrize("D,C", G.PLANES_SHAPES)
def test_planes_against_float64(D, C):
    _, w, mu, cov, _ = G.full_case(D, C, C, seed=D)
    Wt, muf, g, icov = _planes(w, mu, cov)
    W, g64, icov64, cond = G.planes(w, mu, cov)
    assert cond.max() < 4.01
    assert np.all(Wt[:, np.triu_indices(D, 1)[0], np.triu_indices(D, 1)[1]] == 0.0), "Wt is not exactly zero above the diagonal"
    assert np.array_equal(muf, mu.astype(np.float32))
    eW = float(((np.abs(Wt - W) - G.BAR_ROUND * np.abs(W)).max(axis=(1, 2)) / np.abs(W).max(axis=(1, 2))).max())
    eg = float(((np.abs(g - g64) - G.BAR_ROUND * np.abs(g64)) / np.abs(g64).max()).max())
    ei = float((np.abs(icov - icov64).max(axis=1) / np.abs(icov64).max(axis=1)).max())
    print("planes D=%d C=%d: Wt %.3e and g %.3e beyond one float32 rounding, icov %.3e of its largest entry (bar %.1e)" % (D, C, eW, eg, ei, G.BAR_F64))
    assert eW <= G.BAR_F64 and eg <= G.BAR_F64 and ei <= G.BAR_F64


def test_planes_of_a_covariance_that_is_not_positive_definite_are_nan_for_that_gaussian_alone():
    D, C = 13, 6
    _, w, mu, cov, _ = G.full_case(D, C, C, seed=2)
    good = _planes(w, mu, cov)
    bad = cov.copy()
    S = G.unpack(cov[4:5])[0]
    S[7, 7] = S[7, 7] - 10.0                              # the eighth pivot turns negative
    bad[4] = G.tri_pack(S[None])[0]
    got = _planes(w, mu, bad)
    for a, b in zip(got, good):
        assert np.isnan(a[4]).all()
        assert np.array_equal(np.delete(a, 4, axis=0), np.delete(b, 4, axis=0))


# ================================================================================================ selection lists
def test_selection_lists_are_numpys_stable_argsort_at_the_tile_edges():
    tile = _tile()
    idx, want = G.hand_idx(tile)
    C = 9
    start, pairs = _group(idx, C)
    _check_group(idx, C, start, pairs)
    lens = np.diff(start.cpu().numpy())
    assert lens[1:7].tolist() == [0, 1, tile - 1, tile, tile + 1, 3 * tile + 5] and lens[0] == len(idx)


def test_selection_lists_over_many_blocks_and_python_surface():
    case = _case(13, 50, 5, 2000)
    idx = np.tile(case["idx"], (3, 1))                    # 30,000 slots: eight blocks of the counting sort
    start, pairs = _group(idx, 50)
    _check_group(idx, 50, start, pairs)
    s2, p2 = case["ubm"].group(_dev(idx))
    assert torch.equal(s2, start) and torch.equal(p2, pairs)


# ================================================================================================ posteriors
@pytest.mark.parametrize("min_post", (0.0, 0.025))
@pytest.mark.parametrize("D,C,nsel,F", G.POST_SHAPES)
def test_posteriors_against_float64_on_a_given_selection(D, C, nsel, F, min_post):
    case = _case(D, C, nsel, F)
    idx = case["idx"]
    post, ll = _post(case["ubm"], case["Xd"], idx, min_post)
    tol = G.bar(G.MEASURED_LOGLIK[(D, C, nsel)]) * _on(case, "scale", idx).max(axis=1)
    _check_posteriors(post, ll, _on(case, "L", idx), tol, nsel, min_post, "posteriors D=%d C=%d nsel=%d F=%d" % (D, C, nsel, F))


def test_posteriors_of_ill_conditioned_covariances_hold_the_whitened_bar():
    D, C, nsel, F = G.ILL_SHAPE
    case = _case(D, C, nsel, F, cond=G.ILL_COND)
    idx = case["idx"]
    post, ll = _post(case["ubm"], case["Xd"], idx, 0.0)
    tol = G.bar(G.MEASURED_LOGLIK_ILL) * _on(case, "scale", idx).max(axis=1)
    _check_posteriors(post, ll, _on(case, "L", idx), tol, nsel, 0.0, "posteriors at cond 1e3")


def test_posteriors_are_the_same_bits_again_and_for_frames_run_alone():
    case = _case(13, 50, 5, 2000)
    idx, ubm = case["idx"], case["ubm"]
    post, ll = _post(ubm, case["Xd"], idx, 0.025)
    again = _post(ubm, case["Xd"], idx, 0.025)
    assert np.array_equal(post, again[0]) and np.array_equal(ll, again[1])
    a, b = 517, 517 + 2 * _tile() + 3
    alone = _post(ubm, case["Xd"][a:b].contiguous(), np.ascontiguousarray(idx[a:b]), 0.025)
    assert np.array_equal(post[a:b], alone[0]) and np.array_equal(ll[a:b], alone[1])


def test_slots_outside_the_mixture_take_no_part():
    case = _case(13, 50, 5, 2000)
    F, ubm = 300, case["ubm"]
    idx = case["idx"][:F].copy()
    idx[::3, 1] = -1
    idx[1::7, 4] = 50
    idx[5] = -2                                           # a frame with no slot inside
    post, ll = _post(ubm, case["Xd"][:F].contiguous(), idx, 0.0)
    ok = (idx >= 0) & (idx < 50)
    assert np.all(post[~ok] == 0.0) and np.all(post[5] == 0.0) and ll[5] == -np.inf
    live = np.delete(np.arange(F), 5)
    Lsel = np.where(ok, np.take_along_axis(case["L"][:F], np.clip(idx, 0, 49).astype(np.int64), 1), -np.inf)[live]
    _, p_ref, ll_ref = R.posteriors_on(Lsel)
    tol = G.bar(G.MEASURED_LOGLIK[(13, 50, 5)]) * np.where(ok, np.take_along_axis(case["scale"][:F], np.clip(idx, 0, 49).astype(np.int64), 1), 0).max(axis=1)[live]
    assert np.all(np.abs(post[live] - p_ref) <= p_ref * 4 * tol[:, None] + 16 * EPS)
    assert np.all(np.abs(ll[live] - ll_ref) <= 3 * tol + 4 * EPS * np.maximum(1.0, np.abs(ll_ref)))


def test_full_ubm_with_diagonal_covariances_against_the_diagonal_kernel():
    """FullUbm.from_diag against DiagUbm.posteriors on the same selection, within the sum of the two recorded bars."""
    D, C, nsel, F = 13, 50, 5, 2000
    iv = _iv()
    X, w, mu, var = R.gmm_case(D, C, F)
    diag = iv.DiagUbm(_dev(w), _dev(mu), _dev(var))
    full = iv.FullUbm.from_diag(diag)
    Xd = _dev(X)
    idx, pd, ld = diag.posteriors(Xd, nsel)
    idx2, pf, lf = full.posteriors(Xd, nsel)
    assert torch.equal(idx, idx2)                         # the selector is the diagonal mixture itself
    idx3, pf3, lf3 = full.posteriors(Xd, idx=idx)
    assert torch.equal(pf, pf3) and torch.equal(lf, lf3)
    cov = G.from_diag(var)
    ii = idx.cpu().numpy().astype(np.int64)
    tol = (R.BAR_LOGLIK[(D, C, nsel)] * np.take_along_axis(R.loglik_scale(X, w, mu, var), ii, 1).max(axis=1)
           + G.bar(G.MEASURED_LOGLIK[(D, C, nsel)]) * np.take_along_axis(G.loglik_scale(X, w, mu, cov), ii, 1).max(axis=1))
    pdn, pfn = pd.cpu().numpy().astype(np.float64), pf.cpu().numpy().astype(np.float64)
    ep = float((np.abs(pdn - pfn) / (np.maximum(pdn, pfn) * 4 * tol[:, None] + 32 * EPS)).max())
    el = float((np.abs(ld.cpu().numpy() - lf.cpu().numpy()) / (3 * tol + 8 * EPS * np.maximum(1.0, np.abs(lf.cpu().numpy())))).max())
    print("diagonal FullUbm against DiagUbm: post %.3f, loglik %.3f of the summed bars" % (ep, el))
    assert ep <= 1.0 and el <= 1.0


# ================================================================================================ statistics
def _stats(X, mu, idx, post, C):
    """ssv_fgmm_stats on poisoned buffers, muf = mu rounded once."""
    F, D = X.shape
    nsel = idx.shape[1]
    start, pairs = _group(idx, C)
    out = torch.full((C, 1 + D + D * (D + 1) // 2), NAN, dtype=torch.float64, device=DEV)
    ws = _ws("ssv_fgmm_stats_workspace", F, nsel, C, D)
    ws.fill_(0xFF)
    Xd, mud, postd = _dev(X), _dev(mu.astype(np.float32)), _dev(post)
    _call("ssv_fgmm_stats", _p(Xd), _p(mud), _p(postd), _p(start), _p(pairs), _p(out), F, D, C, nsel, _p(ws), ws.numel(), _st())
    return out.cpu().numpy()


def _check_stats(got, X, mu, idx, post, C, bar, what):
    want, scale = G.full_stats(X, mu, idx, post, C), G.full_stats(X, mu, idx, post, C, absolute=True)
    assert np.isfinite(got).all()
    assert np.all(got[scale == 0] == 0.0), "an empty list does not give exact zeros"
    err = float((np.abs(got - want)[scale > 0] / scale[scale > 0]).max())
    print("%s: worst error %.3e of the terms' magnitudes (bar %.3e)" % (what, err, bar))
    assert err <= bar


@pytest.mark.parametrize("D,C,nsel,F", G.STATS_SHAPES)
def test_statistics_against_float64(D, C, nsel, F):
    from spoofsv_amd import _lib
    X, w, mu, cov, idx, post = G.stats_case(D, C, nsel, F)
    assert _lib.lib().ssv_fgmm_stats_runs(F, nsel, C) > 1            # the lists are split into runs
    got = _stats(X, mu, idx, post, C)
    _check_stats(got, X, mu, idx, post, C, G.bar(G.MEASURED_STATS[(D, C, nsel)]), "statistics D=%d C=%d nsel=%d F=%d" % (D, C, nsel, F))
    assert np.array_equal(got, _stats(X, mu, idx, post, C))           # the same bits again


def test_statistics_at_the_list_and_run_edges():
    from spoofsv_amd import _lib
    X, mu, idx, post, want = G.hand_case(_tile())
    assert _lib.lib().ssv_fgmm_stats_runs(len(X), 3, 9) == 2               # the lists of 3 tile + 5 and of every frame are split into two runs
    got = _stats(X, mu, idx, post, 9)
    _check_stats(got, X, mu, idx, post, 9, G.bar(G.MEASURED_STATS_HAND), "statistics on the hand-made lists %s" % (want,))
    assert want[0] == 0 and not got[1].any()                            # the Gaussian with an empty list: exact zeros


# ================================================================================================ M-step
def test_update_against_float64_with_a_starved_gaussian_and_one_in_a_subspace():
    iv = _iv()
    acc, w, mu, cov = G.kept_case()
    C, D = mu.shape
    ubm = iv.FullUbm(_dev(w), _dev(mu), _dev(cov))
    ubm.planes()
    for t in ubm._planes:
        t.fill_(NAN)
    ubm.w.fill_(NAN)
    kept = ubm.update(_dev(acc), **G.KEPT_RULES).cpu().numpy()
    w2, mu2, cov2, kept64, _ = G.update(acc, w, mu, cov, **G.KEPT_RULES)
    gw, gm, gc = ubm.w.cpu().numpy(), ubm.mu.cpu().numpy(), ubm.cov.cpu().numpy()
    assert kept.tolist() == kept64.astype(int).tolist() == [0, 1, 0, 1, 0]
    for c in (1, 3):
        assert np.array_equal(gm[c], mu[c]) and np.array_equal(gc[c], cov[c])                  # bit for bit
    ew, em, ec = float(np.abs(gw - w2).max() / w2.max()), float(np.abs(gm - mu2).max() / np.abs(mu2).max()), float(np.abs(gc - cov2).max() / np.abs(cov2).max())
    print("update: w %.3e, mu %.3e, cov %.3e of the largest entry (bar %.1e)" % (ew, em, ec, G.BAR_F64))
    assert ew <= G.BAR_F64 and em <= G.BAR_F64 and ec <= G.BAR_F64 and abs(gw.sum() - 1) < 1e-12
    n = acc[:, 0] / acc[:, 0].sum()
    mw = G.KEPT_RULES["min_weight"]
    wtot = float(np.where(kept64, np.maximum(n, mw), n).sum())
    assert n[1] < mw / 2 and abs(gw[1] - mw / wtot) <= G.BAR_F64                     # floored: the starved one is lifted to the floor ...
    assert n[3] > 2 * mw and abs(gw[3] - n[3] / wtot) <= G.BAR_F64                   # ... the floor leaves the other kept one where it was
    # the planes are those of the result
    W, g64, icov64, _ = G.planes(w2, mu2, cov2)
    Wt, muf, g, icov = (t.cpu().numpy() for t in ubm.planes())
    assert np.array_equal(muf, gm.astype(np.float32))
    assert np.abs(Wt - W).max() <= 2 * G.BAR_ROUND * np.abs(W).max() and np.abs(g - g64).max() <= 2 * G.BAR_ROUND * np.abs(g64).max()
    assert float((np.abs(icov - icov64).max(axis=1) / np.abs(icov64).max(axis=1)).max()) <= 10 * G.BAR_F64      # (cond 3e3 here, met twice)
    assert np.array_equal(ubm.diag().var.cpu().numpy(), np.einsum("cii->ci", G.unpack(gc)))


# ================================================================================================ EM
@pytest.mark.parametrize("D,C,nsel,F,iters", G.EM_SHAPES)
def test_em_on_a_fixed_selection_follows_the_float64_history(D, C, nsel, F, iters):
    iv = _iv()
    X, w, mu, var = R.gmm_case(D, C, F)
    Xd = _dev(X)
    diag = iv.DiagUbm(_dev(w), _dev(mu), _dev(var))
    idx = diag.posteriors(Xd, nsel)[0].cpu().numpy()      # the selection fit() takes: the reference runs on the device's own
    r = iv.train_full_ubm(diag, Xd, iters=iters, nsel=nsel, log=None, **G.EM_RULES)
    hist = np.array(r.history)
    h64, w64, mu64, cov64, any_kept, _, _ = G.em_fit(X, w, mu, G.from_diag(var), idx, iters, **G.EM_RULES)
    key = (D, C, nsel, F, iters)
    eh, em, ec = float(np.abs(hist - h64).max()), float(np.abs(r.ubm.mu.cpu().numpy() - mu64).max()), float(np.abs(r.ubm.cov.cpu().numpy() - cov64).max())
    print("EM %s: history %s\n  errors: history %.3e (bar %.3e), means %.3e (bar %.3e), covariances %.3e (bar %.3e)"
          % (key, hist, eh, G.bar(G.MEASURED_EM_HISTORY[key]), em, G.bar(G.MEASURED_EM_MEANS[key]), ec, G.bar(G.MEASURED_EM_COVS[key])))
    assert not any_kept and len(hist) == iters
    assert eh <= G.bar(G.MEASURED_EM_HISTORY[key]) and em <= G.bar(G.MEASURED_EM_MEANS[key]) and ec <= G.bar(G.MEASURED_EM_COVS[key])
    assert np.all(np.diff(hist) >= -G.bar(G.MEASURED_EM_HISTORY[key]))
    assert np.abs(r.ubm.w.cpu().numpy() - w64).max() <= G.bar(G.MEASURED_EM_MEANS[key])


# ================================================================================================ the extractor
def _tv_planes(entry, T, second):
    C, D, Rk = T.shape
    Gd = torch.full((C * D, Rk), NAN, dtype=torch.float32, device=DEV)
    Pk = torch.full((C, Rk * (Rk + 1) // 2), NAN, dtype=torch.float32, device=DEV)
    Td, sd = _dev(T), _dev(second)
    _call(entry, _p(Td), _p(sd), _p(Gd), _p(Pk), C, D, Rk, _st())
    return Gd.cpu().numpy(), Pk.cpu().numpy()


@pytest.mark.parametrize("C,D,Rk", G.TV_SHAPES)
def test_extractor_planes_on_full_covariances(C, D, Rk):
    T, cov = G.tv_case(C, D, Rk)
    icov = G.tri_pack(np.linalg.inv(G.unpack(cov)))
    got = _tv_planes("ssv_ivec_tv_planes_full", T, icov)
    for name, a, b in zip(("G", "Pk"), got, G.tv_planes_full(T, icov)):
        err = float(((np.abs(a - b) - G.BAR_ROUND * np.abs(b)) / np.abs(b).max()).max())
        print("full planes (%d, %d, %d) %s: %.3e of the largest entry beyond one float32 rounding (bar %.1e)" % (C, D, Rk, name, err, G.BAR_F64))
        assert np.isfinite(a).all() and err <= G.BAR_F64
    # diagonal covariances: the diagonal entry's planes, within the float32 rounding of the outputs
    var = np.random.default_rng(C).uniform(0.5, 2, (C, D))
    full = _tv_planes("ssv_ivec_tv_planes_full", T, G.from_diag(1.0 / var))
    diag = _tv_planes("ssv_ivec_tv_planes", T, var)
    for a, b in zip(full, diag):
        assert np.all(np.abs(a - b) <= 2 * G.BAR_ROUND * np.abs(b) + 1e-12 * np.abs(b).max())


@functools.lru_cache(maxsize=None)
def _chain_case():
    """40 utterances of 50-150 frames drawn from 16 Gaussians in 13 dimensions, each utterance with an offset of its own."""
    C, D, U = 16, 13, 40
    rng = np.random.default_rng(21)
    w, mu, var = TV.ubm_case(C, D, rng)
    lens = rng.integers(50, 151, U)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    comp = rng.choice(C, off[-1], p=w)
    shift = np.repeat(rng.normal(0, 0.5, (U, D)), lens, axis=0)
    X = (mu[comp] + shift + np.sqrt(var[comp]) * rng.standard_normal((off[-1], D))).astype(np.float32)
    return X, off, w, mu, var


def test_chain_on_the_full_ubm_follows_the_reference_em_on_the_devices_own_statistics():
    iv = _iv()
    X, off, w, mu, var = _chain_case()
    Xd = _dev(X)
    diag = iv.DiagUbm(_dev(w), _dev(mu), _dev(var))
    full = iv.train_full_ubm(diag, Xd, iters=2, nsel=8, log=None).ubm
    r = iv.train_ivector_extractor(full, Xd, off, 8, iters=3, nsel=8, log=None)
    assert r.tv.cov is not None and isinstance(r.tv.ubm(), iv.FullUbm) and torch.equal(r.tv.cov, full.cov)
    N, Ft = r.N.cpu().numpy(), r.Ft.cpu().numpy()
    icov = full.icov.cpu().numpy()
    T0 = TV.init_T(full.var.cpu().numpy(), 8, seed=0)
    h64, scale, T64 = G.tv_em_fit(N, Ft, T0, icov, 3)
    h32, _, _ = G.tv_em_fit(N, Ft, T0, icov, 3, float32=True)
    bar = G.FACTOR * max(float(np.abs(h32 - h64).max()) / scale, G.BAR_ROUND)      # the float32 form's own error on these statistics
    err = float(np.abs(np.array(r.history) - h64).max() / scale)
    print("chain on the full UBM: history %s, error %.3e of the objective's scale (bar %.3e)" % (r.history, err, bar))
    assert err <= bar and np.all(np.diff(r.history) >= -bar * scale)
    assert np.abs(r.tv.T.cpu().numpy() - T64).max() <= 1e-3 * np.abs(T64).max()


def test_extraction_under_the_full_ubm_does_not_depend_on_the_passes(monkeypatch):
    from spoofsv_amd import ops
    iv = _iv()
    X, off, w, mu, var = _chain_case()
    U, nsel, Rk = 6, 8, 8
    Xd = _dev(X[:off[U]])
    _, fw, fmu, cov, _ = G.full_case(13, 16, 16, seed=5)
    full = iv.FullUbm(_dev(w), _dev(mu), _dev(cov))
    tv = iv.TotalVariability.from_ubm(full, Rk, seed=1)
    want = iv.extract_ivectors(tv, Xd, off[:U + 1], nsel=nsel)
    assert bool(torch.isfinite(want).all()) and bool(want.any())
    need = iv.plan_extract_passes(np.diff(off[:U + 1]), 16, 13, Rk, nsel, 0)[1]
    monkeypatch.setattr(ops, "free_bytes", lambda device: need)
    passes = iv.plan_extract_passes(np.diff(off[:U + 1]), 16, 13, Rk, nsel, ops.free_bytes(DEV))[0]
    assert len(passes) > 1
    assert torch.equal(iv.extract_ivectors(tv, Xd, off[:U + 1], nsel=nsel), want)
    one = torch.cat([iv.extract_ivectors(tv, Xd[off[u]:off[u + 1]].contiguous(), np.array([0, off[u + 1] - off[u]]), nsel=nsel) for u in range(U)])
    assert torch.equal(one, want)                         # one utterance per call: the same bits


def test_the_diagonal_chain_keeps_its_bits():
    """The diagonal-UBM chain returns what the diagonal planes route returns when called explicitly: a TotalVariability without cov goes
    through ssv_ivec_tv_planes and nothing else changed under it."""
    iv = _iv()
    X, off, w, mu, var = _chain_case()
    Xd = _dev(X)
    diag = iv.DiagUbm(_dev(w), _dev(mu), _dev(var))
    r = iv.train_ivector_extractor(diag, Xd, off, 8, iters=2, nsel=8, log=None)
    assert r.tv.cov is None and isinstance(r.tv.ubm(), iv.DiagUbm)
    # the same chain with the planes built by the explicit call of the diagonal entry after every update
    N, F = iv.bw_stats(diag, Xd, off, 8, 0.025)
    Ft = iv.centre_stats(diag, N, F, out=F)
    assert torch.equal(N, r.N) and torch.equal(Ft, r.Ft)
    tv = iv.TotalVariability.from_ubm(diag, 8, 0)
    hist = []
    for _ in range(2):
        Gd, Pk = (torch.from_numpy(a).to(DEV) for a in _tv_planes("ssv_ivec_tv_planes", tv.T.cpu().numpy(), var))
        assert torch.equal(Gd, tv.G) and torch.equal(Pk, tv.Pk)
        hist.append(float(tv.em_step(N, Ft)))
    assert hist == r.history and torch.equal(tv.T, r.tv.T)
    assert torch.equal(iv.extract_ivectors(tv, Xd, off, nsel=8), iv.extract_ivectors(r.tv, Xd, off, nsel=8))
    # and the full route on the same diagonal covariances is another computation that agrees to float32 rounding, not the same call
    full_planes = _tv_planes("ssv_ivec_tv_planes_full", tv.T.cpu().numpy(), G.from_diag(1.0 / var))
    assert np.abs(full_planes[0] - tv.G.cpu().numpy()).max() <= 2 * G.BAR_ROUND * np.abs(full_planes[0]).max()
