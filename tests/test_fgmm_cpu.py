"""The full-covariance UBM, the parts that need no device: the recorded bars against a fresh measurement, the reference's EM on the two EM
shapes (no Gaussian kept, history non-decreasing), the kept-rule case lying clear of its thresholds, the new C-ABI entries and their
argument errors, the state round trips and the pass planner."""
import ctypes

import numpy as np
import pytest
import torch

import _fgmm_ref as G
import _ivector_tv_ref as TV
from spoofsv_amd import _lib, ivector

ENTRIES = (("ssv_fgmm_planes", 10), ("ssv_fgmm_pair_tile", 0), ("ssv_fgmm_stats_runs", 3), ("ssv_fgmm_group_workspace", 3), ("ssv_fgmm_post_workspace", 2),
           ("ssv_fgmm_stats_workspace", 4), ("ssv_fgmm_group_selection", 9), ("ssv_fgmm_select_post", 17), ("ssv_fgmm_stats", 13), ("ssv_fgmm_update", 15),
           ("ssv_ivec_tv_planes_full", 8))


# ================================================================================================ the reference
def test_recorded_bars_hold_against_a_fresh_measurement():
    """Another BLAS may block differently: the fresh figure must lie within a factor 4 of the recorded one, not equal it."""
    fresh = [(("loglik",) + sh[:3], G.measure_loglik(*sh), G.MEASURED_LOGLIK[sh[:3]]) for sh in G.POST_SHAPES]
    fresh += [("loglik ill", G.measure_loglik(*G.ILL_SHAPE, cond=G.ILL_COND), G.MEASURED_LOGLIK_ILL),
              ("expanded ill", G.measure_loglik(*G.ILL_SHAPE, cond=G.ILL_COND, expanded=True), G.MEASURED_EXPANDED_ILL)]
    fresh += [(("stats",) + sh[:3], G.measure_stats(*sh), G.MEASURED_STATS[sh[:3]]) for sh in G.STATS_SHAPES]
    fresh += [("stats hand", G.measure_stats_hand(_lib.lib().ssv_fgmm_pair_tile()), G.MEASURED_STATS_HAND)]
    for sh in G.EM_SHAPES:
        h, m, c = G.measure_em(*sh)
        fresh += [(("em history",) + sh, h, G.MEASURED_EM_HISTORY[sh]), (("em means",) + sh, m, G.MEASURED_EM_MEANS[sh]), (("em covs",) + sh, c, G.MEASURED_EM_COVS[sh])]
    for key, val, rec in fresh:
        assert rec / 4 <= val <= 4 * rec, (key, val, rec)
    # why the whitened form: at cond 1e3 it stays at the well-conditioned level, the expanded form is beyond the whitened form's bar
    assert G.MEASURED_LOGLIK_ILL < 2 * max(G.MEASURED_LOGLIK.values()) and G.MEASURED_EXPANDED_ILL > 2 * G.bar(G.MEASURED_LOGLIK_ILL)


def test_direct_form_is_the_whitened_form_in_float64():
    """The reference's two statements of the model agree: solve / slogdet on Sigma against g - 1/2 |W (x - mu)|^2 from its planes."""
    X, w, mu, cov, _ = G.full_case(13, 7, 40, cond=G.ILL_COND)
    W, g, icov, cond = G.planes(w, mu, cov)
    assert np.all(np.triu(W, 1) == 0) and cond.max() < 1.01 * G.ILL_COND
    z = np.einsum("cij,fcj->fci", W, X.astype(np.float64)[:, None, :] - mu[None])
    L = G.loglik_direct(X, w, mu, cov)
    assert np.abs(g[None] - 0.5 * (z * z).sum(2) - L).max() < 1e-9 * np.abs(L).max()
    assert np.abs(np.einsum("cij,cjk->cik", G.unpack(icov), G.unpack(cov)) - np.eye(13)).max() < 1e-10


@pytest.mark.parametrize("D,C,nsel,F,iters", G.EM_SHAPES)
def test_em_of_the_reference_keeps_no_gaussian_and_never_loses_likelihood(D, C, nsel, F, iters):
    X, w, mu, cov, idx = G.em_case(D, C, nsel, F)
    hist, w2, mu2, cov2, any_kept, min_n, min_piv = G.em_fit(X, w, mu, cov, idx, iters, **G.EM_RULES)
    print("EM D=%d C=%d: smallest occupancy %.1f, smallest pivot %.3f, history %s" % (D, C, min_n, min_piv, hist))
    assert not any_kept and min_n > 2 * G.EM_RULES["min_count"] and min_piv > 2 * G.EM_RULES["var_floor"]
    assert len(hist) == iters and np.all(np.diff(hist) >= 0), hist
    assert abs(w2.sum() - 1) < 1e-12 and w2.min() > 2 * G.EM_RULES["min_weight"]
    assert max(np.linalg.cond(S) for S in G.unpack(cov2)) < 1e4            # what BAR_F64 counts on


def test_kept_case_lies_clear_of_its_thresholds():
    """Every pivot and count of the reference lies outside [x / 2, 2 x] of its threshold: the device cannot decide differently by rounding."""
    acc, w, mu, cov = G.kept_case()
    r = G.KEPT_RULES
    w2, mu2, cov2, kept, piv = G.update(acc, w, mu, cov, **r)
    n = acc[:, 0] / acc[:, 0].sum()
    assert n[1] < r["min_weight"] / 2 and n[3] > 2 * r["min_weight"] and w2[1] > 2 * n[1]      # the floor lifts the starved one alone
    assert kept.tolist() == [False, True, False, True, False]
    assert not np.any((acc[:, 0] >= r["min_count"] / 2) & (acc[:, 0] <= 2 * r["min_count"]))
    live = np.isfinite(piv)
    assert live.tolist() == [True, False, True, True, True] and not np.any((piv[live] >= r["var_floor"] / 2) & (piv[live] <= 2 * r["var_floor"]))
    assert 0 < piv[3] < r["var_floor"] / 2
    for c in (1, 3):
        assert np.array_equal(mu2[c], mu[c]) and np.array_equal(cov2[c], cov[c])
    assert abs(w2.sum() - 1) < 1e-12 and max(np.linalg.cond(S) for S in G.unpack(cov2)) < 1e4


def test_grouping_of_the_reference_on_the_hand_made_selection():
    tile = _lib.lib().ssv_fgmm_pair_tile()
    idx, want = G.hand_idx(tile)
    start, pairs = G.group(idx, 9)
    lens = np.diff(start)
    assert lens[1:7].tolist() == want and lens[0] == len(idx) and start[-1] == len(pairs) < idx.size
    flat = idx.reshape(-1)
    for c in range(9):
        sl = pairs[start[c]:start[c + 1]]
        assert np.all(flat[sl] == c) and np.all(np.diff(sl) > 0)


# ================================================================================================ the C ABI
def test_entries_are_declared_and_exported():
    L = _lib.lib()
    protos = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name, nargs in ENTRIES:
        assert name in protos and hasattr(raw, name), name
        assert len(protos[name][1]) == nargs, (name, protos[name][2])
    assert L.ssv_version() == 7 and L.ssv_fgmm_pair_tile() == 64


def _sweep(entry, tag, good, cases, order):
    L = _lib.lib()
    assert set(good) == set(order)
    for key, bad, want in cases:
        a = dict(good, **{key: bad})
        rc = entry(*[a[k] for k in order])
        assert rc == want and tag in L.ssv_last_error(), (tag, key, bad, rc, L.ssv_last_error())


def test_bad_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # `one`: non-null, never dereferenced: the checks come first
    big = 1 << 40
    order = ("w", "mu", "cov", "Wt", "muf", "g", "icov", "C", "D", "st")
    good = dict(w=one, mu=one, cov=one, Wt=one, muf=one, g=one, icov=one, C=16, D=5, st=null)
    _sweep(L.ssv_fgmm_planes, b"fgmm_planes", good, [(k, null, -1) for k in order[:7]] + [("C", 0, -1), ("D", 0, -1), ("C", 2049, -2), ("D", 129, -2)], order)
    order = ("idx", "start", "pairs", "F", "nsel", "C", "ws", "nws", "st")
    good = dict(idx=one, start=one, pairs=one, F=100, nsel=5, C=16, ws=one, nws=big, st=null)
    _sweep(L.ssv_fgmm_group_selection, b"fgmm_group_selection", good,
           [(k, null, -1) for k in ("idx", "start", "pairs", "ws")] + [("F", 0, -1), ("nsel", 0, -1), ("C", 0, -1), ("nws", 0, -1), ("nsel", 33, -2), ("C", 2049, -2),
                                                                        ("F", 1 << 30, -2)], order)
    order = ("X", "Wt", "muf", "g", "idx", "start", "pairs", "post", "ll", "F", "D", "C", "nsel", "mp", "ws", "nws", "st")
    good = dict(X=one, Wt=one, muf=one, g=one, idx=one, start=one, pairs=one, post=one, ll=one, F=100, D=5, C=16, nsel=5, mp=0.0, ws=one, nws=big, st=null)
    _sweep(L.ssv_fgmm_select_post, b"fgmm_select_post", good,
           [(k, null, -1) for k in order[:9] + ("ws",)] + [("F", 0, -1), ("D", 0, -1), ("C", 0, -1), ("nsel", 0, -1), ("mp", -0.1, -1), ("mp", 1.0, -1), ("nws", 0, -1),
                                                             ("D", 129, -2), ("C", 2049, -2), ("nsel", 33, -2)], order)
    order = ("X", "muf", "post", "start", "pairs", "out", "F", "D", "C", "nsel", "ws", "nws", "st")
    good = dict(X=one, muf=one, post=one, start=one, pairs=one, out=one, F=100, D=5, C=16, nsel=5, ws=one, nws=big, st=null)
    _sweep(L.ssv_fgmm_stats, b"fgmm_stats", good,
           [(k, null, -1) for k in order[:6] + ("ws",)] + [("F", 0, -1), ("D", 0, -1), ("C", 0, -1), ("nsel", 0, -1), ("nws", 0, -1), ("D", 129, -2), ("C", 2049, -2),
                                                             ("nsel", 33, -2)], order)
    order = ("stats", "w", "mu", "cov", "Wt", "muf", "g", "icov", "kept", "C", "D", "vf", "mc", "mw", "st")
    good = dict(stats=one, w=one, mu=one, cov=one, Wt=one, muf=one, g=one, icov=one, kept=one, C=16, D=5, vf=1e-3, mc=10.0, mw=1e-5, st=null)
    _sweep(L.ssv_fgmm_update, b"fgmm_update", good,
           [(k, null, -1) for k in order[:9]] + [("C", 0, -1), ("D", 0, -1), ("vf", 0.0, -1), ("mc", -1.0, -1), ("mw", 0.0, -1), ("mw", 1.0, -1), ("C", 2049, -2),
                                                 ("D", 129, -2)], order)
    order = ("T", "icov", "G", "Pk", "C", "D", "R", "st")
    good = dict(T=one, icov=one, G=one, Pk=one, C=16, D=5, R=17, st=null)
    _sweep(L.ssv_ivec_tv_planes_full, b"ivec_tv_planes_full", good,
           [(k, null, -1) for k in order[:4]] + [("C", 0, -1), ("D", 0, -1), ("R", 0, -1), ("R", 193, -2), ("C", 2049, -2), ("D", 129, -2)], order)


def test_workspace_queries():
    L = _lib.lib()
    assert L.ssv_fgmm_group_workspace(100, 5, 16) == 256 and L.ssv_fgmm_group_workspace(200000, 20, 1024) == 977 * 1024 * 4
    assert L.ssv_fgmm_post_workspace(200000, 20) == 16000000 and L.ssv_fgmm_post_workspace(0, 20) == 0 and L.ssv_fgmm_post_workspace(5, 33) == 0
    assert L.ssv_fgmm_stats_runs(200000, 20, 1024) == 8 and L.ssv_fgmm_stats_runs(2000, 5, 50) == 3 and L.ssv_fgmm_stats_runs(10, 3, 9) == 1
    assert L.ssv_fgmm_stats_workspace(200000, 20, 1024, 60) == 8 * 1024 * 1891 * 4 and L.ssv_fgmm_stats_workspace(100, 5, 16, 129) == 0
    assert L.ssv_fgmm_group_workspace(1 << 30, 5, 16) == 0 and L.ssv_fgmm_stats_runs(100, 5, 2049) == 0


# ================================================================================================ host logic
def _host_full(C=6, D=4, seed=1):
    _, w, mu, cov, _ = G.full_case(D, C, 10, seed=seed)
    return ivector.FullUbm(*(torch.from_numpy(a) for a in (w, mu, cov)))


def test_full_ubm_state_round_trip_on_the_host(tmp_path):
    ubm = _host_full()
    path = str(tmp_path / "full.npz")
    ubm.save(path)
    back = ivector.FullUbm.load(path, device="cpu")
    assert sorted(ubm.state_dict()) == ["cov", "mu", "w"] and (back.C, back.D, back.Pd) == (6, 4, 10)
    for k, v in ubm.state_dict().items():
        assert back.state_dict()[k].dtype == torch.float64 and np.array_equal(back.state_dict()[k].numpy(), v.numpy())
    other = _host_full(seed=2).load_state_dict(ubm.state_dict())
    assert np.array_equal(other.cov.numpy(), ubm.cov.numpy())
    # from_diag and diag are inverse to each other; var is the diagonal
    d = ivector.DiagUbm(ubm.w, ubm.mu, ubm.var)
    f = ivector.FullUbm.from_diag(d)
    assert np.array_equal(f.cov.numpy(), G.from_diag(d.var.numpy())) and np.array_equal(f.diag().var.numpy(), d.var.numpy())
    assert np.array_equal(ubm.var.numpy(), np.einsum("cii->ci", G.unpack(ubm.cov.numpy())))
    with pytest.raises(ValueError, match="FullUbm"):
        ivector.FullUbm(ubm.w, ubm.mu, ubm.cov[:, :9])
    with pytest.raises(ValueError, match="FullUbm"):
        ivector.FullUbm(ubm.w, ubm.mu, ubm.cov.float())
    for call in (lambda: ubm.planes(), lambda: ubm.posteriors(torch.zeros(10, 4)), lambda: ubm.fit(torch.zeros(10, 4)),
                 lambda: ubm.group(torch.zeros(10, 3, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


def test_total_variability_state_with_and_without_cov(tmp_path):
    ubm = _host_full()
    rng = np.random.default_rng(0)
    T = torch.from_numpy(rng.normal(0, 1, (6, 4, 3)))
    plain = ivector.TotalVariability(T, ubm.w, ubm.mu, ubm.var)
    assert sorted(plain.state_dict()) == ["T", "mu", "var", "w"] and plain.cov is None and isinstance(plain.ubm(), ivector.DiagUbm)
    path = str(tmp_path / "plain.npz")
    plain.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["T", "mu", "var", "w"]                      # today's four keys
    assert ivector.TotalVariability.load(path, device="cpu").cov is None
    full = ivector.TotalVariability(T, ubm.w, ubm.mu, ubm.var, cov=ubm.cov)
    assert sorted(full.state_dict()) == ["T", "cov", "mu", "var", "w"] and isinstance(full.ubm(), ivector.FullUbm)
    path = str(tmp_path / "full.npz")
    full.save(path)
    back = ivector.TotalVariability.load(path, device="cpu")
    for k, v in full.state_dict().items():
        assert np.array_equal(back.state_dict()[k].numpy(), v.numpy())
    # from_ubm: the same draw order on either mixture, var = diag Sigma
    a = ivector.TotalVariability.from_ubm(ubm, 5, seed=3)
    b = ivector.TotalVariability.from_ubm(ivector.DiagUbm(ubm.w, ubm.mu, ubm.var), 5, seed=3)
    assert np.array_equal(a.T.numpy(), b.T.numpy()) and np.array_equal(a.T.numpy(), TV.init_T(ubm.var.numpy(), 5, seed=3))
    assert np.array_equal(a.cov.numpy(), ubm.cov.numpy()) and b.cov is None
    with pytest.raises(ValueError, match="cov"):
        ivector.TotalVariability(T, ubm.w, ubm.mu, ubm.var, cov=ubm.cov[:, :9])


def test_pass_planning_counts_the_inverse_covariances():
    C, D, Rk = 1024, 60, 192
    P, Pd = Rk * (Rk + 1) // 2, D * (D + 1) // 2
    for train in (True, False):
        plain, need = ivector.plan_tv_passes(2000, C, D, Rk, 10 ** 13, train)
        full, need_full = ivector.plan_tv_passes(2000, C, D, Rk, 10 ** 13, train, full=True)
        assert plain == full == [(0, 2000)] and need_full == need + C * Pd * 8
    fixed = (C * P + C * D * Rk + C + P) * 8 + C * Pd * 8
    per = 2 * P * 4 + Rk * 8 + 8 + 4
    passes, _ = ivector.plan_tv_passes(2000, C, D, Rk, fixed + 2 * 300 * per, True, full=True)      # half of the rest holds exactly 300
    assert passes[0] == (0, 300) and passes[-1] == (1800, 2000)
