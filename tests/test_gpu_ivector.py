"""The i-vector groundwork on the device against the float64 restatement (tests/_ivector_ref.py): cepstral features, Gaussian selection
and posteriors, sufficient statistics and their reduction, the M-step, EM and the whole chain from waveforms.  Every bar is one recorded
in _ivector_ref.py: 4 x the error of the float32 numpy form on these very inputs, relative to the magnitudes of the terms."""
import functools

import numpy as np
import pytest
import torch

import _ivector_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float32).eps)


def _iv():
    from spoofsv_amd import ivector
    return ivector


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ================================================================================================ shared cases (computed once)
@functools.lru_cache(maxsize=None)
def _gmm(D, C, F):
    """Inputs, the device mixture and the float64 reference L and its scale for one shape; nothing in it is modified afterwards."""
    X, w, mu, var = R.gmm_case(D, C, F)
    ubm = _iv().DiagUbm(_dev(w), _dev(mu), _dev(var))
    case = dict(X=X, w=w, mu=mu, var=var, ubm=ubm, Xd=_dev(X), L=R.loglik_direct(X, w, mu, var), scale=R.loglik_scale(X, w, mu, var).max(axis=1))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _gselect(case, F, nsel, min_post):
    """The entry itself on poisoned output buffers, frames [0, F) of the case."""
    from spoofsv_amd import _lib, ops
    ubm = case["ubm"]
    Xd = case["Xd"][:F].contiguous()
    idx = torch.full((F, nsel), -7, dtype=torch.int32, device=DEV)
    post = torch.full((F, nsel), float("nan"), dtype=torch.float32, device=DEV)
    ll = torch.full((F,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("ssv_gmm_diag_gselect", ops._p(Xd), ops._p(ubm.A), ops._p(ubm.B), ops._p(ubm.g), ops._p(idx), ops._p(post), ops._p(ll), F, ubm.D, ubm.C, nsel,
              float(min_post), ops._stream())
    return idx.cpu().numpy(), post.cpu().numpy(), ll.cpu().numpy()


def _check_posteriors(case, key, F, nsel, min_post):
    """Validity of the selection and agreement of post / loglik with the reference evaluated on the device's own selection."""
    C = case["ubm"].C
    idx, post, ll = _gselect(case, F, nsel, min_post)
    L, tol = case["L"][:F], R.BAR_LOGLIK[key] * case["scale"][:F]
    print("posteriors D=%d C=%d nsel=%d F=%d min_post=%g: tol_f max %.3e" % (key[0], key[1], nsel, F, min_post, tol.max()))
    assert idx.min() >= 0 and idx.max() < C and np.isfinite(post).all() and np.isfinite(ll).all()
    srt = np.sort(idx, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), "a Gaussian selected twice"
    kth = np.sort(L, axis=1)[:, C - nsel]                                         # the reference's nsel-th largest
    Lsel = np.take_along_axis(L, idx.astype(np.int64), 1)
    worst_in = float(((kth[:, None] - Lsel) / tol[:, None]).max())
    mask = np.ones(L.shape, bool)
    np.put_along_axis(mask, idx.astype(np.int64), False, 1)
    worst_out = float((((np.where(mask, L, -np.inf)).max(axis=1) - kth) / tol).max()) if nsel < C else -np.inf
    print("  selected below the reference's %d-th by at most %.3f tol_f, unselected above it by at most %.3f tol_f (bar 2)" % (nsel, worst_in, worst_out))
    assert worst_in <= 2.0 and worst_out <= 2.0
    assert np.all(np.diff(post, axis=1) <= 0), "not in descending order by the device's own values"
    # pruning: valid against the reference's unpruned posteriors, then the reference renormalised over the device's kept set
    kept = post > 0
    assert kept[:, 0].all() and np.all(post[:, 0] == post.max(axis=1)), "the largest entry was pruned"
    p0 = R.posteriors_on(Lsel)[0]
    # every L is off by at most tol_f: |d log p| <= 2 tol_f, once more for the renormalised sum; 16 eps for exp, the sums and the divisions
    # in float32.  The log-likelihood: tol_f in the maximum, 2 tol_f in the log-sum, 4 eps of its own magnitude for logf and the final sum.
    ptol = p0 * 4 * tol[:, None] + 16 * EPS
    if min_post > 0:
        assert 1.0 / nsel > min_post               # by construction the largest of nsel posteriors is >= 1 / nsel: no frame loses all of them
        assert np.all(post[~kept] == 0.0) and np.all(p0[kept] >= min_post - ptol[kept]) and np.all(p0[~kept] <= min_post + ptol[~kept])
    _, p_ref, ll_ref = R.posteriors_on(Lsel, keep=kept if min_post > 0 else None)      # (without pruning a float32 posterior may still underflow to 0)
    err_p = float((np.abs(post - p_ref) / ptol).max())
    err_ll = float((np.abs(ll - ll_ref) / (3 * tol + 4 * EPS * np.maximum(1.0, np.abs(ll_ref)))).max())
    rows = float(np.abs(post.astype(np.float64).sum(axis=1) - 1.0).max())
    print("  post err / bar %.3f, loglik err / bar %.3f, |row sum - 1| %.2e (bar %.2e)" % (err_p, err_ll, rows, 4 * EPS * nsel))
    assert err_p <= 1.0 and err_ll <= 1.0 and rows <= 4 * EPS * nsel
    return idx, post


# ================================================================================================ posteriors
@pytest.mark.parametrize("min_post", (0.0, 0.025))
@pytest.mark.parametrize("D,C,nsel,F", R.LOG_SHAPES)
def test_posteriors_selection_valid_and_values_against_float64(D, C, nsel, F, min_post):
    _check_posteriors(_gmm(D, C, F), (D, C, nsel), F, nsel, min_post)


@pytest.mark.parametrize("D,C,nsel,F", R.LOG_SHAPES)
def test_posteriors_at_the_frame_tile_edges(D, C, nsel, F):
    from spoofsv_amd import _lib
    tile = _lib.lib().ssv_gmm_frame_tile(D, C)
    assert tile in (16, 32) and tile + 1 <= F
    case = _gmm(D, C, F)
    for n in (1, tile - 1, tile, tile + 1):
        _check_posteriors(case, (D, C, nsel), n, nsel, 0.025)


def test_posteriors_python_surface():
    """DiagUbm.posteriors: shapes, the same bits on a second run, the argument errors."""
    D, C, F = 13, 50, 2000
    case = _gmm(D, C, F)
    a = case["ubm"].posteriors(case["Xd"], 5, 0.025)
    b = case["ubm"].posteriors(case["Xd"], 5, 0.025)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape == (F, 5) and a[2].shape == (F,)
    with pytest.raises(ValueError, match="nsel"):
        case["ubm"].posteriors(case["Xd"], 51)
    with pytest.raises(ValueError, match="X"):
        case["ubm"].posteriors(case["Xd"][:, :12])


# ================================================================================================ statistics
@functools.lru_cache(maxsize=None)
def _stats_case(D, C, nsel, F):
    case = _gmm(D, C, F)
    idx, post, _ = case["ubm"].posteriors(case["Xd"], nsel, 0.025)       # the DEVICE's selection: it does not enter the comparison
    return case, idx, post


def _layouts(F, tile):
    rng = np.random.default_rng(11)
    ragged = np.sort(rng.integers(0, F + 1, 299))
    return {"one": [0, F],
            "edges": np.cumsum([0, 0, 1, 63, 64, 65, tile - 1, tile + 1, 0, 700]).tolist() + [F],
            "inner": [5, 5, 900, F - 3],                                      # frames before the first and after the last segment belong to none
            "ragged300": [0] + ragged.tolist() + [F]}


@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("D,C,nsel,F", R.STATS_SHAPES)
def test_stats_against_float64_sums(D, C, nsel, F, order):
    from spoofsv_amd import _lib
    case, idx, post = _stats_case(D, C, nsel, F)
    ubm, Xd = case["ubm"], case["Xd"]
    idx_h, post_h = idx.cpu().numpy(), post.cpu().numpy()
    bar = R.BAR_STATS[(D, C, nsel)]
    for name, seg in _layouts(F, _lib.lib().ssv_gmm_frame_tile(D, C)).items():
        seg = np.asarray(seg, dtype=np.int64)
        assert name != "ragged300" or len(seg) - 1 == 300
        slab = ubm.stats(Xd, seg, order, idx, post)
        again = ubm.stats(Xd, _dev(seg), order, idx, post)                  # a device table: no host check; the same bits
        assert slab.shape == (len(seg) - 1, C, 1 + order * D) and torch.equal(slab, again)
        got = slab.cpu().numpy()
        want, scale = R.stats(case["X"], idx_h, post_h, seg, C, order), R.stats(case["X"], idx_h, post_h, seg, C, order, absolute=True)
        empty = np.diff(seg) == 0
        assert not got[empty].any() and not got[scale == 0].any()          # a segment of length 0 (and a Gaussian nobody selected): exact zeros
        err = float((np.abs(got - want)[scale > 0] / scale[scale > 0]).max())
        print("stats D=%d C=%d order=%d %s: S=%d, err / sum|gamma v| %.3e (bar %.3e)" % (D, C, order, name, len(seg) - 1, err, bar))
        assert err <= bar
        # the reduction: ascending s, in double -- bitwise numpy's
        red = ubm.reduce(slab).cpu().numpy()
        assert red.dtype == np.float64 and red.tobytes() == np.sum(got, axis=0, dtype=np.float64).tobytes()


def test_stats_skip_indices_outside_the_mixture():
    D, C, nsel, F = R.STATS_SHAPES[0]
    case, idx, post = _stats_case(D, C, nsel, F)
    bad = idx.clone()
    bad[::3, 1] = -1
    bad[1::3, 0] = C
    bad[2::7, 2] = 2 ** 30
    seg = np.array([0, 1000, F], dtype=np.int64)
    got = case["ubm"].stats(case["Xd"], seg, 2, bad, post).cpu().numpy()
    want = R.stats(case["X"], bad.cpu().numpy(), post.cpu().numpy(), seg, C, 2)
    scale = R.stats(case["X"], bad.cpu().numpy(), post.cpu().numpy(), seg, C, 2, absolute=True)
    assert np.isfinite(got).all() and float((np.abs(got - want)[scale > 0] / scale[scale > 0]).max()) <= R.BAR_STATS[(D, C, nsel)]
    with pytest.raises(ValueError, match="seg_off"):
        case["ubm"].stats(case["Xd"], [0, 900, 800, F], 2, idx, post)
    with pytest.raises(ValueError, match="seg_off"):
        case["ubm"].stats(case["Xd"], [0, F + 1], 2, idx, post)


# ================================================================================================ features
def _features(mel, off, dct, w, order, W):
    """The entry itself on a poisoned output buffer."""
    from spoofsv_amd import _lib, ops
    G, M = mel.shape
    Cc = M if dct is None else dct.shape[0]
    md, od, dd = _dev(mel), _dev(off), (None if dct is None else _dev(dct))
    out = torch.full((G, Cc * (order + 1)), -12345.0, dtype=torch.float32, device=DEV)
    nws = _lib.query("ssv_ivec_features_workspace", G, Cc, order)
    ws = torch.full((nws // 4,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("ssv_ivec_features", ops._p(md), ops._p(od), ops._p(dd), ops._p(out), G, M, len(off) - 1, Cc, w, order, W, ops._p(ws), nws, ops._stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("order", (0, 1, 2))
@pytest.mark.parametrize("use_dct", (False, True))
def test_features_against_float64_on_ragged_utterances(use_dct, order):
    mel, off = R.feature_case()
    assert sorted(np.diff(off).tolist()) == sorted(R.FEATURE_LENGTHS)
    dct = _iv().dct_table(20, mel.shape[1], 22) if use_dct else None
    got = _features(mel, off, dct, 3, order, 300)
    want, scale = R.features(mel, off, dct, 3, order, 300), R.features(mel, off, dct, 3, order, 300, absolute=True)
    live = ~np.isnan(want[:, 0])
    assert live.sum() == off[-1] - off[0] and np.all(got[~live] == -12345.0)           # frames in no utterance: nothing written
    err = float((np.abs(got - want)[live] / scale[live]).max())
    print("features dct=%s order=%d: err / scale %.3e (bar %.3e)" % (use_dct, order, err, R.BAR_FEATURES))
    assert err <= R.BAR_FEATURES
    if order == 2:
        # nothing crosses a boundary: every other utterance's frames (and the frames of none) set to 1e30
        for u in (0, 1, 3, 4):
            a, b = int(off[u]), int(off[u + 1])
            loud = np.full_like(mel, 1e30)
            loud[a:b] = mel[a:b]
            alone = _features(loud, off, dct, 3, order, 300)
            assert np.array_equal(alone[a:b], got[a:b]), "utterance %d reads its neighbours" % u


def test_cepstral_features_python_surface():
    iv = _iv()
    mel, off = R.feature_case()
    out = iv.cepstral_features(_dev(mel), off)
    assert out.shape == (len(mel), 60) and out.dtype == torch.float32
    want = _features(mel, off, iv.dct_table(20, 40, 22), 3, 2, 300)
    live = slice(int(off[0]), int(off[-1]))
    assert np.array_equal(out.cpu().numpy()[live], want[live]) and not out[:int(off[0])].any() and not out[int(off[-1]):].any()
    assert torch.equal(out, iv.cepstral_features(_dev(mel), _dev(off)))
    with pytest.raises(ValueError, match="utt_off"):
        iv.cepstral_features(_dev(mel), [0, 10, 5])
    with pytest.raises(ValueError, match="delta_order"):
        iv.cepstral_features(_dev(mel), off, delta_order=3)


# ================================================================================================ M-step and EM
def test_update_against_float64_with_a_starved_gaussian_and_a_floored_variance():
    iv = _iv()
    C, D = 37, 11
    rng = np.random.default_rng(8)
    w, mu, var = rng.dirichlet(np.ones(C)), rng.normal(0, 2, (C, D)), rng.uniform(0.5, 2, (C, D))
    N = rng.uniform(20, 400, C)
    m_new = rng.normal(0, 2, (C, D))
    acc = np.concatenate([N[:, None], N[:, None] * m_new, N[:, None] * (m_new ** 2 + rng.uniform(0.3, 2, (C, D)))], axis=1)
    acc[4] = 0.0                                                             # starved: N_c = 0
    acc[9, 0], acc[9, 1:] = 3.0, 3.0 * acc[9, 1:] / N[9]                     # starved: below min_count
    acc[20, 1 + D:] = acc[20, 0] * (m_new[20] ** 2 + 1e-5)                   # variance below the floor
    acc[21, 1 + D + 2] = acc[21, 0] * m_new[21, 2] ** 2                      # one dimension exactly at S / N = mu^2
    ubm = iv.DiagUbm(_dev(w), _dev(mu), _dev(var))
    A0 = ubm.A.cpu().numpy()
    for got, want in zip((A0, ubm.B.cpu().numpy(), ubm.g.cpu().numpy()), R.planes(w, mu, var)):
        _within_one_ulp(got, want)
    ubm.update(_dev(acc), var_floor=1e-3, min_count=10.0, min_weight=1e-5)
    wn, mn, vn = R.update(acc, w, mu, var, 1e-3, 10.0, 1e-5)
    for name, got, want in (("w", ubm.w, wn), ("mu", ubm.mu, mn), ("var", ubm.var, vn)):
        got = got.cpu().numpy()
        err = float((np.abs(got - want) / np.abs(want)).max())
        print("update %s: rel err %.3e (bar 1e-12)" % (name, err))
        assert err <= 1e-12
    assert np.array_equal(ubm.mu.cpu().numpy()[[4, 9]], mu[[4, 9]]) and np.array_equal(ubm.var.cpu().numpy()[[4, 9]], var[[4, 9]])
    assert np.all(ubm.var.cpu().numpy()[20] == 1e-3) and ubm.var.cpu().numpy()[21, 2] == 1e-3 and abs(float(ubm.w.sum()) - 1.0) < 1e-14
    for got, want in zip((ubm.A.cpu().numpy(), ubm.B.cpu().numpy(), ubm.g.cpu().numpy()), R.planes(wn, mn, vn)):
        _within_one_ulp(got, want)


def _within_one_ulp(got, want):
    """got (float32) equals the float32 rounding of want (float64) up to one unit in the last place."""
    r = want.astype(np.float32)
    assert got.dtype == np.float32 and np.all((got == r) | (got == np.nextafter(r, np.float32(np.inf))) | (got == np.nextafter(r, np.float32(-np.inf))))


def test_exact_em_follows_the_float64_history():
    iv, s = _iv(), R.EM_SHAPE
    X, w, mu, var = R.em_case()
    href, _, mref, _ = R.em_fit(X, w, mu, var, s["iters"], s["var_floor"], s["min_count"], s["min_weight"])
    ubm = iv.DiagUbm(_dev(w), _dev(mu), _dev(var))
    lines = []
    hist = np.asarray(ubm.fit(_dev(X), iters=s["iters"], nsel=s["C"], var_floor=s["var_floor"], min_count=s["min_count"], min_weight=s["min_weight"],
                              log=lines.append))
    d_hist, d_mu = float(np.abs(hist - href).max()), float(np.abs(ubm.mu.cpu().numpy() - mref).max())
    print("EM history", hist.tolist(), "reference", href.tolist())
    print("EM: |history - reference| %.3e (bar %.3e), |mu - reference| %.3e (bar %.3e)" % (d_hist, R.BAR_EM_HISTORY, d_mu, R.BAR_EM_MEANS))
    assert len(lines) == s["iters"] and hist.dtype == np.float64
    assert np.all(np.diff(hist) >= -R.BAR_EM_HISTORY), "the mean log-likelihood fell by more than its own error bar"
    assert np.all(np.diff(href) > 0) and d_hist <= R.BAR_EM_HISTORY and d_mu <= R.BAR_EM_MEANS


def test_from_frames_and_state_round_trip_on_the_device(tmp_path):
    iv = _iv()
    X = _dev(R.em_case()[0])
    ubm = iv.DiagUbm.from_frames(X, 16, seed=3)
    rows = np.sort(np.random.default_rng(3).choice(X.shape[0], 16, replace=False))
    assert np.array_equal(ubm.mu.cpu().numpy(), X.cpu().numpy()[rows].astype(np.float64)) and len(set(rows.tolist())) == 16
    assert np.allclose(ubm.var.cpu().numpy(), X.cpu().numpy().astype(np.float64).var(axis=0)[None], rtol=1e-12) and np.all(ubm.w.cpu().numpy() == 1 / 16)
    ubm.em_step(X, nsel=16)
    path = str(tmp_path / "ubm.npz")
    ubm.save(path)
    back = iv.DiagUbm.load(path, device=DEV)
    assert all(torch.equal(a, b) for a, b in zip((ubm.w, ubm.mu, ubm.var, ubm.A, ubm.B, ubm.g), (back.w, back.mu, back.var, back.A, back.B, back.g)))


# ================================================================================================ the whole chain
def test_train_diag_ubm_and_bw_stats_end_to_end():
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    iv = _iv()
    rng = np.random.default_rng(21)
    lens = [16000, 9000, 24000, 12345, 400, 20000, 8000, 30000]               # 8 utterances; the fifth is too short for a window: no frame
    n_max = max(lens)
    y = np.full((len(lens), n_max), 7.0, dtype=np.float32)
    for i, n in enumerate(lens):
        t = np.arange(n) / 16000.0
        y[i, :n] = (0.2 * np.sin(2 * np.pi * (110 + 30 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    spans = [[(0, n)] for n in lens]
    res = iv.train_diag_ubm(TisvFrontEnd(device=DEV), _dev(y), torch.tensor(lens, dtype=torch.int32, device=DEV), spans=spans, num_gauss=32, iters=2, nsel=8,
                            min_count=2.0, log=None)
    ubm, X, off = res.ubm, res.features, res.utt_off
    frames = np.diff(off)
    assert len(off) == 9 and frames[4] == 0 and frames.sum() == X.shape[0] and X.shape[1] == 60 and (ubm.C, ubm.D) == (32, 60)
    assert len(res.history) == 2 and np.isfinite(res.history).all()
    assert torch.isfinite(X).all() and all(torch.isfinite(t).all() for t in (ubm.w, ubm.mu, ubm.var, ubm.A, ubm.B, ubm.g))
    assert abs(float(ubm.w.sum()) - 1.0) < 1e-12 and float(ubm.var.min()) >= 1e-3
    N, Fs = iv.bw_stats(ubm, X, off, nsel=8, min_post=0.025)
    assert N.shape == (8, 32) and Fs.shape == (8, 32, 60) and torch.isfinite(N).all() and torch.isfinite(Fs).all()
    rows = N.double().sum(dim=1).cpu().numpy()
    print("bw_stats: frames", frames.tolist(), "row sums", rows.tolist())
    assert rows[4] == 0.0 and not Fs[4].any()
    assert np.all(np.abs(rows - frames) <= 1e-4 * np.maximum(frames, 1))            # posteriors renormalised after pruning: each frame weighs 1
    with pytest.raises(RuntimeError, match="bw_stats.*free"):                       # the refusal names both figures before anything is allocated
        import spoofsv_amd.ops as ops
        real = ops.free_bytes
        ops.free_bytes = lambda device: 1000
        try:
            iv.bw_stats(ubm, X, off)
        finally:
            ops.free_bytes = real
