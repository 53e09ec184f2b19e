"""The i-vector groundwork, the parts that need no device: the float64 reference against literal loops, the new C-ABI entries and their
argument errors, and the host logic of spoofsv_amd.ivector (DCT / lifter table, pass planning of bw_stats, the state round trip, the
CPU-tensor errors)."""
import ctypes

import numpy as np
import pytest
import torch

import _ivector_ref as R
from spoofsv_amd import _lib, ivector

ENTRIES = (("ssv_ivec_features_workspace", 3), ("ssv_ivec_features", 14), ("ssv_gmm_frame_tile", 2), ("ssv_gmm_diag_gselect", 13),
           ("ssv_gmm_diag_stats", 13), ("ssv_gmm_stats_reduce", 5), ("ssv_gmm_diag_update", 13), ("ssv_gmm_diag_planes", 9))


# ================================================================================================ the reference against loops
@pytest.mark.parametrize("lens,w,order,W,use_dct", [
    ((7, 1, 0, 3), 2, 2, 4, True),          # T = 1 and T = 3 < 2 w; T = 7 > W: the window meets both edges and slides between them
    ((2, 9), 3, 2, 300, False),             # T < W everywhere: one mean per utterance; T = 2 < 2 w
    ((6,), 1, 1, 5, True),                  # odd W
    ((5, 4), 2, 0, 2, False)])
def test_feature_reference_is_the_literal_loops(lens, w, order, W, use_dct):
    rng = np.random.default_rng(sum(lens))
    off = 2 + np.concatenate([[0], np.cumsum(lens)])
    mel = rng.normal(0, 1, (int(off[-1]) + 1, 4))
    dct = R.dct_table(3, 4, 22) if use_dct else None
    got, want = R.features(mel, off, dct, w, order, W), R.features_loop(mel, off, dct, w, order, W)
    assert got.shape == want.shape == (len(mel), (3 if use_dct else 4) * (order + 1))
    live = np.zeros(len(mel), bool)
    live[off[0]:off[-1]] = True
    assert np.isnan(got[~live]).all() and np.isnan(want[~live]).all()          # frames in no utterance are not written
    assert np.abs(got[live] - want[live]).max() < 1e-13


def test_cmn_window_edges():
    assert [R.cmn_window(t, 10, 4) for t in (0, 1, 2, 5, 8, 9)] == [(0, 4), (0, 4), (0, 4), (3, 7), (6, 10), (6, 10)]
    assert [R.cmn_window(t, 3, 300) for t in range(3)] == [(0, 3)] * 3            # T < W: the whole utterance
    assert R.cmn_window(0, 1, 1) == (0, 1) and R.cmn_window(4, 9, 5) == (2, 7)  # odd W: lo = t - W // 2


def test_an_impulse_reproduces_the_coefficient_vectors():
    w, T, t0 = 3, 41, 20
    mel = np.zeros((T, 1))
    mel[t0, 0] = 1.0
    c1, c2 = R.delta_coeffs(w)
    assert len(c1) == 2 * w + 1 and len(c2) == 4 * w + 1 and abs(c1[w + 1] - 1.0 / 28.0) < 1e-17 and abs(c2.sum()) < 1e-17
    v = R._utt_rows(mel, w, 2, False, np.float64)
    # d_t = sum_j c_j s_{t+j}: the impulse at t0 shows c reversed around t0
    assert np.array_equal(v[t0 - w:t0 + w + 1, 1], c1[::-1]) and np.array_equal(v[t0 - 2 * w:t0 + 2 * w + 1, 2], c2[::-1])
    assert not v[:t0 - 2 * w, 1:].any() and not v[t0 + 2 * w + 1:, 1:].any()
    # at T = 1 every clamped index is the frame itself: the coefficients sum to zero
    one = R._utt_rows(np.array([[2.5]]), w, 2, False, np.float64)
    assert one[0, 0] == 2.5 and abs(one[0, 1]) < 1e-16 and abs(one[0, 2]) < 1e-16


def test_mixture_reference_is_consistent():
    X, w, mu, var = R.gmm_case(7, 12, 40, seed=2)
    A, B, g = R.planes(w, mu, var)
    L = R.loglik_direct(X, w, mu, var, chunk=7)
    X64 = X.astype(np.float64)
    assert np.abs(L - (X64 @ A.T + (X64 * X64) @ B.T + g)).max() < 1e-10
    loop = np.array([[np.log(w[c]) - 0.5 * sum((X64[f, d] - mu[c, d]) ** 2 / var[c, d] + np.log(2 * np.pi * var[c, d]) for d in range(7)) for c in range(12)]
                     for f in range(3)])
    assert np.abs(L[:3] - loop).max() < 1e-11
    assert np.array_equal(R.select(np.array([[1.0, 3.0, 3.0, 0.0, 3.0]]), 3), [[1, 2, 4]])            # equal values: ascending index
    p0, p, ll = R.posteriors_on(np.log(np.array([[0.6, 0.3, 0.08, 0.02]])), 0.05)
    assert np.allclose(p0, [[0.6, 0.3, 0.08, 0.02]]) and np.allclose(p, [[0.6 / 0.98, 0.3 / 0.98, 0.08 / 0.98, 0.0]]) and abs(ll[0]) < 1e-15
    # statistics: the dense product against a literal loop, with entries outside [0, C) skipped and a repeated index adding
    idx = R.select(L, 4)
    post = R.posteriors_on(np.take_along_axis(L, idx, 1))[1]
    idx[0, 1], idx[1, 0], idx[2, 3] = -1, 12, idx[2, 0]
    seg = np.array([0, 0, 1, 17, 40])
    for order in (1, 2):
        want = np.zeros((4, 12, 1 + order * 7))
        for s in range(4):
            for f in range(seg[s], seg[s + 1]):
                for j in range(4):
                    if 0 <= idx[f, j] < 12:
                        want[s, idx[f, j]] += post[f, j] * np.concatenate([[1.0], X64[f]] + ([X64[f] ** 2] if order == 2 else []))
        assert np.abs(R.stats(X, idx, post, seg, 12, order) - want).max() < 1e-12
        assert np.abs(R.stats(X, idx, post, seg, 12, order, dtype=np.float32) - want).max() < 1e-3
    # M-step: a starved Gaussian keeps its parameters and a floored weight, a variance below the floor is raised to it
    acc = R.stats(X, idx, post, np.array([0, 40]), 12, 2)[0]
    big = int(acc[:, 0].argmax())
    dead = (big + 1) % 12
    acc[dead] = 0.0
    acc[big, 1 + 7:] = acc[big, 0] * (acc[big, 1:8] / acc[big, 0]) ** 2
    wn, m, v = R.update(acc, w, mu, var, 1e-3, 1e-9, 1e-5)
    assert abs(wn.sum() - 1) < 1e-15 and np.array_equal(m[dead], mu[dead]) and np.array_equal(v[dead], var[dead])
    assert abs(wn[dead] - 1e-5 / (1 + 1e-5)) < 1e-17 and abs(wn[big] - acc[big, 0] / acc[:, 0].sum() / (1 + 1e-5)) < 1e-15
    assert np.all(v[big] == 1e-3) and np.allclose(m[big], acc[big, 1:8] / acc[big, 0], rtol=1e-15)
    # numpy adds the rows of a (S, n) float32 array in ascending s when asked for a float64 sum over axis 0
    slab = np.random.default_rng(0).normal(0, 1, (37, 501)).astype(np.float32)
    seq = np.zeros(501)
    for s in range(37):
        seq += slab[s].astype(np.float64)
    assert np.array_equal(np.sum(slab, axis=0, dtype=np.float64), seq)


def test_exact_em_of_the_reference_never_loses_likelihood():
    s = R.EM_SHAPE
    X, w, mu, var = R.em_case()
    hist, wn, m, v = R.em_fit(X[:1500], w, mu, var, 4, s["var_floor"], s["min_count"], s["min_weight"])
    assert np.all(np.diff(hist) > 0) and abs(wn.sum() - 1) < 1e-14 and np.isfinite(m).all() and np.all(v >= s["var_floor"])


def test_recorded_bars_hold_against_a_fresh_measurement():
    """The recorded float32 errors were measured with one BLAS; another may block differently, so the fresh figure must lie within a
    factor 4 of the recorded one -- that is, under the bar the device tests use -- not equal it."""
    fresh = {("loglik",) + sh[:3]: R.measure_loglik(*sh) for sh in R.LOG_SHAPES[1:]}      # (the 60 / 1024 shape: the GPU module's time, not this one's)
    fresh[("stats",) + R.STATS_SHAPES[0][:3]] = R.measure_stats(*R.STATS_SHAPES[0])
    for key, val in fresh.items():
        rec = (R.MEASURED_LOGLIK if key[0] == "loglik" else R.MEASURED_STATS)[key[1:]]
        assert rec / 4 <= val <= 4 * rec, (key, val, rec)
    h, m = R.measure_em()
    assert R.MEASURED_EM_HISTORY / 4 <= h <= R.BAR_EM_HISTORY and R.MEASURED_EM_MEANS / 4 <= m <= R.BAR_EM_MEANS
    assert 1e-8 < R.MEASURED_FEATURES < 4e-6 and all(5e-8 < v < 2e-6 for v in list(R.MEASURED_LOGLIK.values()) + list(R.MEASURED_STATS.values()))


# ================================================================================================ the C ABI
def test_ivector_entries_are_declared_and_exported():
    L = _lib.lib()
    protos = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name, nargs in ENTRIES:
        assert name in protos and hasattr(raw, name), name
        assert len(protos[name][1]) == nargs, (name, protos[name][2])
    assert L.ssv_version() == 7
    assert L.ssv_gmm_frame_tile(60, 1024) in (16, 32) and L.ssv_gmm_frame_tile(128, 2048) in (16, 32) and L.ssv_gmm_frame_tile(1, 1) in (16, 32)
    assert L.ssv_ivec_features_workspace(1000, 20, 2) >= 1000 * 60 * 4


def _sweep(entry, tag, good, cases, order):
    L = _lib.lib()
    for key, bad, want in cases:
        a = dict(good, **{key: bad})
        rc = entry(*[a[k] for k in order])
        assert rc == want and tag in L.ssv_last_error(), (tag, key, bad, rc, L.ssv_last_error())


def test_bad_ivector_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # `one`: non-null, 16-byte aligned, never dereferenced: the checks come first
    # ---- features
    good = dict(mel=one, off=one, dct=one, out=one, G=100, M=40, U=3, Cc=20, w=3, order=2, W=300, ws=one, wsb=1 << 20, st=null)
    order = ("mel", "off", "dct", "out", "G", "M", "U", "Cc", "w", "order", "W", "ws", "wsb", "st")
    _sweep(L.ssv_ivec_features, b"ivec_features", good,
           [("mel", null, -1), ("off", null, -1), ("out", null, -1), ("ws", null, -1), ("G", 0, -1), ("G", -5, -1), ("M", 0, -1), ("U", 0, -1), ("Cc", 0, -1),
            ("w", 0, -1), ("order", 3, -1), ("order", -1, -1), ("W", 0, -1), ("wsb", 100, -1), ("dct", null, -1),       # no table: Cc must equal M
            ("Cc", 129, -2), ("w", 9, -2)], order)
    assert L.ssv_ivec_features_workspace(0, 20, 2) == 0 and L.ssv_ivec_features_workspace(10, 20, 3) == 0
    # ---- frame tile
    for D, C, want in ((0, 10, -1), (10, 0, -1), (-1, 10, -1), (129, 10, -2), (10, 2049, -2)):
        assert L.ssv_gmm_frame_tile(D, C) == want and b"gmm_frame_tile" in L.ssv_last_error()
    # ---- selection
    good = dict(X=one, A=one, B=one, g=one, idx=one, post=one, ll=one, F=10, D=60, C=1024, nsel=20, mp=0.025, st=null)
    order = ("X", "A", "B", "g", "idx", "post", "ll", "F", "D", "C", "nsel", "mp", "st")
    _sweep(L.ssv_gmm_diag_gselect, b"gmm_diag_gselect", good,
           [(k, null, -1) for k in ("X", "A", "B", "g", "idx", "post", "ll")] +
           [("F", 0, -1), ("F", -1, -1), ("D", 0, -1), ("C", 0, -1), ("nsel", 0, -1), ("nsel", 1025, -1), ("mp", -0.1, -1), ("mp", 1.0, -1),
            ("A", ctypes.c_void_p(4100), -1),                                                       # D % 4 == 0: the planes must be 16-byte aligned
            ("nsel", 33, -2), ("D", 129, -2), ("C", 2049, -2)], order)
    assert L.ssv_gmm_diag_gselect(one, one, one, one, one, one, one, 10, 60, 16, 17, 0.0, null) == -1     # nsel > C
    # ---- statistics
    asc = (ctypes.c_long * 4)(0, 3, 3, 10)
    good = dict(X=one, idx=one, post=one, off=one, host=asc, slab=one, F=10, D=60, C=1024, nsel=20, S=3, order=2, st=null)
    order = ("X", "idx", "post", "off", "host", "slab", "F", "D", "C", "nsel", "S", "order", "st")
    _sweep(L.ssv_gmm_diag_stats, b"gmm_diag_stats", good,
           [(k, null, -1) for k in ("X", "idx", "post", "off", "slab")] +
           [("F", 0, -1), ("D", 0, -1), ("C", 0, -1), ("nsel", 0, -1), ("nsel", 1025, -1), ("S", 0, -1), ("order", 0, -1), ("order", 3, -1),
            ("host", (ctypes.c_long * 4)(0, 5, 3, 10), -1),                                         # descending
            ("host", (ctypes.c_long * 4)(-1, 3, 3, 10), -1), ("host", (ctypes.c_long * 4)(0, 3, 3, 11), -1),      # outside [0, F]
            ("nsel", 33, -2), ("D", 129, -2), ("C", 2049, -2)], order)
    # ---- reduce
    good = dict(slab=one, out=one, S=4, n=100, st=null)
    _sweep(L.ssv_gmm_stats_reduce, b"gmm_stats_reduce", good, [("slab", null, -1), ("out", null, -1), ("S", 0, -1), ("n", 0, -1), ("n", -2, -1)],
           ("slab", "out", "S", "n", "st"))
    # ---- M-step and planes
    good = dict(stats=one, w=one, mu=one, var=one, A=one, B=one, g=one, C=16, D=5, vf=1e-3, mc=10.0, mw=1e-5, st=null)
    order = ("stats", "w", "mu", "var", "A", "B", "g", "C", "D", "vf", "mc", "mw", "st")
    _sweep(L.ssv_gmm_diag_update, b"gmm_diag_update", good,
           [(k, null, -1) for k in ("stats", "w", "mu", "var", "A", "B", "g")] +
           [("C", 0, -1), ("D", 0, -1), ("vf", 0.0, -1), ("vf", -1.0, -1), ("mc", -1.0, -1), ("mw", 0.0, -1), ("mw", 1.0, -1), ("C", 2049, -2), ("D", 129, -2)], order)
    good = dict(w=one, mu=one, var=one, A=one, B=one, g=one, C=16, D=5, st=null)
    _sweep(L.ssv_gmm_diag_planes, b"gmm_diag_planes", good,
           [(k, null, -1) for k in ("w", "mu", "var", "A", "B", "g")] + [("C", 0, -1), ("D", -1, -1), ("C", 2049, -2), ("D", 129, -2)],
           ("w", "mu", "var", "A", "B", "g", "C", "D", "st"))


# ================================================================================================ host logic
@pytest.mark.parametrize("n_ceps,n_mels,lifter", [(20, 40, 22), (13, 23, 22), (5, 5, 0), (1, 8, 22)])
def test_dct_lifter_table_against_the_closed_form(n_ceps, n_mels, lifter):
    got, want = ivector.dct_table(n_ceps, n_mels, lifter), R.dct_table(n_ceps, n_mels, lifter)
    assert got.dtype == np.float32 and got.shape == (n_ceps, n_mels)
    assert np.abs(got - want).max() <= 2.0 ** -24 * np.abs(want).max()          # rounded once from double
    if lifter == 0:                                                              # orthonormal rows
        assert np.abs(want @ want.T - np.eye(n_ceps)).max() < 1e-14
    with pytest.raises(ValueError, match="dct_table"):
        ivector.dct_table(n_mels + 1, n_mels, lifter)


def test_pass_planning_of_bw_stats():
    C, D, nsel = 1024, 60, 20
    row, per_frame = C * (1 + D) * 4, nsel * 8 + 4
    n = [300, 0, 1000, 250, 250, 4000, 10]
    cost = [f * per_frame + row for f in n]
    passes, need = ivector.plan_bw_passes(n, C, D, nsel, free=10 ** 12)
    assert passes == [(0, len(n))] and need == len(n) * row + 2 * max(cost)
    free = len(n) * row + 2 * (cost[0] + cost[1] + cost[2])                      # half of the rest holds exactly the first three
    passes, need2 = ivector.plan_bw_passes(n, C, D, nsel, free)
    assert need2 == need and passes[0] == (0, 3)
    assert [a for a, _ in passes[1:]] == [b for _, b in passes[:-1]] and passes[-1][1] == len(n)         # contiguous, complete
    assert all(sum(cost[a:b]) <= (free - len(n) * row) // 2 or b - a == 1 for a, b in passes)
    passes, _ = ivector.plan_bw_passes(n, C, D, nsel, free=0)                    # below `need` (the caller refuses): no pass above the costliest utterance
    assert (5, 6) in passes and all(sum(cost[a:b]) <= max(cost) for a, b in passes) and passes[-1][1] == len(n)
    with pytest.raises(ValueError, match="plan_bw_passes"):
        ivector.plan_bw_passes([], C, D, nsel, 1)
    with pytest.raises(ValueError, match="plan_bw_passes"):
        ivector.plan_bw_passes([3, -1], C, D, nsel, 1)


def test_frames_per_utterance_of_a_plan():
    from spoofsv_amd import dvector
    pl = dvector.plan([[(0, 16000)], [(0, 100)], [(0, 8000), (8000, 20000)]], hop=160)
    n = ivector.frames_per_utterance(pl, 3)
    assert n[1] == 0 and n.sum() == pl.n_frames and n[0] == dvector.frames_of(16000, 160)


def test_state_round_trip_on_the_host(tmp_path):
    rng = np.random.default_rng(1)
    w, mu, var = rng.dirichlet(np.ones(6)), rng.normal(0, 1, (6, 4)), rng.uniform(0.5, 2, (6, 4))
    ubm = ivector.DiagUbm(*(torch.from_numpy(a) for a in (w, mu, var)))
    path = str(tmp_path / "ubm.npz")
    ubm.save(path)
    back = ivector.DiagUbm.load(path, device="cpu")
    for a, b in ((back.w, w), (back.mu, mu), (back.var, var)):
        assert a.dtype == torch.float64 and np.array_equal(a.numpy(), b)
    other = ivector.DiagUbm(torch.full((6,), 1 / 6, dtype=torch.float64), torch.zeros(6, 4, dtype=torch.float64), torch.ones(6, 4, dtype=torch.float64))
    other.load_state_dict(back.state_dict())
    assert all(np.array_equal(other.state_dict()[k].numpy(), back.state_dict()[k].numpy()) for k in ("w", "mu", "var")) and (other.C, other.D) == (6, 4)
    for bad in ((torch.ones(6), torch.zeros(6, 4), torch.ones(6, 4)),                                              # float32
                (torch.ones(5, dtype=torch.float64), torch.zeros(6, 4, dtype=torch.float64), torch.ones(6, 4, dtype=torch.float64))):
        with pytest.raises(ValueError, match="DiagUbm"):
            ivector.DiagUbm(*bad)


def test_cpu_tensors_are_a_loud_error_and_bad_arguments_name_themselves():
    ubm = ivector.DiagUbm(torch.full((4,), 0.25, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64))
    X = torch.zeros(10, 3)
    for call in (lambda: ubm.posteriors(X), lambda: ubm.stats(X, [0, 10], 1), lambda: ubm.em_step(X), lambda: ubm.planes(),
                 lambda: ivector.DiagUbm.from_frames(X, 2), lambda: ivector.bw_stats(ubm, X, [0, 10]),
                 lambda: ivector.cepstral_features(torch.zeros(10, 40), [0, 10]), lambda: ivector.DiagUbm.reduce(torch.zeros(2, 3))):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()
    with pytest.raises(ValueError, match="mel"):
        ivector.cepstral_features(np.zeros((10, 40), np.float32), [0, 10])
    with pytest.raises(ValueError, match="X"):
        ubm.posteriors([[0.0, 0.0, 0.0]])
