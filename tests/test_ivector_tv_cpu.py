"""The i-vector extractor, the parts that need no device: the float64 restatement against literal loops, exact EM never losing
objective, the packed triangle, the new C-ABI entries and their argument errors, the pass planners, the state round trip, the CPU-tensor
errors, the recorded bars against a fresh measurement, and the host trial logic against the reference's two scripts."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _ivector_tv_ref as R
from spoofsv_amd import _lib, ge2e_harness, ivector

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRIES = (("ssv_ivec_tv_planes", 8), ("ssv_ivec_centre_stats", 8), ("ssv_ivec_product_run", 0), ("ssv_ivec_product_tile", 0), ("ssv_ivec_product", 7),
           ("ssv_ivec_product_tn", 7), ("ssv_ivec_estep", 8), ("ssv_ivec_tv_update", 10), ("ssv_ivec_cosine_trials", 10))


# ================================================================================================ the reference against loops
def test_restatement_is_the_literal_loops():
    C, D, Rk, U = 3, 2, 4, 5
    N, F, _, mu, var, T, _ = R.stats_case(C, D, Rk, U, seed=1, starved=2, empty=1)
    Ft = R.centre(N, F, mu)
    loop = np.array([[[float(F[u, c, d]) - float(N[u, c]) * mu[c, d] for d in range(D)] for c in range(C)] for u in range(U)])
    assert np.abs(Ft - loop).max() < 1e-12
    w, obj, M, scale, Lp, b = R.estep(N, Ft, T, var)
    wl, ol, Ml = R.estep_loop(N, Ft, T, var)
    assert np.abs(w - wl).max() < 1e-11 and np.abs(obj - ol).max() < 1e-10 and np.abs(R.tri_unpack(M) - Ml).max() < 1e-11
    assert np.all(scale >= np.abs(obj)) and not w[1].any() and obj[1] == 0 and np.array_equal(R.tri_unpack(M[1]), np.eye(Rk))      # the empty utterance
    w2, obj2, M2, _ = R.estep_from(Lp, b)
    assert np.array_equal(w2, w) and np.array_equal(obj2, obj) and np.array_equal(M2, M)
    A, Cm, Nc, Msum = R.accumulate(N, Ft, w, M)
    J = R.min_div_factor(Msum, U)
    assert np.abs(J @ J.T - Ml.mean(0)).max() < 1e-12 and np.all(np.triu(J, 1) == 0)
    for Jm in (None, J):
        got, want = R.mstep(A, Cm, Nc, T, Jm, 1.0), R.mstep_loop(N, Ft, w, Ml, T, Jm, 1.0)
        assert np.abs(got - want).max() < 1e-9 * np.abs(want).max()
        assert np.array_equal(got[2], T[2]) and not np.array_equal(got[0], T[0])              # the starved Gaussian keeps its bits, J or not
    # the float32 form differs from float64 and stays near it
    w32 = R.estep(N, Ft, T, var, float32=True)[0]
    assert 0 < np.abs(w32 - w).max() < 1e-3


@pytest.mark.parametrize("min_div", [True, False])
def test_exact_em_of_the_reference_never_loses_objective(min_div):
    s = R.MONOTONE_SHAPE
    N, Ft, T0, var = R.em_case(s)
    assert not N[:, s["C"] - 1].any() and not N[3].any() and N[5].sum() > 4000
    hist, T = R.em_fit(N, Ft, T0, var, s["iters"], min_div, s["min_count"])
    assert len(hist) == 6 and np.all(np.diff(hist) >= 0), hist
    assert np.array_equal(T[-1], T0[-1]) and np.isfinite(T).all()


def test_packing_and_unpacking_of_the_triangle():
    for n in (1, 2, 5, 17):
        S = np.random.default_rng(n).normal(0, 1, (3, n, n))
        S = S + S.transpose(0, 2, 1)
        p = ivector.tri_pack(S)
        assert p.shape == (3, ivector.tri_size(n)) and np.array_equal(ivector.tri_unpack(p), S) and np.array_equal(p, R.tri_pack(S))
        for i in range(n):
            for j in range(i + 1):
                assert p[1, i * (i + 1) // 2 + j] == S[1, i, j]
    with pytest.raises(ValueError, match="tri_unpack"):
        ivector.tri_unpack(np.zeros(7))
    with pytest.raises(ValueError, match="tri_unpack"):
        ivector.tri_unpack(np.zeros(6), R=4)


def test_recorded_bars_hold_against_a_fresh_measurement():
    """The recorded float32 errors were measured with one BLAS; another may block differently, so the fresh figure must lie within a
    factor 4 of the recorded one, not equal it."""
    fresh = [(("product",) + sh, R.measure_product(*sh), R.MEASURED_PRODUCT[sh]) for sh in R.PRODUCT_SHAPES]
    fresh += [(("product_tn",) + sh, R.measure_product(*sh, tn=True), R.MEASURED_PRODUCT_TN[sh]) for sh in R.PRODUCT_TN_SHAPES]
    for Rk in R.ESTEP_RANKS:
        ew, eM, eo = R.measure_estep(Rk)
        fresh += [(("estep w", Rk), ew, R.MEASURED_ESTEP_W[Rk]), (("estep M", Rk), eM, R.MEASURED_ESTEP_M[Rk]), (("estep obj", Rk), eo, R.MEASURED_ESTEP_OBJ[Rk])]
    h, t = R.measure_em()
    fresh += [("em history", h, R.MEASURED_EM_HISTORY), ("em T", t, R.MEASURED_EM_T), ("cosine", R.measure_cosine(), R.MEASURED_COSINE)]
    for key, val, rec in fresh:
        assert rec / 4 <= val <= 4 * rec, (key, val, rec)
    assert all(2e-8 < v < 1e-6 for v in list(R.MEASURED_PRODUCT.values()) + list(R.MEASURED_PRODUCT_TN.values()))
    assert R.RUN + 1 in [sh[2] for sh in R.PRODUCT_SHAPES] and 1 in [sh[2] for sh in R.PRODUCT_SHAPES]


# ================================================================================================ the C ABI
def test_extractor_entries_are_declared_and_exported():
    L = _lib.lib()
    protos = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name, nargs in ENTRIES:
        assert name in protos and hasattr(raw, name), name
        assert len(protos[name][1]) == nargs, (name, protos[name][2])
    assert L.ssv_version() == 7 and L.ssv_ivec_product_run() == R.RUN and L.ssv_ivec_product_tile() == R.TILE


def _sweep(entry, tag, good, cases, order):
    L = _lib.lib()
    assert set(good) == set(order)
    for key, bad, want in cases:
        a = dict(good, **{key: bad})
        rc = entry(*[a[k] for k in order])
        assert rc == want and tag in L.ssv_last_error(), (tag, key, bad, rc, L.ssv_last_error())


def test_bad_extractor_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # `one`: non-null, never dereferenced: the checks come first
    good = dict(T=one, var=one, G=one, Pk=one, C=16, D=5, R=17, st=null)
    _sweep(L.ssv_ivec_tv_planes, b"ivec_tv_planes", good,
           [(k, null, -1) for k in ("T", "var", "G", "Pk")] + [("C", 0, -1), ("D", 0, -1), ("R", 0, -1), ("R", -3, -1), ("R", 193, -2), ("C", 2049, -2), ("D", 129, -2)],
           ("T", "var", "G", "Pk", "C", "D", "R", "st"))
    good = dict(N=one, F=one, mu=one, Ft=one, U=4, C=16, D=5, st=null)
    _sweep(L.ssv_ivec_centre_stats, b"ivec_centre_stats", good,
           [(k, null, -1) for k in ("N", "F", "mu", "Ft")] + [("U", 0, -1), ("C", 0, -1), ("D", 0, -1), ("C", 2049, -2), ("D", 129, -2)],
           ("N", "F", "mu", "Ft", "U", "C", "D", "st"))
    good = dict(A=one, B=one, out=one, m=5, n=6, K=7, st=null)
    _sweep(L.ssv_ivec_product, b"ivec_product", good, [(k, null, -1) for k in ("A", "B", "out")] + [("m", 0, -1), ("n", 0, -1), ("K", 0, -1), ("m", 65536 * 64, -2)],
           ("A", "B", "out", "m", "n", "K", "st"))
    good = dict(A=one, B=one, acc=one, U=5, m=6, n=7, st=null)
    _sweep(L.ssv_ivec_product_tn, b"ivec_product_tn", good, [(k, null, -1) for k in ("A", "B", "acc")] + [("U", 0, -1), ("m", 0, -1), ("n", -1, -1), ("m", 65536 * 64, -2)],
           ("A", "B", "acc", "U", "m", "n", "st"))
    good = dict(Lp=one, b=one, w=one, M=one, obj=one, U=3, R=17, st=null)
    _sweep(L.ssv_ivec_estep, b"ivec_estep", good,
           [(k, null, -1) for k in ("Lp", "b", "w", "obj")] + [("U", 0, -1), ("R", 0, -1), ("R", 193, -2), ("U", 1 << 31, -2)],
           ("Lp", "b", "w", "M", "obj", "U", "R", "st"))
    good = dict(A=one, Cm=one, Nc=one, J=one, T=one, C=16, D=5, R=17, mc=10.0, st=null)
    _sweep(L.ssv_ivec_tv_update, b"ivec_tv_update", good,
           [(k, null, -1) for k in ("A", "Cm", "Nc", "T")] + [("C", 0, -1), ("D", 0, -1), ("R", 0, -1), ("mc", -1.0, -1), ("R", 193, -2), ("C", 2049, -2), ("D", 129, -2)],
           ("A", "Cm", "Nc", "J", "T", "C", "D", "R", "mc", "st"))
    asc = (ctypes.c_long * 4)(0, 3, 3, 10)
    good = dict(en=one, off=one, host=asc, ev=one, sc=one, n=10, S=3, E=5, R=17, st=null)
    _sweep(L.ssv_ivec_cosine_trials, b"ivec_cosine_trials", good,
           [(k, null, -1) for k in ("en", "off", "ev", "sc")] + [("n", 0, -1), ("S", 0, -1), ("E", 0, -1), ("R", 0, -1),
            ("host", (ctypes.c_long * 4)(0, 5, 3, 10), -1),                                          # descending
            ("host", (ctypes.c_long * 4)(-1, 3, 3, 10), -1), ("host", (ctypes.c_long * 4)(0, 3, 3, 11), -1),       # outside [0, n_enroll]
            ("R", 193, -2)], ("en", "off", "host", "ev", "sc", "n", "S", "E", "R", "st"))
    assert L.ssv_ivec_cosine_trials(one, one, None, one, one, 10, 1000, 5, 192, null) == -2 and b"LDS" in L.ssv_last_error()        # 1000 models of rank 192


# ================================================================================================ host logic
def test_pass_planning_of_the_extractor():
    C, D, Rk = 1024, 60, 192
    P = Rk * (Rk + 1) // 2
    fixed = (C * P + C * D * Rk + C + P) * 8
    per = 2 * P * 4 + Rk * 8 + 8 + 4
    passes, need = ivector.plan_tv_passes(2000, C, D, Rk, 10 ** 13, True)
    assert passes == [(0, 2000)] and need == fixed + per
    passes, need2 = ivector.plan_tv_passes(2000, C, D, Rk, fixed + 2 * 300 * per, True)          # half of the rest holds exactly 300
    assert need2 == need and passes[0] == (0, 300) and passes[-1] == (1800, 2000) and [a for a, _ in passes[1:]] == [b for _, b in passes[:-1]]
    passes, _ = ivector.plan_tv_passes(5, C, D, Rk, 0, True)                                      # below `need` (the caller refuses): one by one
    assert passes == [(u, u + 1) for u in range(5)]
    passes, need = ivector.plan_tv_passes(7, C, D, Rk, 10 ** 12, False)
    assert passes == [(0, 7)] and need == 7 * Rk * 4 + P * 4 + Rk * 8 + 8
    with pytest.raises(ValueError, match="plan_tv_passes"):
        ivector.plan_tv_passes(0, C, D, Rk, 1, True)
    # extraction from frames
    n, nsel = [300, 0, 1000, 250, 250, 4000, 10], 20
    row = 2 * C * (1 + D) * 4 + P * 4 + Rk * 4 + 8
    cost = [f * (nsel * 8 + 4) + row for f in n]
    out = len(n) * Rk * 4
    passes, need = ivector.plan_extract_passes(n, C, D, Rk, nsel, 10 ** 12)
    assert passes == [(0, len(n))] and need == out + 2 * max(cost)
    passes, _ = ivector.plan_extract_passes(n, C, D, Rk, nsel, out + 2 * sum(cost[:3]))
    assert passes[0] == (0, 3) and passes[-1][1] == len(n) and [a for a, _ in passes[1:]] == [b for _, b in passes[:-1]]
    passes, _ = ivector.plan_extract_passes(n, C, D, Rk, nsel, need)                               # exactly `need`: no pass above the costliest utterance
    assert (5, 6) in passes and all(sum(cost[a:b]) <= max(cost) for a, b in passes) and passes[-1][1] == len(n)
    m = [300, 310, 0, 290]                                                                         # lengths alike: then no two utterances share a pass
    assert ivector.plan_extract_passes(m, C, D, Rk, nsel, ivector.plan_extract_passes(m, C, D, Rk, nsel, 0)[1])[0] == [(u, u + 1) for u in range(4)]
    with pytest.raises(ValueError, match="plan_extract_passes"):
        ivector.plan_extract_passes([3, -1], C, D, Rk, nsel, 1)


def _host_tv(C=6, D=4, Rk=3, seed=1):
    rng = np.random.default_rng(seed)
    w, mu, var = R.ubm_case(C, D, rng)
    return ivector.TotalVariability(*(torch.from_numpy(a) for a in (rng.normal(0, 1, (C, D, Rk)), w, mu, var)))


def test_state_round_trip_on_the_host(tmp_path):
    tv = _host_tv()
    path = str(tmp_path / "tv.npz")
    tv.save(path)
    back = ivector.TotalVariability.load(path, device="cpu")
    for k, v in tv.state_dict().items():
        assert back.state_dict()[k].dtype == torch.float64 and np.array_equal(back.state_dict()[k].numpy(), v.numpy())
    assert (back.C, back.D, back.R, back.P) == (6, 4, 3, 6)
    ubm = ivector.DiagUbm(tv.w, tv.mu, tv.var)
    a, b = ivector.TotalVariability.from_ubm(ubm, 5, seed=3), ivector.TotalVariability.from_ubm(ubm, 5, seed=3)
    assert np.array_equal(a.T.numpy(), b.T.numpy()) and np.array_equal(a.T.numpy(), R.init_T(tv.var.numpy(), 5, seed=3))
    with pytest.raises(ValueError, match="TotalVariability"):
        ivector.TotalVariability(tv.T.float(), tv.w, tv.mu, tv.var)
    with pytest.raises(ValueError, match="TotalVariability"):
        ivector.TotalVariability(torch.zeros(6, 4, 193, dtype=torch.float64), tv.w, tv.mu, tv.var)
    with pytest.raises(ValueError, match="from_ubm"):
        ivector.TotalVariability.from_ubm(ubm, 0)


def test_cpu_tensors_are_a_loud_error():
    tv = _host_tv()
    N, Ft = torch.zeros(5, 6), torch.zeros(5, 6, 4)
    for call in (lambda: tv.planes(), lambda: tv.estep(N, Ft), lambda: tv.em_step(N, Ft), lambda: tv.extract(N, Ft), lambda: ivector.centre_stats(tv, N, Ft),
                 lambda: ivector.product(torch.zeros(3, 4), torch.zeros(4, 2)), lambda: ivector.product_tn(torch.zeros(3, 4), torch.zeros(3, 2), torch.zeros(4, 2)),
                 lambda: ivector.cosine_trials(torch.zeros(4, 3), [0, 2, 4], torch.zeros(2, 3)), lambda: ivector.extract_ivectors(tv, torch.zeros(10, 4), [0, 10])):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()
    with pytest.raises(ValueError, match="N"):
        tv.estep(np.zeros((5, 6), np.float32), Ft)


def _lines(part):
    with open(os.path.join(GOLDEN, "ivector_trials_%s.txt" % part)) as f:
        return f.read().splitlines()


def test_host_trial_logic_is_the_reference_scripts(tmp_path):
    """tools/gen_ivector_trials_golden.py recorded what the reference's local/split_data_enroll_eval.py and local/produce_trials.py read and
    wrote."""
    utt2spk = _lines("utt2spk")
    enroll, ev = ivector.split_enroll_eval(utt2spk)
    assert enroll == _lines("enroll") and ev == _lines("eval") and len(enroll) + len(ev) == len(utt2spk)
    assert ivector.trial_list(ev) == _lines("trials")
    assert ivector.split_enroll_eval([l + "\n" for l in utt2spk], enroll_num=1)[0] == ["S07_001 S07", "S02_001 S02", "S11_004 S11", "S05_001 S05"]
    with pytest.raises(ValueError, match="split_enroll_eval"):
        ivector.split_enroll_eval(["lonely"])
    # the score file: utterance-major like the trial list, read back by the harness's parser
    speakers, utts = ["S07", "S02"], ["S07_004", "S02_030", "S07_031"]
    scores = np.array([[0.5, -0.25], [0.125, 0.75], [np.float32(1) / 3, 0.0]], dtype=np.float32)
    path = str(tmp_path / "scores.txt")
    ivector.write_trial_scores(path, speakers, utts, scores)
    rows = [l.split() for l in open(path).read().splitlines()]
    assert [(r[0], r[1]) for r in rows] == [(s, u) for u in utts for s in speakers]
    assert np.array_equal(np.array([np.float32(r[2]) for r in rows]).reshape(3, 2), scores)
    real, fake = ge2e_harness.parse_ivector_scores(path)
    assert np.array_equal(real, [0.5]) and np.array_equal(fake.astype(np.float32), np.array([0.75, np.float32(1) / 3], dtype=np.float32))      # 9 digits: the float32 survives
    with pytest.raises(ValueError, match="write_trial_scores"):
        ivector.write_trial_scores(path, speakers, utts[:2], scores)


def test_end_to_end_case_separates_speakers_in_the_reference():
    """What test_gpu_ivector_tv.py's whole chain relies on: on the generated data the float64 chain scores targets well above non-targets."""
    scores, target = R.e2e_reference()
    assert scores.shape == (24, 4) and target.sum() == 24
    assert scores[target].mean() - scores[~target].mean() > 0.5, (scores[target].mean(), scores[~target].mean())
