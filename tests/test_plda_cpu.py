"""CPU checks of the PLDA back end: the float64 restatement (tests/_plda_ref.py) against its own identities -- EM does not decrease the
objective, the score's product form equals its direct form, finalisation diagonalises -- the equal error rate walk, ivector_eer, the recorded
figures against a fresh measurement, and every new entry's refusal of bad arguments before the device."""
import ctypes

import numpy as np
import pytest

import _plda_ref as R


@pytest.mark.parametrize("shape", R.MONOTONE_SHAPES)
def test_reference_objective_does_not_decrease(shape):
    Rk, S = shape
    X, off = R.train_case(Rk, S)
    Xd, means, mu, counts = R.class_stats(X, off)
    hist, W, B = R.em_fit(R.scatter(Xd), means, mu, counts, 10)
    print("objective at %s: %s" % (shape, " ".join("%.6f" % h for h in hist)))
    assert hist.size == 11 and np.isfinite(hist).all() and (np.diff(hist) >= 0).all()
    # the conditioning the float64 bar's derivation assumes (BAR_F64)
    Winv, Binv = np.linalg.inv(W), np.linalg.inv(B)
    worst = max(np.linalg.cond(W), np.linalg.cond(B), max(np.linalg.cond(Binv + n * Winv) for n in np.unique(counts)))
    print("worst condition number %.1f" % worst)
    assert worst < 1e3


@pytest.mark.parametrize("Rk", R.SCORE_RANKS)
def test_product_form_equals_direct_form(Rk):
    t, y, n, psi = R.score_case(65, 17, Rk)
    H, k = R.planes(y, n, psi)
    err = float((np.abs(R.score_product(t, H, k) - R.score_direct(t, y, n, psi)) / np.maximum(R.term_scale(t, H, k), 1e-300)).max())
    assert err <= 1e-12, err
    assert (R.score_direct(t, y, n, psi)[:, n == 0] == 0).all() and (R.score_product(t, H, k)[:, n == 0] == 0).all()


@pytest.mark.parametrize("Rk", (1, 17, 64))
def test_finalize_diagonalises(Rk):
    from spoofsv_amd.plda import finalize_host
    _, W, B = R.model_case(Rk)
    for A, psi in (R.finalize(W, B), finalize_host(W, B)):
        assert np.abs(A @ W @ A.T - np.eye(Rk)).max() <= 1e-9
        assert np.abs(A @ B @ A.T - np.diag(psi)).max() <= 1e-9 * max(1.0, psi.max())
        assert (np.diff(psi) <= 0).all() and (psi >= 0).all()
        assert (A[np.arange(Rk), np.abs(A).argmax(1)] > 0).all()
    assert np.array_equal(R.finalize(W, B)[0], finalize_host(W, B)[0])


def test_compute_eer():
    from spoofsv_amd.plda import compute_eer
    for f in (compute_eer, R.compute_eer):
        assert f([1, 2, 3, 4], [0, 0.5, 2.5, 3.5]) == (0.5, 3.0)          # the case worked by hand
        assert f([4, 2, 1, 3], [3.5, 0, 2.5, 0.5]) == (0.5, 3.0)          # order does not matter
        assert f([1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]) == (0.75, 1.0)   # ties: non[q] < target[p] never holds, the walk ends at the last target
        assert f([2.0, 2.0], [1.0, 3.0]) == (0.5, 2.0)
        assert f([5.0], [1.0, 9.0]) == (0.0, 5.0)                          # one target: no step is taken
        assert f([0.0, 10.0, 11.0], [-1.0, -2.0]) == (0.0, 0.0)            # separable
        for bad in (([], [1.0]), ([1.0], []), ([], [])):
            with pytest.raises(ValueError):
                f(*bad)
    rng = np.random.default_rng(0)
    for _ in range(20):
        t, non = rng.normal(1, 1, rng.integers(1, 30)), rng.normal(0, 1, rng.integers(1, 40))
        assert compute_eer(t, non) == R.compute_eer(t, non)


def test_ivector_eer_pairs_lines_in_order(tmp_path):
    from spoofsv_amd.ge2e_harness import ivector_eer
    trials = ["u1 A target", "u1 B nontarget", "u2 A nontarget", "u2 B target", "u3 A target", "u3 B nontarget", "u4 A nontarget", "u4 B target"]
    scores = [1, 0, 0.5, 2, 3, 2.5, 3.5, 4]
    path = tmp_path / "s.score"
    path.write_text("".join("%s %s %.9g\n" % (tr.split()[1], tr.split()[0], sc) for tr, sc in zip(trials, scores)))
    assert ivector_eer(str(path), trials) == (0.5, 3.0)
    with pytest.raises(ValueError):
        ivector_eer(str(path), trials[:-1])
    with pytest.raises(ValueError):
        ivector_eer(str(path), trials[:-1] + ["u4 B maybe"])


def _within(fresh, recorded):
    return recorded / 4.0 <= fresh <= recorded * 4.0 or fresh == recorded


def test_recorded_figures_against_a_fresh_measurement():
    for Rk in R.SCORE_RANKS:
        assert _within(R.measure_score(Rk), R.MEASURED_SCORE[Rk]), Rk
    for Rk in R.TRANSFORM_RANKS:
        fresh = R.measure_transform(Rk)
        assert _within(fresh[0], R.MEASURED_TRANSFORM[Rk][0]) and _within(fresh[1], R.MEASURED_TRANSFORM[Rk][1]), (Rk, fresh)
    for Rk in R.STATS_RANKS:
        assert _within(R.measure_scatter(Rk), R.MEASURED_SCATTER[Rk]), Rk
    assert _within(R.measure_chain(), R.MEASURED_CHAIN)


def test_every_entry_refuses_bad_arguments_before_the_device():
    from spoofsv_amd import _lib
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)     # non-null dummy, never dereferenced: the checks come first
    up = (ctypes.c_long * 3)(0, 2, 4)
    down = (ctypes.c_long * 3)(0, 3, 2)
    out = (ctypes.c_long * 3)(0, 2, 9)
    calls = {
        "ssv_plda_class_stats": lambda Rk=4, host=up, Xd=one, S=2: L.ssv_plda_class_stats(one, one, host, Xd, Xd, null, null, 4, S, Rk, 1, null),
        "ssv_plda_mixed_inverse": lambda Rk=4, J=1, o=one: L.ssv_plda_mixed_inverse(null, one, 0, null, o, null, J, Rk, null),
        "ssv_plda_em_classes": lambda Rk=4, J=1, o=one: L.ssv_plda_em_classes(one, one, one, one, one, one, o, o, o, 2, J, Rk, null),
        "ssv_plda_wsyrk_f64": lambda Rk=4, o=one: L.ssv_plda_wsyrk_f64(one, null, o, 2, Rk, null),
        "ssv_plda_em_update": lambda Rk=4, J=1, o=one: L.ssv_plda_em_update(one, one, one, one, one, one, one, one, one, one, one, one, one, o, o, o, J, 2, Rk, 2.0, 4.0, null),
        "ssv_plda_transform": lambda Rk=4, o=ctypes.c_void_p(32): L.ssv_plda_transform(one, one, one, one, null, 1, ctypes.c_void_p(48), o, 2, Rk, 1, null),
        "ssv_plda_speaker_planes": lambda Rk=4, o=one: L.ssv_plda_speaker_planes(one, one, one, o, o, 2, Rk, null),
        "ssv_plda_score": lambda Rk=4, o=one: L.ssv_plda_score(one, one, one, o, 2, 2, Rk, null),
    }
    assert set(calls) == {n for n in _lib.parse_header() if n.startswith("ssv_plda_")}
    for name, f in calls.items():
        assert f(Rk=0) == -1 and name[4:].encode() in L.ssv_last_error(), name
        assert f(Rk=193) == -2 and b"193" in L.ssv_last_error(), name
    for name in ("ssv_plda_mixed_inverse", "ssv_plda_em_classes", "ssv_plda_em_update"):
        assert calls[name](J=0) == -1 and b"J" in L.ssv_last_error(), name
    for name in calls:
        if name == "ssv_plda_class_stats":
            assert calls[name](Xd=null) == -1 and b"null" in L.ssv_last_error()
        else:
            assert calls[name](o=null) == -1 and b"null" in L.ssv_last_error(), name
    assert calls["ssv_plda_class_stats"](host=down) == -1 and b"descends" in L.ssv_last_error()
    assert calls["ssv_plda_class_stats"](host=out) == -1 and b"leave" in L.ssv_last_error()
    assert L.ssv_plda_transform(one, one, one, one, null, 0, ctypes.c_void_p(48), ctypes.c_void_p(32), 2, 4, 1, null) == -1      # neither nex nor a count
    assert L.ssv_plda_score(one, one, one, one, 65535 * 64 + 1, 2, 4, null) == -2 and b"grid" in L.ssv_last_error()
