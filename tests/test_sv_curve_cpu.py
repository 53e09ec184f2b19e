"""The spoof-rate / FRR curves, the parts that need no device: the new C-ABI entries and their argument errors, the numpy reference
against its own literal loop, curve.py's two rate formulas and the score-file parsers against the fixture recorded from the reference's
scripts (tools/gen_sv_curve_golden.py), and the operators' threshold checks.  Every comparison is bitwise."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _sv_curve_ref as C
from _golden import GOLDEN, load
from spoofsv_amd import _lib, ge2e
from spoofsv_amd import ge2e_harness as GH

SIMMAT, SCORES = os.path.join(GOLDEN, "sv_curve_simmat.npy"), os.path.join(GOLDEN, "sv_curve_scores.txt")


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ================================================================================================ the C ABI
def test_curve_entries_are_declared_and_exported():
    L = _lib.lib()
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH)
    for name, nargs in (("ssv_sv_score_curve", 10), ("ssv_score_list_curve_f32", 8), ("ssv_score_list_curve_f64", 8), ("ssv_sv_curve_tile", 0)):
        assert name in protos and hasattr(lib, name), name
        assert len(protos[name][1]) == nargs, (name, protos[name][2])
    assert L.ssv_sv_curve_tile() > 0
    assert L.ssv_version() == 7


def test_bad_curve_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)       # `one`: non-null dummy, never dereferenced: the checks come first
    good = dict(sim=one, nmat=2, N=3, V=6, head=4, tail=4, thr=one, nthr=50, counts=one)
    cases = [("sim", null), ("thr", null), ("counts", null), ("nmat", 0), ("N", 0), ("V", 0), ("nthr", 0), ("nthr", -1), ("head", 7), ("tail", 7),
             ("head", -1), ("tail", -1)]
    for key, bad in cases:
        a = dict(good, **{key: bad})
        rc = L.ssv_sv_score_curve(a["sim"], a["nmat"], a["N"], a["V"], a["head"], a["tail"], a["thr"], a["nthr"], a["counts"], null)
        assert rc == -1 and b"sv_score_curve" in L.ssv_last_error(), (key, rc)
    rc = L.ssv_sv_score_curve(one, 1, 40000, 2, 0, 0, one, 50, one, null)                 # 3.2e9 trials per matrix: past the int32 counts
    assert rc == -2 and b"sv_score_curve" in L.ssv_last_error()
    for entry, tag in ((L.ssv_score_list_curve_f32, b"score_list_curve_f32"), (L.ssv_score_list_curve_f64, b"score_list_curve_f64")):
        good = dict(scores=one, cls=one, n=10, nclass=2, thr=one, nthr=5, counts=one)
        for key, bad in (("scores", null), ("cls", null), ("thr", null), ("counts", null), ("n", 0), ("n", -3), ("nclass", 0), ("nclass", 5), ("nthr", 0)):
            a = dict(good, **{key: bad})
            rc = entry(a["scores"], a["cls"], a["n"], a["nclass"], a["thr"], a["nthr"], a["counts"], null)
            assert rc == -1 and tag in L.ssv_last_error(), (tag, key, rc)
        rc = entry(one, one, 2 ** 31, 1, one, 1, one, null)
        assert rc == -2 and tag in L.ssv_last_error()


# ================================================================================================ the numpy reference
def _with_specials(x, rng):
    flat = x.reshape(-1)
    k = rng.choice(flat.size, size=min(6, flat.size), replace=False)
    for pos, v in zip(k, (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        flat[pos] = v
    return x


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_searchsorted_counts_are_the_literal_loops(seed):
    rng = np.random.RandomState(seed)
    grid = np.round(rng.rand(9), 2)                                     # scores and thresholds drawn from one small grid: ties everywhere
    thr = np.sort(np.concatenate([rng.choice(grid, 7), rng.rand(4), [grid[0], grid[0]]])).tolist()
    stack = _with_specials(rng.choice(np.concatenate([grid, rng.rand(20)]), size=(2, 3, 5, 3)).astype(np.float32), rng)
    idx = np.arange(3)
    stack[0, idx, 0, idx] = (np.nan, np.inf, -np.inf)                   # specials inside the own column's head rows ...
    stack[1, idx, 4, idx] = (np.inf, np.nan, -np.inf)                   # ... and tail rows
    for head, tail in ((2, 2), (4, 3), (0, 0), (5, 5)):
        got, want = C.stack_counts(stack, thr, head, tail), C.stack_counts_loop(stack, thr, head, tail)
        assert got.shape == (2, len(thr), 4) and np.array_equal(got, want)
        assert np.all(np.diff(got, axis=1) <= 0) and int(got[0, :, 2].max()) <= max(3 * head - 2, 0)   # a NaN and -inf are above nothing
    for dtype in (np.float32, np.float64):
        scores = _with_specials(rng.choice(np.concatenate([grid, rng.randn(20)]), size=61).astype(dtype), rng)
        cls = rng.randint(0, 5, size=61).astype(np.uint8)
        for nclass in (1, 2, 3, 4):
            assert np.array_equal(C.list_counts(scores, cls, thr, nclass), C.list_counts_loop(scores, cls, thr, nclass))


# ================================================================================================ the reference's logs
def test_rate_formulas_reproduce_the_reference_logs_bitwise():
    g = load("sv_curve.npz")
    sim = np.load(SIMMAT)
    assert sim.dtype == np.float32 and sim.shape == (4, 80, 4)
    counts = C.stack_counts(sim[None], C.GE2E_THR, 40, 40)[0]
    for mine in (C.ge2e_rates, GH.ge2e_curve_rates):
        spoof, frr = mine(counts[:, 2], counts[:, 3], 4, 40)
        assert _same_bits(spoof, g["spoof_rate_log"]) and _same_bits(frr, g["gt_frr_log"])
    assert 0.0 < g["spoof_rate_log"][2500] < 1.0                        # (a curve, not a constant)
    # the planted scores: equal to float32(threshold) is rejected at that threshold whichever way the rounding went, the next float32 is accepted
    own = sim[np.arange(4), :, np.arange(4)]
    for t in list(g["planted_up"]) + list(g["planted_down"]):
        t32 = np.float32(C.GE2E_THR[t])
        assert int((own == t32).sum()) == 2 and int((own == np.nextafter(t32, np.float32(2))).sum()) == 2
        assert counts[t, 1] == int((own > t32).sum()) == int((own >= t32).sum()) - 2
    assert all(float(np.float32(C.GE2E_THR[t])) > C.GE2E_THR[t] for t in g["planted_up"])
    assert all(float(np.float32(C.GE2E_THR[t])) < C.GE2E_THR[t] for t in g["planted_down"])
    real, fake = C.parse_scores(SCORES)
    assert len(real) == len(fake) == 69
    counts2 = C.list_counts(np.concatenate([real, fake]), np.repeat(np.array([0, 1], dtype=np.uint8), 69), C.IVECTOR_THR, 2)
    spoof2, frr2 = C.ivector_rates(counts2[:, 0], counts2[:, 1], 69)
    assert _same_bits(spoof2, g["spoof_rate_log_2"]) and _same_bits(frr2, g["gt_frr_log_2"])


def test_threshold_lists_and_the_score_file_parsers():
    assert GH.curve_thresholds("ge2e") == C.GE2E_THR and GH.curve_thresholds("ivector") == C.IVECTOR_THR
    with pytest.raises(ValueError, match="curve_thresholds"):
        GH.curve_thresholds("plda")
    real, fake = GH.parse_ivector_scores(SCORES)
    want_real, want_fake = C.parse_scores(SCORES)
    assert _same_bits(real, want_real) and _same_bits(fake, want_fake)
    real2, fake2 = GH.parse_ivector_scores(SCORES, enroll_utt_num=0, eval_utt_num=10)
    assert len(real2) == 30 and len(fake2) == 108 and _same_bits(np.sort(np.concatenate([real2, fake2])), np.sort(np.concatenate([real, fake])))


def test_unequal_classes_and_wrong_totals_raise_before_the_device(tmp_path):
    with pytest.raises(ValueError, match="ivector_curve"):               # 10 real, 36 spoofing trials per speaker
        GH.ivector_curve(SCORES, enroll_utt_num=0, eval_utt_num=10, device="cpu")
    short = tmp_path / "short.txt"
    short.write_text("".join(open(SCORES).readlines()[:-1]))            # one spoofing trial of the last speaker missing
    with pytest.raises(ValueError, match="ivector_curve"):
        GH.ivector_curve(str(short), device="cpu")
    with pytest.raises(ValueError, match="ivector_spoofrate"):           # the defaults expect (108 - 88) * 20 trials
        GH.ivector_spoofrate(SCORES, 0.0, device="cpu")
    with pytest.raises(ValueError, match="ivector_spoofrate"):
        GH.ivector_spoofrate(SCORES, 0.0, train_spk_num=105, enroll_utt_num=3, eval_utt_num=20, device="cpu")


def test_decreasing_thresholds_raise_a_value_error():
    stack, scores, cls = torch.zeros(1, 2, 2, 2), torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.uint8)
    for bad in ([0.5, 0.4], [0.1, 0.2, 0.2, 0.19999], [0.5, float("nan")], []):
        with pytest.raises(ValueError, match="thresholds"):
            ge2e.sv_score_curve(stack, bad, 1, 1)
        with pytest.raises(ValueError, match="thresholds"):
            ge2e.score_list_curve(scores, cls, bad, 2)
    with pytest.raises(RuntimeError, match="ROCm device"):               # equal neighbours pass the check: the device check is next
        ge2e.sv_score_curve(stack, [0.5, 0.5, 0.6], 1, 1)
    cfg = GH.default_config()
    with pytest.raises(ValueError, match="spoof_curve"):
        GH.spoof_curve(cfg, 20)
    with pytest.raises(ValueError, match="spoof_curve"):                 # the fixture has 4 speakers, the configuration 20
        GH.spoof_curve(cfg, 20, simmat=SIMMAT)
