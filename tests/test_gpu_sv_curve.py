"""The spoof-rate / FRR curves on the device: ssv_sv_score_curve and ssv_score_list_curve_f32 / _f64 against the numpy reference
(tests/_sv_curve_ref.py) and against ssv_sv_eer_sweep's table at its 50 thresholds, then ``spoof_curve``, ``ivector_curve``,
``ivector_spoofrate`` and ``evaluate(curve=True)`` against the logs recorded from the reference's own scripts (tests/golden/sv_curve.npz).
Everything is an integer count or a fixed sequence of roundings of one: every comparison is bitwise.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest
import torch

import _sv_curve_ref as C
from _golden import GOLDEN, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
GARBAGE = -77
SIMMAT, SCORES = os.path.join(GOLDEN, "sv_curve_simmat.npy"), os.path.join(GOLDEN, "sv_curve_scores.txt")


def _tile():
    from spoofsv_amd import _lib
    return int(_lib.lib().ssv_sv_curve_tile())


def _nthr(kind):
    t = _tile()
    return {"1": 1, "tile-1": t - 1, "tile": t, "tile+1": t + 1, "2tile+3": 2 * t + 3}[kind]


def _thresholds(rng, K, dtype=np.float32, lo=0.3, hi=0.9):
    """K sorted thresholds of the scores' type with duplicates among them (every fifth repeats its neighbour), as Python floats."""
    t = np.sort(rng.uniform(lo, hi, K).astype(dtype))
    t[1::5] = t[0::5][:len(t[1::5])]
    t = np.sort(t)
    assert K < 3 or (np.diff(t) == 0).any()
    return [float(x) for x in t]


def _scores(rng, shape, thr, dtype=np.float32, lo=0.2, hi=1.0):
    """A third random, a third EQUAL to a threshold (rejected there), a third one ulp above one (accepted there)."""
    n = int(np.prod(shape))
    t = np.asarray(thr, dtype=dtype)
    pick = t[rng.randint(0, len(t), n)]
    kind = rng.randint(0, 3, n)
    x = np.where(kind == 0, rng.uniform(lo, hi, n).astype(dtype), np.where(kind == 1, pick, np.nextafter(pick, dtype(np.inf))))
    return x.astype(dtype).reshape(shape)


def _plant_specials(stack, head, tail):
    """NaN, +inf and -inf in each of the four classes of every matrix: off the own column, in the own column's head rows, in its tail rows
    and (V allowing) in its rows that are in neither."""
    nmat, N, V, _ = stack.shape
    sp = (np.nan, np.inf, -np.inf)
    for m in range(nmat):
        if N * V < 6:
            stack[m, 0, 0, 1] = np.nan
            continue
        for k, v in enumerate(sp):
            stack[m, k % N, k % V, (k % N + 1) % N] = v                  # off the own column
            stack[m, k % N, (k // N) % max(head, 1), k % N] = v          # head rows
            stack[m, (k + 1) % N, V - 1 - (k // N) % max(tail, 1), (k + 1) % N] = v   # tail rows
        if head + tail < V:
            stack[m, 0, head, 0] = np.nan
    return stack


def _run_stack(stack, thr, head, tail):
    """The C entry on a counts table pre-filled with garbage, guard words on both sides.  Returns the table (nmat, K, 4) int64."""
    from spoofsv_amd import _lib
    from spoofsv_amd.ops import _p, _stream
    nmat, N, V, _ = stack.shape
    K = len(thr)
    flat = torch.full((GUARD + nmat * K * 4 + GUARD,), GARBAGE, dtype=torch.int32, device=DEV)
    counts = flat[GUARD:GUARD + nmat * K * 4]
    sim = torch.from_numpy(stack).to(DEV)
    t = torch.tensor(thr, dtype=torch.float64).float().to(DEV)
    _lib.call("ssv_sv_score_curve", _p(sim), nmat, N, V, head, tail, _p(t), K, _p(counts), _stream())
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert np.all(host[:GUARD] == GARBAGE) and np.all(host[GUARD + nmat * K * 4:] == GARBAGE), "guard words written"
    return host[GUARD:GUARD + nmat * K * 4].reshape(nmat, K, 4).astype(np.int64), sim


# ================================================================================================ 1. the stack entry
STACK_SHAPES = (((1, 2, 2), 1, 1), ((3, 3, 5), 2, 2), ((3, 3, 5), 4, 3), ((2, 7, 37), 18, 18))


@pytest.mark.parametrize("kind", ("1", "tile-1", "tile", "tile+1", "2tile+3"))
@pytest.mark.parametrize("shape,head,tail", STACK_SHAPES, ids=["1x2x2", "3x3x5", "3x3x5-overlap", "2x7x37"])
def test_stack_counts_are_the_numpy_references(shape, head, tail, kind):
    """(2, 7, 37): 1813 trials per matrix, no multiple of the workgroup.  head = 4, tail = 3 of V = 5: two rows are in both classes."""
    from spoofsv_amd.ge2e import sv_score_curve
    (nmat, N, V), K = shape, _nthr(kind)
    rng = np.random.RandomState(1000 * N + 10 * V + K)
    thr = _thresholds(rng, K)
    stack = _plant_specials(_scores(rng, (nmat, N, V, N), thr), head, tail)
    want = C.stack_counts(stack, thr, head, tail)
    got, sim = _run_stack(stack, thr, head, tail)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert N * V < 6 or (want[:, 0, 1:].min() > 0 and want[:, -1, 0].min() < N * V * N - 3)      # (the case counts something)
    again = sv_score_curve(sim, thr, head, tail)                        # the operator, a table of its own: the same bits
    assert again.dtype == torch.int32 and tuple(again.shape) == (nmat, K, 4) and np.array_equal(again.cpu().numpy(), got)


@pytest.mark.parametrize("value,accepted", ((0.1, False), (2.0, True)), ids=["all-below", "all-above"])
def test_scores_outside_every_threshold(value, accepted):
    nmat, N, V, head, tail = 3, 3, 5, 4, 3
    thr = _thresholds(np.random.RandomState(3), _nthr("2tile+3"))
    stack = np.full((nmat, N, V, N), value, dtype=np.float32)
    got, _ = _run_stack(stack, thr, head, tail)
    sizes = np.array([N * V * N, N * V, N * head, N * tail]) * int(accepted)
    assert np.array_equal(got, np.broadcast_to(sizes, got.shape)) and np.array_equal(got, C.stack_counts(stack, thr, head, tail))


def test_stack_counts_are_the_50_threshold_sweeps():
    from spoofsv_amd.ge2e import sv_eer_sweep, sv_score_curve
    size_1, es1, N = 16, 4, 5
    thr = [0.01 * i + 0.5 for i in range(50)]
    g = torch.Generator().manual_seed(5)
    stack = 0.45 + 0.6 * torch.rand(3, N, size_1 - es1, N, generator=g)
    idx = torch.arange(N)
    stack[:, idx, :, idx] += 0.15
    stack[1, 2, 3, 2], stack[2, 0, 11, 0], stack[0, 1, 0, 3] = (float(np.float32(thr[k])) for k in (7, 20, 33))   # ON float32 thresholds
    stack = stack.to(DEV)
    half = (size_1 - es1) // 2
    got = sv_score_curve(stack, thr, half, half).cpu().numpy()
    for m in range(3):
        _, table = sv_eer_sweep(stack[m], size_1, es1, spoof=True, return_counts=True)
        assert np.array_equal(got[m], table.cpu().numpy()), m


def test_configuration_shape_against_searchsorted():
    """N = 20, V = 80, the script's 5,000 thresholds, two matrices."""
    from spoofsv_amd.ge2e import sv_score_curve
    rng = np.random.RandomState(20)
    stack = _scores(rng, (2, 20, 80, 20), C.GE2E_THR, lo=0.3, hi=1.1)
    idx = np.arange(20)
    stack[:, idx, :, idx] = _scores(rng, (2, 20, 80), C.GE2E_THR, lo=0.5, hi=1.0).transpose(1, 0, 2)
    got = sv_score_curve(torch.from_numpy(stack).to(DEV), C.GE2E_THR, 40, 40).cpu().numpy()
    want = C.stack_counts(stack, C.GE2E_THR, 40, 40)
    assert np.array_equal(got, want) and want[0, 0, 3] > want[0, -1, 3]


# ================================================================================================ 2. the list entries
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=["f32", "f64"])
@pytest.mark.parametrize("n", (1, 257, 5000))
def test_list_counts_are_the_numpy_references(n, dtype):
    from spoofsv_amd import _lib
    from spoofsv_amd.ge2e import score_list_curve
    from spoofsv_amd.ops import _p, _stream
    rng = np.random.RandomState(n + (dtype == np.float64))
    K = _nthr("tile+1")
    thr = _thresholds(rng, K, dtype, -2.0, 2.0)
    scores = _scores(rng, (n,), thr, dtype, -2.5, 2.5)
    if n >= 257:
        scores[[3, 50, 90, 130, 170, 210]] = (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)
    entry = "ssv_score_list_curve_f32" if dtype == np.float32 else "ssv_score_list_curve_f64"
    for nclass in (1, 2, 3, 4):
        codes = [nclass, 0] if n == 1 else [None]
        for code in codes:
            cls = rng.randint(0, 5, n).astype(np.uint8) if code is None else np.full(n, code, dtype=np.uint8)
            assert (cls >= nclass).any() or n == 1
            want = C.list_counts(scores, cls, thr, nclass)
            s_dev, c_dev = torch.from_numpy(scores).to(DEV), torch.from_numpy(cls).to(DEV)
            flat = torch.full((GUARD + K * nclass + GUARD,), GARBAGE, dtype=torch.int32, device=DEV)
            t_dev = torch.from_numpy(np.asarray(thr, dtype=dtype)).to(DEV)
            _lib.call(entry, _p(s_dev), _p(c_dev), n, nclass, _p(t_dev), K, _p(flat[GUARD:]), _stream())
            torch.cuda.synchronize()
            host = flat.cpu().numpy()
            assert np.all(host[:GUARD] == GARBAGE) and np.all(host[GUARD + K * nclass:] == GARBAGE), "guard words written"
            assert np.array_equal(host[GUARD:GUARD + K * nclass].reshape(K, nclass), want), (n, nclass, code)
            again = score_list_curve(s_dev, c_dev, thr, nclass)
            assert tuple(again.shape) == (K, nclass) and np.array_equal(again.cpu().numpy(), want)
            assert code != nclass or not want.any()                     # an item of a class past nclass is counted nowhere


# ================================================================================================ 3. the harness
def test_spoof_curve_and_ivector_curve_are_the_reference_logs():
    from spoofsv_amd import ge2e_harness as GH
    g = load("sv_curve.npz")
    cfg = GH.default_config()
    cfg["device"], cfg["test"]["N"] = DEV, 4
    out = GH.spoof_curve(cfg, 20, simmat=SIMMAT)
    assert out["thresholds"] == C.GE2E_THR and out["counts"].shape == (1, 5000, 4)
    for mine, ref in ((out["spoof_rate"], g["spoof_rate_log"]), (out["gt_frr"], g["gt_frr_log"])):
        assert mine.dtype == np.float64 and mine.shape == (1, 5000) and mine[0].tobytes() == ref.tobytes()
    # one matrix: the pooled rates are the same quotients taken in float64
    assert np.abs(out["pooled"]["spoof_rate"] - out["spoof_rate"][0]).max() < 1e-7 and np.abs(out["pooled"]["gt_frr"] - out["gt_frr"][0]).max() < 1e-7
    iv = GH.ivector_curve(SCORES, device=DEV)
    assert iv["thresholds"] == C.IVECTOR_THR
    assert iv["spoof_rate"].tobytes() == g["spoof_rate_log_2"].tobytes() and iv["gt_frr"].tobytes() == g["gt_frr_log_2"].tobytes()
    train, enroll, evl = (int(v) for v in g["spoofrate_args"])
    rate = GH.ivector_spoofrate(SCORES, float(g["spoofrate_thres"]), train, enroll, evl, device=DEV)
    assert isinstance(rate, float) and rate == float(g["spoofrate_value"]) and 0.0 < rate < 1.0


def test_curve_writes_the_scripts_four_logs(tmp_path):
    from spoofsv_amd import ge2e_harness as GH
    g = load("sv_curve.npz")
    cfg = GH.default_config()
    cfg["device"], cfg["test"]["N"] = DEV, 4
    sim_file = str(tmp_path / "simmat_e1_b1")
    torch.save(torch.from_numpy(np.load(SIMMAT)), sim_file)             # as ``test`` saves it and curve.py loads it
    GH.curve(cfg, sim_file, SCORES, out_dir=str(tmp_path / "out"), plot=False)
    assert sorted(os.listdir(tmp_path / "out")) == ["curve.npz"]
    z = np.load(tmp_path / "out" / "curve.npz")
    for k in ("spoof_rate_log", "gt_frr_log", "spoof_rate_log_2", "gt_frr_log_2"):
        assert z[k].tobytes() == g[k].tobytes(), k
    assert z["thresholds"].tolist() == C.GE2E_THR and z["thresholds_2"].tolist() == C.IVECTOR_THR


def test_evaluate_with_curve_is_spoof_curve_of_its_own_stack(tmp_path):
    import test_gpu_sv_eval as E
    from spoofsv_amd import ge2e_harness as GH
    cfg, model_path = E._e2e_config(tmp_path, E.E2E_SEED)
    E._seed(E.E2E_SEED)
    plain = GH.evaluate(cfg, model_path, E.ENR_, E.EVAL_)
    E._seed(E.E2E_SEED)
    out = GH.evaluate(cfg, model_path, E.ENR_, E.EVAL_, curve=True)
    assert "curve" not in plain and {k: v for k, v in out.items() if k != "curve"} == plain
    held = GH.evaluate.last_step.sims()
    want = GH.spoof_curve(cfg, E.EVAL_, sims=held)
    got = out["curve"]
    assert sorted(got) == ["counts", "gt_frr", "pooled", "spoof_rate", "thresholds"] and got["thresholds"] == want["thresholds"] == C.GE2E_THR
    assert got["spoof_rate"].shape == (held.shape[0], 5000) and held.shape[0] == 2
    for k in ("counts", "spoof_rate", "gt_frr"):
        assert got[k].tobytes() == want[k].tobytes(), k
    rows = 2 * E.EVAL_
    ref = C.stack_counts(held.cpu().numpy(), C.GE2E_THR, rows, rows)
    assert np.array_equal(got["counts"], ref)
    spoof, frr = C.ge2e_rates(ref[:, :, 2], ref[:, :, 3], E.N_, rows)
    assert got["spoof_rate"].tobytes() == spoof.tobytes() and got["gt_frr"].tobytes() == frr.tobytes()
    total = float(2 * E.N_ * rows)
    assert got["pooled"]["spoof_rate"].tobytes() == (ref[:, :, 3].sum(0) / total).tobytes()
    assert got["pooled"]["gt_frr"].tobytes() == ((total - ref[:, :, 2].sum(0)) / total).tobytes()
