"""The verification test on the device: ssv_sv_trial_scores against the float64 restatement (bar: twice what float32 ``cossim_eval`` itself
misses float64 ``cossim_eval`` by on the same inputs, floor 1e-6), ssv_sv_eer_sweep's counts, index and floats against ``eer_sweep`` on
crafted matrices, ssv_sv_accept_rate against ``spoof_rate_at``, ``SvEvalStep`` (embeddings bitwise the module's, replay bitwise eager), and
``test`` / ``test_nospoof`` / ``evaluate`` / ``spoof_evaluation`` with the device path against the host path.  Run with `-m gpu` on an MI355X.

Measured on an MI355X (profiles/sv_eval.txt): over the shapes below float32 ``cossim_eval`` misses float64 by at most 6.3e-8 and the kernel by at
most 8.0e-8, so the bar is its floor, 1e-6, everywhere.  The end-to-end seed is E2E_SEED = 11: there the host path's scores stay 4.9e-5 or more
away from every threshold (the condition asks for 4e-6); of the seeds 11 ... 16 tried, 12 does not meet it (1.0e-6)."""
import contextlib
import io
import os
import random

import numpy as np
import pytest
import torch

import _sv_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
E2E_SEED = 11


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _unit_rows(rng, *shape):
    x = rng.standard_normal(shape)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _score_bar(enr, ver, V):
    """(bar, what float32 cossim_eval misses float64 cossim_eval by) on these inputs, both on the device."""
    from spoofsv_amd.ge2e_harness import cossim_eval
    e, v = torch.from_numpy(enr).to(DEV), torch.from_numpy(ver[:, :V]).to(DEV)
    lo = cossim_eval(v, e.mean(dim=1)).double()
    hi = cossim_eval(v.double(), e.double().mean(dim=1))
    miss = float((lo - hi).abs().max())
    return max(2.0 * miss, 1e-6), miss


def _clear_of_thresholds(mats, margin):
    """Smallest distance of any entry to any of the 50 float32 thresholds, asserted above ``margin``: only then do two scorings that agree
    to margin / 4 accept the same trials."""
    thr = R.THR32.astype(np.float64)
    gap = min(float(np.abs(np.asarray(m, dtype=np.float64).reshape(-1, 1) - thr[None, :]).min()) for m in mats)
    print("smallest distance of a score to a threshold: %.3e (needs > %.1e)" % (gap, margin))
    assert gap > margin, "this seed puts a score within reach of a threshold: the two paths may count it differently"
    return gap


# ================================================================================================ 1. scores
SCORE_SHAPES = ((2, 1, 2, 2, 1), (3, 2, 5, 5, 33), (5, 4, 12, 12, 64), (20, 6, 80, 80, 256), (70, 3, 4, 4, 256), (5, 4, 12, 16, 64), (3, 2, 3, 3, 8000))


@pytest.mark.parametrize("N,E,V,Vs,D", SCORE_SHAPES)
def test_trial_scores_against_float64(N, E, V, Vs, D):
    """(70, ., ., ., 256): N * D past the LDS tile, two centroid tiles.  (., ., 12, 16, .): V < ver_stride.  D = 8000: no centroid fits, the
    unstaged form."""
    from spoofsv_amd.ge2e import sv_trial_scores
    rng = np.random.RandomState(N * 1000 + D + Vs)
    enr, ver = _unit_rows(rng, N, E, D), _unit_rows(rng, N, Vs, D)
    zi, zv = N - 1, V // 2
    ver[zi, zv] = 0.0                                                   # one all-zero verification row
    want, want_cent = R.scores_ref(enr, ver, V)
    bar, miss = _score_bar(enr, ver, V)
    n = N * V * N
    flat = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    before = _bits(flat)
    out = flat[GUARD:GUARD + n].view(N, V, N)
    cent = torch.full((N, D), float("nan"), dtype=torch.float32, device=DEV)
    e_dev, v_dev = torch.from_numpy(enr).to(DEV), torch.from_numpy(ver).to(DEV)
    sv_trial_scores(e_dev, v_dev, V=V, out=out, cent=cent)
    torch.cuda.synchronize()
    after = _bits(flat)
    assert np.array_equal(after[:GUARD], before[:GUARD]) and np.array_equal(after[GUARD + n:], before[GUARD + n:]), "guard words written"
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("scores (N=%d E=%d V=%d of %d D=%d): kernel %.3e, float32 cossim_eval %.3e, bar %.3e" % (N, E, V, Vs, D, err, miss, bar))
    assert err <= bar, (err, bar)
    assert np.abs(cent.cpu().numpy().astype(np.float64) - want_cent).max() <= 2.0 ** -22
    off = [j for j in range(N) if j != zi]
    assert np.all(got[zi, zv, off] == np.float32(1e-6))
    # a second run, and a run without the centroid output, give the same bits
    again = sv_trial_scores(e_dev, v_dev, V=V)
    assert np.array_equal(_bits(again), _bits(out))


def test_trial_scores_do_not_depend_on_the_tiling():
    """An off-speaker score depends on its verification row and its centroid alone: speakers 60 ... 69 of the two-tile problem (N = 70,
    D = 256: centroids 0 ... 57 and 58 ... 69) scored by themselves (one tile of 10) give the same bits; so do the first 4 rows of a
    6-row problem (the own column aside, which averages other rows)."""
    from spoofsv_amd.ge2e import sv_trial_scores
    rng = np.random.RandomState(5)
    enr, ver = torch.from_numpy(_unit_rows(rng, 70, 3, 256)).to(DEV), torch.from_numpy(_unit_rows(rng, 70, 6, 256)).to(DEV)
    full, part = sv_trial_scores(enr, ver), sv_trial_scores(enr[60:].contiguous(), ver[60:].contiguous())
    sub = full[60:, :, 60:]
    assert np.array_equal(_bits(sub), _bits(part))
    fewer = sv_trial_scores(enr, ver, V=4)
    offdiag = ~torch.eye(70, dtype=torch.bool, device=DEV).unsqueeze(1).expand(70, 4, 70)
    assert torch.equal(fewer[offdiag], full[:, :4][offdiag]) and not torch.equal(fewer, full[:, :4])


# ================================================================================================ 2. the sweep
def _crafted(N, V, seed):
    g = torch.Generator().manual_seed(seed)
    sim = 0.45 + 0.6 * torch.rand(N, V, N, generator=g)
    idx = torch.arange(N)
    sim[idx, :, idx] += 0.15
    return sim


def _at_thresholds(N, V):
    """The random recipe with entries put EXACTLY on float32 thresholds, on and off the own column, in both halves."""
    sim = _crafted(N, V, 99)
    thr = torch.from_numpy(R.THR32)
    for k, (i, v, j) in enumerate(((0, 0, 0), (1, V - 1, 1), (0, 1, 1), (1, 0, 0), (N - 1, V // 2, N - 1), (N - 1, V - 1, 0), (0, V // 2 - 1, 0))):
        sim[i, v, j] = thr[(7 * k + 3) % 50]
    sim[0, 2, 1], sim[1, 2, 1] = thr[0], thr[49]
    return sim


def _tied(N, V):
    """FAR falls to 0 at threshold 20 (every off-speaker score is below 0.70), FRR leaves 0 at threshold 41 (every own score is 0.905):
    |FAR - FRR| = 0 at thresholds 20 ... 40, and the first of them wins."""
    sim = torch.empty(N, V, N)
    vals = torch.tensor([0.505 + 0.01 * k for k in range(20)])
    sim[:] = vals[torch.arange(N * V * N) % 20].reshape(N, V, N)
    idx = torch.arange(N)
    sim[idx, :, idx] = 0.905
    return sim


SWEEP_CASES = [("random-%d" % N, lambda N=N: _crafted(N, 12, N)) for N in (2, 5, 20)] + [
    ("at-thresholds", lambda: _at_thresholds(5, 12)), ("tied", lambda: _tied(5, 12)),
    ("all-accept", lambda: torch.full((5, 12, 5), 1.5)), ("all-reject", lambda: torch.full((5, 12, 5), 0.1))]


@pytest.mark.parametrize("spoof", (True, False))
@pytest.mark.parametrize("name,make", SWEEP_CASES, ids=[c[0] for c in SWEEP_CASES])
def test_sweep_counts_index_and_floats_are_the_hosts(name, make, spoof):
    from spoofsv_amd.ge2e import sv_eer_sweep
    from spoofsv_amd.ge2e_harness import eer_sweep
    size_1, es1 = 16, 4
    sim = make() if spoof else make()[:, :6].contiguous()
    want = eer_sweep(sim, size_1, es1, spoof=spoof)
    ref, counts = R.sweep_ref(sim.numpy(), size_1, es1, spoof)
    if name == "tied":
        assert ref["diffs"].count(min(ref["diffs"])) >= 2 and 0 < ref["best"] == ref["diffs"].index(min(ref["diffs"]))
    if name == "at-thresholds":
        assert int((sim.reshape(-1, 1) == torch.from_numpy(R.THR32)[None, :]).sum()) >= 5
    got, got_counts = sv_eer_sweep(sim.to(DEV), size_1, es1, spoof=spoof, return_counts=True)
    assert np.array_equal(got_counts.cpu().numpy().astype(np.int64), counts), name
    assert sorted(got) == sorted(want) and got["thres"] == want["thres"] == ref["thres"]
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, (name, spoof, k, got[k], want[k])


def test_three_sweeps_fill_three_history_slots():
    from spoofsv_amd import ge2e
    from spoofsv_amd.ge2e_harness import eer_sweep
    size_1, es1, hist_len = 16, 4, 5
    sims = [_crafted(5, 12, s) for s in (1, 2, 3)]
    hist = torch.full((hist_len, 6), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.zeros((ge2e.SV_NTHR, 4), dtype=torch.int32, device=DEV)
    step_dev = torch.zeros((1,), dtype=torch.int32, device=DEV)
    for s in sims:
        ge2e._sv_sweep_call(s.to(DEV), ge2e.sv_sweep_constants(size_1, es1, True), counts, hist, hist_len, step_dev)
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 3
    h = hist.cpu().numpy()
    assert np.all(h[3:] == -7.0)
    for k, s in enumerate(sims):
        want = eer_sweep(s, size_1, es1, spoof=True)
        row = ge2e._sv_row(h[k], True)
        for key in want:
            assert abs(row[key] - want[key]) <= 1e-12, (k, key)
    for s in sims:                                                      # two more, then the sixth wraps into slot 0
        ge2e._sv_sweep_call(s.to(DEV), ge2e.sv_sweep_constants(size_1, es1, True), counts, hist, hist_len, step_dev)
    h2 = hist.cpu().numpy()
    assert int(step_dev.item()) == 6 and np.array_equal(h2[0], h[2]) and np.array_equal(h2[3], h[0]) and np.array_equal(h2[1:3], h[1:3])


# ================================================================================================ 3. accept rate
def test_accept_rate_is_spoof_rate_at(tmp_path):
    from spoofsv_amd import ge2e_harness as GH
    from spoofsv_amd.ge2e import sv_accept_rate
    N, V, eval_num, thres = 5, 12, 3, 0.6
    mats = [_crafted(N, V, s) for s in (1, 2, 3)]
    mats[1][2, -1, 2] = float(np.float32(thres))                        # equal to float32(thres) (which lies above 0.6): not accepted
    mats[1][3, -2, 3] = float(np.nextafter(np.float32(thres), np.float32(1)))
    cfg = GH.default_config()
    cfg["test"]["N"], cfg["save_simmat_dir"] = N, str(tmp_path)
    for k, m in enumerate(mats):
        torch.save(m, tmp_path / ("simmat_e1_b%d" % (k + 1)))
    stack = torch.stack(mats).to(DEV)
    rates = sv_accept_rate(stack, thres, eval_num)
    assert rates == R.accept_rate_ref(stack.cpu().numpy(), thres, eval_num)
    assert GH.spoof_rate_at(cfg, thres, eval_num, sims=stack) == GH.spoof_rate_at(cfg, thres, eval_num)


# ================================================================================================ 4. the step
N_, M_, ENR_, EVAL_ = 5, 16, 2, 3
NMELS, FRAMES, HID, PROJ = 40, 24, 32, 16


def _net(seed=0):
    from spoofsv_amd.ge2e import SpeechEmbedder
    torch.manual_seed(seed)
    return SpeechEmbedder(NMELS, HID, 1, PROJ).to(DEV).eval()


def _corpus_tensor(speakers=7, per=16, seed=3):
    rng = np.random.RandomState(seed)
    data = np.concatenate([rng.randn(1, NMELS, 1) + 0.3 * rng.randn(per, NMELS, FRAMES) for _ in range(speakers)]).astype(np.float32)
    return torch.from_numpy(data).to(DEV)


def _tables(total, seed, n=3):
    """Row tables as the test loader draws them (a speaker's first M rows; speakers may repeat), one per batch."""
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, total // 16, N_)[:, None] * 16 + np.arange(M_)[None, :]).reshape(-1).astype(np.int64) for _ in range(n)]


def test_step_embeddings_are_the_modules_and_its_sweep_is_eer_sweep():
    from spoofsv_amd import ge2e
    from spoofsv_amd.ge2e_harness import cossim_eval, eer_sweep
    net, data = _net(), _corpus_tensor()
    step = ge2e.SvEvalStep(net, data, N_, M_, ENR_, EVAL_, graph=False, hist_len=4)
    rows = _tables(data.shape[0], 1, 1)[0]
    step.run(rows)
    torch.cuda.synchronize()
    assert net not in ge2e._FWD_CACHE                                    # the module's own inference cache is not touched
    r = torch.from_numpy(rows).reshape(N_, M_)
    es1 = 2 * ENR_
    x = data[r.to(DEV)].transpose(2, 3)                                  # (N, M, frames, nmels): the host loader's batch
    with torch.no_grad():
        e_enr = net(x[:, :es1].reshape(N_ * es1, FRAMES, NMELS).contiguous()).reshape(N_, es1, -1)
        e_ver = net(x[:, es1:].reshape(N_ * (M_ - es1), FRAMES, NMELS).contiguous()).reshape(N_, M_ - es1, -1)
    assert np.array_equal(_bits(step.e_enr), _bits(e_enr)) and np.array_equal(_bits(step.e_ver), _bits(e_ver))
    bar, _ = _score_bar(e_enr.cpu().numpy(), e_ver.cpu().numpy(), M_ - es1)
    assert float((step.sim - cossim_eval(e_ver, e_enr.mean(dim=1))).abs().max()) <= bar
    assert float((step.sim_nospoof - cossim_eval(e_ver[:, :2 * EVAL_], e_enr.mean(dim=1))).abs().max()) <= bar
    got = step.results(1)[0]
    for want, mine in ((eer_sweep(step.sim.cpu(), M_, es1, spoof=True), got), (eer_sweep(step.sim_nospoof.cpu(), M_, es1, spoof=False), got["nospoof"])):
        assert mine["thres"] == want["thres"]
        for k in want:
            assert abs(mine[k] - want[k]) <= 1e-12, k
    assert np.array_equal(_bits(step.sims()[0]), _bits(step.sim))
    with pytest.raises(ValueError, match="row table"):
        step.load(np.full(N_ * M_, data.shape[0]))


def test_step_replayed_is_bitwise_eager():
    from spoofsv_amd import ge2e
    net, data = _net(), _corpus_tensor()
    tables = _tables(data.shape[0], 2, 3)
    runs = []
    for graph in (False, True):
        step = ge2e.SvEvalStep(net, data, N_, M_, ENR_, EVAL_, graph=graph, hist_len=8).prepare()
        assert step.batches == 0 and int(step.step_dev.sum().item()) == 0
        kept = []
        for rows in tables:
            step.run(rows)
            kept.append((_bits(step.e_enr), _bits(step.e_ver), _bits(step.sim), _bits(step.sim_nospoof), step.counts.cpu().numpy().copy()))
        assert step.step_dev.cpu().tolist() == [3, 3]
        runs.append((kept, step.hist.cpu().numpy().copy(), _bits(step.sims()), step.results(3)))
        if graph:
            assert step.stepper.plan is not None
            step.release()
    (ek, eh, es, er), (gk, gh, gs, gr) = runs
    for a, b in zip(ek, gk):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert np.array_equal(eh, gh) and np.array_equal(es, gs) and er == gr
    assert len({k[2].tobytes() for k in ek}) == 3                        # three different batches


# ================================================================================================ 5. end to end
def _e2e_config(tmp_path, seed):
    from spoofsv_amd import ge2e_harness as GH
    rng = np.random.RandomState(seed)
    d = tmp_path / "test"
    d.mkdir()
    for s in range(7):
        np.save(d / ("spk%02d.npy" % s), (rng.randn(1, NMELS, 1) + 0.3 * rng.randn(M_, NMELS, FRAMES)).astype(np.float32))
    cfg = GH.default_config()
    cfg["data"].update(test_path=str(d))
    cfg["model"].update(hidden=HID, num_layer=1, proj=PROJ)
    cfg["test"].update(N=N_, M=M_, epochs=2)
    cfg["save_simmat_dir"] = str(tmp_path / "simmat")
    model_path = str(tmp_path / "net.model")
    torch.save({k: v.cpu() for k, v in _net(seed).state_dict().items()}, model_path)
    return cfg, model_path


def _captured(fn, *args):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*args)
    return out, buf.getvalue()


def _e2e_margin():
    rng = np.random.RandomState(0)
    return 4.0 * _score_bar(_unit_rows(rng, N_, 2 * ENR_, PROJ), _unit_rows(rng, N_, M_ - 2 * ENR_, PROJ), M_ - 2 * ENR_)[0]


@pytest.mark.parametrize("graph", (True, False))
def test_resident_test_and_test_nospoof_are_the_host_paths(tmp_path, graph):
    from spoofsv_amd import ge2e_harness as GH
    cfg, model_path = _e2e_config(tmp_path, E2E_SEED)
    margin = _e2e_margin()
    _seed(E2E_SEED)
    (eer, spoof), lines = _captured(GH.test, cfg, model_path, ENR_)
    host_files = sorted(os.listdir(cfg["save_simmat_dir"]))
    host_mats = [torch.load(os.path.join(cfg["save_simmat_dir"], f)).numpy() for f in host_files]
    _clear_of_thresholds(host_mats, margin)
    _seed(E2E_SEED)
    thres, lines2 = _captured(GH.test_nospoof, cfg, model_path, ENR_, EVAL_)
    _seed(E2E_SEED)
    with torch.no_grad():
        net = GH._load(cfg, model_path, torch.device(DEV))
        ns = [GH.cossim_eval(e_ver[:, :2 * EVAL_], cent).cpu().numpy() for _, _, _, _, e_ver, cent in GH._verification_batches(cfg, net, ENR_, torch.device(DEV))]
    _clear_of_thresholds(ns, margin)

    res = {k: (dict(v) if isinstance(v, dict) else v) for k, v in cfg.items()}
    res["test"].update(resident=True, graph=graph)
    res["save_simmat_dir"] = str(tmp_path / "simmat_resident")
    _seed(E2E_SEED)
    (eer_r, spoof_r), lines_r = _captured(GH.test, res, model_path, ENR_)
    assert abs(eer_r - eer) <= 1e-9 and abs(spoof_r - spoof) <= 1e-9 and lines_r == lines and lines.count("EER :") == 2
    assert sorted(os.listdir(res["save_simmat_dir"])) == host_files
    for f, m in zip(host_files, host_mats):
        assert np.abs(torch.load(os.path.join(res["save_simmat_dir"], f)).numpy() - m).max() <= margin / 4
    held = GH.test.last_step.sims()
    assert tuple(held.shape) == (2, N_, M_ - 2 * ENR_, N_)
    assert GH.spoof_rate_at(res, 0.7, EVAL_, sims=held) == GH.spoof_rate_at(res, 0.7, EVAL_)
    res["test"]["save_simmat"], res["save_simmat_dir"] = False, str(tmp_path / "never")
    _seed(E2E_SEED)
    (eer_q, _), _ = _captured(GH.test, res, model_path, ENR_)
    assert eer_q == eer_r and not os.path.exists(res["save_simmat_dir"])
    _seed(E2E_SEED)
    thres_r, lines2_r = _captured(GH.test_nospoof, res, model_path, ENR_, EVAL_)
    assert abs(thres_r - thres) <= 1e-9 and lines2_r == lines2 and lines2.count("FRR:") == 2


def test_evaluate_is_one_pass_over_its_own_matrices(tmp_path):
    from spoofsv_amd import ge2e_harness as GH
    cfg, model_path = _e2e_config(tmp_path, E2E_SEED)
    _seed(E2E_SEED)
    out = GH.evaluate(cfg, model_path, ENR_, EVAL_)
    assert sorted(out) == ["EER", "spoof_rate", "spoof_rate_at_eer", "threshold"] and all(np.isfinite(v) for v in out.values())
    assert 0.0 <= out["EER"] <= 1.0 and 0.5 <= out["threshold"] < 1.0 and 0.0 <= out["spoof_rate_at_eer"] <= 1.0
    assert not os.path.exists(cfg["save_simmat_dir"])                   # no disk
    held = GH.evaluate.last_step.sims()
    os.makedirs(cfg["save_simmat_dir"])
    for k, m in enumerate(held.cpu()):
        torch.save(m.clone(), os.path.join(cfg["save_simmat_dir"], "simmat_e1_b%d" % (k + 1)))
    assert abs(out["spoof_rate_at_eer"] - GH.spoof_rate_at(cfg, out["threshold"], EVAL_)) <= 1e-12
    # the mixture figures are those of the resident ``test`` under the same seeds: the same draws, the same embeddings
    cfg["test"].update(resident=True, save_simmat=False)
    _seed(E2E_SEED)
    (eer, spoof), _ = _captured(GH.test, cfg, model_path, ENR_)
    assert abs(eer - out["EER"]) <= 1e-12 and abs(spoof - out["spoof_rate"]) <= 1e-12


def test_spoof_evaluation_with_device_scoring(tmp_path):
    from spoofsv_amd import ge2e_harness as GH
    net = _net(E2E_SEED)
    rng = np.random.RandomState(E2E_SEED)
    base = rng.randn(N_, 1, 1, 1, NMELS)

    def side(k):
        return torch.from_numpy((base + 0.3 * rng.randn(N_, k, 2, FRAMES, NMELS)).astype(np.float32)).to(DEV)
    enrol, genuine, spoof = side(2), side(3), side(3)
    want = GH.spoof_evaluation(GH.default_config(), net, enrol, genuine, spoof)
    _clear_of_thresholds([want["sim"].cpu().numpy()], _e2e_margin())
    got = GH.spoof_evaluation(GH.default_config(), net, enrol, genuine, spoof, device_scoring=True)
    assert sorted(got) == sorted(want) and got["thres"] == want["thres"]
    for k in want:
        if k != "sim":
            assert abs(got[k] - want[k]) <= 1e-9, k
    assert float((got["sim"] - want["sim"]).abs().max()) <= _e2e_margin() / 4
