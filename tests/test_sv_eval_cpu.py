"""The verification test on the device, the parts that need none: the float64 restatement against the host functions, the fixture and the
oracle; ``ResidentSpeakerCorpus.test_batches`` against the host test loader's random stream; the shape checks; the new C-ABI entries'
argument errors."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import _sv_eval_ref as R
from _golden import load
from oracle import ge2e_oracle as GO
from spoofsv_amd import _lib, ge2e
from spoofsv_amd import ge2e_harness as GH


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _crafted(N, V, seed):
    """The existing host test's recipe: 0.45 + 0.6 rand with the own-speaker column raised."""
    g = torch.Generator().manual_seed(seed)
    sim = 0.45 + 0.6 * torch.rand(N, V, N, generator=g)
    idx = torch.arange(N)
    sim[idx, :, idx] += 0.15
    return sim


# ================================================================================================ the restatement
@pytest.mark.parametrize("N,E,V,D", ((2, 1, 2, 1), (3, 2, 5, 33), (5, 4, 12, 64)))
def test_scores_restatement_is_cossim_eval(N, E, V, D):
    rng = np.random.RandomState(N * 100 + D)
    enr, ver = rng.standard_normal((N, E, D)), rng.standard_normal((N, V + 2, D))
    ver[0, 1] = 0.0                                                     # a zero row: the clamp decides
    for use in (V, V + 2):
        sim, cent = R.scores_ref(enr, ver, use)
        want = GH.cossim_eval(torch.from_numpy(ver[:, :use]), torch.from_numpy(enr).mean(dim=1)).numpy()
        assert sim.shape == (N, use, N) and np.abs(sim - want).max() < 1e-12
        assert np.abs(cent - enr.mean(1)).max() == 0.0
    off = [j for j in range(N) if j != 0]
    assert np.all(R.scores_ref(enr, ver, V)[0][0, 1, off] == 1e-6)


def test_scores_restatement_on_the_reference_fixture():
    g = load("ge2e_train.npz")
    sim, cent = R.scores_ref(g["ev_enr"], g["ev_ver"])
    assert np.abs(cent - g["ev_cent"]).max() < 1e-6 * np.abs(g["ev_cent"]).max()
    assert np.abs(sim - g["ev_sim"]).max() < 1e-5 * np.abs(g["ev_sim"]).max()


@pytest.mark.parametrize("N", (2, 5, 20))
def test_sweep_restatement_is_eer_sweep_and_the_oracle(N):
    size_1, es1 = 16, 4
    against_oracle = 0
    for trial in range(3):
        sim = _crafted(N, size_1 - es1, 10 * N + trial)
        for spoof, m in ((True, sim), (False, sim[:, :6].contiguous())):
            got, counts = R.sweep_ref(m.numpy(), size_1, es1, spoof)
            want, orc = GH.eer_sweep(m, size_1, es1, spoof=spoof), GO.eer_sweep(m, size_1, es1, spoof=spoof)
            assert got["thres"] == want["thres"]
            # the oracle's loops run in float32: where two thresholds tie in |FAR - FRR| to within its rounding it may take the other one
            d = sorted(got["diffs"])
            unique = d[1] - d[0] > 1e-5
            against_oracle += unique
            for k in want:
                assert abs(got[k] - want[k]) < 1e-12, (N, trial, spoof, k)
                assert not unique or abs(got[k] - orc[k]) < 1e-6, (N, trial, spoof, k)
            assert counts.shape == (50, 4) and counts[0, 0] >= counts[-1, 0] and np.all(counts[:, 1] <= counts[:, 0])
            assert ge2e.sv_sweep_constants(size_1, es1, spoof) == R.sweep_constants(size_1, es1, spoof)
    assert against_oracle >= 2


def test_accept_rate_restatement_is_spoof_rate_at(tmp_path):
    N, V, eval_num, thres = 5, 12, 3, 0.6
    assert float(np.float32(thres)) > thres                             # the float32 rounding lies ABOVE: the two comparisons differ on it
    mats = [_crafted(N, V, s) for s in (1, 2, 3)]
    mats[1][2, -1, 2] = float(np.float32(thres))                        # equal to float32(thres): not accepted
    mats[1][3, -2, 3] = float(np.nextafter(np.float32(thres), np.float32(1)))
    cfg = GH.default_config()
    cfg["test"]["N"], cfg["save_simmat_dir"] = N, str(tmp_path)
    want = []
    for k, m in enumerate(mats):
        for f in os.listdir(tmp_path):
            os.remove(tmp_path / f)
        torch.save(m, tmp_path / ("simmat_e1_b%d" % (k + 1)))
        want.append(GH.spoof_rate_at(cfg, thres, eval_num))
    got = R.accept_rate_ref(torch.stack(mats).numpy(), thres, eval_num)
    assert got == want
    assert not bool((mats[1][2, -1, 2] > thres))                        # torch compares the float32 tensor with float32(thres)


# ================================================================================================ the test loader's row tables
def _write_tagged(path, counts, nmels=3, frames=4):
    """Speaker s's utterance u holds the value 100 * s + u everywhere."""
    os.makedirs(path, exist_ok=True)
    for s, c in enumerate(counts):
        arr = np.zeros((c, nmels, frames), dtype=np.float32) + (100.0 * s + np.arange(c, dtype=np.float32))[:, None, None]
        np.save(os.path.join(path, "speaker%d.npy" % s), arr)
    return path


def test_test_batches_follow_the_host_test_loaders_random_stream(tmp_path):
    counts, N, M = (8, 6, 9, 6, 7), 2, 6
    path = _write_tagged(str(tmp_path / "test"), counts)
    cfg = GH.default_config()
    cfg["data"]["test_path"] = path
    cfg["test"].update(N=N, M=M, epochs=2)

    class _Tags(torch.nn.Module):                                       # "embedder": the utterance's tag, so the loader's picks can be read off
        def forward(self, x):
            return x[:, 0, :1]
    _seed(77)
    want = []
    for e, b, size_1, es1, e_ver, cent in GH._verification_batches(cfg, _Tags(), 1, "cpu"):
        assert size_1 == M and es1 == 2
        want.append(e_ver.reshape(N, M - 2).numpy().copy())
    assert len(want) == 2 * (len(counts) // N)                          # drop_last: 5 speakers, 2 batches of 2 per epoch
    corpus = GH.ResidentSpeakerCorpus(path, "cpu")
    _seed(77)
    batches = corpus.test_batches(N, M)
    assert len(batches) == len(counts) // N
    tables = [rows for _ in range(2) for rows in batches]
    assert len(tables) == len(want)
    tags = corpus.data[:, 0, 0].numpy()
    speakers = []
    for rows, w in zip(tables, want):
        assert rows.dtype == torch.int32 and tuple(rows.shape) == (N * M,)
        got = tags[rows.numpy()].reshape(N, M)
        assert np.array_equal(got[:, 2:], w)                            # the verification rows the host loader yielded
        assert np.array_equal(got % 100, np.tile(np.arange(M), (N, 1)))  # a speaker's FIRST M utterances, in order
        speakers.append(tuple((got[:, 0] // 100).astype(int)))
    assert len(set(speakers)) > 1                                       # (the stream moves)


def test_short_speaker_file_and_bad_shapes_are_refused(tmp_path):
    path = _write_tagged(str(tmp_path / "short"), (6, 5, 6))
    corpus = GH.ResidentSpeakerCorpus(path, "cpu")
    with pytest.raises(ValueError, match="speaker1.npy"):
        corpus.test_batches(2, 6)
    assert len(corpus.test_batches(2, 4)) == 1
    assert ge2e.sv_eval_shapes(20, 86, 3, 20) == (6, 80, 40)
    assert ge2e.sv_eval_shapes(5, 16, 2) == (4, 12, None)
    for bad in (dict(M=15), dict(N=1), dict(enroll_num=8), dict(enroll_num=9), dict(enroll_num=0), dict(eval_num=7), dict(eval_num=0)):
        a = dict(dict(N=5, M=16, enroll_num=2, eval_num=3), **bad)
        with pytest.raises(ValueError, match="verification test"):
            ge2e.sv_eval_shapes(a["N"], a["M"], a["enroll_num"], a["eval_num"])
    with pytest.raises(ValueError, match="verification test"):           # the step checks its shapes before it touches a device
        ge2e.SvEvalStep(None, None, 5, 15, 2)


# ================================================================================================ the C ABI
def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    L = _lib.lib()
    protos = _lib.parse_header()
    for name in ("ssv_sv_trial_scores", "ssv_sv_eer_sweep", "ssv_sv_accept_rate"):
        assert name in protos and hasattr(ctypes.CDLL(_lib.LIBPATH), name), name
    assert L.ssv_version() == 7
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)       # `one`: non-null dummy, never dereferenced: the checks come first
    good = dict(enr=one, ver=one, sim=one, cent=null, N=3, E=2, V=5, vs=5, D=8)
    cases = [("enr", null), ("ver", null), ("sim", null), ("N", 1), ("N", 0), ("V", 1), ("E", 0), ("vs", 4), ("D", 0), ("D", -1)]
    for key, bad in cases:
        a = dict(good, **{key: bad})
        rc = L.ssv_sv_trial_scores(a["enr"], a["ver"], a["sim"], a["cent"], a["N"], a["E"], a["V"], a["vs"], a["D"], null)
        assert rc == -1 and b"sv_trial_scores" in L.ssv_last_error(), (key, rc)
    good = dict(sim=one, N=3, V=6, thr=one, nthr=50, head=3, tail=3, counts=one, hist=one, hl=4, step=one)
    cases = [("sim", null), ("thr", null), ("counts", null), ("hist", null), ("step", null), ("N", 1), ("V", 0), ("nthr", 0), ("hl", 0),
             ("head", 7), ("tail", 7), ("head", -1)]
    for key, bad in cases:
        a = dict(good, **{key: bad})
        rc = L.ssv_sv_eer_sweep(a["sim"], a["N"], a["V"], a["thr"], a["nthr"], a["head"], a["tail"], 6.0, 6.0, 3.0, 3.0, a["counts"], a["hist"], a["hl"],
                                a["step"], null)
        assert rc == -1 and b"sv_eer_sweep" in L.ssv_last_error(), (key, rc)
    rc = L.ssv_sv_eer_sweep(one, 40000, 2, one, 50, 0, 0, 1.0, 1.0, 1.0, 1.0, one, one, 1, one, null)      # 3.2e9 trials: past the int32 counts
    assert rc == -2 and b"sv_eer_sweep" in L.ssv_last_error()
    good = dict(stack=one, nmat=2, N=3, V=6, tail=4, rates=one)
    for key, bad in (("stack", null), ("rates", null), ("nmat", 0), ("N", 0), ("V", 0), ("tail", 0), ("tail", 7)):
        a = dict(good, **{key: bad})
        rc = L.ssv_sv_accept_rate(a["stack"], a["nmat"], a["N"], a["V"], a["tail"], 0.7, a["rates"], null)
        assert rc == -1 and b"sv_accept_rate" in L.ssv_last_error(), (key, rc)
