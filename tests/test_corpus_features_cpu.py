"""CPU-only checks of the ragged corpus front end (csrc/corpus_features.hip, spoofsv_amd.corpus_features, the harness entries built on
it): the length arithmetic, the memory estimate, the C ABI's new entries, the float64 restatement the GPU tests compare against
(tests/_corpus_features_ref.py) on an identity of its own, and the CORPUS_FEATURES switch of ``CorpusSource`` on a machine without a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _corpus_features_ref as C
from spoofsv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = json.load(open(os.path.join(ROOT, "config.json")))
ENTRIES = ["ssv_preemph_frames_ragged", "ssv_corpus_normalize_pack"]


@pytest.fixture
def no_gpu(monkeypatch):
    """What a machine without a ROCm device answers, on any machine."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_header_declares_and_library_exports_the_new_entries():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIBPATH)
    for name in ENTRIES:
        assert name in protos, name
        assert hasattr(L, name), name
    assert _lib.lib().ssv_version() == 7


def test_lengths_over_a_sweep_of_n():
    """T = 1 + n // hop, rt = T // r, lin width r * rt; n <= n_fft // 2 gives 0 (no reflect padding exists): the module's host arithmetic
    against the restatement's and against the formulas written out."""
    from spoofsv_amd import corpus_features as cf
    n_fft, hop, r = 1024, 256, 4
    sweep = list(range(0, 3 * n_fft)) + [n_fft // 2, n_fft // 2 + 1, 22050, 48000, 132300, 132301] + [hop * k + d for k in (4, 5, 517) for d in (-1, 0, 1)]
    for n in sweep:
        T, rt, w = cf.feature_lengths(n, n_fft, hop, r)
        assert (T, rt, w) == C.lengths(n, n_fft, hop, r)
        if n <= n_fft // 2:
            assert (T, rt, w) == (0, 0, 0)
        else:
            assert T == 1 + n // hop and rt == T // r and w == r * rt and w <= T
    assert cf.feature_lengths(512, 1024, 256, 4) == (0, 0, 0) and cf.feature_lengths(513, 1024, 256, 4) == (3, 0, 0)
    assert cf.feature_lengths(768, 1024, 256, 4) == (4, 1, 4)
    for n_fft, hop, r in ((128, 32, 4), (512, 160, 3), (1024, 1024, 1)):
        for n in (0, n_fft // 2, n_fft // 2 + 1, 10 * hop - 1, 10 * hop, 99999):
            assert cf.feature_lengths(n, n_fft, hop, r) == C.lengths(n, n_fft, hop, r)


def test_byte_estimate_is_monotone():
    from spoofsv_amd import corpus_features as cf
    sizes = [cf.corpus_feature_bytes(B, 4 * 22050, CFG) for B in (1, 2, 8, 32, 33, 64)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    sizes = [cf.corpus_feature_bytes(32, n, CFG) for n in (1, 300, 22050, 22050 + 256, 8 * 22050, 60 * 22050)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[2] < sizes[-1]
    # resampling adds the resampled rows; 48 kHz input of the same DURATION costs what 22.05 kHz input does, plus those rows
    same = cf.corpus_feature_bytes(32, 8 * 22050, CFG)
    res = cf.corpus_feature_bytes(32, 8 * 48000, CFG, 48000)
    assert same < res <= same + 4 * 32 * (8 * 22050 + 256)
    # the three (B, ~n_fft, T_max) arrays dominate: frames, spectrum, magnitudes + their normalised copy
    B, T = 32, 1 + 8 * 22050 // 256
    assert same >= 4 * B * T * (1024 + 1026 + 513 + 80) + 4 * B * (T // 4) * (80 + 4 * 513)
    with pytest.raises(ValueError):
        cf.corpus_feature_bytes(0, 100, CFG)


def test_bad_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one, two = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(32)     # non-null dummies, never dereferenced: the checks come first
    err = L.ssv_last_error
    f = L.ssv_preemph_frames_ragged
    for args in ((null, one, two, one), (one, null, two, one), (one, one, null, one), (one, one, two, null), (one, one, one, one)):
        assert f(*args, 2, 1000, 1024, 256, 4, 0.97, null) == -1 and b"preemph_frames_ragged" in err()          # NULL / aliased pointers
    assert f(one, one, two, one, 0, 1000, 1024, 256, 4, 0.97, null) == -1                                           # B
    assert f(one, one, two, one, 2, 0, 1024, 256, 4, 0.97, null) == -1                                              # n_max
    assert f(one, one, two, one, 2, 1000, 0, 256, 4, 0.97, null) == -1                                              # n_fft
    assert f(one, one, two, one, 2, 1000, 1023, 256, 4, 0.97, null) == -1                                           # odd n_fft
    assert f(one, one, two, one, 2, 1000, 1024, 0, 4, 0.97, null) == -1                                             # hop
    assert f(one, one, two, one, 2, 1000, 1024, 2048, 4, 0.97, null) == -1                                          # hop > n_fft
    assert f(one, one, two, one, 2, 1000, 1024, 256, 0, 0.97, null) == -1                                           # T_max
    assert f(one, one, two, one, 2, 1000, 1024, 256, 3, 0.97, null) == -1 and b"T_max" in err()                     # < 1 + n_max / hop
    assert f(one, one, two, one, 2, 100000, 16384, 4096, 30, 0.97, null) == -2 and b"LDS" in err()                 # 16 frames do not fit
    g = L.ssv_corpus_normalize_pack
    ok = (2, 513, 80, 100, 25, 4)
    ptrs = [one, two, one, one, one, ctypes.c_void_p(48), ctypes.c_void_p(64), one]
    for k in (0, 1, 4, 5, 6, 7):
        bad = list(ptrs)
        bad[k] = null
        assert g(*bad, *ok, 0, 0.6, 20.0, 100.0, null) == -1 and b"corpus_normalize_pack" in err()
    assert g(one, two, null, one, one, ctypes.c_void_p(48), ctypes.c_void_p(64), one, *ok, 0, 0.6, 20.0, 100.0, null) == -1   # maxima are needed ...
    assert g(one, two, null, null, one, ctypes.c_void_p(48), ctypes.c_void_p(64), one, *ok, 1, 0.6, 20.0, 0.0, null) == -1    # ... or MAX_DB > 0
    for k in range(6):
        bad = list(ok)
        bad[k] = 0
        assert g(*ptrs, *bad, 0, 0.6, 20.0, 100.0, null) == -1
    assert g(*ptrs, 2, 513, 80, 100, 26, 4, 0, 0.6, 20.0, 100.0, null) == -1 and b"fit" in err()                   # r * RT_max > T_max
    assert g(*ptrs, *ok, 0, 0.0, 20.0, 100.0, null) == -1                                                           # power


def test_restatement_reduction_identity():
    """The restatement against itself: the reduced mel columns are columns 0, r, 2r, ... of the normalised mel, i.e. of the mel product of
    the columns ``lin[:, :r * rt][:, ::r]`` -- for the LOG_FEATURE normalisation, which is element-wise, that holds on the CACHE arrays."""
    rng = np.random.default_rng(3)
    sr, r = CFG["SAMPLING_RATE"], CFG["COARSE_MELSPEC"]["REDUCTION"]
    y = rng.standard_normal(9000) * np.hanning(9000)
    for log in (False, True):
        cfg = dict(CFG, LOG_FEATURE=log)
        f = C.features(y, cfg, sr, bounds=(100, 8900))
        T, rt = f["T"], f["rt"]
        assert (T, rt) == (1 + 8800 // 256, (1 + 8800 // 256) // r) and f["mel"].shape == (80, rt) and f["lin"].shape == (513, r * rt)
        cols = f["lin_mag"][:, :r * rt][:, ::r]
        assert cols.shape == (513, rt)
        mel_cols = C.mel_basis(cfg, sr) @ cols
        assert np.array_equal(mel_cols, f["mel_mag"][:, :r * rt][:, ::r]) or np.allclose(mel_cols, f["mel_mag"][:, :r * rt][:, ::r], rtol=1e-13, atol=0)
        lin_n, mel_n = C.normalise(f["lin_mag"], f["mel_mag"], cfg)
        assert np.array_equal(f["mel"], mel_n[:, :r * rt][:, ::r]) and np.array_equal(f["lin"], lin_n[:, :r * rt])
        if log:
            assert np.allclose(f["mel"], C.log_norm(mel_cols, cfg), rtol=1e-12, atol=0)
            assert f["lin"].min() >= 1e-8 and f["lin"].max() <= 1
        else:
            assert f["lin"].max() <= 1 and abs(lin_n.max() - 1) < 1e-15 and abs(mel_n.max() - 1) < 1e-15
    # pre-emphasis is relative to the segment, and a segment too short to reflect has no frames
    p = C.preemphasis(y[100:8900], 0.97)
    assert p[0] == y[100] and p[1] == y[101] - 0.97 * y[100]
    assert C.features(y[:512], CFG, sr, bounds=(0, 512))["T"] == 0 and C.features(y[:0], CFG, sr, bounds=(0, 0))["lin"].shape == (513, 0)
    pad = C.collate_pad([np.ones((3, 2)), np.ones((3, 5))])
    assert pad.shape == (2, 3, 5) and pad[0, :, 2:].sum() == 0 and pad[1].sum() == 15


def test_corpus_source_without_the_key_takes_the_old_path(tmp_path, monkeypatch):
    """CORPUS_FEATURES absent (or "cache"): missing cache entries go to ``extract_features``, and to nothing else."""
    from test_host_cpu import _make_corpus
    from spoofsv_amd import harness
    cfg, spec = _make_corpus(str(tmp_path), n_items=5, with_cache=False, wav=True)
    calls = []

    def fake(paths, c, cache):
        calls.append(("extract_features", list(paths), cache))
        for w in paths:                                          # what the real one leaves behind, so that iteration works
            os.makedirs(os.path.dirname(cache + w[-17:-4]), exist_ok=True)
            np.save(cache + w[-17:-4] + "_mel.npy", np.ones((80, 3), np.float32))
            np.save(cache + w[-17:-4] + "_lin.npy", np.ones((513, 12), np.float32))

    def never(*a, **k):
        raise AssertionError("the batched extraction was called without CORPUS_FEATURES")

    monkeypatch.setattr(harness, "extract_features", fake)
    monkeypatch.setattr(harness, "extract_features_batched", never)
    assert "CORPUS_FEATURES" not in cfg
    src = harness.CorpusSource(cfg, "train_ssrn", "conditional", "validate", 2, spec)
    assert len(calls) == 1 and calls[0][0] == "extract_features" and len(calls[0][1]) == 5 and calls[0][2] == spec
    assert src.features == "cache" and src.extractor is None
    b = next(iter(src))
    assert set(b) == {"data_0", "data_1"} and tuple(b["data_1"].shape) == (2, 513, 12) and not b["data_0"].is_cuda
    harness.CorpusSource(dict(cfg, CORPUS_FEATURES="cache"), "train_ssrn", "conditional", "validate", 2, spec)       # nothing missing now
    assert len(calls) == 1
    with pytest.raises(ValueError, match="CORPUS_FEATURES"):
        harness.CorpusSource(dict(cfg, CORPUS_FEATURES="gpu"), "train_ssrn", "conditional", "validate", 2, spec)


@pytest.mark.parametrize("mode", ["device", "batched"])
def test_device_and_batched_modes_do_not_fall_back_without_a_gpu(tmp_path, monkeypatch, no_gpu, mode):
    from test_host_cpu import _make_corpus
    from spoofsv_amd import harness
    cfg, spec = _make_corpus(str(tmp_path), n_items=3, with_cache=False, wav=True)

    def never(*a, **k):
        raise AssertionError("fell back to the per-utterance extraction")

    monkeypatch.setattr(harness, "extract_features", never)
    with pytest.raises(RuntimeError, match="needs a ROCm device"):
        harness.CorpusSource(dict(cfg, CORPUS_FEATURES=mode), "train_ssrn", "conditional", "train", 2, spec)
    assert not os.path.exists(spec) or not any(fs for _, _, fs in os.walk(spec))


def test_extractor_has_no_cpu_fallback(no_gpu):
    from spoofsv_amd.corpus_features import CorpusFeatureExtractor
    with pytest.raises(RuntimeError, match="needs a ROCm device"):
        CorpusFeatureExtractor(CFG, device="cpu")
    with pytest.raises(RuntimeError, match="needs a ROCm device"):
        CorpusFeatureExtractor(CFG)


def test_prefetcher_passes_device_tensors_through_and_finishes_on_the_consumer_thread():
    """``Prefetcher`` with a source whose ``device_features`` is true: ``host_batches`` runs on the background thread, ``finish_batch`` on
    the consuming one, and what ``finish_batch`` returns is yielded as it is (same tensor objects for the target device)."""
    import threading
    from spoofsv_amd import harness
    seen = {}

    class Src:
        device_features = True

        def __len__(self):
            return 2

        def host_batches(self):
            seen["host_thread"] = threading.get_ident()
            for i in range(2):
                yield {"_wav": torch.full((1, 4), float(i)), "_sr": 22050}

        def finish_batch(self, hb):
            seen["finish_thread"] = threading.get_ident()
            assert hb["_sr"] == 22050
            out = {"data_0": hb["_wav"] + 1}
            seen.setdefault("made", []).append(out["data_0"])
            return out

        def __iter__(self):
            raise AssertionError("a device-features source is read through host_batches")

    got = list(harness.Prefetcher(Src(), torch.device("cpu")))
    assert [float(g["data_0"][0, 0]) for g in got] == [1.0, 2.0]
    assert all(g["data_0"] is m for g, m in zip(got, seen["made"]))                      # unchanged: not copied, not re-wrapped
    assert seen["finish_thread"] == threading.get_ident() != seen["host_thread"]
    plain = list(harness.Prefetcher([{"data_0": torch.ones(2)}], torch.device("cpu")))    # a plain source: as before
    assert len(plain) == 1 and torch.equal(plain[0]["data_0"], torch.ones(2))
