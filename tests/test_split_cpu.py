"""CPU-only checks of the voiced-interval split (GE2E/synthetic_data_preprocess.py): ``vocoder.split_silence`` against the independent
float64 restatement (tests/_split_ref.py) and against ``trim_silence``, the bookkeeping of ``ge2e_harness.preprocess_tisv_synthetic``
with the restatement injected, and the argument checks of the three C-ABI entries."""
import ctypes
import os

import numpy as np
import pytest

import _split_ref as S
import _sv_frontend_ref as R
from spoofsv_amd import _lib

ENTRIES = ["ssv_split_intervals", "ssv_select_spans", "ssv_tisv_frames_table"]
T = 24                                                           # tisv_frame of the bookkeeping tests: intervals of ~4,240 samples are kept


def _bursts(rng, n, loud, level=1e-4):
    """Noise at ``level`` with noise of amplitude ~0.3 over every (start, end) of ``loud``."""
    y = level * rng.standard_normal(n)
    for s, e in loud:
        y[s:e] += 0.3 * rng.standard_normal(e - s)
    return y.astype(np.float32)


def _rows():
    rng = np.random.default_rng(5)
    return [_bursts(rng, 150000, [(5000, 30000), (41000, 70000), (73000, 100000), (118000, 140000)]),
            _bursts(rng, 64000, [(0, 20000), (33000, 64000)]),
            (0.3 * rng.standard_normal(50000)).astype(np.float32),           # all-loud
            np.zeros(20000, dtype=np.float32),                               # all-zero: the loudest frame passes, one interval (0, n)
            _bursts(rng, 700, [(100, 500)]),                                 # no longer than half a frame: zero padding
            _bursts(rng, 1500, [(200, 1200)]),
            _bursts(rng, 33333, [(3000, 9000), (20000, 33333)]),             # not a multiple of the hop: the last edge is clipped to n
            np.zeros(0, dtype=np.float32)]


def test_split_silence_equals_the_restatement_and_brackets_like_trim():
    from spoofsv_amd.vocoder import split_silence, trim_silence
    counts = []
    for y in _rows():
        for top_db in (30, 60):
            ref, _ = S.split(y, top_db)
            got = split_silence(y, top_db)
            assert got.shape == ref.shape and got.ndim == 2 and got.shape[1] == 2 and np.array_equal(got, ref), (len(y), top_db, got, ref)
            assert np.issubdtype(got.dtype, np.integer)
            bounds = trim_silence(y, top_db)[1]
            if len(got):
                assert (int(got[0, 0]), int(got[-1, 1])) == bounds == R.trim(y, top_db)[:2]
                assert np.all(got[:, 0] <= got[:, 1]) and np.all(got[1:, 0] > got[:-1, 1])      # ascending, runs apart
            else:
                assert len(y) == 0 and bounds == (0, 0)
        counts.append(len(S.split(y, 30)[0]))
    assert counts == [4, 2, 1, 1, 1, 1, 2, 0]
    assert split_silence(np.zeros(0, dtype=np.float32), 30).shape == (0, 2)
    assert split_silence(np.zeros(20000, dtype=np.float32), 30).tolist() == [[0, 20000]]
    assert split_silence(_rows()[6], 30)[-1, 1] == 33333


# ------------------------------------------------------------------------------------------ bookkeeping
def _write(path, y, sr=16000):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, np.asarray(y, dtype=np.float32))


def _tail_interval(rng, length):
    """A file whose LAST voiced interval has exactly ``length`` samples: quiet, then loud up to the end of the file (the only edge that
    is no multiple of the hop is the one clipped to n).  The interval's first frame is found on a long file, then the file is cut."""
    y = _bursts(rng, 20000, [(6000, 20000)])
    start = int(S.split(y, 30)[0][-1, 0])
    y = y[:start + length]
    iv = S.split(y, 30)[0]
    assert len(iv) == 1 and tuple(iv[0]) == (start, start + length)
    return y


def _speakers(tmp_path):
    rng = np.random.default_rng(6)
    ml = int(np.floor(R.utter_min_len(tisv_frame=T)))            # the largest integer length that :37 drops
    assert not ml > R.utter_min_len(tisv_frame=T) and ml + 1 > R.utter_min_len(tisv_frame=T)
    waves = {
        "spk0": [_bursts(rng, 16000, [(0, 6000), (9500, 16000)]), _bursts(rng, 27000, [(1000, 7500), (12000, 14000), (19000, 26000)])],
        "spk1": [_tail_interval(rng, ml), _tail_interval(rng, ml + 1)],
        "spk2": [_bursts(rng, 3000, [(0, 3000)])],               # too short: a speaker without any slice
    }
    for s in range(3, 10):
        waves["spk%d" % s] = [_bursts(rng, 9000 + 100 * s, [(1000, 8000)])]
    speakers = {}
    for name, ws in waves.items():
        speakers[name] = []
        for k, w in enumerate(ws):
            p = str(tmp_path / "wav" / name / ("u%02d.wav" % k))
            _write(p, w)
            speakers[name].append(p)
    speakers["spk2"].append(str(tmp_path / "wav" / "spk2" / "notes.txt"))     # not a wav: skipped (:32)
    return speakers, waves


def _cfg(tmp_path, name):
    from spoofsv_amd import ge2e_harness
    c = ge2e_harness.default_config()
    c["data"]["train_path"], c["data"]["test_path"] = str(tmp_path / name / "train"), str(tmp_path / name / "test")
    c["data"]["tisv_frame"] = T
    return c


def _fe(wavs, orig_sr):
    return S.front_end(wavs, orig_sr, tisv_frame=T)


def test_preprocess_tisv_synthetic_bookkeeping_with_the_restatement_injected(tmp_path):
    from spoofsv_amd import ge2e_harness
    speakers, waves = _speakers(tmp_path)
    for n_spk, n_train in ((10, 8), (7, 0)):                     # (total // 10) * 8
        spk = dict(list(speakers.items())[:n_spk])
        cfg, cfg_r = _cfg(tmp_path, "mine%d" % n_spk), _cfg(tmp_path, "ref%d" % n_spk)
        written = ge2e_harness.preprocess_tisv_synthetic(cfg, spk, front_end=_fe)
        S.save_spectrogram_tisv_synthetic(spk, ge2e_harness.read_wav, cfg_r["data"]["train_path"], cfg_r["data"]["test_path"], tisv_frame=T)
        want = ["train/speaker%d.npy" % i for i in range(n_train)] + ["test/speaker%d.npy" % i for i in range(n_spk - n_train)]
        assert [os.sep.join(p.split(os.sep)[-2:]) for p in written] == want
        for sub in ("train", "test"):
            names = sorted(os.listdir(cfg["data"]["%s_path" % sub]))
            assert names == sorted(os.listdir(cfg_r["data"]["%s_path" % sub])) and len(names) == (n_train if sub == "train" else n_spk - n_train)
            for nm in names:
                a, b = np.load(os.path.join(cfg["data"]["%s_path" % sub], nm)), np.load(os.path.join(cfg_r["data"]["%s_path" % sub], nm))
                if b.size == 0:                                  # the one stated difference: the reference's np.array([]) has shape (0,)
                    assert b.shape == (0,) and a.shape == (0, 40, T) and a.dtype == np.float32
                else:
                    assert a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a, b), (sub, nm)
    by_index = [np.load(p) for p in written]                     # the 7-speaker run: speaker i is test/speaker<i>.npy
    # file, then interval, then first before last: spk0 has 2 + 2 kept intervals (the 2,000-sample burst of its second file is dropped)
    f0, kept0, all0 = S.interval_slices(waves["spk0"][0], tisv_frame=T)
    f1, kept1, all1 = S.interval_slices(waves["spk0"][1], tisv_frame=T)
    assert (len(kept0), len(all0), len(kept1), len(all1)) == (2, 2, 2, 3)
    order = [f0[0, 0], f0[0, 1], f0[1, 0], f0[1, 1], f1[0, 0], f1[0, 1], f1[1, 0], f1[1, 1]]
    assert by_index[0].shape == (8, 40, T)
    for got, ref in zip(by_index[0], order):
        assert np.array_equal(got, ref.T.astype(np.float32))
    assert not np.array_equal(by_index[0][0], by_index[0][1])
    # the strict compare of :37: an interval of floor(utter_min_len) samples is dropped, one sample more is kept
    assert by_index[1].shape == (2, 40, T)
    assert np.array_equal(by_index[1][0], S.interval_slices(waves["spk1"][1], tisv_frame=T)[0][0, 0].T.astype(np.float32))
    assert by_index[2].shape == (0, 40, T)                       # the empty speaker
    ds = ge2e_harness.SpeakerDatasetPreprocessed(cfg["data"]["test_path"], 2, utter_start=0)
    assert ds.file_list[0] == "speaker0.npy" and np.load(os.path.join(ds.path, "speaker0.npy")).shape[1:] == (40, T)


def test_preprocess_tisv_synthetic_raises_on_more_intervals_than_max_intervals(tmp_path):
    from spoofsv_amd import ge2e_harness
    speakers, _ = _speakers(tmp_path)
    with pytest.raises(RuntimeError, match=r"u00\.wav has 2 voiced intervals"):
        ge2e_harness.preprocess_tisv_synthetic(_cfg(tmp_path, "over"), {"spk0": speakers["spk0"]}, front_end=_fe, max_intervals=1)
    with pytest.raises(ValueError, match="device tuple"):
        ge2e_harness.preprocess_tisv_synthetic(_cfg(tmp_path, "tuple"), {"spk0": (None, None, 16000)}, front_end=_fe)


# ------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_split_entries():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIBPATH)
    for name, nargs in zip(ENTRIES, (11, 11, 12)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert hasattr(L, name), name
    assert _lib.lib().ssv_version() == 7                         # additions only


def test_bad_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # `one`: non-null dummy, never dereferenced: the checks come first
    err = L.ssv_last_error
    assert L.ssv_split_intervals(null, one, one, one, 1, 100, 16, 30.0, 2048, 512, null) == -1 and b"split_intervals" in err()
    assert L.ssv_split_intervals(one, one, one, null, 1, 100, 16, 30.0, 2048, 512, null) == -1
    assert L.ssv_split_intervals(one, one, one, one, 0, 100, 16, 30.0, 2048, 512, null) == -1
    assert L.ssv_split_intervals(one, one, one, one, 1, 100, 0, 30.0, 2048, 512, null) == -1                       # K <= 0
    assert L.ssv_split_intervals(one, one, one, one, 1, 100, 16, 30.0, 2048, 4096, null) == -1                     # hop > frame_length
    assert L.ssv_split_intervals(one, one, one, one, 1, 1 << 30, 16, 30.0, 2048, 512, null) == -2 and b"frames per row" in err()
    assert L.ssv_split_intervals(one, one, one, one, 1, 8192 * 512, 16, 30.0, 2048, 512, null) == -2               # 8193 frames
    assert L.ssv_select_spans(one, one, null, one, 1, 16, 100, 10, 0, 2, null) == -1 and b"select_spans" in err()
    assert L.ssv_select_spans(one, one, one, one, 1, 16, 100, 10, -1, 2, null) == -1                               # first < 0
    assert L.ssv_select_spans(one, one, one, one, 1, 16, 100, 10, 0, 0, null) == -1                                # R <= 0
    assert L.ssv_select_spans(one, one, one, one, 1 << 20, 1 << 12, 100, 10, 0, 2, null) == -2
    assert L.ssv_tisv_frames_table(one, null, one, one, 1, 100, 2, 512, 160, 120, 19600, null) == -1 and b"tisv_frames_table" in err()
    assert L.ssv_tisv_frames_table(one, one, one, one, 1, 100, 0, 512, 160, 120, 19600, null) == -1                # R <= 0
    assert L.ssv_tisv_frames_table(one, one, one, one, 1, 100, 2, 512, 600, 120, 99999, null) == -1                # hop > n_fft
    assert L.ssv_tisv_frames_table(one, one, one, one, 1, 100, 2, 512, 160, 120, 100, null) == -1 and b"min_len" in err()
    assert L.ssv_tisv_frames_table(one, one, one, one, 1, 100, 2, 2048, 512, 24, 20000, null) == -2 and b"LDS tile" in err()   # 63 * 512 + 2048 floats


def test_no_cpu_fallback():
    import torch
    from spoofsv_amd import sv_frontend
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sv_frontend.split_intervals(torch.zeros(1, 100), torch.tensor([100], dtype=torch.int32))
