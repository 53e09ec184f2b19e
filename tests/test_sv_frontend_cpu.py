"""CPU-only checks of the speaker-verification front end (csrc/sv_frontend.hip, spoofsv_amd.sv_frontend, ge2e_harness.preprocess_tisv):
the C ABI's new entries, the float64 restatement the GPU tests compare against (tests/_sv_frontend_ref.py) anchored on what can be
checked without librosa / resampy, the host-built polyphase bank, and the preprocessing bookkeeping with the restatement injected."""
import ctypes
import os

import numpy as np
import pytest

import _sv_frontend_ref as R
from spoofsv_amd import _lib

ENTRIES = ["ssv_resample_sinc", "ssv_trim_bounds", "ssv_tisv_frames", "ssv_power_mel_log", "ssv_segment_peak"]
# The float64 restatement's own error on pure tones, 22,050 -> 16,000 Hz, amplitude 1, 0.5 s, 2,000 samples away from each end
# (profiles/round8_sv_frontend.txt); the bars are these figures times 2: they pin the restatement, not the kernels.
# Both are ~6e-4, not the filter's design stop band: resampy 0.2.x walks its table in steps of int(ratio * 512) = 371 entries where the
# exact stride is 371.52, which stretches the filter by 0.14 % -- restated as it is, since that is what the reference ran.
TONE_1K_ERR = 6.052e-4         # max |resampled - analytic 1 kHz tone|
TONE_9K_LEAK = 6.429e-4        # max |resampled 9 kHz tone| (above the new Nyquist frequency)


def test_header_declares_and_library_exports_the_new_entries():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIBPATH)
    for name in ENTRIES:
        assert name in protos, name
        assert hasattr(L, name), name
    assert _lib.lib().ssv_version() == 7


def test_bad_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # `one`: non-null dummy, never dereferenced: the checks come first
    err = L.ssv_last_error
    assert L.ssv_resample_sinc(one, one, one, ctypes.c_void_p(32), one, 0, 100, 100, 320, 441, 178, 88, null) == -1 and b"resample_sinc" in err()
    assert L.ssv_resample_sinc(one, one, null, ctypes.c_void_p(32), one, 1, 100, 100, 320, 441, 178, 88, null) == -1        # no bank
    assert L.ssv_resample_sinc(one, one, one, ctypes.c_void_p(32), one, 1, 100, 50, 320, 441, 178, 88, null) == -1 and b"m_max" in err()
    # 44,100 -> 44,101 Hz: 44,101 phases
    assert L.ssv_resample_sinc(one, one, one, ctypes.c_void_p(32), one, 1, 100, 101, 44101, 44100, 130, 64, null) == -2 and b"ratio" in err()
    assert L.ssv_trim_bounds(one, one, one, 0, 100, 30.0, 2048, 512, null) == -1 and b"trim_bounds" in err()
    assert L.ssv_trim_bounds(one, one, one, 1, 100, 30.0, 2048, 4096, null) == -1
    assert L.ssv_trim_bounds(one, one, one, 1, 1 << 30, 30.0, 2048, 512, null) == -2
    assert L.ssv_tisv_frames(one, one, one, one, 0, 100, 512, 160, 120, 19600, null) == -1 and b"tisv_frames" in err()
    assert L.ssv_tisv_frames(one, one, one, one, 1, 100, 512, 600, 120, 99999, null) == -1                                   # hop > n_fft
    assert L.ssv_tisv_frames(one, one, one, one, 1, 100, 512, 160, 0, 19600, null) == -1                                     # tisv_frame <= 0
    assert L.ssv_tisv_frames(one, one, one, one, 1, 100, 512, 160, 120, 100, null) == -1 and b"min_len" in err()
    assert L.ssv_power_mel_log(one, one, one, 0, 257, 120, 40, 1e-6, null) == -1 and b"power_mel_log" in err()
    assert L.ssv_power_mel_log(one, one, one, 1, 4097, 120, 40, 1e-6, null) == -2
    assert L.ssv_segment_peak(one, one, ctypes.c_void_p(32), one, 0, 100, 10, 0.75, null) == -1 and b"segment_peak" in err()


def test_unsupported_ratio_raises_on_the_host():
    from spoofsv_amd import sv_frontend
    with pytest.raises(ValueError, match="unsupported"):
        sv_frontend.polyphase_bank(44100, 44101)


def test_no_cpu_fallback():
    import torch
    from spoofsv_amd import sv_frontend
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sv_frontend.trim_bounds(torch.zeros(1, 100), torch.tensor([100], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sv_frontend.TisvFrontEnd(device="cpu")


def test_config_carries_the_reference_keys():
    from spoofsv_amd import ge2e_harness
    d = ge2e_harness.default_config()["data"]
    assert (d["sr"], d["nfft"], d["window"], d["hop"], d["nmels"], d["tisv_frame"]) == (16000, 512, 0.025, 0.01, 40, 120)


# ------------------------------------------------------------------------------------------ anchors of the restatement
def test_restated_dft_is_rfft_of_the_windowed_padded_frame():
    rng = np.random.default_rng(0)
    y = rng.standard_normal(3000)
    S = R.stft(y, 512, 160, 400)
    yp = np.pad(y, 256, mode="reflect")
    w = np.zeros(512)
    w[56:456] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400)
    assert S.shape == (257, 1 + 3000 // 160)
    for t in (0, 1, 7, S.shape[1] - 1):
        ref = np.fft.rfft(yp[t * 160:t * 160 + 512] * w)
        assert np.abs(S[:, t] - ref).max() <= 1e-11 * np.abs(ref).max()


def test_stft_basis_of_the_package_is_the_restated_one():
    from spoofsv_amd import sv_frontend
    b = sv_frontend.stft_basis(512, 400)[:, :, 0].astype(np.float64)
    fr = np.random.default_rng(1).standard_normal((512, 3))
    S = R.dft(fr, 512, 400)
    got = b @ fr
    assert np.abs(got[:257] - S.real).max() < 1e-5 and np.abs(got[257:] - S.imag).max() < 1e-5       # float32 basis entries


def _bursts(rng, n, lead, tail, level=1e-4):
    y = level * rng.standard_normal(n)
    y[lead:n - tail] += rng.standard_normal(n - lead - tail) * np.hanning(n - lead - tail)
    return y.astype(np.float32)


def test_restated_trim_equals_trim_silence():
    from spoofsv_amd.vocoder import trim_silence
    rng = np.random.default_rng(2)
    for n, lead, tail in [(30000, 5000, 7000), (83200, 12345, 20000), (2500, 300, 400), (1000, 100, 100), (600, 0, 0), (40000, 0, 9000)]:
        y = _bursts(rng, n, lead, tail)
        for top_db in (30, 22, 60):
            s, e, _ = R.trim(y, top_db)
            assert (s, e) == trim_silence(y, top_db)[1], (n, top_db)
    assert R.trim(np.zeros(0, dtype=np.float32), 30)[:2] == trim_silence(np.zeros(0, dtype=np.float32), 30)[1] == (0, 0)
    assert R.trim(np.zeros(5000, dtype=np.float32), 30)[:2] == trim_silence(np.zeros(5000, dtype=np.float32), 30)[1]


def test_restated_filterbank_is_slaney_mel():
    from spoofsv_amd.vocoder import _slaney_mel
    fb = R.mel_filterbank(16000, 512, 40)
    ref = _slaney_mel(16000, 512, 40)
    assert fb.shape == ref.shape == (40, 257)
    assert np.abs(fb - ref).max() <= 1e-7 * np.abs(ref).max()                                        # ref is rounded to float32


def _tone(freq, sr, n):
    return np.sin(2 * np.pi * freq * np.arange(n) / sr)


def test_restated_resampler_on_pure_tones():
    n = 11025
    y1 = R.resample(_tone(1000.0, 22050, n), 22050, 16000)
    assert y1.shape[0] == int(np.ceil(n * (16000 / 22050)))
    e1 = np.abs(y1 - _tone(1000.0, 16000, y1.shape[0]))[2000:-2000].max()
    e9 = np.abs(R.resample(_tone(9000.0, 22050, n), 22050, 16000))[2000:-2000].max()
    print("restatement 22050 -> 16000: 1 kHz tone error %.3e, 9 kHz leak %.3e" % (e1, e9))
    assert e1 <= 2 * TONE_1K_ERR and e9 <= 2 * TONE_9K_LEAK
    assert np.array_equal(R.resample(np.arange(5.0), 16000, 16000), np.arange(5.0))


def test_polyphase_bank_reproduces_the_direct_evaluation():
    from spoofsv_amd import sv_frontend
    rng = np.random.default_rng(3)
    for orig, new, n in [(22050, 16000, 5000), (22050, 16000, 441), (8000, 16000, 1500), (48000, 16000, 4000), (22050, 16000, 37)]:
        x = rng.standard_normal(n)
        bank, up, down, left = sv_frontend.polyphase_bank(orig, new)
        ref = R.resample(x, orig, new)
        ratio = float(new) / orig
        n_res, n_fix = int(n * ratio), int(np.ceil(n * ratio))
        taps = bank.shape[1]
        xp = np.concatenate([np.zeros(left), x, np.zeros(taps + down)])
        t = np.arange(n_res)
        q = t * down
        cols = (q // up)[:, None] + np.arange(taps)[None, :]                 # x[n - left + j] in the padded signal
        y = np.zeros(n_fix)
        y[:n_res] = np.einsum("tj,tj->t", bank[q % up], xp[cols])
        assert y.shape == ref.shape
        assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max(), (orig, new, n)


# ------------------------------------------------------------------------------------------ bookkeeping
def _write(path, y, sr):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, y.astype(np.float32))


def test_preprocess_tisv_bookkeeping_with_the_restatement_injected(tmp_path):
    from spoofsv_amd import ge2e_harness
    rng = np.random.default_rng(4)
    sr = 16000                                                   # equal rates: the resampler is a copy, lengths are exact
    # data_preprocess.py:25 in floats: (120 * 0.01 + 0.025) * 16000 = 19599.999999999996, so the strict > of :48 KEEPS 19,600 samples
    assert 19599 < R.utter_min_len() < 19600
    min_len = 19600
    speakers = {}
    for s in range(4):
        files = []
        for k in range(6 if s != 3 else 5):
            n = 24000 + 1000 * k
            y = rng.standard_normal(n)                           # loud throughout: trim keeps everything
            if s == 2 and k == 1:
                y = y[:min_len - 1]                              # the longest length that is too short
            if s == 2 and k in (2, 3):
                y = y[:min_len + k - 2]                          # 19,600 (utter_min_len as the config's numbers read) and 19,601: kept
            p = str(tmp_path / "wav" / ("spk%d" % s) / ("u%02d.wav" % k))
            _write(p, 0.1 * y, sr)
            files.append(p)
        speakers["spk%d" % s] = files
    speakers["spk1"].append(str(tmp_path / "wav" / "spk1" / "notes.txt"))     # not a wav: skipped, but it counts in k (:41-43)
    for p in speakers["spk2"][1:4]:
        n = len(ge2e_harness.read_wav(p)[1])
        s_, e_, _ = R.trim(ge2e_harness.read_wav(p)[1], 30)
        assert (s_, e_) == (0, n)                                # the too-short rule is tested at exactly these lengths

    def cfg_for(name):
        c = ge2e_harness.default_config()
        c["data"]["train_path"], c["data"]["test_path"] = str(tmp_path / name / "train"), str(tmp_path / name / "test")
        return c

    calls = []

    def fe(wavs, orig_sr):
        calls.append((len(wavs), orig_sr))
        return R.front_end(wavs, orig_sr)

    enroll_num, eval_num = 4, 3
    cfg = cfg_for("mine")
    np.random.seed(11)
    written = ge2e_harness.preprocess_tisv(cfg, speakers, 2, enroll_num, eval_num, front_end=fe)
    cfg_r = cfg_for("ref")
    np.random.seed(11)
    R.save_spectrogram_tisv(speakers, ge2e_harness.read_wav, cfg_r["data"]["train_path"], cfg_r["data"]["test_path"], 2, enroll_num, eval_num)
    assert calls == [(6, sr), (6, sr), (6, sr), (5, sr)]         # one batch per speaker
    assert [os.path.basename(p) for p in written] == ["speaker0.npy", "speaker1.npy", "speaker0.npy", "speaker1.npy"]
    for sub in ("train", "test"):
        names = sorted(os.listdir(cfg["data"]["%s_path" % sub]))
        assert names == ["speaker0.npy", "speaker1.npy"] == sorted(os.listdir(cfg_r["data"]["%s_path" % sub]))
        for nm in names:
            a, b = np.load(os.path.join(cfg["data"]["%s_path" % sub], nm)), np.load(os.path.join(cfg_r["data"]["%s_path" % sub], nm))
            assert a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a, b), (sub, nm)
    tr0 = np.load(os.path.join(cfg["data"]["train_path"], "speaker0.npy"))
    assert tr0.shape == (12, 40, 120)                            # 6 utterances x (first, last), (slices, nmels, frames)
    te0 = np.load(os.path.join(cfg["data"]["test_path"], "speaker0.npy"))      # spk2: k = 1 dropped -> 3 enrol utterances + 1 duplicated, 2 eval + 1
    assert te0.shape == (2 * (enroll_num + eval_num), 40, 120)
    f, v = R.front_end([ge2e_harness.read_wav(p)[1] for p in speakers["spk2"]], sr)
    assert list(v) == [True, False, True, True, True, True]
    assert np.array_equal(te0[0], f[0, 0].T) and np.array_equal(te0[1], f[0, 1].T) and np.array_equal(te0[2], f[2, 0].T)
    assert np.array_equal(te0[8], f[4, 0].T)                     # evaluation block starts after 2 * enroll_num slices: utterance k = 4
    np.random.seed(11)                                           # the duplication draws, in the reference's order
    draws = [np.random.randint(0, 3) for _ in range(2)]
    enrol = [f[0, 0], f[0, 1], f[2, 0], f[2, 1], f[3, 0], f[3, 1]]
    assert np.array_equal(te0[6], enrol[draws[0]].T) and np.array_equal(te0[7], enrol[draws[1]].T)
    ds = ge2e_harness.SpeakerDatasetPreprocessed(cfg["data"]["test_path"], 6)
    assert tuple(ds[0].shape) == (6, 120, 40)                    # the existing loader reads it unchanged
