"""Float64 restatement of the reference's GE2E preprocessing (GE2E/data_preprocess.py:15-93) in numpy / scipy, for the tests only.

Neither librosa 0.7.0 nor resampy is available to this project, so this file restates what they compute from their published
algorithms; parity with the packages themselves is unpinned.  It is test infrastructure: nothing under ``spoofsv_amd/``
imports it, and it imports nothing from there -- the tests anchor it on what can be checked independently (numpy.fft, analytic tones,
``vocoder.trim_silence``, ``vocoder._slaney_mel``).

* ``resample``: resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') inside librosa.core.resample (fix_length to
  ceil(n * ratio), scale=False).  The filter is resampy's published 'kaiser_best': resampy.filters.sinc_window(num_zeros=64,
  precision=9, window=scipy.signal.kaiser(beta=14.769656459379492), rolloff=0.9475937167399596); the interpolation loop is
  resampy/interpn.py's (left wing over x[n - i], right wing over x[n + k + 1], linear interpolation between table entries).  Sample
  positions are the exact rationals t * orig / new where resampy accumulates ``time_register += 1 / ratio`` in float64.  The table
  stride is resampy 0.2.x's ``int(min(1, ratio) * 2^9)`` (371 for 22,050 -> 16,000 Hz, exact: 371.52), truncation included: the
  release contemporary with librosa 0.7.0, restated as it computes, not as it was later corrected.
* ``trim``: librosa.effects.trim (feature.rms on centred reflect-padded frames, power_to_db against the maximum, 1e-10 floor).
* ``stft``: librosa.core.stft with win_length < n_fft (periodic Hann, pad_center), as an explicit DFT.
* ``mel_filterbank``: librosa.filters.mel defaults (Slaney scale and normalisation).
"""
import os
from fractions import Fraction

import numpy as np
import scipy.signal

NUM_ZEROS, PRECISION, BETA, ROLLOFF = 64, 9, 14.769656459379492, 0.9475937167399596


def _kaiser_best():
    n = (2 ** PRECISION) * NUM_ZEROS
    sinc_win = ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, num=n + 1, endpoint=True))
    taper = scipy.signal.windows.kaiser(2 * n + 1, BETA)[n:]
    return taper * sinc_win, 2 ** PRECISION


def resample(x, orig_sr, sr, dtype=np.float64):
    """librosa.core.resample(x, orig_sr, sr) -- the body of librosa.load(path, sr).  ``dtype``: the arithmetic of the weighted sum (the
    table itself is always built in float64, as resampy ships it)."""
    x = np.asarray(x)
    if int(orig_sr) == int(sr):
        return x.astype(dtype).copy()
    ratio = float(sr) / float(orig_sr)
    n_fix = int(np.ceil(x.shape[0] * ratio))
    n_res = int(x.shape[0] * ratio)
    win, num_table = _kaiser_best()
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    r = Fraction(int(sr), int(orig_sr))
    up, down = r.numerator, r.denominator
    t = np.arange(n_res, dtype=np.int64)
    q = t * down
    n = q // up
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    nwin = win.shape[0]
    xs = x.astype(dtype)
    y = np.zeros(n_fix, dtype=dtype)
    frac = scale * ((q % up) / float(up))
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        idx = frac * num_table
        off = idx.astype(np.int64)
        eta = idx - off
        cnt = (nwin - off) // step
        for i in range(int(cnt.max()) if n_res else 0):
            src = n - i if wing == 0 else n + i + 1
            ok = (i < cnt) & (src >= 0) & (src < x.shape[0])
            w = (win[(off + i * step)[ok]] + eta[ok] * delta[(off + i * step)[ok]]).astype(dtype)
            y[:n_res][ok] += w * xs[src[ok]]
    return y


def trim(y, top_db=60.0, frame_length=2048, hop_length=512):
    """librosa.effects.trim -> (start, end)."""
    y = np.asarray(y, dtype=np.float64)
    pad = frame_length // 2
    yp = np.pad(y, pad, mode="reflect" if len(y) > pad else "constant")
    n_frames = 1 + (len(yp) - frame_length) // hop_length
    frames = np.stack([yp[f * hop_length:f * hop_length + frame_length] for f in range(n_frames)])
    mse = np.mean(np.abs(frames) ** 2, axis=1)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))
    nz = np.flatnonzero(db > -top_db)
    if nz.size == 0:
        return 0, 0, db
    return int(nz[0]) * hop_length, min(len(y), (int(nz[-1]) + 1) * hop_length), db


def window(n_fft, win_length):
    w = scipy.signal.get_window("hann", win_length, fftbins=True)
    lpad = (n_fft - win_length) // 2
    return np.pad(w, (lpad, n_fft - win_length - lpad), mode="constant")


def frames(y, n_fft, hop):
    yp = np.pad(np.asarray(y, dtype=np.float64), n_fft // 2, mode="reflect")
    T = 1 + (len(yp) - n_fft) // hop
    return np.stack([yp[t * hop:t * hop + n_fft] for t in range(T)], axis=1)          # (n_fft, T)


def dft(fr, n_fft, win_length):
    """Windowed real DFT of the columns of fr (n_fft, T) -> complex (F, T), as an explicit matrix product."""
    F = n_fft // 2 + 1
    k, n = np.arange(F)[:, None], np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * ((k * n) % n_fft) / n_fft
    basis = (np.cos(ang) - 1j * np.sin(ang)) * window(n_fft, win_length)[None, :]
    return basis @ fr


def stft(y, n_fft=512, hop=160, win_length=400):
    return dft(frames(y, n_fft, hop), n_fft, win_length)


def mel_filterbank(sr, n_fft, n_mels):
    """librosa.filters.mel(sr, n_fft, n_mels): Slaney mel scale, Slaney area normalisation, float64."""
    def hz_to_mel(f):
        f = np.asanyarray(f, dtype=np.float64)
        m = f / (200.0 / 3)
        log_t = f >= 1000.0
        return np.where(log_t, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) / (np.log(6.4) / 27.0), m)

    def mel_to_hz(m):
        m = np.asanyarray(m, dtype=np.float64)
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)

    fftfreqs = np.linspace(0, float(sr) / 2, 1 + n_fft // 2, endpoint=True)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(float(sr) / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def utter_min_len(sr=16000, window_s=0.025, hop_s=0.01, tisv_frame=120):
    return (tisv_frame * hop_s + window_s) * sr


def log_mel(utter, sr=16000, nfft=512, window_s=0.025, hop_s=0.01, nmels=40):
    """data_preprocess.py:49-52 for one trimmed utterance: (nmels, T) log-mel spectrogram and max |S|."""
    S = stft(utter, nfft, int(hop_s * sr), int(window_s * sr))
    P = np.abs(S) ** 2
    return np.log10(mel_filterbank(sr, nfft, nmels) @ P + 1e-6), np.abs(S)


def slices_of(utter, sr=16000, nfft=512, window_s=0.025, hop_s=0.01, nmels=40, tisv_frame=120):
    """data_preprocess.py:48-60 for one trimmed utterance: ((2, tisv_frame, nmels) frames-major features, valid)."""
    if not len(utter) > utter_min_len(sr, window_s, hop_s, tisv_frame):
        return np.zeros((2, tisv_frame, nmels)), False
    S, _ = log_mel(utter, sr, nfft, window_s, hop_s, nmels)
    return np.stack([S[:, :tisv_frame].T, S[:, -tisv_frame:].T]), True


def features(y, orig_sr, sr=16000, **kw):
    """librosa.load resampling, trim(30), slices: ((2, tisv_frame, nmels), valid, (start, end), resampled)."""
    r = resample(y, orig_sr, sr).astype(np.float32).astype(np.float64)          # librosa.load returns float32
    s, e, _ = trim(r, 30)
    f, v = slices_of(r[s:e], sr, **kw)
    return f, v, (s, e), r


def front_end(wavs, orig_sr, sr=16000, **kw):
    """The injectable form ``ge2e_harness.preprocess_tisv(front_end=...)`` takes: list of waveforms -> ((B, 2, T, nmels), (B,) bool)."""
    out = [features(w, orig_sr, sr, **kw)[:2] for w in wavs]
    return np.stack([o[0] for o in out]).astype(np.float32), np.array([o[1] for o in out], dtype=bool)


def _fill(specs, want):
    """data_preprocess.py:69-74 / :76-81: two random earlier entries per missing utterance, indices drawn below HALF the list's length."""
    have = len(specs)
    if 2 * want - have > 0:
        for _ in range(want - have // 2):
            a = np.random.randint(0, have // 2)
            b = np.random.randint(0, have // 2)
            specs.extend([specs[a], specs[b]])


def save_spectrogram_tisv(speakers, read, train_path, test_path, train_spk_num, enroll_num, eval_num, sr=16000, **kw):
    """data_preprocess.py:15-93; ``speakers``: ordered {name: [paths]}, ``read``: path -> (orig_sr, float waveform).
    ``np.random.randint`` is drawn from the global generator in the reference's order."""
    os.makedirs(train_path, exist_ok=True)
    os.makedirs(test_path, exist_ok=True)
    for i, (_, files) in enumerate(speakers.items()):
        utterances_spec, eval_spec = [], []
        utts_list = list(files)[:100] if i < train_spk_num else sorted(files, key=lambda x: os.path.basename(x)[:-4])      # :37-40
        for k, path in enumerate(utts_list):
            if path[-4:] != ".wav":
                continue
            osr, y = read(path)
            f, valid = features(y, osr, sr, **kw)[:2]
            if not valid:
                continue
            first, last = f[0].T.astype(np.float32), f[1].T.astype(np.float32)        # (nmels, frames) as S[:, :tisv_frame]
            (eval_spec if (i >= train_spk_num and k >= enroll_num) else utterances_spec).extend([first, last])
        if i >= train_spk_num:                                   # :66-83
            _fill(utterances_spec, enroll_num)
            _fill(eval_spec, eval_num)
            utterances_spec.extend(eval_spec)
        arr = np.array(utterances_spec)
        if i >= train_spk_num:
            assert arr.shape[0] == 2 * (enroll_num + eval_num)
            np.save(os.path.join(test_path, "speaker%d.npy" % (i - train_spk_num)), arr)
        else:
            np.save(os.path.join(train_path, "speaker%d.npy" % i), arr)
