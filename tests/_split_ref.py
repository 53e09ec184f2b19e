"""Float64 restatement of the reference's synthetic-data GE2E preprocessing (GE2E/synthetic_data_preprocess.py:13-52) in numpy, for the
tests only: ``librosa.effects.split`` of librosa 0.7.0 restated from its published algorithm (parity with the package itself is
unpinned), the per-interval slices, and the script's loop.  Nothing under ``spoofsv_amd/`` imports it and it imports nothing
from there; in particular it shares no code with ``vocoder.split_silence`` (per-frame Python loops here, no cumulative sums).
"""
import os

import numpy as np

import _sv_frontend_ref as R


def split(y, top_db=60.0, frame_length=2048, hop_length=512):
    """librosa.effects.split -> ((n, 2) int intervals, dB per frame).  An empty signal has no frame and no interval."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    if n == 0:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    pad = frame_length // 2
    yp = np.pad(y, pad, mode="reflect" if n > pad else "constant")
    n_frames = 1 + (len(yp) - frame_length) // hop_length
    mse = np.zeros(n_frames)
    for f in range(n_frames):
        fr = yp[f * hop_length:f * hop_length + frame_length]
        mse[f] = np.mean(np.abs(fr) ** 2)
    db = np.zeros(n_frames)
    for f in range(n_frames):
        db[f] = 10.0 * np.log10(max(1e-10, mse[f])) - 10.0 * np.log10(max(1e-10, mse.max()))
    out, begun = [], None
    for f in range(n_frames):                                    # frames_to_samples of the edges, clipped to the signal
        if db[f] > -top_db:
            if begun is None:
                begun = f
        elif begun is not None:
            out.append((min(n, begun * hop_length), min(n, f * hop_length)))
            begun = None
    if begun is not None:
        out.append((min(n, begun * hop_length), min(n, n_frames * hop_length)))
    return np.array(out, dtype=np.int64).reshape(-1, 2), db


def interval_slices(y16, top_db=30.0, sr=16000, nfft=512, window_s=0.025, hop_s=0.01, nmels=40, tisv_frame=120):
    """synthetic_data_preprocess.py:35-45 for one loaded utterance: ((k, 2, tisv_frame, nmels) frames-major features of the k intervals
    that are long enough, their (k, 2) bounds, all intervals)."""
    y16 = np.asarray(y16, dtype=np.float64)
    intervals, _ = split(y16, top_db)
    min_len = R.utter_min_len(sr, window_s, hop_s, tisv_frame)
    feats, kept = [], []
    for s, e in intervals:
        if (e - s) > min_len:                                    # :37, strict
            S, _ = R.log_mel(y16[s:e], sr, nfft, window_s, hop_s, nmels)
            feats.append(np.stack([S[:, :tisv_frame].T, S[:, -tisv_frame:].T]))
            kept.append((s, e))
    feats = np.stack(feats) if feats else np.zeros((0, 2, tisv_frame, nmels))
    return feats, np.array(kept, dtype=np.int64).reshape(-1, 2), intervals


def front_end(wavs, orig_sr, sr=16000, **kw):
    """The injectable form ``ge2e_harness.preprocess_tisv_synthetic(front_end=...)`` takes: per utterance a (k, 2, T, nmels) float32 array."""
    out = []
    for w in wavs:
        r = R.resample(w, orig_sr, sr).astype(np.float32).astype(np.float64)      # librosa.load returns float32
        out.append(interval_slices(r, sr=sr, **kw)[0].astype(np.float32))
    return out


def save_spectrogram_tisv_synthetic(speakers, read, train_path, test_path, sr=16000, **kw):
    """synthetic_data_preprocess.py:13-52; ``speakers``: ordered {name: [paths]}, ``read``: path -> (orig_sr, float waveform).  As the
    reference, a speaker without any slice is saved as ``np.array([])``."""
    os.makedirs(train_path, exist_ok=True)
    os.makedirs(test_path, exist_ok=True)
    train_speaker_num = (len(speakers) // 10) * 8                # :25
    tisv_frame = kw.get("tisv_frame", 120)
    for i, (_, files) in enumerate(speakers.items()):
        utterances_spec = []
        for path in files:
            if path[-4:] != ".wav":
                continue
            osr, y = read(path)
            utter = R.resample(y, osr, sr).astype(np.float32).astype(np.float64)
            intervals, _ = split(utter, 30)
            for s, e in intervals:
                if (e - s) > R.utter_min_len(sr, kw.get("window_s", 0.025), kw.get("hop_s", 0.01), tisv_frame):
                    S, _ = R.log_mel(utter[s:e], sr, kw.get("nfft", 512), kw.get("window_s", 0.025), kw.get("hop_s", 0.01), kw.get("nmels", 40))
                    utterances_spec.append(S[:, :tisv_frame].astype(np.float32))
                    utterances_spec.append(S[:, -tisv_frame:].astype(np.float32))
        arr = np.array(utterances_spec)
        if i < train_speaker_num:
            np.save(os.path.join(train_path, "speaker%d.npy" % i), arr)
        else:
            np.save(os.path.join(test_path, "speaker%d.npy" % (i - train_speaker_num)), arr)
