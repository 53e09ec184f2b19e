"""Float64 restatement of the reference's corpus feature extraction (data/dataset.py:94-118) and collate padding (:215-258) in numpy, for
the tests only.

librosa is not available to this project, so this file restates what data/dataset.py asks of it from its published algorithms; parity
with the package itself is unpinned.  It is test infrastructure: nothing under ``spoofsv_amd/`` imports it, and it imports
nothing from there.  The resampler, ``librosa.effects.trim``, the reflect framing, the explicit DFT and the Slaney mel filter bank are
those of ``tests/_sv_frontend_ref.py``.
"""
import numpy as np

import _sv_frontend_ref as R

TOP_DB = 22.0              # data/dataset.py:95


def lengths(n, n_fft, hop, r):
    """(T, rt, r * rt) for a trimmed segment of n samples; a segment of n <= n_fft // 2 samples cannot be reflect-padded: no frames."""
    T = 1 + n // hop if n > n_fft // 2 else 0
    return T, T // r, r * (T // r)


def trim(y):
    """librosa.effects.trim(y, 22) -> (start, end, dB of every frame against the loudest)."""
    return R.trim(y, TOP_DB)


def preemphasis(x, a):
    """np.append(speech[0], speech[1:] - preemph * speech[:-1]) (:96)."""
    x = np.asarray(x, dtype=np.float64)
    return np.append(x[0], x[1:] - a * x[:-1]) if len(x) else x


def frames(seg, n_fft, hop, a):
    """The DFT's input: centred, reflect-padded frames (n_fft, T) of the pre-emphasised segment."""
    return R.frames(preemphasis(seg, a), n_fft, hop)


def frame_rounding_bound(seg, n_fft, hop, a):
    """|x_i| + a |x_(i-1)| (0 for i = 0, which is copied) framed like the signal: times 2^-23, one fp32 rounding of the one subtraction."""
    x = np.abs(np.asarray(seg, dtype=np.float64))
    q = np.append(0.0, x[1:] + a * x[:-1]) if len(x) else x
    return R.frames(q, n_fft, hop)


def magnitudes(seg, cfg, sr):
    """(lin (F, T), mel (M, T)) before normalisation (:96-99); None, None for a segment without frames."""
    n_fft, hop = cfg["STFT"]["FFT_LENGTH"], cfg["STFT"]["HOP_LENGTH"]
    if lengths(len(seg), n_fft, hop, 1)[0] == 0:
        return None, None
    lin = np.abs(R.dft(frames(seg, n_fft, hop, cfg["PREEMPH"]), n_fft, n_fft))
    return lin, mel_basis(cfg, sr) @ lin


def mel_basis(cfg, sr):
    return R.mel_filterbank(sr, cfg["STFT"]["FFT_LENGTH"], cfg["COARSE_MELSPEC"]["FREQ_BINS"])


def log_norm(x, cfg):
    """:102-105 for either spectrogram."""
    return np.clip((20 * np.log10(np.maximum(1e-5, x)) - cfg["REF_DB"] + cfg["MAX_DB"]) / cfg["MAX_DB"], 1e-8, 1)


def normalise(lin, mel, cfg):
    """:101-112.  A maximum of 0 gives zeros here (the reference divides 0 by 0)."""
    if cfg.get("LOG_FEATURE", False):
        return log_norm(lin, cfg), log_norm(mel, cfg)
    p = cfg["NORM_POWER"]["ANALYSIS"]
    out = []
    for x in (lin, mel):
        m = x.max()
        out.append((x / m) ** p if m > 0 else np.zeros_like(x))
    return out[0], out[1]


def reduce(lin_n, mel_n, r):
    """:115-118 -> (reduced mel (M, rt), lin (F, r * rt))."""
    rt = mel_n.shape[1] // r
    return mel_n[:, [r * k for k in range(rt)]], lin_n[:, :r * rt]


def features(y, cfg, sr, bounds=None):
    """data/dataset.py:95-118 for one loaded waveform: dict with the trim bounds, T, rt, the raw magnitudes and the two cache arrays
    (``mel`` (M, rt), ``lin`` (F, r * rt); empty when the segment gives no frame)."""
    n_fft, hop, r = cfg["STFT"]["FFT_LENGTH"], cfg["STFT"]["HOP_LENGTH"], cfg["COARSE_MELSPEC"]["REDUCTION"]
    y = np.asarray(y, dtype=np.float64)
    start, end, db = trim(y) if bounds is None else (bounds[0], bounds[1], None)
    seg = y[start:end]
    T, rt, _ = lengths(len(seg), n_fft, hop, r)
    F, M = n_fft // 2 + 1, cfg["COARSE_MELSPEC"]["FREQ_BINS"]
    out = dict(start=start, end=end, db=db, T=T, rt=rt, lin_mag=None, mel_mag=None, mel=np.zeros((M, 0)), lin=np.zeros((F, 0)))
    if T == 0:
        return out
    lin, mel = magnitudes(seg, cfg, sr)
    assert lin.shape == (F, T)
    lin_n, mel_n = normalise(lin, mel, cfg)
    out["lin_mag"], out["mel_mag"] = lin, mel
    out["mel"], out["lin"] = reduce(lin_n, mel_n, r)
    return out


def from_file_rate(y, orig_sr, cfg):
    """metagen.py:29-62 then data/dataset.py: resample to SAMPLING_RATE (librosa.load returns float32), then ``features``."""
    sr = cfg["SAMPLING_RATE"]
    res = R.resample(y, orig_sr, sr).astype(np.float32).astype(np.float64) if int(orig_sr) != int(sr) else np.asarray(y, dtype=np.float64)
    return features(res, cfg, sr), res


def collate_pad(items):
    """collate_pad_2 / collate_pad_3 (:215-258) for one key: zero padding of (C, w_i) arrays to the widest, stacked."""
    w = max(it.shape[1] for it in items)
    out = np.zeros((len(items), items[0].shape[0], w), dtype=items[0].dtype)
    for b, it in enumerate(items):
        out[b, :, :it.shape[1]] = it
    return out
