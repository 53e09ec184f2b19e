"""GPU speaker-verification front end: waveforms -> GE2E input features.

Replaces ``GE2E/data_preprocess.py:45-60`` of the reference -- ``librosa.core.load(path, sr)`` (resampy ``kaiser_best``),
``librosa.effects.trim(utter, 30)``, ``librosa.core.stft(n_fft=512, win_length=400, hop_length=160)``, ``np.abs(S) ** 2``,
``np.dot(mel_basis, S)``, ``np.log10(. + 1e-6)`` and the first / last ``tisv_frame`` frames -- for ragged batches: waveforms are
``(B, n_max)`` float32 ROCm tensors with int32 live lengths ON THE DEVICE.  No length is read on the host and every shape is static,
so the chain from the vocoder's output to the embedder's input runs without a host round trip and replays from a captured graph.

Only the 2 x ``tisv_frame`` frames the reference keeps are ever transformed.  The DFT is the library's 1x1 convolution
(``ssv_conv1d_fwd``) with a Fourier basis whose 400-sample periodic Hann window is zero-padded to 512 and centred, as librosa does
for ``win_length < n_fft``.  It runs in exact fp32 (``dft_mode="fp32"``) by default: the features are a LOGARITHM of squared
magnitudes, which magnifies the split modes' 2e-5-of-the-peak error in quiet bands, and the product is tiny.
``interval_slices`` / ``split_call`` are the same chain for ``GE2E/synthetic_data_preprocess.py:35-45``, which does not trim but keeps
the first / last ``tisv_frame`` frames of every interval of ``librosa.effects.split(utter, top_db=30)`` longer than ``utter_min_len``:
intervals, their selection across rows and the framing from the selected spans stay device tables of static shape.
There is no CPU fallback: a non-ROCm tensor raises.
"""
import contextlib

import numpy as np
import torch

from . import _lib, ops
from .ops import _p
from .vocoder import _slaney_mel
from .wave import (KAISER_BEST, Resampler, check_wave, fp32_products, polyphase_bank, rocm_device, sinc_table, split_intervals,  # noqa: F401 (re-exported)
                   trim_bounds)

_F32, _I32 = torch.float32, torch.int32


def stft_basis(n_fft, win_length):
    """Forward Fourier basis (2F, n_fft, 1) of ``librosa.stft(n_fft, win_length)``: a periodic Hann window of ``win_length`` samples
    zero-padded to ``n_fft`` and centred (librosa.util.pad_center), float32 from float64."""
    N, F = n_fft, n_fft // 2 + 1
    w = np.zeros(N)
    lpad = (N - win_length) // 2
    w[lpad:lpad + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    n = np.arange(N)
    ang = 2.0 * np.pi * ((np.arange(F)[:, None] * n[None, :]) % N) / N
    fwd = np.concatenate([np.cos(ang) * w[None, :], -np.sin(ang) * w[None, :]], 0)
    return np.ascontiguousarray(fwd, dtype=np.float32)[:, :, None]


def segment_peak(y, bounds, clip, peak=0.75):
    """generate_test_utterances.py:135-139 after the trim: (B, clip) rows y[start:end][:clip] / max * peak, zero-padded, and their lengths."""
    check_wave(y, bounds, bounds=True)
    B, n_max = y.shape
    out = torch.empty((B, int(clip)), dtype=_F32, device=y.device)
    n = torch.empty((B,), dtype=_I32, device=y.device)
    _lib.call("ssv_segment_peak", _p(y), _p(bounds), _p(out), _p(n), B, n_max, int(clip), float(peak), ops._stream())
    return out, n


class TisvFrontEnd:
    """data_preprocess.py's feature extraction on one ROCm device.  ``dft_mode``: "fp32" (default, exact) or "default" (the library's
    arithmetic mode in force, split-fp16 unless changed)."""

    def __init__(self, sr=16000, nfft=512, window=0.025, hop=0.01, nmels=40, tisv_frame=120, device="cuda", dft_mode="fp32"):
        dev = rocm_device(device, "sv_frontend")
        if dft_mode not in ("fp32", "default"):
            raise ValueError("dft_mode must be 'fp32' or 'default'")
        self.sr, self.nfft, self.nmels, self.tisv_frame, self.device, self.dft_mode = int(sr), int(nfft), int(nmels), int(tisv_frame), dev, dft_mode
        self.win_length, self.hop_length = int(window * sr), int(hop * sr)                     # data_preprocess.py:49
        if self.nfft % 2 or not 0 < self.win_length <= self.nfft or not 0 < self.hop_length <= self.nfft or self.tisv_frame <= 0:
            raise ValueError("need an even nfft, 0 < window * sr <= nfft, 0 < hop * sr <= nfft and tisv_frame > 0")
        self.utter_min_len = (tisv_frame * hop + window) * sr                                  # :25, a float, compared with a strict > (:48)
        self.min_len = int(np.floor(self.utter_min_len))                                       # len > x  <=>  len > floor(x) for integer len
        self.F = self.nfft // 2 + 1
        self.w_fwd = torch.from_numpy(stft_basis(self.nfft, self.win_length)).to(dev)
        self.mel = torch.from_numpy(np.ascontiguousarray(_slaney_mel(self.sr, self.nfft, self.nmels))).to(dev)
        self.resampler = Resampler(self.sr, dev)

    @classmethod
    def from_config(cls, ge2e_cfg, device=None, **kw):
        """From a ``ge2e_harness.default_config()`` dict (its ``data`` block) or that block itself."""
        d = ge2e_cfg.get("data", ge2e_cfg)
        dev = device or (ge2e_cfg.get("device", "cuda") if "data" in ge2e_cfg else "cuda")
        return cls(sr=d["sr"], nfft=d["nfft"], window=d["window"], hop=d["hop"], nmels=d["nmels"], tisv_frame=d["tisv_frame"], device=dev, **kw)

    # ------------------------------------------------------------------ stages
    def resample(self, y, lengths, orig_sr):
        """``librosa.load(path, sr)``'s resampling of every row: ((B, m_max) waveforms at ``sr``, (B,) int32 lengths)."""
        check_wave(y, lengths, device=self.device)
        return self.resampler.resample(y, lengths, orig_sr)

    def trim_bounds(self, y, lengths, top_db=30):
        return trim_bounds(y, lengths, top_db)

    def frames(self, y, bounds):
        """((2B, nfft, tisv_frame) frames of the first / last slices, (B,) int32 valid flags)."""
        check_wave(y, bounds, bounds=True, device=self.device)
        B, n_max = y.shape
        fr = torch.empty((2 * B, self.nfft, self.tisv_frame), dtype=_F32, device=y.device)
        valid = torch.empty((B,), dtype=_I32, device=y.device)
        _lib.call("ssv_tisv_frames", _p(y), _p(bounds), _p(fr), _p(valid), B, n_max, self.nfft, self.hop_length, self.tisv_frame, self.min_len,
                  ops._stream())
        return fr, valid

    def dft(self, fr):
        """(R, nfft, T) frames -> (R, 2F, T) spectra through the library's 1x1 convolution."""
        R, _, T = fr.shape
        S = torch.empty((R, 2 * self.F, T), dtype=_F32, device=fr.device)
        with fp32_products() if self.dft_mode == "fp32" else contextlib.nullcontext():
            ops._conv_fwd(fr, self.nfft * T, self.w_fwd, None, None, S, 2 * self.F * T, 1, 1, 0)
        return S

    def mel_log(self, S, out=None):
        """(R, 2F, T) spectra -> (R, T, nmels) log-mel frames; into ``out``, R * T * nmels contiguous floats, when given."""
        R, _, T = S.shape
        if out is None:
            out = torch.empty((R, T, self.nmels), dtype=_F32, device=S.device)
        elif not (out.dtype == _F32 and out.device == S.device and out.is_contiguous() and out.numel() == R * T * self.nmels):
            raise RuntimeError("spoofsv_amd.sv_frontend: mel_log's out must hold %d x %d x %d contiguous float32 on %s" % (R, T, self.nmels, S.device))
        _lib.call("ssv_power_mel_log", _p(S), _p(self.mel), _p(out), R, self.F, T, self.nmels, 1e-6, ops._stream())
        return out

    def slices(self, y, bounds):
        """Trimmed segments -> (features (B, 2, tisv_frame, nmels), valid (B,) int32): slice 0 the first ``tisv_frame`` frames of the
        log-mel spectrogram, slice 1 the last; rows no longer than ``utter_min_len`` ("Too short!!") have valid = 0."""
        fr, valid = self.frames(y, bounds)
        feats = self.mel_log(self.dft(fr))
        return feats.view(y.shape[0], 2, self.tisv_frame, self.nmels), valid

    def __call__(self, y, lengths, orig_sr):
        y16, n16 = self.resample(y, lengths, orig_sr)
        return self.slices(y16, self.trim_bounds(y16, n16, 30))

    # ------------------------------------------------------------------ voiced intervals (synthetic_data_preprocess.py:35-45)
    def select_spans(self, intervals, count, n_max, capacity, first=0):
        """The intervals longer than ``utter_min_len`` of a whole batch, in (row, interval) order: ((capacity, 3) int32 table of
        (row, start, end) holding the selected spans ``first .. first + capacity - 1``, (-1, 0, 0) after the last; (1,) int32 total)."""
        B, K, _ = intervals.shape
        table = torch.empty((int(capacity), 3), dtype=_I32, device=intervals.device)
        total = torch.empty((1,), dtype=_I32, device=intervals.device)
        _lib.call("ssv_select_spans", _p(intervals), _p(count), _p(table), _p(total), B, K, int(n_max), self.min_len, int(first), int(capacity),
                  ops._stream())
        return table, total

    def frames_table(self, y, table):
        """((2R, nfft, tisv_frame) frames of the first / last slices of the (R, 3) table's spans, (R,) int32 valid flags)."""
        B, n_max = y.shape
        R = table.shape[0]
        fr = torch.empty((2 * R, self.nfft, self.tisv_frame), dtype=_F32, device=y.device)
        valid = torch.empty((R,), dtype=_I32, device=y.device)
        _lib.call("ssv_tisv_frames_table", _p(y), _p(table), _p(fr), _p(valid), B, n_max, R, self.nfft, self.hop_length, self.tisv_frame, self.min_len,
                  ops._stream())
        return fr, valid

    def interval_slices(self, y, lengths, top_db=30, max_intervals=16, capacity=None, first=0):
        """synthetic_data_preprocess.py:35-45 for a ragged batch: ``librosa.effects.split(utter, top_db)`` of every row, every interval
        longer than ``utter_min_len`` in (row, interval) order, its first and last ``tisv_frame`` log-mel frames.  Returns (features
        (R, 2, tisv_frame, nmels), table (R, 3) int32 (row, start, end), valid (R,) int32, total (1,) int32, count (B,) int32), all on
        the device, R = ``capacity`` (default 2 B): the table holds the selected spans ``first .. first + R - 1`` and (-1, 0, 0) with
        valid = 0 after the last; ``total`` is the number of selected spans of the batch (``total > first + R``: call again with a
        larger ``first``), ``count[b]`` the number of intervals of row b (``count[b] > max_intervals``: some were not looked at).
        No length is read on the host and every shape is static."""
        check_wave(y, lengths, device=self.device)
        R = 2 * y.shape[0] if capacity is None else int(capacity)
        intervals, count = split_intervals(y, lengths, top_db, max_intervals)
        table, total = self.select_spans(intervals, count, y.shape[1], R, first)
        fr, valid = self.frames_table(y, table)
        feats = self.mel_log(self.dft(fr))
        return feats.view(R, 2, self.tisv_frame, self.nmels), table, valid, total, count

    def split_call(self, y, lengths, orig_sr, **kw):
        """``librosa.load(path, sr)``'s resampling, then ``interval_slices`` (its keywords pass through)."""
        y16, n16 = self.resample(y, lengths, orig_sr)
        return self.interval_slices(y16, n16, **kw)
