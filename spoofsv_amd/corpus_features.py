"""Corpus spectrograms for ragged batches on the GPU: waveforms -> the collated (mel, linear) training batch.

Replaces ``data/dataset.py:94-118`` of the reference -- ``librosa.effects.trim(speech, 22)``, the pre-emphasis ``np.append``,
``np.abs(librosa.stft(n_fft, hop_length))``, ``np.dot(mel_filterbank, lin_spec)``, both normalisations (``LOG_FEATURE`` or per-utterance
maximum and ``NORM_POWER.ANALYSIS``) and the time reduction -- and the zero padding of ``collate_pad_2`` / ``collate_pad_3`` for B
utterances at once, with ``metagen.py:29-62``'s resampling in front when the files are not at ``SAMPLING_RATE``.  Waveforms are
``(B, n_max)`` float32 ROCm tensors with int32 live lengths ON THE DEVICE; every shape is static.

    resample (ssv_resample_sinc)  ->  trim bounds at 22 dB (ssv_trim_bounds)  ->  ssv_preemph_frames_ragged  ->  DFT (ssv_conv1d_fwd, k = 1)
    ->  ssv_complex_abs  ->  mel product (ssv_conv1d_fwd)  ->  [ssv_rowmax x 2]  ->  ssv_corpus_normalize_pack

The DFT of a batch is one product over B * T_max columns (32 x 690 = 22,080 at 8 s), where ``Vocoder.wav2spectrogram`` gives it one
utterance's few hundred.  It runs in exact fp32 (``dft_mode="fp32"``) by default, as in ``sv_frontend.TisvFrontEnd``: a row's result then
does not depend on its batch mates (the split-fp16 mode scales an operand tile by its own largest magnitude).
There is no CPU fallback: a non-ROCm tensor raises.
"""
import contextlib

import numpy as np
import torch

from . import _lib, ops
from .ops import _p
from .wave import Resampler, check_wave, fp32_products, resampled_width, rocm_device, trim_bounds

_F32, _I32 = torch.float32, torch.int32
TRIM_TOP_DB = 22.0        # data/dataset.py:95
_ALIGN = 64               # floats: every arena view starts on a 256-byte line


def feature_lengths(n, n_fft, hop, r):
    """(T, rt, r * rt) of a trimmed segment of ``n`` samples: T = 1 + n // hop centred frames (0 when n <= n_fft // 2: nothing to reflect
    from), rt = T // r reduced mel columns, r * rt linear columns (data/dataset.py:97,115-118)."""
    n = int(n)
    T = 1 + n // hop if n > n_fft // 2 else 0
    return T, T // r, r * (T // r)


def _dims(B, n_max, cfg, orig_sr=None):
    sr = int(cfg["SAMPLING_RATE"])
    N, hop = int(cfg["STFT"]["FFT_LENGTH"]), int(cfg["STFT"]["HOP_LENGTH"])
    r, M = int(cfg["COARSE_MELSPEC"]["REDUCTION"]), int(cfg["COARSE_MELSPEC"]["FREQ_BINS"])
    B, n_max = int(B), int(n_max)
    if B <= 0 or n_max <= 0:
        raise ValueError("need B > 0 and n_max > 0")
    resampled = orig_sr is not None and int(orig_sr) != sr
    m_max = resampled_width(n_max, orig_sr, sr) if resampled else n_max
    T_max = max(1 + m_max // hop, r)
    return dict(B=B, n_max=n_max, m_max=m_max, resampled=resampled, N=N, hop=hop, F=N // 2 + 1, M=M, r=r, T_max=T_max, RT_max=T_max // r)


def _buffers(d):
    """(name, element count) of the intermediate buffers of one call, in arena order; all 4-byte elements."""
    B, T = d["B"], d["T_max"]
    bufs = []
    if d["resampled"]:
        bufs += [("y_res", B * d["m_max"]), ("n_res", B)]
    bufs += [("bounds", 2 * B), ("n_frames", B), ("fr", B * d["N"] * T), ("spec", B * 2 * d["F"] * T), ("lin", B * d["F"] * T),
             ("mel", B * d["M"] * T), ("max_lin", B), ("max_mel", B)]
    return bufs


def _round(n):
    return -(-n // _ALIGN) * _ALIGN


def corpus_feature_bytes(B, n_max, cfg, orig_sr=None):
    """Device bytes one ``CorpusFeatureExtractor`` call on ``(B, n_max)`` waveforms holds: its intermediate buffers (frames, spectrum,
    magnitudes, mel, the resampled waveforms when ``orig_sr`` differs from SAMPLING_RATE) plus the three result tensors at their full
    width.  The Vocoder's bases (16 MB at n_fft = 1024) and the caller's waveforms are not counted.  Nearly all of it is the three
    (B, ~n_fft, T_max) arrays: 3.3 MB per second of audio and item at n_fft = 1024, hop = 256, 22,050 Hz."""
    return _total_bytes(_dims(B, n_max, cfg, orig_sr))


def _total_bytes(d):
    total = sum(_round(n) for _, n in _buffers(d))
    return 4 * (total + d["B"] * (d["M"] * d["RT_max"] + d["F"] * d["r"] * d["RT_max"] + 1))


class CorpusFeatureExtractor:
    """data/dataset.py's feature extraction for ragged batches on one ROCm device.  ``dft_mode``: "fp32" (default, exact, batch-independent)
    or "default" (the library's arithmetic mode in force, split-fp16 unless changed)."""

    def __init__(self, cfg, device="cuda", dft_mode="fp32"):
        if not torch.cuda.is_available():
            raise RuntimeError("spoofsv_amd.corpus_features: needs a ROCm device (no CPU fallback exists), got %s" % torch.device(device))
        dev = rocm_device(device, "corpus_features")
        if dft_mode not in ("fp32", "default"):
            raise ValueError("dft_mode must be 'fp32' or 'default'")
        from .vocoder import Vocoder
        self.cfg, self.device, self.dft_mode = cfg, dev, dft_mode
        self.sr = int(cfg["SAMPLING_RATE"])
        d = _dims(1, 1, cfg)
        self.n_fft, self.hop, self.F, self.M, self.r = d["N"], d["hop"], d["F"], d["M"], d["r"]
        self.preemph = float(cfg["PREEMPH"])
        self.log_feature = bool(cfg.get("LOG_FEATURE", False))
        self.power = float(cfg["NORM_POWER"]["ANALYSIS"])
        self.ref_db, self.max_db = float(cfg.get("REF_DB", 20)), float(cfg.get("MAX_DB", 100))
        self.voc = Vocoder(self.n_fft, self.hop, dev)                       # the Fourier bases and their resident planes
        self.w_mel = self.voc.mel_basis(self.sr, self.M)
        self.resampler = Resampler(self.sr, dev)
        self._arena = None
        self.nbytes = 0

    # ------------------------------------------------------------------ buffers
    def _views(self, d):
        """The intermediate buffers of a call as views of ONE arena, sized from (B, n_max) and kept: a call of the same shape gets the
        same views, a larger one replaces the arena (after asking whether the device has the memory)."""
        bufs = _buffers(d)
        need = sum(_round(n) for _, n in bufs)
        if self._arena is None or self._arena.numel() < need:
            total = _total_bytes(d)                                         # corpus_feature_bytes(B, n_max, cfg, orig_sr)
            self._arena = None                                              # the old arena's memory counts as free below
            ops.require_free_bytes(total, self.device, "CorpusFeatureExtractor on (B=%d, n_max=%d) waveforms needs" % (d["B"], d["n_max"]),
                                   "run fewer utterances per batch")
            self._arena = torch.empty((need,), dtype=_F32, device=self.device)
            self.nbytes = 4 * need
        out, off = {}, 0
        for name, n in bufs:
            v = self._arena[off:off + n]
            out[name] = v.view(_I32) if name in ("n_res", "bounds", "n_frames") else v
            off += _round(n)
        return out

    # ------------------------------------------------------------------ stages
    def _dft(self, w, x, out):
        with fp32_products() if self.dft_mode == "fp32" else contextlib.nullcontext():
            self.voc._dft(w, x, out)
        return out

    def _front(self, y, lengths, orig_sr, tick=lambda name: None):
        """Everything up to the maxima: returns (dims, views) with lin / mel / n_frames filled.  ``tick(name)`` is called after each stage
        has been issued (tools/bench_corpus_features.py synchronises there)."""
        check_wave(y, lengths, device=self.device)
        B, n_max = y.shape
        d = _dims(B, n_max, self.cfg, orig_sr)
        if d["resampled"]:
            self.resampler.bank(orig_sr, upload=False)                               # an unsupported ratio raises before anything is allocated
        v = self._views(d)
        st, T = ops._stream(), d["T_max"]
        if d["resampled"]:
            y, lengths = self.resampler.resample(y, lengths, orig_sr, out=v["y_res"].view(B, d["m_max"]), n_out=v["n_res"])
            tick("resample")
        trim_bounds(y, lengths, TRIM_TOP_DB, out=v["bounds"])
        tick("trim_bounds")
        fr = v["fr"].view(B, self.n_fft, T)
        _lib.call("ssv_preemph_frames_ragged", _p(y), _p(v["bounds"]), _p(fr), _p(v["n_frames"]), B, d["m_max"], self.n_fft, self.hop, T,
                  self.preemph, st)
        tick("preemph_frames_ragged")
        spec = self._dft(self.voc.w_fwd, fr, v["spec"].view(B, 2 * self.F, T))
        tick("dft")
        lin = v["lin"].view(B, self.F, T)
        _lib.call("ssv_complex_abs", _p(spec), _p(lin), B, self.F, T, st)
        tick("complex_abs")
        self._dft(self.w_mel, lin, v["mel"].view(B, self.M, T))
        tick("mel")
        if not self.log_feature:
            _lib.call("ssv_rowmax", _p(v["lin"]), _p(v["max_lin"]), B, self.F * T, st)
            _lib.call("ssv_rowmax", _p(v["mel"]), _p(v["max_mel"]), B, self.M * T, st)
            tick("rowmax x 2")
        return d, v

    def _split(self, flat, B, RT, i32):
        """The three views of a flat result [mel | lin | rt], a torch tensor or its numpy copy (``i32``: that library's int32)."""
        n_mel, n_lin = B * self.M * RT, B * self.F * self.r * RT
        return flat[:n_mel].reshape(B, self.M, RT), flat[n_mel:n_mel + n_lin].reshape(B, self.F, self.r * RT), flat[n_mel + n_lin:].view(i32)

    def _pack(self, d, v, RT):
        """One flat result tensor [mel | lin | rt] (so that a caller who wants the batch on the host copies once) and its three views."""
        B, r = d["B"], self.r
        flat = torch.empty((B * (self.M * RT + self.F * r * RT + 1),), dtype=_F32, device=self.device)
        mel, lin, rt = self._split(flat, B, RT, _I32)
        log = self.log_feature
        _lib.call("ssv_corpus_normalize_pack", _p(v["lin"]), _p(v["mel"]), None if log else _p(v["max_lin"]), None if log else _p(v["max_mel"]),
                  _p(v["n_frames"]), _p(mel), _p(lin), _p(rt), B, self.F, self.M, d["T_max"], RT, r, int(log), self.power, self.ref_db, self.max_db,
                  ops._stream())
        return flat, mel, lin, rt

    def resample(self, y, lengths, orig_sr):
        """The first stage alone: ((B, m_max) waveforms at SAMPLING_RATE, (B,) int32 lengths), fresh tensors (``metagen.py:29-62``)."""
        check_wave(y, lengths, device=self.device)
        if int(orig_sr) == self.sr:
            return y.clone(), lengths.clone()
        return self.resampler.resample(y, lengths, orig_sr)

    def trim_bounds(self, y, lengths):
        """``librosa.effects.trim(speech, 22)`` bounds of rows already at SAMPLING_RATE: (B, 2) int32."""
        return trim_bounds(y, lengths, TRIM_TOP_DB)

    def frames(self, y, bounds):
        """``ssv_preemph_frames_ragged`` alone: ((B, n_fft, T_max) frames, (B,) int32 frame counts), T_max = 1 + n_max // hop."""
        check_wave(y, bounds, bounds=True, device=self.device)
        B, n_max = y.shape
        T = 1 + n_max // self.hop
        fr = torch.empty((B, self.n_fft, T), dtype=_F32, device=y.device)
        nf = torch.empty((B,), dtype=_I32, device=y.device)
        _lib.call("ssv_preemph_frames_ragged", _p(y), _p(bounds), _p(fr), _p(nf), B, n_max, self.n_fft, self.hop, T, self.preemph, ops._stream())
        return fr, nf

    # ------------------------------------------------------------------ entry points
    def __call__(self, y, lengths, orig_sr, tick=lambda name: None):
        """``y`` (B, n_max) float32, ``lengths`` (B,) int32, both on the device -> (mel (B, M, RT_max), lin (B, F, r * RT_max), rt (B,) int32),
        RT_max = (1 + n_max' // hop) // r for n_max' the row width after resampling.  Item b is live in its first rt[b] / r * rt[b] columns
        and exactly zero after; a row too short to frame (or empty) is all zero with rt = 0.  No host synchronisation."""
        d, v = self._front(y, lengths, orig_sr, tick)
        out = self._pack(d, v, d["RT_max"])[1:]
        tick("corpus_normalize_pack")
        return out

    def to_host(self, y, lengths, orig_sr):
        """``__call__`` followed by ONE device-to-host copy of the whole result: numpy (mel, lin, rt)."""
        d, v = self._front(y, lengths, orig_sr)
        flat = self._pack(d, v, d["RT_max"])[0].cpu().numpy()
        return self._split(flat, d["B"], d["RT_max"], np.int32)

    def collated(self, y, lengths, orig_sr):
        """The batch as the collate functions pad it -- to its OWN longest item: (mel (B, M, w), lin (B, F, r * w), rt) with w = max(rt) (at
        least 1) and ``rt`` a host list.  The frame counts (B int32) are copied to the host once, after the transforms have been issued,
        to size the result; batch preparation only, never inside a captured graph."""
        d, v = self._front(y, lengths, orig_sr)
        rt = [int(t) // self.r for t in v["n_frames"].cpu().tolist()]
        _, mel, lin, _ = self._pack(d, v, max(1, min(max(rt), d["RT_max"])))
        return mel, lin, rt
