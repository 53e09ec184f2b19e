"""The waveform stages every GPU front end shares (``sv_frontend``, ``dvector``, ``corpus_features``): the argument check of a ragged
``(B, n_max)`` float32 batch with int32 device lengths or bounds, the device lookup of a constructor, resampy's ``kaiser_best``
resampling (``ssv_resample_sinc`` and its polyphase filter banks), ``librosa.effects.trim``'s bounds (``ssv_trim_bounds``),
``librosa.effects.split``'s intervals (``ssv_split_intervals``) and the switch to exact fp32 for one product.  There is no CPU fallback: a non-ROCm tensor raises.
"""
import contextlib
from fractions import Fraction

import numpy as np
import torch

from . import _lib, ops
from .ops import _p

_F32, _I32 = torch.float32, torch.int32

# resampy's 'kaiser_best' filter as published with resampy (resampy/filters.py, data/kaiser_best.npz): a Kaiser-windowed sinc of 64 zero
# crossings sampled 2^9 times per crossing
KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)
_BANK_MAX = 1 << 20       # up * taps (ssv_resample_sinc)
_SPAN_MAX = 8192


def rocm_device(device, who):
    """``torch.device(device)`` with its index filled in, for the constructor of ``spoofsv_amd.<who>``; anything but a ROCm device raises."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("spoofsv_amd.%s: needs a ROCm device (no CPU fallback exists), got %s" % (who, dev))
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


@contextlib.contextmanager
def fp32_products():
    """The library's products in exact fp32 inside the block.  The arithmetic mode is a process-global of the library
    (``ssv_set_precision``), read when a call is issued: it is switched here and put back.  Correct for one issuing thread, and under
    capture (the kernel is chosen at capture time); another thread that issues library calls inside the block would run them in fp32
    as well, so callers keep feature extraction on the thread that trains."""
    prev = _lib.lib().ssv_set_precision(0)
    try:
        yield
    finally:
        _lib.lib().ssv_set_precision(prev)


def check_wave(y, ints, bounds=False, device=None):
    """``ints``: the rows' live lengths (B,), or with ``bounds`` their (start, end) pairs (B, 2); ``device``: where the caller's constants live."""
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == _F32 and y.dim() == 2 and y.is_contiguous() and y.shape[0] > 0 and y.shape[1] > 0):
        raise RuntimeError("spoofsv_amd.wave: waveforms must be a contiguous float32 ROCm tensor (B, n_max); no CPU fallback exists")
    if device is not None and y.device != device:
        raise RuntimeError("spoofsv_amd.wave: waveforms are on %s, this front end's bases and filter banks on %s" % (y.device, device))
    want = (y.shape[0], 2) if bounds else (y.shape[0],)
    if not (torch.is_tensor(ints) and ints.dtype == _I32 and ints.is_contiguous() and tuple(ints.shape) == want and ints.device == y.device):
        raise RuntimeError("spoofsv_amd.wave: %s must be a contiguous int32 tensor %s on the waveforms' device, got %s"
                           % ("bounds" if bounds else "lengths", want, (tuple(ints.shape), ints.dtype, ints.device) if torch.is_tensor(ints) else type(ints)))


def sinc_table(num_zeros, precision, beta, rolloff):
    """resampy.filters.sinc_window with a Kaiser window: the right half of the filter, num_zeros * 2^precision + 1 samples (float64)."""
    n = (1 << precision) * num_zeros
    sinc = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    return np.kaiser(2 * n + 1, beta)[n:] * sinc


def polyphase_bank(orig_sr, sr, filt=None):
    """The (up, taps) float64 filter bank of ``resampy.resample(x, orig_sr, sr)`` for the rational ratio up / down = sr / orig_sr, and
    ``left``: tap j of phase p weighs x[n - left + j] for the output at input time n + p / up.  resampy's inner loops (interpolation
    between table entries, the ``min(1, ratio)`` stretch of the table index and of the gain) are evaluated once per phase here instead
    of once per output sample there; entries its loops never reach are zero.  Returns (bank, up, down, left)."""
    r = Fraction(int(sr), int(orig_sr))
    up, down = r.numerator, r.denominator
    f = dict(KAISER_BEST, **(filt or {}))
    win = sinc_table(f["num_zeros"], f["precision"], f["beta"], f["rolloff"])
    ratio = float(sr) / float(orig_sr)
    num_table = 1 << f["precision"]
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    nwin = win.shape[0]
    reach = nwin // step + 1
    if up * (2 * reach) > _BANK_MAX or 255 * down // up + 2 * reach + 2 > _SPAN_MAX:
        raise ValueError("spoofsv_amd.wave: the ratio %d/%d (%d Hz -> %d Hz) needs a filter bank of %d x %d taps; unsupported"
                         % (up, down, orig_sr, sr, up, 2 * reach))
    left = reach - 1
    bank = np.zeros((up, 2 * reach), dtype=np.float64)
    for p in range(up):
        frac = scale * (p / up)                                   # left wing: x[n - i]
        idx = frac * num_table
        off = int(idx)
        eta = idx - off
        i = np.arange((nwin - off) // step)
        bank[p, left - i] = win[off + i * step] + eta * delta[off + i * step]
        frac = scale - frac                                       # right wing: x[n + k + 1]
        idx = frac * num_table
        off = int(idx)
        eta = idx - off
        k = np.arange((nwin - off) // step)
        bank[p, left + 1 + k] = win[off + k * step] + eta * delta[off + k * step]
    return bank, up, down, left


def resampled_width(n_max, orig_sr, sr):
    """m_max = ceil(n_max * up / down) for up / down = sr / orig_sr in lowest terms, in double as ``ssv_resample_sinc`` checks it."""
    r = Fraction(int(sr), int(orig_sr))
    return int(np.ceil(n_max * (float(r.numerator) / float(r.denominator))))


class Resampler:
    """``librosa.load(path, sr)``'s resampling (resampy ``kaiser_best``) to the rate ``sr`` on one device: the float32 filter banks, kept
    by source rate, and the ``ssv_resample_sinc`` call."""

    def __init__(self, sr, device):
        self.sr, self.device = int(sr), device
        self._banks = {}

    def bank(self, orig_sr, upload=True):
        """[bank, up, down, left, taps] of a source rate.  Built on the host -- ``ValueError`` for a ratio the kernel's tiles cannot take,
        which ``upload=False`` gives before anything is uploaded or allocated -- and uploaded once.  Equal rates have no bank (taps = 0:
        the kernel copies)."""
        key = int(orig_sr)
        b = self._banks.get(key)
        if b is None:
            if key == self.sr:
                b = [None, 1, 1, 0, 0]
            else:
                bank, up, down, left = polyphase_bank(key, self.sr)
                b = [np.ascontiguousarray(bank, dtype=np.float32), up, down, left, bank.shape[1]]
            self._banks[key] = b
        if upload and isinstance(b[0], np.ndarray):
            b[0] = torch.from_numpy(b[0]).to(self.device)
        return b

    def resample(self, y, lengths, orig_sr, out=None, n_out=None):
        """Every row of ``y`` (B, n_max) at ``orig_sr`` -> ((B, ``resampled_width``) waveforms at ``sr``, (B,) int32 lengths); into ``out`` / ``n_out`` when given."""
        w, up, down, left, taps = self.bank(orig_sr)
        B, n_max = y.shape
        m_max = resampled_width(n_max, orig_sr, self.sr)
        out = out if out is not None else torch.empty((B, m_max), dtype=_F32, device=y.device)
        n_out = n_out if n_out is not None else torch.empty((B,), dtype=_I32, device=y.device)
        _lib.call("ssv_resample_sinc", _p(y), _p(lengths), _p(w), _p(out), _p(n_out), B, n_max, m_max, up, down, taps, left, ops._stream())
        return out, n_out


def trim_bounds(y, lengths, top_db=30.0, frame_length=2048, hop_length=512, out=None):
    """``librosa.effects.trim(y, top_db)`` bounds of every row (the device form of ``vocoder.trim_silence``): (B, 2) int32 (start, end);
    into ``out`` (2 B int32) when given."""
    check_wave(y, lengths)
    B, n_max = y.shape
    bounds = out if out is not None else torch.empty((B, 2), dtype=_I32, device=y.device)
    _lib.call("ssv_trim_bounds", _p(y), _p(lengths), _p(bounds), B, n_max, float(top_db), int(frame_length), int(hop_length), ops._stream())
    return bounds


def split_intervals(y, lengths, top_db=30.0, max_intervals=16, frame_length=2048, hop_length=512):
    """``librosa.effects.split(y, top_db)`` intervals of every row (the device form of ``vocoder.split_silence``): ((B, max_intervals, 2)
    int32 (start, end) pairs in ascending order, (0, 0) from ``min(count, max_intervals)`` on; (B,) int32 count).  ``count`` is the true
    number of intervals of a row: ``count > max_intervals`` tells the caller that some were not stored.  The frame energies are those
    of ``trim_bounds``, so a row's first start and last end are its trim bounds."""
    check_wave(y, lengths)
    B, n_max = y.shape
    K = int(max_intervals)
    intervals = torch.empty((B, K, 2), dtype=_I32, device=y.device)
    count = torch.empty((B,), dtype=_I32, device=y.device)
    _lib.call("ssv_split_intervals", _p(y), _p(lengths), _p(intervals), _p(count), B, n_max, K, float(top_db), int(frame_length), int(hop_length),
              ops._stream())
    return intervals, count
