"""Float32 emulation of the vocoder chain on ``scipy.fft`` and the bar rule of the FFT back end's tests.  TEST INFRASTRUCTURE ONLY.

The emulation is what a careful complex64 implementation leaves against the float64 oracle (oracle/vocoder_oracle.py): float32 frames
give complex64 spectra (scipy.fft keeps single precision), the overlap-add runs in float32 in the order of ``vocoder_oracle.istft``, and
the Griffin-Lim loop runs in complex64.  The bar for a given input is TEN TIMES the emulation's own worst error against the oracle on
that same input, relative to the oracle's peak (the house rule: a bar is ten times the measurement) -- computed from the two references
alone, never from the code under test.  Measured here: 1.1e-7 .. 1.7e-7 for one transform, 1.6e-7 .. 3.0e-7 after one Griffin-Lim
iteration, 3.5e-7 .. 8.6e-7 after four, so the bars come out near 1.5e-6, 3e-6 and 9e-6.
"""
import numpy as np
import scipy.fft

from oracle import vocoder_oracle as vo

F32, C64 = np.float32, np.complex64


def window32(n_fft):
    return vo.hann_periodic(n_fft).astype(F32)


def stft32(y, n_fft=1024, hop=256):
    """vocoder_oracle.stft on float32 samples: (F, T) complex64."""
    y = np.asarray(y, dtype=F32)
    w = window32(n_fft)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    T = 1 + (len(yp) - n_fft) // hop
    out = np.empty((1 + n_fft // 2, T), dtype=C64)
    for t in range(T):
        out[:, t] = scipy.fft.rfft(w * yp[t * hop:t * hop + n_fft])
    assert out.dtype == C64
    return out


def inverse_frames32(S, n_fft):
    """windowed inverse frames (T, N) float32 of a complex64 spectrum (F, T)"""
    S = np.asarray(S, dtype=C64)
    w = window32(n_fft)
    fr = np.stack([w * scipy.fft.irfft(S[:, t], n_fft) for t in range(S.shape[1])])
    assert fr.dtype == F32
    return fr


def overlap_add32(fr, hop):
    """float32 overlap-add of frames (T, N) in increasing frame index, envelope, centre trim: vocoder_oracle.istft from its loop on"""
    T, n_fft = fr.shape
    y = np.zeros(n_fft + hop * (T - 1), dtype=F32)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += fr[t]
    env = vo.window_sumsquare(T, n_fft, hop)
    nz = env > np.finfo(np.float32).tiny
    y[nz] /= env[nz].astype(F32)
    return y[n_fft // 2:-(n_fft // 2)]


def istft32(S, hop=256):
    n_fft = 2 * (S.shape[0] - 1)
    return overlap_add32(inverse_frames32(S, n_fft), hop)


def griffinlim32(S, angles0, n_iter, hop=256, momentum=0.99):
    """vocoder_oracle.griffinlim in complex64 / float32"""
    n_fft = 2 * (S.shape[0] - 1)
    S = np.asarray(S, dtype=F32)
    angles = np.asarray(angles0, dtype=C64)
    alpha = F32(momentum / (1 + momentum))
    rebuilt = None
    for _ in range(n_iter):
        tprev = rebuilt
        rebuilt = stft32(istft32(S * angles, hop), n_fft, hop)
        angles = rebuilt - alpha * tprev if tprev is not None else rebuilt
        angles = (angles / (np.abs(angles) + F32(1e-16))).astype(C64)
    return istft32(S * angles, hop)


def rel_err(got, ref):
    """worst error relative to the reference's peak"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def bar(emulation, oracle):
    """ten times the emulation's own worst error against the float64 oracle on this input, relative to the oracle's peak"""
    return 10.0 * rel_err(emulation, oracle)


def packed(c):
    """complex (..., F, T) -> (..., 2F, T): real rows, then imaginary rows"""
    return np.concatenate([c.real, c.imag], -2)


# the shapes the single-transform figures above were measured at: (n_fft, hop, T)
SHAPES = ((1024, 256, 25), (128, 32, 22), (512, 160, 30), (2048, 512, 9))


def wave(rng, n):
    return (rng.randn(n) * np.hanning(n) * 0.3).astype(F32)
