"""GPU parity of the vocoder's FFT back end (Vocoder(transform="fft"), csrc/fft.hip) against oracle/vocoder_oracle.py.

Bars: for every input, ten times the worst error of the float32 emulation in tests/_fft_vocoder_ref.py against the float64 oracle on that
same input, relative to the oracle's peak -- near 1.5e-6 for one transform, 3e-6 after one Griffin-Lim iteration, 9e-6 after four.  Each
figure is printed before it is asserted; the worst ones measured on an MI355X are in profiles/fft_vocoder.txt.
"""
import json
import os

import numpy as np
import pytest
import torch

import _fft_vocoder_ref as R
from oracle import vocoder_oracle as vo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = json.load(open(os.path.join(ROOT, "config.json")))
GUARD = 4096
_VOC = {}


def _voc(n_fft=1024, hop=256, transform="fft"):
    from spoofsv_amd.vocoder import Vocoder
    key = (n_fft, hop, transform)
    if key not in _VOC:
        _VOC[key] = Vocoder(n_fft, hop, transform=transform)
    return _VOC[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _pack(c):
    return _dev(R.packed(c))


class Guarded:
    """An output buffer filled with NaN with a guard band behind it: after the call every element is written and the band is untouched."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.flat = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.flat[n:] = 12345.0
        self.t = self.flat[:n].view(*shape)

    def check(self, what):
        n = self.t.numel()
        assert bool(torch.isfinite(self.flat[:n]).all()), "%s: elements left unwritten" % what
        assert bool((self.flat[n:] == 12345.0).all()), "%s: wrote behind its output" % what
        return self.t


def _tile(n_fft):
    from spoofsv_amd import _lib
    return int(_lib.lib().ssv_fft_frame_tile(n_fft))


def _shape_cases():
    t = _tile(1024)
    for T in (4, t - 1, t, t + 1, 67):                 # T = 4: the shortest the reflect padding allows; T <= tile: first tile = last tile
        yield 1024, 256, 256 * (T - 1)
    yield 128, 32, 32 * 21 + 7                         # no multiple of hop
    yield 512, 160, 160 * 29                           # hop does not divide n_fft (the GE2E front end's setting)
    yield 2048, 512, 512 * 8
    yield 64, 16, 16 * 39


@pytest.mark.parametrize("n_fft,hop,n", list(_shape_cases()))
def test_stft_istft_match_oracle_and_write_exactly_their_outputs(n_fft, hop, n):
    from spoofsv_amd import _lib, ops
    from spoofsv_amd.vocoder import _p
    v = _voc(n_fft, hop)
    B, F, T = 3, n_fft // 2 + 1, 1 + n // hop
    rng = np.random.RandomState(n_fft + n)
    y = np.stack([R.wave(rng, n) for _ in range(B)])
    st, yd = ops._stream(), _dev(y)
    # forward
    ref = np.stack([vo.stft(y[b], n_fft, hop) for b in range(B)])
    emu = np.stack([R.stft32(y[b], n_fft, hop) for b in range(B)])
    spec = Guarded(B, 2 * F, T)
    _lib.call("ssv_stft_fft", _p(yd), _p(v._tab), _p(spec.t), B, n, n_fft, hop, T, st)
    S = spec.check("stft_fft")
    assert torch.equal(v.stft(yd), S) and tuple(S.shape) == (B, 2 * F, T)
    e, b = R.rel_err(S.cpu().numpy(), R.packed(ref)), R.bar(emu, ref)
    print("stft (%d, %d, T=%d): %.2e, bar %.2e" % (n_fft, hop, T, e, b))
    assert e <= b
    e = R.rel_err(v.magnitude(S).cpu().numpy(), np.abs(ref))
    assert e <= b
    # inverse of an inconsistent spectrum whose DC and Nyquist rows carry imaginary parts, which count for nothing
    z = (rng.randn(B, F, T) + 1j * rng.randn(B, F, T)).astype(np.complex64)
    refi = np.stack([vo.istft(z[b].astype(np.complex128), hop) for b in range(B)])
    emui = np.stack([R.istft32(z[b], hop) for b in range(B)])
    zd = _pack(z)
    fr, out = Guarded(B, T, n_fft), Guarded(B, hop * (T - 1))
    _lib.call("ssv_istft_frames_fft", _p(zd), _p(v._tab), _p(fr.t), B, n_fft, T, st)
    _lib.call("ssv_ola_signal_fm", _p(fr.check("istft_frames_fft")), _p(v._inv_env(T)), _p(out.t), B, n_fft, T, hop, st)
    yi = out.check("ola_signal_fm")
    assert torch.equal(v.istft(zd), yi) and tuple(yi.shape) == refi.shape
    z0 = z.copy()
    z0[:, 0].imag = 0
    z0[:, -1].imag = 0
    assert torch.equal(v.istft(_pack(z0)), yi)
    e, b = R.rel_err(yi.cpu().numpy(), refi), R.bar(emui, refi)
    print("istft (%d, %d, T=%d): %.2e, bar %.2e" % (n_fft, hop, T, e, b))
    assert e <= b
    # the Griffin-Lim step on the same frames: both outputs written in full, nothing behind them
    mag = _dev(rng.rand(B, F, T))
    reb, proj = Guarded(B, 2 * F, T), Guarded(B, 2 * F, T)
    _lib.call("ssv_gl_step_fft", _p(fr.t), _p(v._inv_env(T)), _p(v._tab), _p(mag), None, 0.0, _p(reb.t), _p(proj.t), B, n_fft, T, hop, st)
    refr = np.stack([vo.stft(refi[b], n_fft, hop) for b in range(B)])
    emur = np.stack([R.stft32(emui[b], n_fft, hop) for b in range(B)])
    e, b = R.rel_err(reb.check("gl_step_fft reb").cpu().numpy(), R.packed(refr)), R.bar(emur, refr)
    print("rebuilt spectrum (%d, %d, T=%d): %.2e, bar %.2e" % (n_fft, hop, T, e, b))
    assert e <= b
    pr = proj.check("gl_step_fft proj")
    # |proj| = mag: the phase step normalises.  Two square roots, a division, two products and a sum of squares, each within an ulp or two
    # of 6e-8: 16 ulp of the peak bounds them (|a| is nowhere near the 1e-16 of the denominator here)
    assert R.rel_err(v.magnitude(pr).cpu().numpy(), mag.cpu().numpy()) <= 16 * 2.0 ** -24
    # exact reconstruction
    back = v.istft(S).cpu().numpy()
    emub = np.stack([R.istft32(emu[b], hop) for b in range(B)])
    yt = y[:, :hop * (T - 1)]
    e, b = R.rel_err(back, yt), R.bar(emub, yt)
    print("istft(stft(y)) (%d, %d, T=%d): %.2e, bar %.2e" % (n_fft, hop, T, e, b))
    assert e <= b


@pytest.fixture(scope="module")
def gl_refs():
    """Oracle and emulation of 1 and 4 Griffin-Lim iterations, computed once: {(n_fft, hop, T): (mag, a0, {it: (oracle, emulation)})}"""
    out = {}
    for n_fft, hop, T in ((1024, 256, 25), (512, 160, 30)):
        rng = np.random.RandomState(7 + n_fft)
        B, F = 3, n_fft // 2 + 1
        mag = np.abs(np.stack([vo.stft(R.wave(rng, hop * (T - 1)), n_fft, hop) for _ in range(B)])).astype(np.float32)
        a0 = vo.random_angles((B, F, T), rng).astype(np.complex64)
        its = {}
        for it in (1, 4):
            o = np.stack([vo.griffinlim(mag[b].astype(np.float64), a0[b].astype(np.complex128), it, hop) for b in range(B)])
            e = np.stack([R.griffinlim32(mag[b], a0[b], it, hop) for b in range(B)])
            its[it] = (o, e)
        out[(n_fft, hop, T)] = (mag, a0, its)
    return out


@pytest.mark.parametrize("n_fft,hop,T", [(1024, 256, 25), (512, 160, 30)])
def test_griffinlim_matches_oracle_after_1_and_4_iterations(gl_refs, n_fft, hop, T):
    v = _voc(n_fft, hop)
    mag, a0, its = gl_refs[(n_fft, hop, T)]
    for it in (1, 4):
        o, emu = its[it]
        g = v.griffinlim(_dev(mag), _pack(a0), it).cpu().numpy()
        e, b = R.rel_err(g, o), R.bar(emu, o)
        print("griffinlim (%d, %d, T=%d) %d iterations: %.2e, bar %.2e" % (n_fft, hop, T, it, e, b))
        assert e <= b, (it, e, b)


def test_griffinlim_64_iterations_converge_as_far_as_the_oracle(gl_refs):
    v = _voc()
    mag, a0, _ = gl_refs[(1024, 256, 25)]
    tr_o, tr_g = [], []
    w = vo.griffinlim(mag[0].astype(np.float64), a0[0].astype(np.complex128), 64, trace=tr_o)
    g = v.griffinlim(_dev(mag[:1]), _pack(a0[:1]), 64, trace=tr_g).cpu().numpy()[0]
    print("inconsistency first %.3e last %.3e (oracle last %.3e), waveform %.2e of the peak" % (tr_g[0], tr_g[-1], tr_o[-1], R.rel_err(g, w)))
    assert len(tr_g) == 64
    assert tr_g[-1] <= 1.1 * tr_o[-1] and tr_g[-1] < 0.25 * tr_g[0]
    assert np.abs(g - w).max() <= 2e-2 * np.abs(w).max()


def test_the_two_back_ends_agree_on_the_same_inputs(gl_refs):
    f, d = _voc(transform="fft"), _voc(transform="dft")
    mag, a0, _ = gl_refs[(1024, 256, 25)]
    rng = np.random.RandomState(3)
    y = _dev(np.stack([R.wave(rng, 256 * 24) for _ in range(3)]))
    Sf, Sd = f.stft(y), d.stft(y)
    assert R.rel_err(Sf.cpu().numpy(), Sd.cpu().numpy()) <= 2e-5
    z = _dev(rng.randn(3, 1026, 25))
    assert R.rel_err(f.istft(z).cpu().numpy(), d.istft(z).cpu().numpy()) <= 2e-5
    gf, gd = f.griffinlim(_dev(mag), _pack(a0), 1), d.griffinlim(_dev(mag), _pack(a0), 1)
    assert R.rel_err(gf.cpu().numpy(), gd.cpu().numpy()) <= 2e-5
    assert not hasattr(f, "w_fwd") and not hasattr(f, "_planes")         # the GEMM bases are not built


def test_bitwise_replay_repeat_and_arithmetic_mode():
    from spoofsv_amd import _lib
    v = _voc()
    rng = np.random.RandomState(9)
    B, T = 3, 30
    S = _dev(rng.rand(B, 513, T))
    for seed in (1, 2):                         # the second call replays the cached graph on new inputs
        a0 = _pack(vo.random_angles((B, 513, T), np.random.RandomState(seed)))
        eager = v.griffinlim(S, a0, 6)
        assert torch.equal(v.griffinlim_graph(S, a0, 6), eager)
        assert torch.equal(v.griffinlim(S, a0, 6), eager)
        S = S * 0.5 + 0.1
    y = _dev(np.stack([R.wave(rng, 256 * (T - 1)) for _ in range(B)]))
    L = _lib.lib()
    prev = L.ssv_get_precision()
    try:
        res = []
        for p in (0, 1, 2):
            L.ssv_set_precision(p)
            sp = v.stft(y)
            res.append((sp, v.istft(sp), v.griffinlim(S, a0, 3)))
    finally:
        L.ssv_set_precision(prev)
    for r in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, res[0]))


def test_reference_call_sequences():
    """spectrogram2wav and wav2spectrogram as tests/test_gpu_vocoder.py holds them for the basis path: 1e-4; 2e-5."""
    v = _voc()
    rng = np.random.RandomState(11)
    B, T = 2, 20
    lin = rng.rand(B, 513, T).astype(np.float32)
    a0 = vo.random_angles((B, 513, T), rng)

    def ref(l, a):
        spec = (l.astype(np.float64) / l.max()) ** (CFG["NORM_POWER"]["RECONSTRUCTION"] / CFG["NORM_POWER"]["ANALYSIS"])
        yy = vo.deemphasis(vo.griffinlim(spec, a, 8), CFG["PREEMPH"])
        return yy / yy.max() * 0.75
    want = np.stack([ref(lin[b], a0[b]) for b in range(B)])
    got = v.spectrogram2wav(_dev(lin), CFG, _pack(a0), n_iter=8).cpu().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-4
    assert np.allclose(got.max(1), 0.75, atol=1e-6)
    assert torch.equal(v.spectrogram2wav(_dev(lin), CFG, _pack(a0), n_iter=8, graph=True), torch.from_numpy(got).cuda())
    y = R.wave(np.random.RandomState(17), 256 * 30 + 100)
    mel, ln = v.wav2spectrogram(_dev(y), CFG["SAMPLING_RATE"], CFG)
    mr, lr = vo.wav2spectrogram(y, CFG["SAMPLING_RATE"], CFG)
    assert tuple(mel.shape) == mr.shape == (80, 7) and tuple(ln.shape) == lr.shape == (513, 28)
    assert np.abs(mel.cpu().numpy() - mr).max() <= 2e-5 and np.abs(ln.cpu().numpy() - lr).max() <= 2e-5


def test_full_size_batch_round_trip_and_fixed_point():
    """Synthesis size, T = 1300 frames, 4 utterances (82 tiles each, the last one short): ISTFT(STFT(y)) = y at the single-transform bar,
    one item against the oracle, and Griffin-Lim from the TRUE phases stays at the fixed point."""
    v = _voc()
    rng = np.random.RandomState(23)
    B, T = 4, 1300
    n = 256 * (T - 1)
    y = (rng.randn(B, n) * 0.1).astype(np.float32)
    S = v.stft(_dev(y))
    assert tuple(S.shape) == (B, 1026, T)
    back = v.istft(S).cpu().numpy()
    emu = [R.stft32(y[b]) for b in range(B)]
    e, b = R.rel_err(back, y), R.bar(np.stack([R.istft32(s) for s in emu]), y)
    print("full size round trip: %.2e, bar %.2e" % (e, b))
    assert e <= b
    emu3 = emu[3]
    ref = vo.stft(y[3])
    e, b = R.rel_err(S[3].cpu().numpy(), R.packed(ref)), R.bar(emu3, ref)
    print("full size stft: %.2e, bar %.2e" % (e, b))
    assert e <= b
    mag = v.magnitude(S)
    ang = S / torch.cat([mag, mag], 1).clamp_min(1e-12)
    w = v.griffinlim(mag, ang.contiguous(), 3).cpu().numpy()
    assert np.abs(w - y).max() <= 1e-3 * np.abs(y).max()


def test_generate_test_utterances_with_the_fft_vocoder(tmp_path):
    """harness.generate_test_utterances with VOCODER_TRANSFORM "fft" against the default: the same file names and lengths, waveforms within
    2e-2 of the peak (the bar tests/test_gpu_wide_synth.py gives two runs of that function that differ only in rounding).  Each call starts
    from the same generator state (see that test)."""
    from scipy.io import wavfile
    from spoofsv_amd import harness
    cfg = json.load(open(os.path.join(ROOT, "config.json")))
    cfg.update(SRC_ROOT_DIR=str(tmp_path) + os.sep, MAX_TEXT_LEN=24, MAX_FRAME_NUM=40, HIDDEN_DIM=32, TEXT_EMB_DIM=16, SSRN_DIM=32,
               TTS_TEXTS=os.path.join(ROOT, "tts_texts.txt"), GRIFFIN_LIM_ITERS=8, SYNTH_INCREMENTAL=True)
    cfg["STFT"] = {"FFT_LENGTH": 128, "HOP_LENGTH": 32}
    rng = np.random.RandomState(5)
    spk = {"p%d" % (225 + i): (0.04 + 0.05 * rng.rand(200)).astype(np.float32) for i in range(2)}
    texts = ["The birch canoe slid.", "Glue the sheet."]
    runs = {}
    for tr in ("dft", "fft"):
        c = dict(cfg) if tr == "dft" else dict(cfg, VOCODER_TRANSFORM="fft")
        torch.manual_seed(2024)
        runs[tr] = harness.generate_test_utterances(c, tr, eval_utt_num=2, speakers=spk, texts=texts, max_frames=24)
    assert list(runs["dft"]) == list(runs["fft"]) == list(spk)
    for name in spk:
        assert [os.path.basename(p) for p in runs["dft"][name]] == [os.path.basename(p) for p in runs["fft"][name]] == \
            ["s%s_%03d.wav" % (name[1:], k + 1) for k in range(2)]
        for pa, pb in zip(runs["dft"][name], runs["fft"][name]):
            (ra, ya), (rb, yb) = wavfile.read(pa), wavfile.read(pb)
            assert ra == rb == cfg["SAMPLING_RATE"] and len(ya) == len(yb) > 0, (pa, len(ya), len(yb))
            peak = float(np.abs(ya).max())
            d = float(np.abs(ya - yb).max())
            print("%s: %d samples, difference %.2e of the peak" % (os.path.basename(pa), len(ya), d / peak))
            assert d <= 2e-2 * peak, (pa, d, peak)
    with pytest.raises(ValueError, match="transform"):
        harness.generate_test_utterances(dict(cfg, VOCODER_TRANSFORM="dct"), "bad", eval_utt_num=2, speakers=spk, texts=texts, max_frames=24)
