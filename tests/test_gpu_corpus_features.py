"""GPU tests of the ragged corpus front end (csrc/corpus_features.hip, spoofsv_amd.corpus_features, harness.extract_features_batched and
CorpusSource's CORPUS_FEATURES modes).  Every comparison is against the float64 restatement in tests/_corpus_features_ref.py, never
against the code under test.  Run with `-m gpu` on an MI355X.

Bars.  A transform's magnitude is within d = 2e-5 * max|S| of float64 (tests/test_gpu_vocoder.py), per utterance.
* default normalisation, linear: out ** (1 / p) against S / max S.  Numerator and maximum each carry d and values are <= 1: 2 * 2e-5, plus
  1e-6 for the fp32 power and its float64 inverse.
* default normalisation, mel: the mel magnitude carries e[m] = d * sum_f basis[m][f] (the linear error through the basis, as
  test_features_vs_restatement of tests/test_gpu_sv_frontend.py pushes it) + 2e-5 * max(mel) (the mel product is a transform of its own);
  the maximum carries max_m e[m]; a ratio a / A with |da| <= e[m], |dA| <= E, a <= A moves by at most (e[m] + E) / (A - E); plus 1e-6.
* LOG_FEATURE: the normalisation g is monotone, so the output lies in [g(s - e) - 1e-6, g(s + e) + 1e-6] for an element of magnitude s
  and error bar e (d, or e[m]), the clip applied on both sides; 1e-6 covers log10f and the fp32 affine step on values <= 1.
The worst ratio to these bars is printed (run with -s) and part of every assertion message.
"""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

import _corpus_features_ref as C
import _sv_frontend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = json.load(open(os.path.join(ROOT, "config.json")))
SR, N_FFT, HOP, RED = CFG["SAMPLING_RATE"], CFG["STFT"]["FFT_LENGTH"], CFG["STFT"]["HOP_LENGTH"], CFG["COARSE_MELSPEC"]["REDUCTION"]
F, M, A = N_FFT // 2 + 1, CFG["COARSE_MELSPEC"]["FREQ_BINS"], CFG["PREEMPH"]
RESAMPLE_F32_DEV = 1.862e-6          # tests/test_gpu_sv_frontend.py: the float32 evaluation's own deviation; the kernel's bar is 4x this
D_REL = 2e-5
FLOOR = np.float32(1e-8)


def _cfg(log):
    return dict(CFG, LOG_FEATURE=bool(log))


def speechlike(rng, n, lead, tail, sr):
    """The voiced-speech stand-in of tests/test_gpu_sv_frontend.py at any rate: harmonics of f0 under a syllable envelope with a falling
    tilt, a 1e-4 noise floor, and ``lead`` / ``tail`` samples of near-silence (1e-5) at the edges."""
    f0 = rng.uniform(90, 220)
    t = np.arange(n) / float(sr)
    y = np.zeros(n)
    for h in range(1, 25):
        y += rng.uniform(0.3, 1.0) / h ** 1.5 * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.5, 4.0) * t + rng.uniform(0, 6.28))
    y = 0.25 * y * env + 1e-4 * rng.standard_normal(n)
    gate = np.zeros(n)
    gate[lead:n - tail] = 1.0
    return (y * gate + 1e-5 * rng.standard_normal(n)).astype(np.float32)


def _rows(seed, B, sr):
    """B - 3 utterances of 0.4-6 s with silent edges, and at rows 1, 3, 5: an empty row, a row of n_fft // 2 samples (at SAMPLING_RATE: too
    short to frame), an all-zero row."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(B - 3):
        n = int(rng.uniform(0.4, 6.0) * sr)
        rows.append(speechlike(rng, n, int(rng.uniform(0, 0.12) * sr), int(rng.uniform(0, 0.12) * sr), sr))
    short = N_FFT // 2 if sr == SR else 1000                              # 1000 samples at 48 kHz are 460 at 22,050 Hz
    rows.insert(1, np.zeros(0, dtype=np.float32))
    rows.insert(3, speechlike(rng, short, 0, 0, sr))
    rows.insert(5, np.zeros(int(0.9 * sr), dtype=np.float32))
    return rows


def _clear(refs):
    """The condition of test_trim_bounds_equal_the_restatement: no frame within 1e-3 dB of the threshold in float64."""
    return all(np.abs(f["db"] + C.TOP_DB).min() > 1e-3 for f in refs)


@functools.lru_cache(maxsize=None)
def _case(B):
    """(rows, float64 references) of a ragged batch at SAMPLING_RATE whose EVERY row is clear of the trim threshold; the first seed that is."""
    for seed in range(40, 48):
        rows = _rows(seed + 100 * B, B, SR)
        refs = [C.features(w, _cfg(False), SR) for w in rows]
        if _clear(refs):
            return rows, refs
    pytest.fail("no seed gave inputs clear of the trim threshold")


def _batch(wavs, n_max=None):
    """(B, n_max) rows with JUNK (7.0) past every row's live length, and the lengths."""
    n_max = max(n_max or 0, max(len(w) for w in wavs), 1)
    y = np.full((len(wavs), n_max), 7.0, dtype=np.float32)
    for i, w in enumerate(wavs):
        y[i, :len(w)] = w
    return torch.from_numpy(y).to(DEV), torch.tensor([len(w) for w in wavs], dtype=torch.int32, device=DEV)


def _poison(ex):
    """NaN in the extractor's arena and in the allocator's free blocks the results will be carved from."""
    if ex._arena is not None:
        ex._arena.fill_(float("nan"))
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 24, 1 << 22, 1 << 20, 1 << 16)]
    del junk
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _extractor(log, dft_mode):
    from spoofsv_amd.corpus_features import CorpusFeatureExtractor
    return CorpusFeatureExtractor(_cfg(log), device=DEV, dft_mode=dft_mode)


def _bars(ref, log):
    """One item's live columns in the compared domain (module docstring): [(want, lo, hi)] for the linear and the mel part, and the map into
    that domain (out ** (1 / p), or the identity under LOG_FEATURE).  None for an item whose maximum is 0 under the default normalisation."""
    rt, cfg = ref["rt"], _cfg(log)
    S, Sm = ref["lin_mag"][:, :RED * rt], ref["mel_mag"][:, :RED * rt:RED]
    d = D_REL * ref["lin_mag"].max()
    e = (d * C.mel_basis(cfg, SR).sum(1) + D_REL * ref["mel_mag"].max())[:, None]           # (M, 1)
    if log:
        out = []
        for s, err in ((S, d), (Sm, e)):
            out.append((C.log_norm(s, cfg), C.log_norm(np.maximum(s - err, 0.0), cfg) - 1e-6, C.log_norm(s + err, cfg) + 1e-6))
        return out, (lambda x: x)
    if ref["lin_mag"].max() == 0:
        return None, None
    p = cfg["NORM_POWER"]["ANALYSIS"]
    want_l, bar_l = S / ref["lin_mag"].max(), 2 * D_REL + 1e-6
    want_m, bar_m = Sm / ref["mel_mag"].max(), (e + e.max()) / (ref["mel_mag"].max() - e.max()) + 1e-6
    return [(want_l, want_l - bar_l, want_l + bar_l), (want_m, want_m - bar_m, want_m + bar_m)], (lambda x: x ** (1 / p))


def _ratios(ref, mel_g, lin_g, log):
    """Worst |deviation| / bar of one item's live columns; ``ref``: C.features of the item, ``mel_g`` (M, >= rt) and ``lin_g`` (F, >= r * rt)
    float64."""
    rt = ref["rt"]
    if rt == 0:
        return 0.0
    bars, dom = _bars(ref, log)
    lin_g, mel_g = lin_g[:, :RED * rt], mel_g[:, :rt]
    if bars is None:
        return 0.0 if not (lin_g.any() or mel_g.any()) else np.inf
    worst = 0.0
    for got, (mid, lo, hi) in zip((dom(lin_g), dom(mel_g)), bars):
        worst = max(worst, float(np.maximum((got - mid) / (hi - mid), (mid - got) / (mid - lo)).max()))
    return worst


def _check_batch(refs, mel, lin, rt, log, what):
    """Integers, live values against the bars, bitwise zeros beyond; returns the worst ratio."""
    mel, lin, rt = mel.cpu().numpy(), lin.cpu().numpy(), rt.cpu().numpy()
    assert mel.shape[:2] == (len(refs), M) and lin.shape[:2] == (len(refs), F) and lin.shape[2] == RED * mel.shape[2]
    assert not np.isnan(mel).any() and not np.isnan(lin).any()
    worst = 0.0
    for b, ref in enumerate(refs):
        assert rt[b] == ref["rt"], (what, b, rt[b], ref["rt"])
        assert not mel[b, :, rt[b]:].any() and not lin[b, :, RED * rt[b]:].any(), (what, b, "padding is not zero")
        worst = max(worst, _ratios(ref, mel[b].astype(np.float64), lin[b].astype(np.float64), log))
    return worst


def _specials_are_zero(rows, mel, lin, log):
    mel, lin = mel.cpu().numpy(), lin.cpu().numpy()
    for b, w in enumerate(rows):
        if len(w) <= N_FFT // 2:
            assert not mel[b].any() and not lin[b].any(), b                    # empty / too short: no frame
        elif not w.any():
            # an all-zero row HAS frames.  Default: its maximum is 0 -> zeros (the reference: 0 / 0).  LOG_FEATURE: the reference's own value
            # for silence, the clip floor 1e-8, in the live columns (data/dataset.py:104-105); zero beyond them (checked by the caller).
            rt = (1 + len(w) // HOP) // RED
            if log:
                assert np.all(mel[b, :, :rt] == FLOOR) and np.all(lin[b, :, :RED * rt] == FLOOR), b
            else:
                assert not mel[b].any() and not lin[b].any(), b


# ---------------------------------------------------------------------------------------------------------------- (1) integers
@pytest.mark.parametrize("B", [7, 33])
def test_integers_equal_the_restatement(B):
    """Trim bounds, T_b and rt equal the restatement's for EVERY row (inputs clear of the 22 dB threshold by 1e-3 dB in float64: _case)."""
    rows, refs = _case(B)
    ex = _extractor(False, "fp32")
    y, n = _batch(rows)
    ex(y, n, SR)
    _poison(ex)
    bounds = ex.trim_bounds(y, n)
    fr, nf = ex.frames(y, bounds)
    _, _, rt = ex(y, n, SR)
    bounds, nf, rt = bounds.cpu().numpy(), nf.cpu().numpy(), rt.cpu().numpy()
    for b, ref in enumerate(refs):
        assert (int(bounds[b, 0]), int(bounds[b, 1])) == (ref["start"], ref["end"]), (b, bounds[b], ref["start"], ref["end"])
        assert nf[b] == ref["T"] and rt[b] == ref["rt"], (b, nf[b], ref["T"], rt[b], ref["rt"])
    assert [refs[k]["T"] for k in (1, 3)] == [0, 0] and refs[5]["T"] == 1 + len(rows[5]) // HOP
    assert any(r["start"] > 0 for r in refs) and any(r["end"] < len(w) for r, w in zip(refs, rows))     # the edges were trimmed


# ---------------------------------------------------------------------------------------------------------------- (2) frames
@pytest.mark.parametrize("B", [7, 33])
def test_frames_vs_restatement(B):
    """ssv_preemph_frames_ragged: each element within 2^-23 (|x_i| + PREEMPH |x_(i-1)|); frames t >= T_b bitwise zero; a row with
    start > 0 does not see y[start - 1], which is set to 1e6."""
    rows, refs = _case(B)
    ex = _extractor(False, "fp32")
    segs = []
    for b, (w, ref) in enumerate(zip(rows, refs)):
        s, e = ref["start"], ref["end"]
        if s == 0 and e - s > 2000:
            s = 777 + b                                                       # every long row gets an interior start
        segs.append((s, e))
    rows = [w.copy() for w in rows]
    for w, (s, e) in zip(rows, segs):
        if s > 0:
            w[s - 1] = 1e6
    assert sum(s > 0 for s, _ in segs) >= B - 3
    y, _ = _batch(rows, n_max=max(len(w) for w in rows) + 300)
    fr, nf = ex.frames(y, torch.tensor(segs, dtype=torch.int32, device=DEV))
    fr, nf = fr.cpu().numpy(), nf.cpu().numpy()
    assert not np.isnan(fr).any()
    worst = 0.0
    for b, (w, (s, e)) in enumerate(zip(rows, segs)):
        T = C.lengths(e - s, N_FFT, HOP, RED)[0]
        assert nf[b] == T, (b, nf[b], T)
        assert not fr[b, :, T:].any(), (b, "frames past T_b are not zero")
        if T == 0:
            continue
        want = C.frames(w[s:e], N_FFT, HOP, A)
        bar = 2.0 ** -23 * C.frame_rounding_bound(w[s:e], N_FFT, HOP, A)
        dev = np.abs(fr[b, :, :T].astype(np.float64) - want)
        assert np.all(dev <= bar), (b, float(dev.max()), "a frame element is further than one fp32 rounding from float64")
        nz = bar > 0                                                      # an all-zero segment has a bar of 0 everywhere: equality, checked above
        if nz.any():
            worst = max(worst, float((dev[nz] / bar[nz]).max()))
    print("frames B=%d: worst deviation %.3f of the one-rounding bar" % (B, worst))


# ---------------------------------------------------------------------------------------------------------------- (3) features
@pytest.mark.parametrize("log", [False, True], ids=["norm_power", "log_feature"])
@pytest.mark.parametrize("dft_mode", ["fp32", "default"])
@pytest.mark.parametrize("B", [7, 33])
def test_features_vs_restatement(B, dft_mode, log):
    rows, refs = _case(B)
    ex = _extractor(log, dft_mode)
    y, n = _batch(rows)
    ex(y, n, SR)
    _poison(ex)
    mel, lin, rt = ex(y, n, SR)
    assert tuple(mel.shape) == (B, M, (1 + y.shape[1] // HOP) // RED) and rt.dtype == torch.int32
    worst = _check_batch(refs, mel, lin, rt, log, "B=%d" % B)
    print("features B=%d %s DFT %s: worst deviation %.4f of its bar" % (B, dft_mode, "LOG_FEATURE" if log else "default norm", worst))
    assert worst <= 1.0, "worst deviation / bar = %.4f (B=%d, %s DFT, LOG_FEATURE=%s)" % (worst, B, dft_mode, log)
    _specials_are_zero(rows, mel, lin, log)


# ---------------------------------------------------------------------------------------------------------------- (4) batch independence
@pytest.mark.parametrize("log", [False, True], ids=["norm_power", "log_feature"])
def test_rows_do_not_depend_on_their_batch_mates_in_fp32(log):
    """dft_mode="fp32": every row of the B = 33 batch against the same row alone (B = 1, its own n_max): within the bar of (3) of the
    restatement -- hence of each other by at most twice that -- and directly within that bar of each other in the compared domain.
    Whether they are bitwise equal is printed, not required."""
    rows, refs = _case(33)
    ex = _extractor(log, "fp32")
    mel, lin, rt = ex(*_batch(rows), SR)
    mel, lin, rt = mel.cpu().numpy(), lin.cpu().numpy(), rt.cpu().numpy()
    bitwise, worst = 0, 0.0
    for b, (w, ref) in enumerate(zip(rows, refs)):
        m1, l1, r1 = ex(*_batch([w]), SR)
        m1, l1 = m1.cpu().numpy()[0], l1.cpu().numpy()[0]
        k = int(r1.cpu()[0])
        assert k == rt[b] == ref["rt"]
        assert not m1[:, k:].any() and not l1[:, RED * k:].any()
        worst = max(worst, _ratios(ref, m1.astype(np.float64), l1.astype(np.float64), log))
        pairs = ((lin[b, :, :RED * k], l1[:, :RED * k]), (mel[b, :, :k], m1[:, :k]))
        same = all(np.array_equal(u, v) for u, v in pairs)
        bitwise += int(same)
        bars, dom = _bars(ref, log) if k else (None, None)
        if bars is not None and not same:
            for (u, v), (mid, lo, hi) in zip(pairs, bars):
                assert np.all(np.abs(dom(u.astype(np.float64)) - dom(v.astype(np.float64))) <= np.maximum(hi - mid, mid - lo)), b
    print("batch independence (LOG_FEATURE=%s): %d of %d rows bitwise equal alone and in the batch; worst lone-row deviation %.4f of its bar"
          % (log, bitwise, len(rows), worst))
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------- (5) resampling
def test_resampling_path_48k():
    """48 kHz rows: the resampled waveform within 4 x RESAMPLE_F32_DEV of the restatement's; integers and features against the restatement
    evaluated on the DEVICE's resampled waveform (resampler error and feature error are not stacked)."""
    ex = _extractor(False, "fp32")
    for seed in range(60, 68):
        rows = _rows(seed, 7, 48000)
        y, n = _batch(rows)
        res, n_res = ex.resample(y, n, 48000)
        res, n_res = res.cpu().numpy(), n_res.cpu().numpy()
        refs = [C.features(res[b, :n_res[b]], _cfg(False), SR) for b in range(len(rows))]
        if _clear(refs):
            break
    else:
        pytest.fail("no seed gave inputs clear of the trim threshold")
    worst_wave = 0.0
    for b, w in enumerate(rows):
        want = R.resample(w, 48000, SR)
        assert n_res[b] == want.shape[0], (b, n_res[b], want.shape[0])
        assert not res[b, n_res[b]:].any()
        if want.shape[0]:
            worst_wave = max(worst_wave, float(np.abs(res[b, :n_res[b]] - want).max()))
    print("resample 48000 -> %d: worst |gpu - float64 restatement| %.3e (bar %.3e)" % (SR, worst_wave, 4 * RESAMPLE_F32_DEV))
    assert worst_wave <= 4 * RESAMPLE_F32_DEV
    _poison(ex)
    mel, lin, rt = ex(y, n, 48000)
    assert mel.shape[2] == (1 + res.shape[1] // HOP) // RED
    worst = _check_batch(refs, mel, lin, rt, False, "48 kHz")
    print("features of 48 kHz rows: worst deviation %.4f of its bar" % worst)
    assert worst <= 1.0, worst
    assert refs[1]["T"] == 0 and refs[3]["T"] == 0 and max(r["rt"] for r in refs) > 20
    with pytest.raises(ValueError, match="unsupported"):
        ex(y, n, 44101)


# ---------------------------------------------------------------------------------------------------------------- (7) buffer reuse
def test_consecutive_calls_of_different_shapes():
    rows7, refs7 = _case(7)
    rows33, _ = _case(33)
    ex = _extractor(False, "fp32")
    a = [t.clone() for t in ex(*_batch(rows7), SR)]
    ex(*_batch(rows33), SR)
    ex(*_batch(rows7[:3], n_max=200000), SR)
    b = ex(*_batch(rows7), SR)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert _check_batch(refs7, a[0], a[1], a[2], False, "first call") <= 1.0


def test_inputs_are_checked():
    ex = _extractor(False, "fp32")
    y, n = _batch([np.ones(5000, dtype=np.float32)] * 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ex(y.cpu(), n.cpu(), SR)
    with pytest.raises(RuntimeError, match="lengths"):
        ex(y, n.long(), SR)
    from spoofsv_amd import corpus_features as cf
    assert ex.nbytes > 0 and cf.corpus_feature_bytes(2, 5000, CFG) > 4 * 2 * (1 + 5000 // HOP) * (N_FFT + 2 * F + F + M)


# ---------------------------------------------------------------------------------------------------------------- (6) harness
def _write_wavs(root, seed):
    """About 12 wavs pXXX/pXXX_NNN.wav: int16 and float32, 22,050 and 48,000 Hz; returns (paths, decoded float32 waveforms, rates)."""
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    paths, waves, rates = [], [], []
    for i in range(12):
        sr = 48000 if i % 3 == 2 else SR
        n = int(rng.uniform(0.5, 2.0) * sr)
        w = speechlike(rng, n, int(rng.uniform(0, 0.1) * sr), int(rng.uniform(0, 0.1) * sr), sr)
        spk = "p%d" % (225 + i % 3)
        os.makedirs(os.path.join(root, "wav", spk), exist_ok=True)
        path = os.path.join(root, "wav", spk, "%s_%03d.wav" % (spk, i + 1))
        if i % 2:
            q = (w * 32767).astype(np.int16)
            wavfile.write(path, sr, q)
            w = q.astype(np.float32) / 32768.0
        else:
            wavfile.write(path, sr, w)
        paths.append(path); waves.append(w); rates.append(sr)
    return paths, waves, rates


def test_extract_features_batched_against_extract_features(tmp_path):
    """Same file names as ``extract_features`` on the same corpus; same shapes for every file at SAMPLING_RATE (``extract_features`` does not
    resample: for a 48 kHz file it transforms the signal at its native rate, so THAT file's shape is checked against the restatement of
    resample + features instead); contents of both within the bar of (3) of their own float64 reference; one short file: None, no files."""
    from scipy.io import wavfile
    from spoofsv_amd import harness
    ex = _extractor(False, "fp32")
    cfg = _cfg(False)
    for seed in range(70, 78):
        root = os.path.join(str(tmp_path), "s%d" % seed)
        paths, waves, rates = _write_wavs(root, seed)
        refs = []
        for w, sr in zip(waves, rates):
            if sr != SR:                                                     # the device's own resampled waveform: errors are not stacked
                res, k = ex.resample(*_batch([w]), sr)
                w = res.cpu().numpy()[0, :int(k.cpu()[0])]
            refs.append(C.features(w, cfg, SR))
        own = [C.features(w, cfg, sr) for w, sr in zip(waves, rates)]        # what extract_features computes: no resampling
        if _clear(refs) and _clear(own):
            break
    else:
        pytest.fail("no seed gave inputs clear of the trim threshold")
    short = os.path.join(root, "wav", "p225", "p225_099.wav")
    wavfile.write(short, SR, (0.1 * np.ones(300)).astype(np.float32))
    old_dir, new_dir = os.path.join(root, "old") + os.sep, os.path.join(root, "new") + os.sep
    old = harness.extract_features(paths, cfg, old_dir)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        new = harness.extract_features_batched(paths[:5] + [short] + paths[5:], cfg, new_dir, utterances_per_batch=4, extractor=ex)
    assert new[5] is None and any("p225_099" in str(c.message) for c in caught)
    new = new[:5] + new[6:]
    listing = lambda d: sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)
    assert listing(new_dir) == listing(old_dir) and len(listing(new_dir)) == 24 and not any("099" in f for f in listing(new_dir))
    worst_new = worst_old = 0.0
    for i, path in enumerate(paths):
        key = path[-17:-4]
        m_new, l_new = np.load(new_dir + key + "_mel.npy"), np.load(new_dir + key + "_lin.npy")
        m_old, l_old = np.load(old_dir + key + "_mel.npy"), np.load(old_dir + key + "_lin.npy")
        assert new[i] == (m_new.shape, l_new.shape) and old[i] == (m_old.shape, l_old.shape)
        assert m_new.dtype == np.float32 and m_new.shape == (M, refs[i]["rt"]) and l_new.shape == (F, RED * refs[i]["rt"])
        if rates[i] == SR:
            assert new[i] == old[i], (path, new[i], old[i])
            worst_old = max(worst_old, _ratios(own[i], m_old.astype(np.float64), l_old.astype(np.float64), False))
        worst_new = max(worst_new, _ratios(refs[i], m_new.astype(np.float64), l_new.astype(np.float64), False))
    print("cache files: batched worst %.4f of the bar, extract_features worst %.4f of the bar" % (worst_new, worst_old))
    assert worst_new <= 1.0 and worst_old <= 1.0, (worst_new, worst_old)


def _corpus(tmp_path):
    from test_host_cpu import _make_corpus
    from scipy.io import wavfile
    cfg, _ = _make_corpus(str(tmp_path), n_items=5, with_cache=False, wav=True)
    cfg.update(BATCH_SIZE=2, HIDDEN_DIM=32, TEXT_EMB_DIM=16, SSRN_DIM=32, VAL_EVERY_ITER=1000, MAX_ITERATIONS=1, MAX_EPOCHS=1)
    lists = os.path.join(cfg["DATA_ROOT_DIR"], "data_path", "ordinary", "wav.path.train")
    waves = []
    for path in open(lists).read().split():
        sr, q = wavfile.read(path)
        assert sr == SR
        waves.append(q.astype(np.float32) / 32768.0)
    refs = [C.features(w, _cfg(False), SR) for w in waves]
    assert _clear(refs), "the corpus of tests/test_host_cpu.py has a frame at the trim threshold"
    return cfg, refs


@pytest.mark.parametrize("step", ["train_ssrn", "train_text2mel", "synthesize"])
def test_corpus_source_device_mode_yields_the_cache_modes_batches(tmp_path, step):
    from spoofsv_amd import harness
    cfg, refs = _corpus(tmp_path)
    spec = os.path.join(str(tmp_path), "spec") + os.sep
    mode = "train"
    cache = harness.CorpusSource(cfg, step, "conditional", mode, 2, spec, seed=3)
    dev = harness.CorpusSource(dict(cfg, CORPUS_FEATURES="device"), step, "conditional", mode, 2, os.path.join(str(tmp_path), "unused") + os.sep, seed=3)
    assert not os.path.exists(os.path.join(str(tmp_path), "unused"))
    order = np.random.RandomState(3).permutation(5)
    worst = 0.0
    n = 0
    for i, (bc, bd) in enumerate(zip(cache, dev)):
        n += 1
        idx = order[2 * i:2 * i + 2]
        assert list(bc) == list(bd), (list(bc), list(bd))
        lin_key = {"train_ssrn": "data_1", "synthesize": "data_3"}.get(step)
        for key in bc:
            assert tuple(bc[key].shape) == tuple(bd[key].shape) and bc[key].dtype == bd[key].dtype, (key, bc[key].shape, bd[key].shape)
            if key in ("data_0", lin_key):
                assert bd[key].is_cuda and not bc[key].is_cuda
            else:
                assert torch.equal(bc[key], bd[key].cpu())                   # texts and speaker codes: as today
        assert dev.last_rt == [refs[k]["rt"] for k in idx]
        for src in (bc, bd):
            mel = src["data_0"].cpu().numpy().astype(np.float64)
            lin = src[lin_key].cpu().numpy().astype(np.float64) if lin_key else None
            for j, k in enumerate(idx):
                rt = refs[k]["rt"]
                assert not mel[j, :, rt:].any() and (lin is None or not lin[j, :, RED * rt:].any())
                l = lin[j] if lin is not None else refs[k]["lin"]          # no linear batch in this step: the mel part alone is compared
                worst = max(worst, _ratios(refs[k], mel[j], l, False))
    assert n == 3
    print("CorpusSource %s: worst deviation of either mode %.4f of its bar" % (step, worst))
    assert worst <= 1.0, worst
    # through the Prefetcher: the same batches, device tensors passed through unchanged
    dev.epoch = 0
    direct = list(dev)
    dev.epoch = 0
    for a, b in zip(direct, harness.Prefetcher(dev, torch.device(DEV))):
        assert list(a) == list(b) and all(torch.equal(a[k].to(DEV), b[k]) for k in a) and all(v.is_cuda for v in b.values())


@pytest.mark.parametrize("step", ["train_ssrn", "train_text2mel"])
def test_one_training_iteration_on_a_device_mode_source(tmp_path, step):
    """One ``ordinary_train`` iteration on CORPUS_FEATURES = "device" against the same iteration on the cache: the loss within 1e-5 (the bar
    the README quotes for the trainers' loss terms, used as tests/test_gpu_harness.py uses it)."""
    from spoofsv_amd import harness
    cfg, _ = _corpus(tmp_path)
    spec = os.path.join(str(tmp_path), "spec") + os.sep
    losses = {}
    for mode in ("cache", "device"):
        torch.manual_seed(11)
        c = dict(cfg, CORPUS_FEATURES=mode, SRC_ROOT_DIR=os.path.join(str(tmp_path), "runs_" + mode) + os.sep)
        _, hist = harness.ordinary_train(step, "conditional", c, spec_dir=spec, current_time="c")
        assert len(hist) == 1 and hist[0] == hist[0]
        losses[mode] = hist[0]
    diff = abs(losses["cache"] - losses["device"])
    print("%s: loss on the cache %.8f, on the device source %.8f, difference %.3e" % (step, losses["cache"], losses["device"], diff))
    assert diff <= 1e-5 * max(1.0, abs(losses["cache"])), (losses, diff)
