"""GPU tests of the speaker-verification front end (csrc/sv_frontend.hip, spoofsv_amd.sv_frontend, the harness entries built on it).
Every comparison is against the float64 restatement in tests/_sv_frontend_ref.py, never against the code under test.
Run with `-m gpu` on an MI355X."""
import contextlib
import json
import os
import random

import numpy as np
import pytest
import torch

import _sv_frontend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Largest deviation of the restatement evaluated in float32 (weights, samples and the running sum in float32, numpy on the CPU) from
# its float64 evaluation on the inputs of test_resample_ragged_batch, measured on the development machine
# (profiles/round8_sv_frontend.txt).  The kernel's bar is 4x this: the margin covers another summation order, nothing more.
RESAMPLE_F32_DEV = 1.862e-6
F32_COS = 2 * 3 * (8 + 2) * 2.0 ** -24       # float32 evaluation of two cosine matrices, D = 256 (test_end_to_end_files_and_memory_agree)
MIN_LEN = 19600              # the shortest utterance data_preprocess.py:48 keeps: utter_min_len is 19599.999999999996 in floats


@contextlib.contextmanager
def _mode(name):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(name)
    try:
        yield
    finally:
        spoofsv_amd.set_precision(prev)


def speechlike(rng, n, lead, tail, f0=None):
    """A voiced-speech stand-in: harmonics of f0 under a slow syllable envelope with a falling spectral tilt (so the upper mel bands are
    quiet), a 1e-4 noise floor, and ``lead`` / ``tail`` samples of near-silence (1e-5) at the edges."""
    f0 = f0 or rng.uniform(90, 220)
    t = np.arange(n) / 16000.0
    y = np.zeros(n)
    for h in range(1, 25):
        y += rng.uniform(0.3, 1.0) / h ** 1.5 * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.5, 4.0) * t + rng.uniform(0, 6.28))
    y = 0.25 * y * env + 1e-4 * rng.standard_normal(n)
    gate = np.zeros(n)
    gate[lead:n - tail] = 1.0
    return (y * gate + 1e-5 * rng.standard_normal(n)).astype(np.float32)


def resample_inputs():
    rng = np.random.default_rng(10)
    lens = [198450, 300, 0, 83200, 441, 1, 30011, 120000]
    return [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in lens]


def _batch(wavs, n_max=None):
    """(B, n_max) rows with JUNK (7.0) past every row's live length -- a kernel that read beyond n[b] would show it -- and the lengths."""
    n_max = max(n_max or 0, max(len(w) for w in wavs), 1)
    y = np.full((len(wavs), n_max), 7.0, dtype=np.float32)
    for i, w in enumerate(wavs):
        y[i, :len(w)] = w
    return torch.from_numpy(y).to(DEV), torch.tensor([len(w) for w in wavs], dtype=torch.int32, device=DEV)


def test_resample_ragged_batch():
    """ssv_resample_sinc 22,050 -> 16,000 Hz on lengths from 0 to 9 s: n_out equal, samples within 4 x RESAMPLE_F32_DEV, zeros after.
    Every row is followed by junk up to n_max, which is longer than the longest row: the live-length mask is part of what is compared."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    wavs = resample_inputs()
    fe = TisvFrontEnd(device=DEV)
    y, n = _batch(wavs, n_max=200000)
    out, n_out = fe.resample(y, n, 22050)
    out, n_out = out.cpu().numpy(), n_out.cpu().numpy()
    worst = 0.0
    for b, w in enumerate(wavs):
        ref = R.resample(w, 22050, 16000)
        assert n_out[b] == ref.shape[0], (b, n_out[b], ref.shape[0])
        assert not out[b, n_out[b]:].any()
        if ref.shape[0]:
            worst = max(worst, float(np.abs(out[b, :n_out[b]] - ref).max()))
    print("resample: worst |gpu - float64 restatement| %.3e (bar %.3e)" % (worst, 4 * RESAMPLE_F32_DEV))
    assert worst <= 4 * RESAMPLE_F32_DEV
    same, n_same = fe.resample(y, n, 16000)                                 # equal rates: a copy
    assert torch.equal(n_same, n)
    for b, w in enumerate(wavs):
        assert np.array_equal(same[b, :len(w)].cpu().numpy(), w) and not same[b, len(w):].any()


def _trim_rows(seed):
    rng = np.random.default_rng(seed)
    rows = [speechlike(rng, 60000, 9000, 14000), speechlike(rng, 83200, 0, 30000), speechlike(rng, 40000, 11111, 0),
            np.zeros(20000, dtype=np.float32),                                   # all-silent
            (0.3 * rng.standard_normal(50000)).astype(np.float32),               # all-loud
            speechlike(rng, 1500, 200, 300), speechlike(rng, 700, 0, 0),         # shorter than one frame / than half a frame
            np.zeros(0, dtype=np.float32)]
    return rows


def test_trim_bounds_equal_the_restatement():
    """ssv_trim_bounds: integers equal for every row.  Condition on the inputs, checked on the CPU first: no frame within 1e-3 dB of the
    threshold in float64 (next seed otherwise, at most 3 times)."""
    from spoofsv_amd import sv_frontend
    for seed in (20, 21, 22, 23):
        rows = _trim_rows(seed)
        refs = [R.trim(r, 30) for r in rows]
        if all(np.abs(db + 30.0).min() > 1e-3 for _, _, db in refs):
            break
    else:
        pytest.fail("no seed gave inputs clear of the threshold")
    y, n = _batch(rows, n_max=90000)                                             # live lengths shorter than n_max
    got = sv_frontend.trim_bounds(y, n, 30).cpu().numpy()
    for b, (s, e, _) in enumerate(refs):
        assert (int(got[b, 0]), int(got[b, 1])) == (s, e), (b, got[b], s, e)
    assert tuple(got[7]) == (0, 0) and tuple(got[3]) == (0, 20000)
    assert refs[0][0] > 0 and refs[0][1] < 60000                                # the edges were trimmed


def _feature_rows(seed=30):
    rng = np.random.default_rng(seed)
    rows = [speechlike(rng, 52000, 0, 0), speechlike(rng, 31000, 0, 0), speechlike(rng, MIN_LEN - 1, 0, 0), speechlike(rng, MIN_LEN, 0, 0),
            speechlike(rng, MIN_LEN + 1, 0, 0), speechlike(rng, 144000, 0, 0), speechlike(rng, 3000, 0, 0), np.zeros(0, dtype=np.float32)]
    return rows


def _whole(rows):
    """(waveforms, bounds that keep every row whole)"""
    y, n = _batch(rows)
    return y, torch.stack([torch.zeros_like(n), n], 1).contiguous()


def _slices(fe, rows):
    f, v = fe.slices(*_whole(rows))
    return f.cpu().numpy().astype(np.float64), v.cpu().numpy()


@pytest.mark.parametrize("dft_mode", ["fp32", "default"])
def test_features_vs_restatement(dft_mode):
    """ssv_tisv_frames + DFT + ssv_power_mel_log: valid flags exact (rows of utter_min_len - 1, utter_min_len, utter_min_len + 1 samples);
    mel POWER (10 ** feature) within mel_basis . (2 |S| d + d^2), d = 2e-5 max|S| (the per-transform bar of tests/test_gpu_vocoder.py);
    the log-domain deviation is printed (its bar is the embedding test's)."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    fe = TisvFrontEnd(device=DEV, dft_mode=dft_mode)
    rows = _feature_rows()
    f, v = _slices(fe, rows)
    assert list(v) == [1, 1, 0, 1, 1, 1, 0, 0]
    mel = R.mel_filterbank(16000, 512, 40)
    worst_log = worst_ratio = 0.0
    for b, w in enumerate(rows):
        if not v[b]:
            assert R.slices_of(w)[1] is False
            continue
        S, mag = R.log_mel(w)
        d = 2e-5 * mag.max()
        bound = mel @ (2 * mag * d + d * d)                                   # (nmels, T)
        for s, sl in ((0, slice(0, 120)), (1, slice(S.shape[1] - 120, S.shape[1]))):
            ref, got = S[:, sl].T, f[b, s]
            p_ref, p_got = 10.0 ** ref, 10.0 ** got
            worst_ratio = max(worst_ratio, float((np.abs(p_got - p_ref) / bound[:, sl].T).max()))
            worst_log = max(worst_log, float(np.abs(got - ref).max()))
    print("features (%s DFT): worst mel-power deviation %.3e of its bound, worst log10 deviation %.3e" % (dft_mode, worst_ratio, worst_log))
    assert worst_ratio <= 1.0


@pytest.mark.parametrize("dft_mode", ["fp32", "default"])
def test_features_of_interior_segments(dft_mode):
    """ssv_tisv_frames with start > 0 and end < n: the rows are loud THROUGHOUT, so a gather that reflected at the row's edges instead of
    the segment's, or started at sample 0, would read other samples than R.slices_of(y[start:end]) does.  Same bound as above; a segment
    of utter_min_len - 1 samples inside a long row is too short, one of utter_min_len samples is not."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    fe = TisvFrontEnd(device=DEV, dft_mode=dft_mode)
    rng = np.random.default_rng(33)
    rows = [speechlike(rng, 60000, 0, 0) for _ in range(5)]
    segs = [(7001, 52003), (1, 59999), (30000, 30000 + MIN_LEN - 1), (30000, 30000 + MIN_LEN), (12345, 12345 + 19703)]
    y, _ = _batch(rows, n_max=61000)
    f, v = fe.slices(y, torch.tensor(segs, dtype=torch.int32, device=DEV))
    f, v = f.cpu().numpy().astype(np.float64), v.cpu().numpy()
    assert list(v) == [1, 1, 0, 1, 1]
    mel = R.mel_filterbank(16000, 512, 40)
    worst_log = worst_ratio = 0.0
    for b, (s, e) in enumerate(segs):
        if not v[b]:
            assert not f[b].any() or np.all(f[b] == f[b].flat[0])             # zero frames: every feature is log10(1e-6)
            continue
        S, mag = R.log_mel(rows[b][s:e])
        d = 2e-5 * mag.max()
        bound = mel @ (2 * mag * d + d * d)
        for k, sl in ((0, slice(0, 120)), (1, slice(S.shape[1] - 120, S.shape[1]))):
            worst_ratio = max(worst_ratio, float((np.abs(10.0 ** f[b, k] - 10.0 ** S[:, sl].T) / bound[:, sl].T).max()))
            worst_log = max(worst_log, float(np.abs(f[b, k] - S[:, sl].T).max()))
    print("interior segments (%s DFT): worst mel-power deviation %.3e of its bound, worst log10 deviation %.3e" % (dft_mode, worst_ratio, worst_log))
    assert worst_ratio <= 1.0


def test_lengths_and_bounds_are_not_interchangeable():
    from spoofsv_amd.sv_frontend import TisvFrontEnd, trim_bounds
    fe = TisvFrontEnd(device="cuda")                                          # "cuda" is the current device: cuda:0 tensors are accepted
    y, n = _batch([np.ones(30000, dtype=np.float32)] * 2)
    b = torch.stack([torch.zeros_like(n), n], 1).contiguous()
    fe.slices(y, b)
    with pytest.raises(RuntimeError, match="bounds"):
        fe.slices(y, n)
    with pytest.raises(RuntimeError, match="lengths"):
        trim_bounds(y, b)
    with pytest.raises(RuntimeError, match="lengths"):
        fe.resample(y, b, 22050)


def _unit(e):
    e = e.detach().cpu().double()
    return e / e.norm(dim=-1, keepdim=True)


def _one_minus_cos(a, b):
    """1 - cosine of matching rows, in float64 as half the squared distance of the unit vectors (no cancellation)."""
    return 0.5 * ((_unit(a) - _unit(b)) ** 2).sum(-1)


def _embedder(seed=0):
    from spoofsv_amd.ge2e import SpeechEmbedder
    torch.manual_seed(seed)
    return SpeechEmbedder(40, 768, 3, 256).to(DEV).eval()


@torch.no_grad()
def _baseline(net, feats):
    """The embedder's own arithmetic noise on identical features: worst 1 - cos between the library's fp32 and default modes.  The
    library runs products of fewer than 128 columns in plain fp32 in EVERY mode (measured: below that the two modes' embeddings are
    bit-identical and this figure is 0), so the batch is tiled up to at least 128 rows."""
    assert feats.dim() == 3
    feats = feats.repeat(-(-128 // feats.shape[0]), 1, 1).contiguous()
    with _mode("fp32"):
        a = net(feats)
    b = net(feats)
    return float(_one_minus_cos(a, b).max())


@torch.no_grad()
def test_embeddings_of_gpu_features_vs_restatement_features():
    """What the features are for: the same seeded full-size SpeechEmbedder on GPU features and on restatement features.  The front end
    passes if its worst pair is no further from cosine 1 than 4 x the embedder's own fp32-vs-default noise on the restatement features."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    rng = np.random.default_rng(31)
    rows = [speechlike(rng, int(rng.integers(MIN_LEN, 60000)), 0, 0) for _ in range(72)]      # 144 slices: the split products are in play
    ref = torch.from_numpy(np.stack([R.slices_of(r)[0] for r in rows]).astype(np.float32)).to(DEV).reshape(-1, 120, 40)
    net = _embedder()
    base = _baseline(net, ref)
    e_ref = net(ref)
    figs = {}
    for mode in ("fp32", "default"):
        f, _ = TisvFrontEnd(device=DEV, dft_mode=mode).slices(*_whole(rows))
        figs[mode] = float(_one_minus_cos(net(f.reshape(-1, 120, 40).contiguous()), e_ref).max())
    print("embeddings: baseline 1 - cos %.3e; front end fp32 DFT %.3e, split-fp16 DFT %.3e" % (base, figs["fp32"], figs["default"]))
    assert TisvFrontEnd(device=DEV).dft_mode == "fp32"
    assert figs["fp32"] <= 4 * base, (figs, base)


def test_captured_replay_equals_eager():
    """The whole chain from (y, lengths) to features under torch.cuda.graph, replayed on two different ragged batches."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    fe = TisvFrontEnd(device=DEV)
    rng = np.random.default_rng(40)
    batches = [[speechlike(rng, n, l, t) for n, l, t in [(60000, 5000, 9000), (30000, 0, 0), (20000, 100, 100), (0, 0, 0)]],
               [speechlike(rng, n, l, t) for n, l, t in [(29000, 0, 1000), (64000, 12000, 3000), (64000, 0, 0), (41000, 3000, 3000)]]]
    n_max = 64000
    eager = []
    for wavs in batches:
        y, n = _batch(wavs, n_max)
        f, v = fe(y, n, 22050)
        eager.append((f.clone(), v.clone()))
    sy, sn = torch.zeros((4, n_max), device=DEV), torch.zeros((4,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gf, gv = fe(sy, sn, 22050)
    for wavs, (f, v) in zip(batches, eager):
        y, n = _batch(wavs, n_max)
        sy.copy_(y)
        sn.copy_(n)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gv, v) and torch.equal(gf, f)
    assert eager[0][1].tolist() == [1, 1, 0, 0] and eager[1][1].tolist() == [1, 1, 1, 1]


def _tiny_cfg(tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "config.json")))
    cfg.update(SRC_ROOT_DIR=str(tmp_path) + os.sep, MAX_TEXT_LEN=24, MAX_FRAME_NUM=40, HIDDEN_DIM=32, TEXT_EMB_DIM=16, SSRN_DIM=32,
               TTS_TEXTS=os.path.join(ROOT, "tts_texts.txt"), GRIFFIN_LIM_ITERS=4, SYNTH_INCREMENTAL=True)
    return cfg


TEXTS = ["The birch canoe slid.", "Glue the sheet.", "It's easy to tell the depth of a well."]


def _speaker_codes():
    rng = np.random.RandomState(5)
    return {"p%d" % (225 + i): (0.04 + 0.05 * rng.rand(200)).astype(np.float32) for i in range(5)}


def test_default_path_writes_the_host_loop_of_the_vocoder_output(tmp_path, monkeypatch):
    """return_waveforms=False, the path that existed before: every written file holds, byte for byte, what the reference's host loop
    (generate_test_utterances.py:135-139: trim_silence(30), [:9 * sr], / max * 0.75) makes of the vocoder's output for that speaker --
    the output is recorded on its way out of Vocoder.spectrogram2wav, the loop is restated here -- and a second call from the same
    generator state writes the same bytes (same seed, same models)."""
    import io
    from scipy.io import wavfile
    from spoofsv_amd import harness, vocoder
    cfg = _tiny_cfg(tmp_path)
    sr = cfg["SAMPLING_RATE"]
    seen = []
    orig = vocoder.Vocoder.spectrogram2wav

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        assert kw.get("peak", 0.75) is None
        seen.append(out.detach().cpu().numpy().copy())
        return out
    monkeypatch.setattr(vocoder.Vocoder, "spectrogram2wav", spy)
    runs = []
    for tag in ("first", "second"):
        torch.manual_seed(2024)
        runs.append(harness.generate_test_utterances(cfg, tag, eval_utt_num=3, speakers=_speaker_codes(), texts=TEXTS, max_frames=40))
    first, second = runs
    assert isinstance(first, dict) and list(first) == list(_speaker_codes()) and len(seen) == 10
    for i, spk in enumerate(first):
        assert [os.path.basename(p) for p in first[spk]] == ["s%s_%03d.wav" % (spk[1:], k + 1) for k in range(3)]
        for k, (pa, pb) in enumerate(zip(first[spk], second[spk])):
            y, _ = vocoder.trim_silence(seen[i][k], 30)
            y = y[:9 * sr]
            if len(y):
                y = (y / np.max(y) * 0.75).astype(np.float32)
            buf = io.BytesIO()
            wavfile.write(buf, sr, y)
            got = open(pa, "rb").read()
            assert got == buf.getvalue(), pa
            assert got == open(pb, "rb").read(), (pa, pb)


def test_return_waveforms_against_the_default_path(tmp_path):
    """return_waveforms=False returns the dict of paths alone, as before.  With True (same seed, same models) the returned device
    waveforms are what the files hold, each file within one 512-sample hop per edge of the default path's (fp32 against float64 frame
    energies at the threshold) and, where the bounds agree, the same samples (the peak is the row's maximum on both paths)."""
    from spoofsv_amd import harness
    cfg = _tiny_cfg(tmp_path)
    with _mode("fp32"):
        torch.manual_seed(2024)
        a = harness.generate_test_utterances(cfg, "a", eval_utt_num=3, speakers=_speaker_codes(), texts=TEXTS, max_frames=40)
        torch.manual_seed(2024)
        b, waves = harness.generate_test_utterances(cfg, "b", eval_utt_num=3, speakers=_speaker_codes(), texts=TEXTS, max_frames=40,
                                                    return_waveforms=True)
    from scipy.io import wavfile
    assert isinstance(a, dict) and list(a) == list(b) == list(waves)
    for spk in a:
        seg, seg_n = waves[spk]
        assert seg.is_cuda and seg_n.dtype == torch.int32
        for k, (pa, pb) in enumerate(zip(a[spk], b[spk])):
            (_, ya), (_, yb) = wavfile.read(pa), wavfile.read(pb)
            assert np.array_equal(yb, seg[k, :int(seg_n[k])].cpu().numpy())
            assert abs(len(ya) - len(yb)) <= 1024, (pa, len(ya), len(yb))      # one hop at each end
            if len(ya) == len(yb):
                assert np.abs(ya - yb).max() <= 1e-6 * np.abs(ya).max()


@torch.no_grad()
def test_end_to_end_files_and_memory_agree(tmp_path):
    """Tiny seeded TTS models, 5 speakers: generate_test_utterances(return_waveforms=True) plus seeded genuine wavs -> preprocess_tisv ->
    ge2e_harness.test, and spoof_evaluation on the same material in memory.  The two similarity matrices agree with the restatement's
    to the embedding figure, and EER / threshold / spoof rate are EQUAL when no entry of the restatement's matrix lies within that
    figure of one of the 50 thresholds (checked first).

    The figure for a matrix ENTRY: a cosine between two unit vectors moves by at most the sum of their displacements, and a unit
    vector whose own cosine to its exact value is 1 - c is displaced by sqrt(2 c); with c = 4 x the embedder's baseline (the bar of
    the embedding test) on both sides that is 2 sqrt(8 x baseline).  The matrices themselves are float32 (cossim_eval on the device):
    an entry is a quotient of a D = 256-term dot product and two norms, each a tree reduction of log2(D) levels plus the final
    operations, i.e. about 3 (log2 D + 2) roundings of u = 2^-24 on values <= 1, and two such matrices are compared:
    2 x 3 x 10 x 2^-24 = 3.6e-6.  That allowance is also MEASURED here (the float32 matrix against cossim_eval in float64 on the same
    embeddings) and printed; it must itself stay inside the allowance."""
    from scipy.io import wavfile
    from spoofsv_amd import ge2e_harness, harness
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    cfg = _tiny_cfg(tmp_path)
    codes = _speaker_codes()
    with _mode("fp32"):
        torch.manual_seed(2024)
        paths, waves = harness.generate_test_utterances(cfg, "e2e", eval_utt_num=3, speakers=codes, texts=TEXTS, max_frames=40, return_waveforms=True)
    sr_tts = cfg["SAMPLING_RATE"]
    rng = np.random.default_rng(50)
    genuine, speakers = {}, {}
    for i, spk in enumerate(codes):
        ws = [speechlike(rng, int(rng.integers(30000, 50000)), 3000, 4000, f0=100.0 + 25 * i) for _ in range(5)]
        files = []
        for k, w in enumerate(ws):
            p = str(tmp_path / "genuine" / spk / ("g%02d.wav" % k))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            wavfile.write(p, sr_tts, w)
            files.append(p)
        genuine[spk] = ws
        speakers[spk] = files + paths[spk]                                       # 2 enrolment, 3 genuine, 3 spoofing utterances
    g = ge2e_harness.default_config()
    g["device"] = DEV
    g["data"]["train_path"], g["data"]["test_path"] = str(tmp_path / "train_tisv"), str(tmp_path / "test_tisv")
    g["save_simmat_dir"] = str(tmp_path / "simmat")
    g["test"].update(N=5, M=16, epochs=1)
    written = ge2e_harness.preprocess_tisv(g, speakers, 0, 5, 3)                 # as data_preprocess.py:102: enrol + eval, eval
    assert len(written) == 5 and np.load(written[0]).shape == (16, 40, 120)
    files = sorted(os.listdir(g["data"]["test_path"]))
    random.seed(7)
    order = [int(random.sample(files, 1)[0][len("speaker"):-4]) for _ in range(5)]      # the speakers data_load.py:70-73 draws
    names = [list(codes)[i] for i in order]
    # the restatement's features of the same material
    fe = TisvFrontEnd.from_config(g)

    def ref_feats(ws):
        f, v = R.front_end(ws, sr_tts)
        assert v.all()
        return f

    def dev_feats(ws):
        f, v = fe(*ge2e_harness.pad_batch(ws, DEV), sr_tts)
        assert bool(v.all())
        return f
    enr_r, gen_r, spo_r, enr_d, gen_d, spo_d = [], [], [], [], [], []
    for spk in names:
        seg, seg_n = waves[spk]
        spoof_host = [seg[k, :int(seg_n[k])].cpu().numpy() for k in range(3)]
        enr_r.append(ref_feats(genuine[spk][:2])); gen_r.append(ref_feats(genuine[spk][2:])); spo_r.append(ref_feats(spoof_host))
        enr_d.append(dev_feats(genuine[spk][:2])); gen_d.append(dev_feats(genuine[spk][2:]))
        f, v = fe(seg, seg_n, sr_tts)                                             # the vocoder's waveforms, never read from disk
        assert bool(v.all())
        spo_d.append(f)
    up = lambda xs: torch.from_numpy(np.stack(xs)).to(DEV)
    thr = torch.tensor([0.01 * i + 0.5 for i in range(50)], dtype=torch.float64)
    for seed in range(3, 11):            # the embedder's seed is chosen on the restatement alone: its matrix must stay clear of the thresholds
        torch.manual_seed(seed)
        net = ge2e_harness._embedder(g, torch.device(DEV)).eval()
        r_ref = ge2e_harness.spoof_evaluation(g, net, up(enr_r), up(gen_r), up(spo_r))
        base = _baseline(net, up(gen_r).reshape(-1, 120, 40).contiguous())
        fig = 2.0 * np.sqrt(8.0 * base) + F32_COS
        gap = float((r_ref["sim"].cpu().double().reshape(-1, 1) - thr.view(1, -1)).abs().min())
        print("embedder seed %d: baseline 1 - cos %.3e, entry figure %.3e, nearest threshold %.3e away" % (seed, base, fig, gap))
        if gap > fig:
            break
    else:
        pytest.fail("no embedder seed keeps the restatement's matrix clear of the thresholds")
    e_enr = net(up(enr_r).reshape(-1, 120, 40).contiguous()).reshape(5, 4, -1).cpu().double()
    e_ver = net(torch.cat([up(gen_r).reshape(5, -1, 120, 40), up(spo_r).reshape(5, -1, 120, 40)], 1).reshape(-1, 120, 40).contiguous())
    sim64 = ge2e_harness.cossim_eval(e_ver.reshape(5, 12, -1).cpu().double(), e_enr.mean(dim=1))
    cos32 = float((r_ref["sim"].cpu().double() - sim64).abs().max())
    print("float32 evaluation of the cosine matrix against float64 on the same embeddings: %.3e (allowance for two: %.3e)" % (cos32, F32_COS))
    assert 2 * cos32 <= F32_COS
    model_path = str(tmp_path / "embedder.pth")
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, model_path)
    r_mem = ge2e_harness.spoof_evaluation(g, net, torch.stack(enr_d), torch.stack(gen_d), torch.stack(spo_d))
    random.seed(7)
    avg_eer, avg_spoof = ge2e_harness.test(g, model_path, 2)
    sim_file = torch.load(os.path.join(g["save_simmat_dir"], "simmat_e1_b1")).double()
    sim_ref, sim_mem = r_ref["sim"].cpu().double(), r_mem["sim"].cpu().double()
    d_mem, d_file = float((sim_mem - sim_ref).abs().max()), float((sim_file - sim_ref).abs().max())
    print("end to end: baseline 1 - cos %.3e, entry figure %.3e; |memory - restatement| %.3e, |files - restatement| %.3e" % (base, fig, d_mem, d_file))
    assert d_mem <= fig and d_file <= fig
    for k in ("EER", "thres", "spoof_rate", "FAR", "FRR", "gt_FRR"):
        assert r_mem[k] == r_ref[k], (k, r_mem[k], r_ref[k])
    assert avg_eer == r_ref["EER"] and avg_spoof == r_ref["spoof_rate"]
