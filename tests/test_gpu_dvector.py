"""GPU tests of whole-utterance d-vector extraction (csrc/dvector.hip, spoofsv_amd.dvector, ge2e_harness.dvector_create).  Every
comparison is against the float64 restatements tests/_sv_frontend_ref.py and tests/_dvector_ref.py or against numpy on the device's own
intermediate, never against the code under test.  Run with `-m gpu` on an MI355X."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import _dvector_ref as DR
import _sv_frontend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dvector_host.npz")
U = 2.0 ** -24
HOP, NFFT, WIN = 160, 512, 24


@contextlib.contextmanager
def _mode(name):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(name)
    try:
        yield
    finally:
        spoofsv_amd.set_precision(prev)


def speechlike(rng, n, lead, tail, f0=None):
    """A copy of test_gpu_sv_frontend.speechlike: harmonics of f0 under a slow syllable envelope with a falling spectral tilt, a 1e-4
    noise floor, ``lead`` / ``tail`` samples of near-silence (1e-5) at the edges."""
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


def _batch(wavs, n_max=None):
    """(B, n_max) rows with JUNK (7.0) past every row's live length, and the lengths."""
    n_max = max(n_max or 0, max(len(w) for w in wavs), 1)
    y = np.full((len(wavs), n_max), 7.0, dtype=np.float32)
    for i, w in enumerate(wavs):
        y[i, :len(w)] = w
    return torch.from_numpy(y).to(DEV), torch.tensor([len(w) for w in wavs], dtype=torch.int32, device=DEV)


def _embedder(seed=0):
    from spoofsv_amd.ge2e import SpeechEmbedder
    torch.manual_seed(seed)
    return SpeechEmbedder(40, 768, 3, 256).to(DEV).eval()


def _extractor(net=None, **kw):
    from spoofsv_amd.dvector import DvectorExtractor
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    return DvectorExtractor(TisvFrontEnd(device=DEV), net or _embedder(), **kw)


def _unit(e):
    e = e.detach().cpu().double()
    return e / e.norm(dim=-1, keepdim=True)


def _one_minus_cos(a, b):
    return 0.5 * ((_unit(a) - _unit(b)) ** 2).sum(-1)


@torch.no_grad()
def _baseline(net, feats):
    """As in test_gpu_sv_frontend: the embedder's own fp32-vs-default noise on identical features, on at least 128 rows."""
    feats = feats.repeat(-(-128 // feats.shape[0]), 1, 1).contiguous()
    with _mode("fp32"):
        a = net(feats)
    b = net(feats)
    return float(_one_minus_cos(a, b).max())


def _ragged_case():
    """Rows loud throughout (a gather that reflected at the row's ends, or started at sample 0, would read other samples), with:
    a span starting at 0, one ending at the row's end, one of exactly WIN * HOP samples, a span without a window, spans whose frames
    cross tile (64) and item (256) boundaries, an utterance without a window."""
    rng = np.random.default_rng(60)
    lens = [52000, 30011, 9000, 61000, 2000]
    rows = [speechlike(rng, n, 0, 0) for n in lens]
    spans = [[(0, 9001), (12000, 12000 + WIN * HOP), (20000, 52000)],
             [(5, 30011)],
             [(100, 4100), (4100, 8100), (8200, 8900)],                 # the third has no window
             [(1, 10777), (10777, 60999)],
             [(0, 2000)]]                                               # no window at all
    return rows, spans


def _compact(fr, G):
    """(R, n_fft, Tc) -> (n_fft, G)"""
    R_, N, Tc = fr.shape
    return fr.permute(1, 0, 2).reshape(N, R_ * Tc)[:, :G]


def test_span_frames_bitwise_against_the_restatement():
    """ssv_span_frames is a pure gather: bitwise equal to _sv_frontend_ref.frames cast to float32, poisoned buffer, zero pad columns;
    a second call for frames [256, G) alone gives the same columns."""
    from spoofsv_amd import dvector as D
    ex = _extractor()
    rows, spans = _ragged_case()
    y, n = _batch(rows, n_max=61500)
    pl = ex.plan(y, n, spans)
    assert pl.empty == [4] and pl.windows_per_utterance[4] == 0 and pl.n_frames > 3 * 256
    assert any(t[5] < D.TILE for t in pl.tiles.tolist()) and len(pl.tiles) > 10
    tiles = torch.from_numpy(pl.tiles).to(DEV)
    G, Tc = pl.n_frames, ex.COLS
    Rn = -(-G // Tc)
    assert Rn * Tc > G                                                   # there ARE pad columns
    fr = torch.full((Rn, NFFT, Tc), float("nan"), device=DEV)
    ex.span_frames(y, tiles, 0, G, out=fr)
    got = fr.cpu().numpy()
    flat = np.transpose(got, (1, 0, 2)).reshape(NFFT, Rn * Tc)
    assert not np.isnan(flat).any()
    assert not flat[:, G:].any()                                         # exactly zero
    g = 0
    framed = 0
    for b, sp in enumerate(spans):
        for s, e in sp:
            F = 1 + (e - s) // HOP
            if F <= WIN:
                continue
            ref = R.frames(rows[b][s:e], NFFT, HOP).astype(np.float32)
            assert ref.shape == (NFFT, F)
            assert np.array_equal(flat[:, g:g + F], ref), (b, s, e)
            g += F
            framed += 1
    assert g == G and framed == 8
    part = torch.full((-(-(G - 256) // Tc), NFFT, Tc), float("nan"), device=DEV)
    ex.span_frames(y, tiles, 256, G - 256, out=part)
    p = np.transpose(part.cpu().numpy(), (1, 0, 2)).reshape(NFFT, -1)
    assert np.array_equal(p[:, :G - 256], flat[:, 256:G]) and not p[:, G - 256:].any()


def test_the_framers_agree_with_each_other():
    """ssv_span_frames, ssv_preemph_frames_ragged at preemph = 0.0 (fmaf(-0.0, p, x) == x for every finite p), ssv_frame_signal on the
    contiguous slice and _sv_frontend_ref.frames cast to float32 are copies of the same samples: equal bit for bit on the live frames,
    the ragged entry exactly zero past T_b, the span entry exactly zero in its pad columns.  At hop 160 and 128 the skew shift is 5 on
    the span path and ctz(hop) = 5 / 7 on the ragged one; both take a 64-frame tile at both hops.  Spans: inside one tile from the row's
    first sample; one frame past a tile boundary, interior at both ends; ending at the row's last sample."""
    from spoofsv_amd import _lib, ops
    from spoofsv_amd import dvector as D
    from spoofsv_amd.dvector import DvectorExtractor
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    from spoofsv_amd.vocoder import Vocoder
    n = 24000
    rng = np.random.default_rng(61)
    rows = [speechlike(rng, n, 0, 0) for _ in range(3)]
    y, _ = _batch(rows)
    assert tuple(y.shape) == (3, n)
    net = _embedder()
    for hop in (160, 128):
        spans = [(0, 30 * hop + 7), (777, 777 + 128 * hop), (n - 70 * hop - 3, n)]
        ref = [R.frames(rows[b][s:e], NFFT, hop).astype(np.float32) for b, (s, e) in enumerate(spans)]
        assert [r.shape for r in ref] == [(NFFT, 31), (NFFT, 129), (NFFT, 71)]
        fe = TisvFrontEnd(hop=hop / 16000.0, device=DEV)
        assert (fe.nfft, fe.hop_length) == (NFFT, hop)
        ex = DvectorExtractor(fe, net)
        pl = D.plan([[s] for s in spans], hop, WIN, 12, lengths=[n] * 3)
        G = pl.n_frames
        assert G == 231 and [t[5] for t in pl.tiles.tolist()] == [31, 64, 64, 1, 64, 7]
        fr = torch.full((1, NFFT, ex.COLS), float("nan"), device=DEV)
        ex.span_frames(y, torch.from_numpy(pl.tiles).to(DEV), 0, G, out=fr)
        span = fr[0].cpu().numpy()
        assert not span[:, G:].any(), hop                                # the pad columns: exactly zero (and no NaN is left)
        T = 1 + n // hop
        bounds = torch.tensor(spans, dtype=torch.int32, device=DEV)
        rag = torch.full((3, NFFT, T), float("nan"), device=DEV)
        nf = torch.full((3,), -1, dtype=torch.int32, device=DEV)
        _lib.call("ssv_preemph_frames_ragged", ops._p(y), ops._p(bounds), ops._p(rag), ops._p(nf), 3, n, NFFT, hop, T, 0.0, ops._stream())
        assert nf.cpu().tolist() == [31, 129, 71]
        rag = rag.cpu().numpy()
        voc = Vocoder(NFFT, hop, DEV)
        g = 0
        for b, (s, e) in enumerate(spans):
            F = ref[b].shape[1]
            assert np.array_equal(span[:, g:g + F], ref[b]), (hop, b, "span_frames")
            assert np.array_equal(rag[b, :, :F], ref[b]), (hop, b, "preemph_frames_ragged")
            assert not rag[b, :, F:].any(), (hop, b)                     # past T_b: exactly zero
            assert np.array_equal(voc.frames(y[b:b + 1, s:e].contiguous())[0].cpu().numpy(), ref[b]), (hop, b, "frame_signal")
            g += F
        assert g == G


def test_all_frame_log_mel_vs_restatement():
    """Every frame of every span: mel POWER within mel_basis . (2 |S| d + d^2), d = 2e-5 max|S| -- the bar test_gpu_sv_frontend.py holds
    the two slices to.  Then ssv_gather_windows, bitwise against numpy slicing of the device's own log-mel array."""
    ex = _extractor()
    rows, spans = _ragged_case()
    y, n = _batch(rows, n_max=61500)
    pl = ex.plan(y, n, spans)
    mel_dev = ex.log_mel(y, pl)
    lm = mel_dev.cpu().numpy().astype(np.float64)
    mel = R.mel_filterbank(16000, 512, 40)
    worst_ratio = worst_log = 0.0
    g = 0
    for b, sp in enumerate(spans):
        for s, e in sp:
            F = 1 + (e - s) // HOP
            if F <= WIN:
                continue
            S, mag = R.log_mel(rows[b][s:e])
            d = 2e-5 * mag.max()
            bound = mel @ (2 * mag * d + d * d)
            got = lm[g:g + F]
            worst_ratio = max(worst_ratio, float((np.abs(10.0 ** got - 10.0 ** S.T) / bound.T).max()))
            worst_log = max(worst_log, float(np.abs(got - S.T).max()))
            g += F
    print("all-frame features: worst mel-power deviation %.3e of its bound, worst log10 deviation %.3e" % (worst_ratio, worst_log))
    assert worst_ratio <= 1.0
    wins, _ = ex.window_features(y, n, spans)
    w = wins.cpu().numpy()
    own = mel_dev.cpu().numpy()
    assert w.shape == (pl.n_windows, WIN, 40) and pl.n_windows > 60
    for k, g0 in enumerate(pl.g0.tolist()):
        assert np.array_equal(w[k], own[g0:g0 + WIN]), k
    # and the windows are the restatement's windows, in its order
    ref = np.concatenate([DR.features(rows[b], spans[b]) for b in range(len(rows))])
    assert ref.shape == w.shape
    assert np.abs(w - ref).max() <= 10 * worst_log + 1e-12


def _segment_mean(e, offs, normalize):
    from spoofsv_amd import _lib, ops
    out = torch.full((len(offs) - 1, e.shape[1]), float("nan"), device=DEV)
    o = torch.tensor(offs, dtype=torch.int32, device=DEV)
    _lib.call("ssv_segment_mean", ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(out.data_ptr()), e.shape[0],
              len(offs) - 1, e.shape[1], normalize, ops._stream())
    return out.cpu().numpy()


def test_segment_mean_vs_float64():
    """Random (600, 256) rows, the golden partitions of n = 600 (at most 4 rows each): within 8 x 2^-24 x max|e| of float64 -- an
    ascending fp32 sum of r rows makes r - 1 roundings of partial sums no larger than r max|e|, and one more for the division: below
    2 r u max|e| for r <= 4.  One partition over all 600 rows: the same factor, 2 r.  normalize = 1: unit rows to 1e-6.  The entry
    exposes no launch shape, so there is nothing to vary."""
    g = np.load(GOLDEN)
    a, b = int(g["part_off"][599]), int(g["part_off"][600])
    offs = [0] + g["part_end"][a:b].astype(int).tolist()
    assert offs[-1] == 600 and max(np.diff(offs)) <= 4
    e64 = np.random.default_rng(70).standard_normal((600, 256))
    e = torch.from_numpy(e64.astype(np.float32)).to(DEV)
    e64 = e.cpu().numpy().astype(np.float64)
    amax = np.abs(e64).max()
    got = _segment_mean(e, offs, 0)
    want = np.stack([e64[p:q].mean(axis=0) for p, q in zip(offs[:-1], offs[1:])])
    err = float(np.abs(got - want).max())
    print("segment mean: worst |fp32 - float64| %.3e (bar %.3e)" % (err, 8 * U * amax))
    assert err <= 8 * U * amax
    one = _segment_mean(e, [0, 600], 0)
    err1 = float(np.abs(one - e64.mean(axis=0)).max())
    print("segment mean, one partition of 600 rows: %.3e (bar %.3e)" % (err1, 2 * 600 * U * amax))
    assert err1 <= 2 * 600 * U * amax
    nrm = _segment_mean(e, offs, 1).astype(np.float64)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-6
    assert np.abs(nrm - want / np.linalg.norm(want, axis=1, keepdims=True)).max() <= 16 * U * amax / np.linalg.norm(want, axis=1).min()
    assert np.array_equal(_segment_mean(e, offs, 0), got)
    assert not _segment_mean(e, [0, 0, 3], 0)[0].any()                    # an empty partition is zeros


def _e2e_case():
    rng = np.random.default_rng(61)
    rows, spans = [], []
    for k in range(13):
        n = int(rng.integers(24000, 64000))
        rows.append(speechlike(rng, n, 0, 0))
        cuts = sorted(int(c) for c in rng.integers(0, n, size=4))
        sp = [(cuts[0], cuts[1]), (cuts[1], cuts[2]), (cuts[2] + int(rng.integers(0, 800)), n if k % 2 else cuts[3])]
        spans.append([(s, min(e, n)) for s, e in sp if e > s])
    return rows, spans


@torch.no_grad()
def test_end_to_end_sequence_vs_restatement():
    """13 ragged utterances with explicit multi-span ``spans``: the device's window embeddings against the same seeded full-size
    SpeechEmbedder on the restatement's float64 features -- worst 1 - cos no more than 4 x the embedder's own fp32-vs-default noise on
    those features (the criterion of test_embeddings_of_gpu_features_vs_restatement_features) -- and the averaged rows against float64
    partition means of the device's own window embeddings under the fp32-sum bound of test_segment_mean_vs_float64."""
    net = _embedder()
    ex = _extractor(net)
    rows, spans = _e2e_case()
    y, n = _batch(rows, n_max=65000)
    ref = [DR.features(rows[b], spans[b]) for b in range(len(rows))]
    nw = [len(r) for r in ref]
    assert len(rows) >= 12 and sum(nw) >= 128 and min(nw) > 0
    ref_t = torch.from_numpy(np.concatenate(ref).astype(np.float32)).to(DEV)
    base = _baseline(net, ref_t)
    e_ref = net(ref_t)
    E, pl = ex.window_embeddings(y, n, spans)
    assert pl.windows_per_utterance == nw
    fig = float(_one_minus_cos(E, e_ref).max())
    seq, rpu = ex(y, n, spans)
    assert seq.is_cuda and seq.dtype == torch.float32 and seq.shape == (sum(rpu), 256)
    E64 = E.cpu().numpy().astype(np.float64)
    want = np.concatenate([DR.align(E64[a:a + k]) for a, k in zip(np.cumsum([0] + nw[:-1]), nw)])
    assert rpu == [len(DR.partitions(k)) for k in nw] and want.shape == tuple(seq.shape)
    err = float(np.abs(seq.cpu().numpy() - want).max())
    bar = 8 * U * np.abs(E64).max()
    print("end to end: %d windows, baseline 1 - cos %.3e, device-vs-restatement windows %.3e (bar %.3e); rows vs float64 means %.3e (bar %.3e)"
          % (sum(nw), base, fig, 4 * base, err, bar))
    assert fig <= 4 * base, (fig, base)
    assert err <= bar
    # utterance-level d-vectors: unit norm, the normalised mean of all windows
    dv, wpu = ex.utterance_dvectors(y, n, spans)
    assert wpu == nw and dv.shape == (len(rows), 256)
    dv = dv.cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(dv, axis=1) - 1.0).max() <= 1e-6
    m = np.stack([E64[a:a + k].mean(axis=0) for a, k in zip(np.cumsum([0] + nw[:-1]), nw)])
    assert np.abs(dv - m / np.linalg.norm(m, axis=1, keepdims=True)).max() <= 2 * max(nw) * U * np.abs(E64).max() / np.linalg.norm(m, axis=1).min()


@torch.no_grad()
def test_window_embeddings_vs_float64_oracle_at_24_frames():
    """The embedder at T = 24 on real window features (a shape no other test runs): against oracle.ge2e_oracle.speech_embedder in
    float64 under the project's 2e-5 embedder bar (max-norm and L2)."""
    from _golden import rel_err, rel_l2
    from oracle import ge2e_oracle as GO
    net = _embedder(3)
    rows, spans = _e2e_case()
    ref = np.concatenate([DR.features(rows[b], spans[b]) for b in range(len(rows))]).astype(np.float32)
    assert ref.shape[0] >= 128 and ref.shape[1:] == (24, 40)
    x = torch.from_numpy(ref).to(DEV)
    eo = GO.speech_embedder(x, net.state_dict(), dtype=torch.float64)
    eg = net(x)
    print("embedder at T = 24 on %d windows: max-norm %.2e, rel L2 %.2e (bar 2e-5)" % (ref.shape[0], rel_err(eg, eo), rel_l2(eg, eo)))
    assert rel_err(eg, eo) < 2e-5 and rel_l2(eg, eo) < 2e-5


@torch.no_grad()
def test_wiring_default_spans_empty_utterances_chunks_and_cache():
    from spoofsv_amd import ge2e
    net = _embedder()
    ex = _extractor(net, windows_per_call=512)
    rng = np.random.default_rng(62)
    rows = [speechlike(rng, 50000, 6000, 9000), speechlike(rng, 3000, 0, 0), speechlike(rng, 64000, 0, 12000), speechlike(rng, 41000, 3000, 0),
            np.zeros(0, dtype=np.float32), speechlike(rng, 57000, 0, 0), speechlike(rng, 60000, 100, 100)]
    rows += [speechlike(rng, 64000 - 500 * k, 0, 0) for k in range(8)]
    y, n = _batch(rows, n_max=64000)
    # spans=None equals the trim bounds read back and passed as spans
    seq, rpu = ex(y, n)
    key1, ws1 = ge2e._FWD_CACHE[net]["key"], ge2e._FWD_CACHE[net]["ws"].data_ptr()
    b = ex.fe.trim_bounds(y, n, 30).cpu().tolist()
    assert b[0][0] > 0 and b[0][1] < 50000
    seq2, rpu2 = ex(y, n, [[(s, e)] for s, e in b])
    assert rpu == rpu2 and torch.equal(seq, seq2)
    # a second call on the same weights re-used the kept workspace: same key, same buffer
    assert ge2e._FWD_CACHE[net]["key"] == key1 and ge2e._FWD_CACHE[net]["ws"].data_ptr() == ws1 and key1[0] == 512
    # utterances without a window give no row
    assert rpu[1] == 0 and rpu[4] == 0 and all(r > 0 for i, r in enumerate(rpu) if i not in (1, 4)) and seq.shape[0] == sum(rpu)
    ref_rows = [len(DR.partitions(len(DR.features(rows[i], [tuple(b[i])])))) if i not in (1, 4) else 0 for i in range(len(rows))]
    assert rpu == ref_rows
    # chunked: several frame chunks, several embedder chunks and a padded last one.  Both chunk sizes are >= 128 windows (below that the
    # library runs every product in plain fp32, another arithmetic); the split-fp16 operand scale of a chunk is the power of two of its
    # largest |feature|, which is the same for every chunk here (checked), so the chunks compute what the single chunk computes.
    wins, pl = ex.window_features(y, n)
    assert 256 < pl.n_windows < 512 and pl.n_windows % 128 != 0 and pl.n_frames > 3 * 512
    amax = [float(wins[lo:lo + 128].abs().max()) for lo in range(0, pl.n_windows, 128)] + [float(wins.abs().max())]
    assert len({int(np.floor(np.log2(a))) for a in amax}) == 1, amax
    small = _extractor(net, windows_per_call=128, frames_per_call=512)
    E_big, _ = ex.window_embeddings(y, n)
    E_small, _ = small.window_embeddings(y, n)
    assert torch.equal(small.window_features(y, n)[0], wins)
    assert torch.equal(E_small, E_big)
    seq3, rpu3 = small(y, n)
    assert rpu3 == rpu and torch.equal(seq3, seq)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ex(y.cpu(), n.cpu())


def _vad_stub(path):
    """A stand-in for VAD_chunk's times: the file's interior in chunks of at most 0.4 s (VAD_segments.py:138-149), with a gap in every
    second file and no voice at all in one."""
    from scipy.io import wavfile
    sr, w = wavfile.read(path)
    dur = len(w) / sr
    if path.endswith("spk3" + os.sep + "u0.wav"):
        return []
    base = os.path.basename(path)
    intervals = [(0.1, dur - 0.1)] if base == "u0.wav" else [(0.05, 0.62), (0.9, dur)]
    times = []
    for t0, t1 in intervals:
        start, end = np.round(t0, decimals=2), np.round(t1, decimals=2)
        j = start
        while j + .4 < end:
            end_j = np.round(j + .4, decimals=2)
            times.append((j, end_j))
            j = end_j
        times.append((j, end))
    return times


@pytest.mark.parametrize("folders", [11, 13])
def test_dvector_create_driver(tmp_path, folders, capsys):
    """11 (and 13) speaker folders x 2 short seeded wavs, one of them at 22,050 Hz, one without voice, a stub VAD: the four files, their
    dtypes and shapes, rows and ids per speaker and the train / test split point (``i > (total // 10) * 9``: after folder 10, which for
    11 folders leaves the test set empty) against _dvector_ref."""
    from scipy.io import wavfile
    from spoofsv_amd import ge2e_harness
    rng = np.random.default_rng(63)
    dirs, counts = [], []
    for i in range(folders):
        d = tmp_path / "audio" / ("spk%d" % i)
        os.makedirs(d)
        (d / "notes.txt").write_text("not a wav")
        per = []
        for k in range(2):
            sr = 22050 if (i, k) == (5, 1) else 16000
            n = int(rng.integers(int(1.3 * sr), int(2.2 * sr)))
            w = speechlike(rng, n, 0, 0)
            p = str(d / ("u%d.wav" % k))
            wavfile.write(p, sr, w)
            n16 = int(np.ceil(n * (16000.0 / sr)))
            times = _vad_stub(p)
            if times:
                per.append(DR.rows_of_file(times, n16))
        dirs.append(str(d))
        counts.append(per)
    cfg = ge2e_harness.default_config()
    cfg["device"] = DEV
    net = _embedder(1)
    out = str(tmp_path / "out")
    paths = ge2e_harness.dvector_create(cfg, dirs, vad=_vad_stub, out_dir=out, utterances_per_batch=8, net=net)
    assert [os.path.basename(p) for p in paths] == ["train_sequence.npy", "train_cluster_id.npy", "test_sequence.npy", "test_cluster_id.npy"]
    assert capsys.readouterr().out.count("No voice activity detected") == 1
    tr_s, tr_i, te_s, te_i = [np.load(p) for p in paths]
    want_tr, want_te = DR.split(counts)
    assert tr_s.dtype == np.float64 and te_s.dtype == np.float64 and tr_i.dtype.kind == "U" and te_i.dtype.kind == "U"
    assert tr_s.shape == (len(want_tr), 256) and te_s.shape == (len(want_te), 256)
    assert tr_i.tolist() == want_tr and te_i.tolist() == want_te
    assert len(counts[3]) == 1 and all(c > 0 for per in counts for c in per)
    assert want_tr[-1] == "10" and (want_te == [] if folders == 11 else (want_te[0] == "11" and want_te[-1] == "12"))
    assert np.isfinite(tr_s).all() and np.abs(np.linalg.norm(tr_s, axis=1) - 1.0).max() < 0.5      # means of unit vectors
