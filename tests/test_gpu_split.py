"""GPU tests of the voiced-interval split (ssv_split_intervals, ssv_select_spans, ssv_tisv_frames_table of csrc/sv_frontend.hip,
TisvFrontEnd.interval_slices / split_call, ge2e_harness.preprocess_tisv_synthetic, dvector_create(vad="split")).  Every comparison is
against the float64 restatements tests/_split_ref.py and tests/_sv_frontend_ref.py, never against the code under test.
Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest
import torch

import _split_ref as S
import _sv_frontend_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0x5A5A5A5A
GAPS_150K = [(0, 5000), (30000, 41000), (70000, 73000), (100000, 118000), (140000, 150000)]


def speechlike(rng, n, gaps=(), f0=None):
    """test_gpu_sv_frontend.speechlike with near-silence (1e-5) over every (start, end) of ``gaps`` instead of a lead and a tail:
    harmonics of f0 under a slow syllable envelope with a falling spectral tilt, a 1e-4 noise floor."""
    f0 = f0 or rng.uniform(90, 220)
    t = np.arange(n) / 16000.0
    y = np.zeros(n)
    for h in range(1, 25):
        y += rng.uniform(0.3, 1.0) / h ** 1.5 * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.5, 4.0) * t + rng.uniform(0, 6.28))
    y = 0.25 * y * env + 1e-4 * rng.standard_normal(n)
    gate = np.ones(n)
    for s, e in gaps:
        gate[s:e] = 0.0
    return (y * gate + 1e-5 * rng.standard_normal(n)).astype(np.float32)


def _batch(wavs, n_max=None):
    """(B, n_max) rows with JUNK (7.0) past every row's live length -- a kernel that read beyond n[b] would show it -- and the lengths."""
    n_max = max(n_max or 0, max(len(w) for w in wavs), 1)
    y = np.full((len(wavs), n_max), 7.0, dtype=np.float32)
    for i, w in enumerate(wavs):
        y[i, :len(w)] = w
    return torch.from_numpy(y).to(DEV), torch.tensor([len(w) for w in wavs], dtype=torch.int32, device=DEV)


def _split_rows(seed):
    rng = np.random.default_rng(seed)
    return [speechlike(rng, 150000, GAPS_150K),                  # 293 frames: more than the workgroup's 256 threads, runs in both chunks
            speechlike(rng, 64000, [(30000, 38000)]),
            speechlike(rng, 33333, [(12000, 16000)]),            # no multiple of the hop: the last end is clipped to n
            (0.3 * rng.standard_normal(50000)).astype(np.float32),
            np.zeros(20000, dtype=np.float32),
            speechlike(rng, 700, [])[:700],                      # no longer than half a frame: zero padding
            np.zeros(0, dtype=np.float32)]


_CLEAR = {}


def clear_rows():
    """The rows of the first seed (40, 41, 42, 43) none of whose frames lies within 1e-3 dB of the threshold in float64, and their
    restated intervals: the condition under which fp32 energies must give the same integers.  Computed once per session, never changed."""
    if not _CLEAR:
        for seed in (40, 41, 42, 43):
            rows = _split_rows(seed)
            refs = [S.split(r, 30) for r in rows]
            margin = min(float(np.abs(db + 30.0).min()) for _, db in refs if len(db))
            if margin > 1e-3:
                _CLEAR.update(rows=rows, refs=[iv for iv, _ in refs], margin=margin, seed=seed)
                break
        else:
            pytest.fail("no seed gave inputs clear of the threshold")
    return _CLEAR["rows"], _CLEAR["refs"]


def _raw_split(y, n, K, guard=0):
    """ssv_split_intervals into poisoned buffers, ``guard`` extra ints after the (B, K, 2) intervals."""
    from spoofsv_amd import _lib, ops
    from spoofsv_amd.ops import _p
    B, n_max = y.shape
    buf = torch.full((B * K * 2 + guard,), POISON, dtype=torch.int32, device=DEV)
    cnt = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    _lib.call("ssv_split_intervals", _p(y), _p(n), _p(buf), _p(cnt), B, n_max, K, 30.0, 2048, 512, ops._stream())
    buf, cnt = buf.cpu().numpy(), cnt.cpu().numpy()
    return buf[:B * K * 2].reshape(B, K, 2), cnt, buf[B * K * 2:]


def test_intervals_equal_the_restatement():
    """ssv_split_intervals: integer for integer, on rows clear of the threshold (asserted on the CPU first)."""
    rows, refs = clear_rows()
    print("split: seed %d, nearest frame %.3f dB from the threshold, intervals per row %s" % (_CLEAR["seed"], _CLEAR["margin"], [len(r) for r in refs]))
    assert [len(r) for r in refs] == [4, 2, 2, 1, 1, 1, 0]
    y, n = _batch(rows, n_max=151000)                            # n_max larger than every row
    K = 6
    iv, cnt, _ = _raw_split(y, n, K)
    for b, ref in enumerate(refs):
        assert cnt[b] == len(ref), (b, cnt[b], ref)
        assert np.array_equal(iv[b, :len(ref)], ref), (b, iv[b], ref)
        assert not iv[b, len(ref):].any()                        # (0, 0) from count on, nothing left of the poison
    assert refs[4].tolist() == [[0, 20000]] and refs[2][-1, 1] == 33333 and refs[0][0, 0] > 0 and refs[0][-1, 1] < 150000
    from spoofsv_amd.sv_frontend import split_intervals
    iv2, cnt2 = split_intervals(y, n, 30, K)                     # the Python entry gives the same
    assert np.array_equal(iv2.cpu().numpy(), iv) and np.array_equal(cnt2.cpu().numpy(), cnt) and tuple(iv2.shape) == (7, K, 2)


def test_first_start_and_last_end_are_the_trim_bounds():
    """Bit for bit on 8 rows of amplitude-modulated noise whose level wanders across the threshold: no margin condition, both kernels
    run the same fp32 energy stage."""
    from spoofsv_amd.sv_frontend import trim_bounds
    rng = np.random.default_rng(44)
    rows = []
    for n in (150000, 90001, 64000, 51200, 40000, 33333, 20480, 9000):
        t = np.arange(n) / 16000.0
        level = 1.2 * np.sin(2 * np.pi * rng.uniform(0.4, 1.5) * t + rng.uniform(0, 6.28)) + 0.8 * np.sin(2 * np.pi * rng.uniform(2, 5) * t)
        rows.append((10.0 ** (level - 2.0) * rng.standard_normal(n)).astype(np.float32))       # -80 dB ... 0 dB
    y, n = _batch(rows, n_max=151000)
    K = 64
    iv, cnt, _ = _raw_split(y, n, K)
    tb = trim_bounds(y, n, 30).cpu().numpy()
    assert cnt.max() <= K and cnt.min() >= 1 and cnt.max() >= 3, cnt
    for b in range(len(rows)):
        assert (iv[b, 0, 0], iv[b, cnt[b] - 1, 1]) == (tb[b, 0], tb[b, 1]), (b, iv[b, :cnt[b]], tb[b])
        assert np.all(iv[b, 1:cnt[b], 0] > iv[b, :cnt[b] - 1, 1])


def test_overflow_is_counted_not_stored():
    rows, refs = clear_rows()
    y, n = _batch([rows[0], rows[4]], n_max=151000)
    iv, cnt, guard = _raw_split(y, n, 2, guard=8)
    assert cnt.tolist() == [4, 1]
    assert np.array_equal(iv[0], refs[0][:2])
    assert iv[1].tolist() == [[0, 20000], [0, 0]]                # the next row is not written over
    assert np.all(guard.view(np.uint32) == POISON)


def _raw_select(intervals, count, n_max, min_len, first, R):
    from spoofsv_amd import _lib, ops
    from spoofsv_amd.ops import _p
    iv = torch.tensor(intervals, dtype=torch.int32, device=DEV)
    cnt = torch.tensor(count, dtype=torch.int32, device=DEV)
    table = torch.full((R * 3 + 4,), POISON, dtype=torch.int32, device=DEV)
    total = torch.full((1,), POISON, dtype=torch.int32, device=DEV)
    _lib.call("ssv_select_spans", _p(iv), _p(cnt), _p(table), _p(total), iv.shape[0], iv.shape[1], n_max, min_len, first, R, ops._stream())
    table = table.cpu().numpy()
    assert np.all(table[R * 3:].view(np.uint32) == POISON)
    return table[:R * 3].reshape(R, 3).tolist(), int(total.item())


def test_select_spans_on_a_hand_written_table():
    """Order, the strict compare at min_len and min_len + 1, a count above K, spans that do not fit the row, paging through ``first``."""
    n_max, min_len = 1000, 100
    intervals = [[(0, 100), (150, 251), (300, 900), (0, 1000)],          # count 3: 100 samples fail, 101 pass; the fourth is not looked at
                 [(0, 500), (500, 601), (610, 650), (700, 1200)],        # count 6 > K: all four looked at; the last ends beyond n_max
                 [(0, 999), (0, 999), (0, 999), (0, 999)],               # count 0
                 [(-5, 400), (10, 990), (0, 0), (0, 0)]]                 # a negative start does not fit
    count = [3, 6, 0, 2]
    want = [[0, 150, 251], [0, 300, 900], [1, 0, 500], [1, 500, 601], [3, 10, 990]]
    pad = [-1, 0, 0]
    table, total = _raw_select(intervals, count, n_max, min_len, 0, 8)
    assert total == 5 and table == want + [pad] * 3
    pages = []
    for first in (0, 2, 4):
        t, tot = _raw_select(intervals, count, n_max, min_len, first, 2)
        assert tot == 5
        pages += t
    assert pages == table[:6]
    t, tot = _raw_select(intervals, count, n_max, min_len, 7, 2)         # first beyond the last span: nothing but padding
    assert tot == 5 and t == [pad, pad]
    # 700 spans: more than one chunk of the workgroup's prefix count; every third passes
    big = [[(0, 101 if (4 * b + k) % 3 == 0 else 100) for k in range(4)] for b in range(175)]
    t, tot = _raw_select(big, [4] * 175, n_max, min_len, 0, 300)
    rows = [i // 4 for i in range(700) if i % 3 == 0]
    assert tot == len(rows) == 234 and [r[0] for r in t[:234]] == rows and t[234:] == [pad] * 66


@pytest.mark.parametrize("tisv_frame", [120, 24])
def test_table_frames_are_the_restated_frames_bitwise(tisv_frame):
    """ssv_tisv_frames_table is a pure gather: [:, :T] and [:, -T:] of _sv_frontend_ref.frames(seg, 512, 160) cast to float32, on rows
    that are loud THROUGHOUT (a reflection at the row's ends instead of the segment's would read other samples); unusable rows give
    zero frames and valid 0, the poison is gone everywhere."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    fe = TisvFrontEnd(device=DEV, tisv_frame=tisv_frame)
    T, ml = tisv_frame, fe.min_len
    assert ml == int(np.floor(R.utter_min_len(tisv_frame=T)))
    rng = np.random.default_rng(45)
    rows = [speechlike(rng, 60000) for _ in range(3)]
    y, _ = _batch(rows, n_max=61000)
    table = [(0, 7001, 52003), (1, 0, 30000), (2, 40000, 60000), (-1, 0, 0), (1, 100, 100 + ml), (1, 100, 101 + ml),
             (3, 0, 30000), (0, 50000, 61001), (2, 12345, 12345 + ml + 160 * 3 + 7)]
    want_valid = [1, 1, 1, 0, 0, 1, 0, 0, 1]
    tb = torch.tensor(table, dtype=torch.int32, device=DEV)
    fr, valid = fe.frames_table(y, tb)
    assert tuple(fr.shape) == (2 * len(table), 512, T) and valid.cpu().tolist() == want_valid
    fr = fr.cpu().numpy()
    for r, (row, s, e) in enumerate(table):
        if not want_valid[r]:
            assert not fr[2 * r].any() and not fr[2 * r + 1].any()
            continue
        ref = R.frames(rows[row][s:e], 512, 160).astype(np.float32)
        assert ref.shape[1] == 1 + (e - s) // 160 >= T
        assert np.array_equal(fr[2 * r], ref[:, :T]) and np.array_equal(fr[2 * r + 1], ref[:, -T:]), r


def _ref_slices(y16, T):
    """Per kept interval of one utterance: (bounds, [(restated log-mel (T, nmels), mel-power bound (T, nmels)) for first, last])."""
    mel = R.mel_filterbank(16000, 512, 40)
    out = []
    for s, e in S.interval_slices(y16, tisv_frame=T)[1]:
        Sm, mag = R.log_mel(np.asarray(y16[s:e], dtype=np.float64))
        d = 2e-5 * mag.max()
        bound = mel @ (2 * mag * d + d * d)
        out.append(((int(s), int(e)), [(Sm[:, sl].T, bound[:, sl].T) for sl in (slice(0, T), slice(Sm.shape[1] - T, Sm.shape[1]))]))
    return out


def _worst_ratio(got, ref_bound):
    """Largest mel-power deviation as a fraction of its bound.  Where the bound is 0 (a segment of exact zeros: |S| = 0) the feature is
    log10(1e-6) evaluated in float32, and its bar is 4 ulp of a float32 in [4, 8), 4 x 2^-21, on the feature itself: the rounding of
    1e-6 to float32 moves it by 3e-8, the rest is log10f's own error."""
    ref, bound = ref_bound
    got = got.astype(np.float64)
    dev = np.abs(10.0 ** got - 10.0 ** ref)
    return float(np.divide(dev, bound, out=np.abs(got - ref) / (4 * 2.0 ** -21), where=bound > 0).max())


def clear_slices():
    """(row, ((start, end), [first, last])) of every kept interval of clear_rows(), in table order; computed once."""
    if "slices" not in _CLEAR:
        rows, _ = clear_rows()
        _CLEAR["slices"] = [(b, sl) for b, r in enumerate(rows) for sl in _ref_slices(r, 120)]
    return _CLEAR["slices"]


@pytest.mark.parametrize("dft_mode", ["fp32", "default"])
def test_interval_slices_vs_restatement(dft_mode):
    """split -> select -> frames_table -> DFT -> mel/log: table, valid, total and count exact; mel POWER (10 ** feature) within
    mel_basis . (2 |S| d + d^2), d = 2e-5 max|S| of the interval (the bar of test_gpu_sv_frontend.test_features_vs_restatement)."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    fe = TisvFrontEnd(device=DEV, dft_mode=dft_mode)
    rows, refs = clear_rows()
    y, n = _batch(rows, n_max=151000)
    f, table, valid, total, count = fe.interval_slices(y, n)
    assert tuple(f.shape) == (14, 2, 120, 40) and tuple(table.shape) == (14, 3) and tuple(valid.shape) == (14,)
    want = clear_slices()
    want_table = [[b, s, e] for b, ((s, e), _) in want]
    assert [t[0] for t in want_table] == [0, 0, 0, 0, 1, 1, 3, 4]         # the intervals of the 33,333-sample row are too short
    assert count.cpu().tolist() == [len(r) for r in refs] and total.cpu().tolist() == [8]
    assert table.cpu().tolist() == want_table + [[-1, 0, 0]] * 6 and valid.cpu().tolist() == [1] * 8 + [0] * 6
    f = f.cpu().numpy()
    worst = max(_worst_ratio(f[r, k], sl[1][k]) for r, (_, sl) in enumerate(want) for k in (0, 1))
    print("interval slices (%s DFT): worst mel-power deviation %.3e of its bound" % (dft_mode, worst))
    assert worst <= 1.0
    # paging: capacity 3, first 3 holds spans 3, 4, 5 -- the same numbers
    f2, table2, valid2, total2, _ = fe.interval_slices(y, n, capacity=3, first=3)
    assert total2.cpu().tolist() == [8] and table2.cpu().tolist() == want_table[3:6] and valid2.cpu().tolist() == [1, 1, 1]
    assert np.array_equal(f2.cpu().numpy(), f[3:6])


def test_captured_replay_equals_eager():
    """split_call, the whole chain from (y, lengths) at 22,050 Hz to features, under torch.cuda.graph, replayed on two ragged batches."""
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    fe = TisvFrontEnd(device=DEV)
    rng = np.random.default_rng(46)
    batches = [[speechlike(rng, 120000, [(0, 4000), (50000, 62000)]), speechlike(rng, 40000), speechlike(rng, 20000, [(8000, 12000)]), np.zeros(0, dtype=np.float32)],
               [speechlike(rng, 45000, [(40000, 45000)]), speechlike(rng, 120000, [(30000, 40000), (75000, 82000)]), speechlike(rng, 64000), speechlike(rng, 90000, [(0, 9000)])]]
    n_max = 120000
    eager = []
    for wavs in batches:
        y, n = _batch(wavs, n_max)
        eager.append([t.clone() for t in fe.split_call(y, n, 22050)])
    sy, sn = torch.zeros((4, n_max), device=DEV), torch.zeros((4,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fe.split_call(sy, sn, 22050)
    for wavs, want in zip(batches, eager):
        y, n = _batch(wavs, n_max)
        sy.copy_(y)
        sn.copy_(n)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a, b)
    assert eager[0][3].tolist() == [3] and eager[0][4].tolist() == [2, 1, 2, 0] and eager[1][3].tolist() == [6]
    assert eager[0][2].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]


def _margin(y16):
    db = S.split(y16, 30)[1]
    return float(np.abs(db + 30.0).min()) if len(db) else np.inf


def test_preprocess_tisv_synthetic_end_to_end(tmp_path):
    """3 speakers x 2 files at tisv_frame = 24 through the device, from wav paths and once more from device tuples: file names and
    shapes equal the run with the restatement injected, values within the bar of test_interval_slices_vs_restatement (inputs clear of
    the threshold by 1e-3 dB, asserted)."""
    from scipy.io import wavfile
    from spoofsv_amd import ge2e_harness
    T = 24
    rng = np.random.default_rng(47)
    shapes = [[(30000, [(0, 2000), (12000, 16000)]), (9000, [])], [(3000, []), (22000, [(8000, 13000), (20000, 22000)])], [(14000, [(0, 6000)]), (40001, [(10000, 14000), (24000, 28000)])]]
    waves = {"spk%d" % i: [speechlike(rng, n, gaps) for n, gaps in per] for i, per in enumerate(shapes)}
    assert min(_margin(w) for ws in waves.values() for w in ws) > 1e-3
    speakers = {}
    for name, ws in waves.items():
        speakers[name] = []
        for k, w in enumerate(ws):
            p = str(tmp_path / "wav" / name / ("u%d.wav" % k))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            wavfile.write(p, 16000, w)
            speakers[name].append(p)

    def cfg_for(name):
        c = ge2e_harness.default_config()
        c["device"] = DEV
        c["data"]["train_path"], c["data"]["test_path"], c["data"]["tisv_frame"] = str(tmp_path / name / "train"), str(tmp_path / name / "test"), T
        return c
    ref = ge2e_harness.preprocess_tisv_synthetic(cfg_for("ref"), speakers, front_end=lambda wavs, sr: S.front_end(wavs, sr, tisv_frame=T))
    dev = ge2e_harness.preprocess_tisv_synthetic(cfg_for("dev"), speakers)
    tuples = {name: ge2e_harness.pad_batch(ws, DEV) + (16000,) for name, ws in waves.items()}
    mem = ge2e_harness.preprocess_tisv_synthetic(cfg_for("mem"), tuples)
    tail = lambda ps: [os.sep.join(p.split(os.sep)[-2:]) for p in ps]
    assert tail(ref) == tail(dev) == tail(mem) == ["test/speaker0.npy", "test/speaker1.npy", "test/speaker2.npy"]
    worst, n_slices = 0.0, []
    for i, name in enumerate(waves):
        bars = [rb for w in waves[name] for _, sl in _ref_slices(w, T) for rb in sl]       # file, interval, first before last
        a, b, c = np.load(ref[i]), np.load(dev[i]), np.load(mem[i])
        assert a.shape == b.shape == c.shape == (len(bars), 40, T) and b.dtype == c.dtype == np.float32
        assert np.array_equal(b, c)                              # the same device pass, from files or from memory
        n_slices.append(len(bars))
        for k, rb in enumerate(bars):
            assert np.array_equal(a[k], rb[0].T.astype(np.float32))
            worst = max(worst, _worst_ratio(b[k].T, rb))
    print("preprocess_tisv_synthetic: slices per speaker %s, worst mel-power deviation %.3e of its bound" % (n_slices, worst))
    assert n_slices == [6, 4, 8] and worst <= 1.0
    with pytest.raises(RuntimeError, match=r"u1\.wav has 3 voiced intervals"):
        ge2e_harness.preprocess_tisv_synthetic(cfg_for("over"), {"spk2": speakers["spk2"]}, max_intervals=2)


def test_dvector_create_with_the_energy_split(tmp_path, capsys):
    """vad="split" writes the same four files, byte for byte, as vad= a callable that returns the restatement's intervals as times
    (inputs clear of the threshold by 1e-3 dB, asserted); an empty file has no interval on either path."""
    from scipy.io import wavfile
    from spoofsv_amd import ge2e_harness
    from spoofsv_amd.ge2e import SpeechEmbedder
    rng = np.random.default_rng(48)
    waves = [speechlike(rng, 40000, [(0, 3000), (18000, 24000)]), speechlike(rng, 30000, [(12000, 15000), (27000, 30000)]), np.zeros(0, dtype=np.float32)]
    assert min(_margin(w) for w in waves) > 1e-3
    dirs, times = [], {}
    for i, w in enumerate(waves):
        d = tmp_path / "audio" / ("spk%d" % min(i, 1))
        os.makedirs(d, exist_ok=True)
        p = str(d / ("u%d.wav" % i))
        wavfile.write(p, 16000, w)
        # (s + 0.5) / sr: int(t * sr), as VAD_chunk's consumers index, is s whatever the rounding of the quotient
        times[p] = [((s + 0.5) / 16000.0, (e + 0.5) / 16000.0) for s, e in S.split(w, 30)[0]]
        if str(d) not in dirs:
            dirs.append(str(d))
    assert [len(t) for t in times.values()] == [2, 2, 0]
    cfg = ge2e_harness.default_config()
    cfg["device"] = DEV
    torch.manual_seed(1)
    net = SpeechEmbedder(40, 768, 3, 256).to(DEV).eval()
    a = ge2e_harness.dvector_create(cfg, dirs, vad="split", out_dir=str(tmp_path / "split"), net=net)
    assert capsys.readouterr().out.count("No voice activity detected") == 1
    b = ge2e_harness.dvector_create(cfg, dirs, vad=lambda p: times[p], out_dir=str(tmp_path / "stub"), net=net)
    assert capsys.readouterr().out.count("No voice activity detected") == 1
    for pa, pb in zip(a, b):
        assert open(pa, "rb").read() == open(pb, "rb").read(), (pa, pb)
    assert np.load(a[0]).shape[0] + np.load(a[2]).shape[0] > 0
    with pytest.raises(ValueError, match="split"):
        ge2e_harness.dvector_create(cfg, dirs, vad="webrtc", out_dir=str(tmp_path / "bad"), net=net)
