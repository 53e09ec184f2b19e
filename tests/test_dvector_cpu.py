"""CPU-only checks of whole-utterance d-vector extraction: the host logic of spoofsv_amd/dvector.py against what the reference's own
``concat_segs`` / ``align_embeddings`` returned (tests/golden/dvector_host.npz, written by tools/gen_dvector_golden.py) and against the
literal loops of GE2E/dvector_create.py, and the C ABI of csrc/dvector.hip without a device."""
import ctypes
import os

import numpy as np
import pytest

from spoofsv_amd import _lib
from spoofsv_amd import dvector as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dvector_host.npz")


def _golden_parts(g, n):
    a, b = int(g["part_off"][n - 1]), int(g["part_off"][n])
    return list(zip(g["part_start"][a:b].tolist(), g["part_end"][a:b].tolist()))


def test_align_partitions_equal_the_reference_for_1_to_600_rows():
    g = np.load(GOLDEN)
    for n in range(1, 601):
        assert D.align_partitions(n) == _golden_parts(g, n), n
    sizes = [b - a for a, b in D.align_partitions(333)]
    assert sizes[:6] == [2, 3, 4, 3, 3, 4] and len(sizes) == 100


def test_partition_means_equal_align_embeddings_output():
    g = np.load(GOLDEN)
    for k, rows in enumerate((1, 7, 40)):
        x, want = g["align_in_%d" % k], g["align_out_%d" % k]
        assert x.shape == (rows, 256) and want.dtype == np.float64
        parts = D.align_partitions(rows)
        got = np.stack([x[a:b].mean(axis=0) for a, b in parts])
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12


def test_spans_from_vad_reproduces_concat_segs():
    """The golden chunks are slices of np.arange(n): every sample carries its index, so concat_segs' segments laid end to end must be
    the samples of the spans, one span per segment."""
    g = np.load(GOLDEN)
    cases = sorted({int(k.split("_")[1]) for k in g.files if k.startswith("concat_")})
    assert len(cases) >= 4
    joined = clipped = False
    for c in cases:
        sr, n = (int(v) for v in g["concat_%d_sr_n" % c])
        times = [tuple(r) for r in g["concat_%d_times" % c]]
        spans = D.spans_from_vad(times, sr, n)
        assert [e - s for s, e in spans] == g["concat_%d_lens" % c].tolist(), c
        tags = np.concatenate([np.arange(s, e) for s, e in spans]) if spans else np.zeros(0)
        assert np.array_equal(tags, g["concat_%d_tags" % c]), c
        joined |= len(spans) < len(times)
        clipped |= any(int(t1 * sr) > n for _, t1 in times)
    assert joined and clipped                                  # the cases exercise both
    assert D.spans_from_vad([], 16000, 100) == []


@pytest.mark.parametrize("window,shift", [(24, 12), (120, 60), (7, 3)])
def test_windows_of_equals_the_literal_loop(window, shift):
    for F in range(1, 3001):
        n = 0
        for j in range(0, F, shift):                           # dvector_create.py:48-52
            if j + window < F:
                n += 1
            else:
                break
        assert D.windows_of(F, window, shift) == n, F
    assert D.windows_of(24) == 0 and D.windows_of(25) == 1 and D.windows_of(37) == 2
    assert D.frames_of(3840, 160) == 25 and D.frames_of(3839, 160) == 24 and D.frames_of(0, 160) == 1


def test_plan_of_a_ragged_batch():
    hop = 160
    spans = [[(0, 8000), (9000, 9100)],                        # 51 frames -> 3 windows; a span without a window: not framed
             [(0, 100)],                                       # an utterance without a window
             [(100, 50000)],                                   # clipped to the row's 40,000 samples: 250 frames, 4 tiles
             [(-5, 3840), (3840, 7999)]]                       # clipped at 0: exactly 24 * hop samples, 25 frames, 1 window; 4159 -> 26 frames, 1
    pl = D.plan(spans, hop, 24, 12, lengths=[9100, 100, 40000, 7999])
    assert pl.tiles.dtype == np.int32 and pl.g0.dtype == np.int32 and pl.offs.dtype == np.int32
    assert pl.tiles.tolist() == [[0, 0, 8000, 0, 0, 51],
                                 [2, 100, 40000, 0, 51, 64], [2, 100, 40000, 64, 115, 64], [2, 100, 40000, 128, 179, 64], [2, 100, 40000, 192, 243, 58],
                                 [3, 0, 3840, 0, 301, 25], [3, 3840, 7999, 0, 326, 26]]
    assert pl.n_frames == 352 and pl.n_windows == 3 + 19 + 1 + 1
    assert pl.g0.tolist() == [0, 12, 24] + [51 + 12 * k for k in range(19)] + [301, 326]
    assert pl.windows_per_utterance == [3, 0, 19, 2] and pl.empty == [1]
    assert pl.utt_offs.tolist() == [0, 3, 3, 22, 24]
    parts = [D.align_partitions(3), D.align_partitions(19), D.align_partitions(2)]
    assert pl.rows_per_utterance == [len(parts[0]), 0, len(parts[1]), len(parts[2])]
    want = [0] + [b for _, b in parts[0]] + [3 + b for _, b in parts[1]] + [22 + b for _, b in parts[2]]
    assert pl.offs.tolist() == want and pl.offs[-1] == pl.n_windows
    # every window lies inside one span's frames
    ends = {int(t[4]) + int(t[5]) for t in pl.tiles}
    span_end = [51, 301, 326, 352]
    for g in pl.g0.tolist():
        assert g + 24 <= min(e for e in span_end if e > g)
    assert ends >= set(span_end)
    empty = D.plan([[], [(0, 10)]], hop)
    assert empty.n_frames == 0 and empty.n_windows == 0 and empty.tiles.shape == (0, 6) and empty.empty == [0, 1] and empty.offs.tolist() == [0]
    assert D.TILE == 64


def test_entries_are_declared_and_exported():
    protos = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name, nargs in (("ssv_span_frames", 14), ("ssv_gather_windows", 8), ("ssv_segment_mean", 8)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert protos[name][0] is ctypes.c_int and hasattr(raw, name)
    assert _lib.lib().ssv_version() == 7                        # additions only


def test_bad_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one, two = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(4096)     # non-null dummies, never dereferenced
    ok = dict(B=2, n_max=16000, n_tiles=3, n_fft=512, hop=160, window=24, Tc=256, R=1, g_base=0, n_frames=100)

    def span(y=one, tiles=one, fr=two, **kw):
        a = dict(ok, **kw)
        return L.ssv_span_frames(y, tiles, fr, a["B"], a["n_max"], a["n_tiles"], a["n_fft"], a["hop"], a["window"], a["Tc"], a["R"], a["g_base"],
                                 a["n_frames"], null)
    for kw in (dict(y=null), dict(tiles=null), dict(fr=null), dict(B=0), dict(n_max=0), dict(n_tiles=0), dict(n_fft=511), dict(hop=0), dict(hop=513),
               dict(window=0), dict(Tc=0), dict(R=0), dict(g_base=-1), dict(n_frames=0)):
        assert span(**kw) == -1 and b"span_frames" in L.ssv_last_error(), kw
    assert span(window=1) == -1 and b"n_fft/2" in L.ssv_last_error()               # 160 <= 256: one reflection would not do
    assert span(n_frames=257) == -1 and span(n_frames=256, R=2) == -1               # frames must end in the last item
    assert span(n_fft=8192, hop=160, window=100, Tc=16, n_frames=10) == -2 and b"LDS" in L.ssv_last_error()
    assert span(n_fft=2048, hop=512, window=24) == -2                               # 63 * 512 + 2048 floats
    for args in ((null, one, two, 100, 4, 24, 40), (one, null, two, 100, 4, 24, 40), (one, one, null, 100, 4, 24, 40), (one, one, one, 100, 4, 24, 40),
                 (one, one, two, 0, 4, 24, 40), (one, one, two, 100, 0, 24, 40), (one, one, two, 100, 4, 0, 40), (one, one, two, 100, 4, 24, 0)):
        assert L.ssv_gather_windows(*args, null) == -1 and b"gather_windows" in L.ssv_last_error(), args
    for args in ((null, one, two, 8, 2, 256, 0), (one, null, two, 8, 2, 256, 0), (one, one, null, 8, 2, 256, 1), (one, one, one, 8, 2, 256, 0),
                 (one, one, two, 0, 2, 256, 0), (one, one, two, 8, 0, 256, 0), (one, one, two, 8, 2, 0, 1)):
        assert L.ssv_segment_mean(*args, null) == -1 and b"segment_mean" in L.ssv_last_error(), args

