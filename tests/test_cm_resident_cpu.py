"""The countermeasure's resident corpus and bucketed replay without a device: the new C entries are declared, exported and refuse bad
arguments on the host, bucket choice and validation, the head-width arithmetic that decides between replay and the eager path, the
arena's size bound and its refusal, and the failure mode of ``train(resident=True)`` without a ROCm device."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(json.load(open(os.path.join(ROOT, "config.json"))), DISC_DIM=16)
NEW = ("ssv_corpus_scatter", "ssv_cm_head_fwd_len", "ssv_cm_head_bwd_len")


def test_new_symbols_are_declared_and_exported():
    import spoofsv_amd.countermeasure as C
    from spoofsv_amd import _lib, ops
    L = _lib.lib()
    assert L.ssv_version() == 7                                   # additions; ABI version unchanged
    protos = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    # the _len entries are the dense ones plus one device int in front of the stream
    for kind in ("fwd", "bwd"):
        dense, live = protos["ssv_cm_head_%s" % kind], protos["ssv_cm_head_%s_len" % kind]
        assert live[2] == dense[2][:-1] + ["live", "stream"] and live[1][:-2] == dense[1][:-1]
    assert protos["ssv_corpus_scatter"][2] == ["src", "src_bs", "B", "F", "width", "arena", "arena_n", "off", "len", "n_items", "item0", "stream"]
    for name in ("CmResidentCorpus", "CmBucketedStep", "head_width", "check_width_buckets", "pick_width_bucket", "frames_bound", "cm_resident_bytes"):
        assert hasattr(C, name), name
    assert callable(ops.mask_cols) and hasattr(C.CmResidentCorpus, "from_features") and hasattr(C.CmResidentCorpus, "gather_into")


def test_new_entries_refuse_bad_arguments_before_the_device():
    from spoofsv_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    scatter = dict(src=p, src_bs=12, B=2, F=3, width=4, arena=p, arena_n=64, off=p, len=p, n_items=5, item0=0)
    call = lambda a: L.ssv_corpus_scatter(a["src"], a["src_bs"], a["B"], a["F"], a["width"], a["arena"], a["arena_n"], a["off"], a["len"], a["n_items"],
                                          a["item0"], None)
    bad = [("src", None), ("arena", None), ("off", None), ("len", None), ("B", 0), ("F", 0), ("width", 0), ("arena_n", 0), ("n_items", 0), ("B", -1),
           ("item0", -1), ("item0", 4), ("src_bs", 11)]
    for key, value in bad:
        assert call(dict(scatter, **{key: value})) == -1 and b"corpus_scatter" in L.ssv_last_error(), (key, value)
    fwd = lambda x=p, w=p, bias=p, pred=p, amean=p, live=p, B=2, C=4, T=3: L.ssv_cm_head_fwd_len(x, w, bias, p, 0.05, pred, amean, p, p, B, C, T, live, None)
    for kw in (dict(x=None), dict(w=None), dict(bias=None), dict(pred=None), dict(amean=None), dict(live=None), dict(B=0), dict(C=0), dict(T=0), dict(C=17)):
        assert fwd(**kw) == -1 and b"cm_head_fwd_len" in L.ssv_last_error(), kw
    assert fwd(T=0) == -1 and b"T=0" in L.ssv_last_error()
    assert fwd(live=None) == -1 and b"live" in L.ssv_last_error()
    bwd = lambda x=p, dx=p, dz=p, live=p, B=2, C=4, T=3: L.ssv_cm_head_bwd_len(x, p, p, p, p, p, 0.05, dx, p, p, dz, B, C, T, live, None)
    for kw in (dict(x=None), dict(dx=None), dict(dz=None), dict(live=None), dict(B=0), dict(C=0), dict(T=0), dict(C=17), dict(T=(1 << 26) + 1)):
        assert bwd(**kw) == -1 and b"cm_head_bwd_len" in L.ssv_last_error(), kw


def test_bucket_choice_and_validation():
    from spoofsv_amd.countermeasure import check_width_buckets, pick_width_bucket
    b = check_width_buckets([64, 96, 160])
    assert b == [64, 96, 160]
    assert [pick_width_bucket(b, w) for w in (1, 63, 64, 65, 96, 97, 160)] == [64, 64, 64, 96, 96, 160, 160]
    assert pick_width_bucket(b, 161) is None                      # too wide for every bucket: the eager path
    assert check_width_buckets((np.int64(8),)) == [8]
    for bad in ([96, 64], [64, 64], [0, 64], [-8], [], [64.0], [True], "64,96", 64, [64, None]):
        with pytest.raises(ValueError):
            check_width_buckets(bad)


class _StubCorpus:
    def __init__(self, feat_type, width, batch_size=4):
        self.feat_type, self._width, self.batch_size = feat_type, width, batch_size

    def width(self, idx):
        return self._width


def test_head_width_arithmetic_and_the_eager_path():
    from spoofsv_amd import countermeasure as C
    assert C.POOLS == {"lin": (8, 4), "mel": (2, 2)}
    for kind, (k1, k2) in C.POOLS.items():
        m = C.build_model(CFG, kind)
        assert (m.pl1.kernel_size[0], m.pl2.kernel_size[0]) == (k1, k2)          # the arithmetic is the model's
        for L in range(0, 200):
            assert C.head_width(kind, L) == (L // k1) // k2
    assert [C.head_width("lin", L) for L in (31, 32, 37, 63, 64)] == [0, 1, 1, 1, 2]
    assert [C.head_width("mel", L) for L in (3, 4, 7, 8)] == [0, 1, 1, 2]
    # width 0 at the head, the partial batch and a batch beyond every bucket run eagerly; everything else replays in the smallest bucket
    model = C.build_model(CFG, "mel")
    opt = type("Opt", (), {"capturable": True})()
    for kind, width, n, want in (("lin", 31, 4, None), ("lin", 32, 4, 40), ("lin", 32, 3, None), ("lin", 41, 4, 64), ("lin", 65, 4, None),
                                 ("mel", 3, 4, None), ("mel", 4, 4, 40)):
        st = C.CmBucketedStep(model, opt, _StubCorpus(kind, width), [40, 64])
        assert st.bucket_of(list(range(n))) == want, (kind, width, n)
        st.close()
    with pytest.raises(ValueError, match="capturable"):
        C.CmBucketedStep(model, type("Opt", (), {"capturable": False})(), _StubCorpus("lin", 32), [40])
    with pytest.raises(ValueError, match="ascending"):
        C.CmBucketedStep(model, opt, _StubCorpus("lin", 32), [64, 40])


def test_size_bound_and_its_refusal():
    from spoofsv_amd import countermeasure as C
    from spoofsv_amd.corpus_features import feature_lengths
    from spoofsv_amd.wave import resampled_width
    n_fft, hop, r = int(CFG["STFT"]["FFT_LENGTH"]), int(CFG["STFT"]["HOP_LENGTH"]), int(CFG["COARSE_MELSPEC"]["REDUCTION"])
    samples = [(16000, 16000), (22050, 22050), (100, 16000), (0, 16000), (64000, 16000), (9601, 22050)]
    lin, mel = C.frames_bound(CFG, samples, "lin"), C.frames_bound(CFG, samples, "mel")
    for (n, rate), a, b in zip(samples, lin, mel):
        m = n if rate == 16000 else resampled_width(n, rate, 16000)
        T = 1 + m // hop if m > n_fft // 2 else 0
        assert (b, a) == (T // r, r * (T // r)) == feature_lengths(m, n_fft, hop, r)[1:]
        # trimming only shortens: every shorter segment stays within the bound
        assert all(feature_lengths(k, n_fft, hop, r)[2] <= a for k in range(0, m + 1, 997))
    assert lin[2] == 0 and lin[3] == 0 and lin[0] == r * ((1 + 16000 // hop) // r)
    F = 1 + n_fft // 2
    need = C.cm_resident_bytes(len(samples), int(lin.sum()), F)
    assert need == 4 * F * int(lin.sum()) + 28 * len(samples)
    assert C.cm_resident_bytes(len(samples), int(lin.sum()), F, free=need) == need
    with pytest.raises(RuntimeError) as e:
        C.cm_resident_bytes(len(samples), int(lin.sum()), F, free=need - 1)
    assert "%d bytes" % need in str(e.value) and "%d are free" % (need - 1) in str(e.value) and "%d items" % len(samples) in str(e.value)
    # the reference's corpus by the config's arithmetic: ~43 k utterances of ~3 s are about 20 GB of linear features
    per_item = int(C.frames_bound(CFG, [(3 * 16000, 16000)], "lin")[0])
    assert 15e9 < C.cm_resident_bytes(43000, 43000 * per_item, F) < 25e9


class _HostSource:
    device, batch_size, seed = torch.device("cpu"), 8, 0

    def __len__(self):
        return 24

    def batch(self, idx):
        raise AssertionError("a corpus that cannot be resident must be refused before one batch is extracted")


def test_resident_training_without_a_device_raises(tmp_path):
    from spoofsv_amd import countermeasure as C
    with pytest.raises(RuntimeError, match="ROCm device"):
        C.train(CFG, _HostSource(), "lin", save_dir=str(tmp_path), resident=True, max_iterations=1, log=lambda *a: None)
    with pytest.raises(RuntimeError, match="ROCm device"):
        C.CmResidentCorpus.from_features([torch.zeros(5, 3)], [1.0], "lin", device="cpu")
    with pytest.raises(ValueError, match="resident"):
        C.train(CFG, _HostSource(), "lin", save_dir=str(tmp_path), width_buckets=[64], max_iterations=1, log=lambda *a: None)
