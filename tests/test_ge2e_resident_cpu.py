"""GE2E training on a resident corpus, the parts that need no device: the row tables of ``ResidentSpeakerCorpus.batches`` against the host
loader's random stream, the corpus's own checks, the new C-ABI entries' argument errors, and the float64 clip + SGD reference itself."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import _ge2e_resident_ref as R
from spoofsv_amd import _lib
from spoofsv_amd.ge2e_harness import ResidentSpeakerCorpus, SpeakerDatasetPreprocessed

COUNTS = (1, 2, 3, 5, 9, 9, 12)


def _write_corpus(path, counts=COUNTS, nmels=5, frames=7):
    os.makedirs(path, exist_ok=True)
    at = 0
    for i, c in enumerate(counts):
        n = c * nmels * frames
        np.save(os.path.join(path, "speaker%d.npy" % i), (at + np.arange(n, dtype=np.float32)).reshape(c, nmels, frames))    # distinct values everywhere
        at += n
    return path


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def test_row_tables_follow_the_host_loaders_random_stream(tmp_path):
    path = _write_corpus(str(tmp_path / "train"))
    _seed(1234)
    loader = DataLoader(SpeakerDatasetPreprocessed(path, 4, shuffle=True), batch_size=3, shuffle=True, drop_last=True)
    want = [b.numpy().copy() for _ in range(2) for b in loader]
    corpus = ResidentSpeakerCorpus(path, "cpu")
    assert corpus.data.dtype == torch.float32 and tuple(corpus.data.shape) == (sum(COUNTS), 5, 7)
    assert corpus.offsets.tolist() == [0, 1, 3, 6, 11, 20, 29] and corpus.counts.tolist() == list(COUNTS)
    _seed(1234)
    batches = corpus.batches(3, 4)
    assert len(batches) == len(loader) == 2
    tables = [rows for _ in range(2) for rows in batches]
    assert len(tables) == len(want) == 4
    data = corpus.data.numpy()
    for rows, w in zip(tables, want):
        assert rows.dtype == torch.int32 and tuple(rows.shape) == (12,)
        got = R.gather_ref(data, rows.numpy()).reshape(3, 4, 7, 5)
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes()
    assert len({t.numpy().tobytes() for t in tables}) > 1               # (the stream moves: not one table four times)


def test_corpus_checks_and_bytes(tmp_path):
    path = _write_corpus(str(tmp_path / "ok"))
    corpus = ResidentSpeakerCorpus(path, "cpu")
    assert corpus.bytes == 4 * sum(COUNTS) * 5 * 7 == corpus.data.numel() * 4
    empty = _write_corpus(str(tmp_path / "empty"), counts=(2, 3))
    np.save(os.path.join(empty, "speaker1.npy"), np.zeros((0, 5, 7), dtype=np.float32))
    with pytest.raises(ValueError, match="speaker1.npy"):
        ResidentSpeakerCorpus(empty, "cpu")
    other = _write_corpus(str(tmp_path / "other"), counts=(2, 3))
    np.save(os.path.join(other, "speaker1.npy"), np.zeros((3, 5, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="speaker1.npy"):
        ResidentSpeakerCorpus(other, "cpu")
    np.save(os.path.join(other, "speaker1.npy"), np.zeros((3, 5, 7), dtype=np.float64))        # another dtype is converted, not refused
    assert ResidentSpeakerCorpus(other, "cpu").data.dtype == torch.float32


def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    L = _lib.lib()
    protos = _lib.parse_header()
    for name in ("ssv_tisv_batch_gather", "ssv_clip_sgd_workspace", "ssv_clip_sgd_multi"):
        assert name in protos and hasattr(ctypes.CDLL(_lib.LIBPATH), name), name
    assert L.ssv_version() == 7
    assert ctypes.sizeof(_lib.ClipSgdChunk) == 32
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)       # `one`: non-null dummy, never dereferenced: the checks come first
    good = dict(corpus=one, U=4, rows=one, out=one, Bn=2, nmels=5, frames=7)
    for key, bad in (("corpus", null), ("rows", null), ("out", null), ("U", 0), ("Bn", 0), ("Bn", -1), ("nmels", 0), ("frames", 0), ("frames", -3)):
        a = dict(good, **{key: bad})
        rc = L.ssv_tisv_batch_gather(a["corpus"], a["U"], a["rows"], a["out"], a["Bn"], a["nmels"], a["frames"], null)
        assert rc == -1 and b"tisv_batch_gather" in L.ssv_last_error(), (key, rc)
    assert _lib.query("ssv_clip_sgd_workspace", 750) == 750 * 8 and _lib.query("ssv_clip_sgd_workspace", 0) == 0
    mn = (ctypes.c_float * 2)(3.0, 1.0)
    good = dict(chunks=one, n=3, mn=mn, ng=2, norms=one, loss=null, hist=null, hl=0, step=null, ws=one, nb=24)
    cases = [("chunks", null), ("mn", null), ("norms", null), ("n", 0), ("ng", 0), ("ng", 9), ("ws", null), ("nb", 16),
             ("hist", one)]                                   # a history without loss / counter / length
    for key, bad in cases:
        a = dict(good, **{key: bad})
        rc = L.ssv_clip_sgd_multi(a["chunks"], a["n"], a["mn"], a["ng"], 0.01, a["norms"], a["loss"], a["hist"], a["hl"], a["step"], a["ws"], a["nb"], null)
        assert rc == -1 and b"clip_sgd_multi" in L.ssv_last_error(), (key, rc)


def test_float64_reference_agrees_with_torch_clip_and_sgd():
    """The reference itself: torch's clip_grad_norm_ + SGD.step on CPU float64 tensors, to 1e-12 relative."""
    g = torch.Generator().manual_seed(7)
    lr = float(np.float32(0.01))
    for scale in (1e-3, 1.0, 30.0):                          # below both max_norms, between them, above both
        shapes = ([(3, 5), (17,), ()], [(), ()])
        params = [[torch.randn(s, generator=g, dtype=torch.float64).requires_grad_(True) for s in grp] for grp in shapes]
        for grp in params:
            for p in grp:
                p.grad = scale * torch.randn(p.shape, generator=g, dtype=torch.float64)
        ref = R.clip_sgd_ref([([(p.detach().numpy().copy(), p.grad.numpy().copy()) for p in grp], mn) for grp, mn in zip(params, (3.0, 1.0))], lr)
        opt = torch.optim.SGD([{"params": grp} for grp in params], lr=lr)
        norms = [float(torch.nn.utils.clip_grad_norm_(grp, mn)) for grp, mn in zip(params, (3.0, 1.0))]
        opt.step()
        for gi, grp in enumerate(params):
            assert abs(norms[gi] - ref.norms[gi]) <= 1e-12 * ref.norms[gi]
            for p, want in zip(grp, ref.p[gi]):
                assert np.all(np.abs(p.detach().numpy() - want) <= 1e-12 * np.abs(want)), (scale, gi)
        assert (ref.coefs[0] == 1.0) == (ref.norms[0] + 1e-6 <= 3.0)
