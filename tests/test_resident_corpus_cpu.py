"""The resident spectrogram corpus (config key CORPUS_RESIDENT), the parts that need no device: ``resident_corpus.plan`` from the files'
headers, the epoch tables against the cache mode's index sequence, the config key's behaviour, the capacity check and the new C-ABI
entries' argument errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _resident_corpus_ref as R
from test_host_cpu import _make_corpus
from spoofsv_amd import _lib, harness, resident_corpus as RC


def _lists(cfg, mode="train"):
    base = os.path.join(cfg["DATA_ROOT_DIR"], "data_path", "ordinary")
    wavs = [ln.strip() for ln in open(os.path.join(base, "wav.path." + mode)) if ln.strip()]
    txts = [ln.strip() for ln in open(os.path.join(base, "txt.path." + mode)) if ln.strip()]
    return wavs, txts


def _no_data_reads(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("plan() must read .npy headers only")
    monkeypatch.setattr(np, "load", refuse)


def test_plan_reads_headers_only_and_counts_every_byte(tmp_path, monkeypatch):
    cfg, spec = _make_corpus(str(tmp_path), n_items=7, with_cache=True)
    wavs, txts = _lists(cfg)
    T = np.array([7 + 3 * i for i in range(7)], dtype=np.int64)          # what _make_corpus wrote
    _no_data_reads(monkeypatch)
    p = RC.plan(cfg, wavs, txts, spec, "train_ssrn", "train")
    assert p.n == 7 and p.parts == ("mel", "lin") and set(p.bytes) == {"mel", "lin"}
    for name, F, w in (("mel", 80, T), ("lin", 513, 4 * T)):
        assert p.off[name].dtype == np.int64 and p.len[name].dtype == np.int32
        assert p.len[name].tolist() == w.tolist()
        assert p.off[name].tolist() == [int(F * w[:i].sum()) for i in range(7)]             # cumulative, in elements
        assert p.elems[name] == F * w.sum() and p.bytes[name] == 4 * F * w.sum() + 7 * (8 + 4)
    assert p.total_bytes == RC.resident_corpus_bytes(p) == 4 * (80 + 4 * 513) * T.sum() + 2 * 7 * 12
    p = RC.plan(cfg, wavs, txts, spec, "train_text2mel", "train")
    assert p.parts == ("mel", "text", "spk")
    texts = [harness.text2id(open(t).readline().strip(), cfg["VOCABULARY"]) for t in txts]
    assert p.text_ids.dtype == np.int32 and p.text_ids.tolist() == [v for t in texts for v in t]
    assert p.len["text"].tolist() == [len(t) for t in texts] and p.off["text"].dtype == np.int64
    assert p.off["text"].tolist() == [sum(len(t) for t in texts[:i]) for i in range(7)]
    assert p.spk_dim == 200 and len(p.spk_files) == 2 and p.spk_index.tolist() == [i % 2 for i in range(7)]
    assert p.total_bytes == 4 * 80 * T.sum() + 4 * len(p.text_ids) + 4 * 2 * 200 + 3 * 7 * 12
    assert RC.plan(cfg, wavs, txts, spec, "synthesize", "synthesize").parts == ("mel", "text", "spk", "lin")
    assert RC.plan(cfg, wavs, txts, spec, "synthesize", "validate").parts == ("mel", "text", "spk")


@pytest.mark.parametrize("case", ["mel_rows", "mel_rank", "mel_dtype", "lin_rows", "lin_width", "lin_rank", "spk_size"])
def test_plan_names_the_malformed_file(tmp_path, monkeypatch, case):
    cfg, spec = _make_corpus(str(tmp_path), n_items=4, with_cache=True)
    wavs, txts = _lists(cfg)
    key = wavs[2][-17:-4]                                               # item 2: T = 13
    bad, arr = {
        "mel_rows": (spec + key + "_mel.npy", np.zeros((79, 13), np.float32)),
        "mel_rank": (spec + key + "_mel.npy", np.zeros((80 * 13,), np.float32)),
        "mel_dtype": (spec + key + "_mel.npy", np.zeros((80, 13), np.int32)),
        "lin_rows": (spec + key + "_lin.npy", np.zeros((512, 52), np.float32)),
        "lin_width": (spec + key + "_lin.npy", np.zeros((513, 51), np.float32)),
        "lin_rank": (spec + key + "_lin.npy", np.zeros((1, 513, 52), np.float32)),
        "spk_size": (os.path.join(cfg["SPK_EMB_DIR"], "p226.npy"), np.zeros((199,), np.float32)),
    }[case]
    np.save(bad, arr)
    _no_data_reads(monkeypatch)

    def no_alloc(*a, **k):
        raise AssertionError("nothing may be allocated before the corpus is validated")
    monkeypatch.setattr(torch, "empty", no_alloc)
    step = "train_text2mel" if case == "spk_size" else "train_ssrn"
    with pytest.raises(ValueError, match=os.path.basename(bad).replace(".", r"\.")):
        RC.plan(cfg, wavs, txts, spec, step, "train")


def test_plan_accepts_a_zero_width_item_and_other_float_widths(tmp_path):
    cfg, spec = _make_corpus(str(tmp_path), n_items=4, with_cache=True)
    wavs, txts = _lists(cfg)
    k1, k3 = wavs[1][-17:-4], wavs[3][-17:-4]
    np.save(spec + k1 + "_mel.npy", np.zeros((80, 0), np.float32))
    np.save(spec + k1 + "_lin.npy", np.zeros((513, 0), np.float32))
    np.save(spec + k3 + "_mel.npy", np.zeros((80, 16), np.float64))     # converted, as the cache mode's .float() converts it
    p = RC.plan(cfg, wavs, txts, spec, "train_ssrn", "train")
    assert p.len["mel"].tolist() == [7, 0, 13, 16] and p.len["lin"].tolist() == [28, 0, 52, 64]
    assert p.off["mel"].tolist() == [0, 560, 560, 560 + 80 * 13]


class _Recorded(harness.CorpusSource):
    """The cache mode with its file reads replaced by a record of the indices it asks for."""

    def _item(self, idx):
        self.asked[-1].append(idx)
        return {}

    def _collate(self, items):
        return {}


def _cache_mode_sequence(cfg, spec, B, seed, rank, world, epochs):
    src = _Recorded(cfg, "train_ssrn", "conditional", "train", B, spec, seed=seed, rank=rank, world=world)
    out = []
    for _ in range(epochs):
        src.asked = []
        it = src.host_batches()
        while True:
            src.asked.append([])
            try:
                next(it)
            except StopIteration:
                src.asked.pop()
                break
        out.append(src.asked)
    return out


def _resident_sequence(cfg, spec, B, seed, rank, world, epochs):
    """host_batches() of the resident mode needs no device: only finish_batch does."""
    src = harness.CorpusSource(cfg, "train_ssrn", "conditional", "train", B, spec, seed=seed, rank=rank, world=world)
    src.resident = object()
    out = []
    for _ in range(epochs):
        hbs = list(src.host_batches())
        assert all(set(hb) == {"_rows", "_row0", "_B"} for hb in hbs)
        assert len({id(hb["_rows"]) for hb in hbs}) == 1                 # one table per epoch
        table = hbs[0]["_rows"].host
        assert table.dtype == np.int32 and hbs[0]["_rows"].dev is None   # nothing uploaded by the thread that runs ahead
        assert [hb["_row0"] for hb in hbs] == list(np.cumsum([0] + [hb["_B"] for hb in hbs])[:-1]) and sum(hb["_B"] for hb in hbs) == len(table)
        out.append([table[hb["_row0"]:hb["_row0"] + hb["_B"]].tolist() for hb in hbs])
    return out


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_epoch_tables_are_the_cache_modes_index_sequence(tmp_path, seed, rank, world):
    cfg, spec = _make_corpus(str(tmp_path), n_items=7, with_cache=True)
    want = [R.epoch_indices(7, 3, world, rank, seed, e) for e in range(3)]                  # epochs 0-2
    assert _cache_mode_sequence(cfg, spec, 3, seed, rank, world, 3) == want
    got = _resident_sequence(cfg, spec, 3, seed, rank, world, 3)
    assert got == want
    if world == 1:
        assert [len(b) for b in got[0]] == [3, 3, 1]                                        # the partial last batch
    else:
        assert [len(b) for b in got[0]] == [3, 3]                                           # full, equal shards on every rank
        flat = [R.epoch_indices(7, 3, 2, r, seed, 0) for r in (0, 1)]
        order = np.random.RandomState(seed).permutation(7).tolist()
        assert flat[0][1] + flat[1][1] == order[6:] + order[:5]                             # the wrap-around to the head of the order


def test_epoch_rows_packs_batches_back_to_back():
    table, spans = RC.epoch_rows([[4, 1, 6], [0, 2, 5], [3]])
    assert table.dtype == np.int32 and table.tolist() == [4, 1, 6, 0, 2, 5, 3] and spans == [(0, 3), (3, 3), (6, 1)]
    table, spans = RC.epoch_rows([])
    assert table.size == 0 and spans == []


def test_without_the_key_the_source_takes_the_old_path(tmp_path):
    cfg, spec = _make_corpus(str(tmp_path), n_items=5, with_cache=True)
    assert "CORPUS_RESIDENT" not in cfg
    for c in (cfg, dict(cfg, CORPUS_RESIDENT=False)):
        src = harness.BatchSource(c, "train_ssrn", 2, spec, mode="validate")
        assert src.corpus.resident is None and not src.device_features
        b = next(iter(src))
        assert not b["data_0"].is_cuda and tuple(b["data_0"].shape) == (2, 80, 10) and tuple(b["data_1"].shape) == (2, 513, 40)


def test_the_key_needs_a_device_and_refuses_device_features(tmp_path, monkeypatch):
    cfg, spec = _make_corpus(str(tmp_path), n_items=5, with_cache=True)
    with pytest.raises(ValueError, match="CORPUS_RESIDENT.*device"):
        harness.CorpusSource(dict(cfg, CORPUS_RESIDENT=True, CORPUS_FEATURES="device"), "train_ssrn", "conditional", "train", 2, spec)
    with pytest.raises(ValueError):                                      # the other values are judged as before
        harness.CorpusSource(dict(cfg, CORPUS_RESIDENT=True, CORPUS_FEATURES="gpu"), "train_ssrn", "conditional", "train", 2, spec)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def no_alloc(*a, **k):
        raise AssertionError("nothing may be allocated without a device")
    monkeypatch.setattr(torch, "empty", no_alloc)
    monkeypatch.setattr(torch.Tensor, "pin_memory", no_alloc)
    for feats in (None, "cache", "batched"):
        c = dict(cfg, CORPUS_RESIDENT=True)
        if feats:
            c["CORPUS_FEATURES"] = feats
        with pytest.raises(RuntimeError, match="needs a ROCm device"):
            harness.CorpusSource(c, "train_ssrn", "conditional", "train", 2, spec)
        with pytest.raises(RuntimeError, match="needs a ROCm device"):    # ... and through BatchSource: no quiet fall-back to the cache mode
            harness.BatchSource(c, "train_ssrn", 2, spec)
    p = RC.plan(cfg, *_lists(cfg), spec, "train_ssrn", "train")
    with pytest.raises(RuntimeError, match="needs a ROCm device"):
        RC.ResidentTtsCorpus(p, "cpu")


def test_a_corpus_beyond_the_free_memory_is_refused_with_both_figures(tmp_path, monkeypatch):
    cfg, spec = _make_corpus(str(tmp_path), n_items=5, with_cache=True)
    p = RC.plan(cfg, *_lists(cfg), spec, "train_ssrn", "train")
    need = p.total_bytes
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda d=None: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda d=None: 0)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (need - 1, 1 << 40))

    def no_alloc(*a, **k):
        raise AssertionError("the capacity check comes before any allocation")
    monkeypatch.setattr(torch, "empty", no_alloc)
    with pytest.raises(RuntimeError) as e:
        RC.resident_corpus_bytes(p, torch.device("cuda", 0))
    assert str(need) in str(e.value) and str(need - 1) in str(e.value)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (need, 1 << 40))
    assert RC.resident_corpus_bytes(p, torch.device("cuda", 0)) == need       # exactly enough is enough


def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    L = _lib.lib()
    protos = _lib.parse_header()
    for name in ("ssv_corpus_gather", "ssv_corpus_gather_ids"):
        assert name in protos and hasattr(ctypes.CDLL(_lib.LIBPATH), name), name
    assert L.ssv_version() == 7
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)       # `one`: non-null dummy, never dereferenced: the checks come first
    good = dict(arena=one, an=100, off=one, len=one, n=4, rows=one, nr=9, row0=3, out=one, B=5, F=3, w=7, bs=21)

    def gather(a):
        return L.ssv_corpus_gather(a["arena"], a["an"], a["off"], a["len"], a["n"], a["rows"], a["nr"], a["row0"], a["out"], a["B"], a["F"], a["w"], a["bs"], null)
    cases = [("arena", null), ("off", null), ("len", null), ("rows", null), ("out", null), ("an", 0), ("n", 0), ("B", 0), ("B", -1), ("F", 0), ("w", 0),
             ("w", -2), ("bs", 20), ("row0", -1), ("row0", 5), ("nr", 7), ("nr", 0)]
    for key, bad in cases:
        rc = gather(dict(good, **{key: bad}))
        assert rc == -1 and b"corpus_gather" in L.ssv_last_error(), (key, rc)
    rc = gather(dict(good, B=0x7fffffff, F=8, w=1, bs=8, nr=1 << 40))                      # 2 (2^31 - 1) workgroups
    assert rc == -2 and b"grid" in L.ssv_last_error()
    good = dict(arena=one, an=100, off=one, len=one, n=4, rows=one, nr=9, row0=3, out=one, B=5, w=7)

    def ids(a):
        return L.ssv_corpus_gather_ids(a["arena"], a["an"], a["off"], a["len"], a["n"], a["rows"], a["nr"], a["row0"], a["out"], a["B"], a["w"], null)
    for key, bad in [("arena", null), ("off", null), ("len", null), ("rows", null), ("out", null), ("an", 0), ("n", 0), ("B", 0), ("w", 0),
                     ("row0", -1), ("row0", 5), ("nr", 0)]:
        rc = ids(dict(good, **{key: bad}))
        assert rc == -1 and b"corpus_gather_ids" in L.ssv_last_error(), (key, rc)
    rc = ids(dict(good, B=0x7fffffff, w=257, nr=1 << 40))
    assert rc == -2 and b"grid" in L.ssv_last_error()
