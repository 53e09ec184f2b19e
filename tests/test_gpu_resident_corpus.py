"""The resident spectrogram corpus on the device (config key CORPUS_RESIDENT): ssv_corpus_gather / ssv_corpus_gather_ids against the
numpy collate (tests/_resident_corpus_ref.py), CorpusSource in resident mode against the cache mode, and the trainers on both.  Every
value check is bitwise."""
import copy
import ctypes
import threading

import numpy as np
import pytest
import torch

import _resident_corpus_ref as R
from spoofsv_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                # floats on either side of a buffer under test (keeps its base 16-byte aligned)
SENTINEL = -7777.0
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)
TABLE = (5, 11, 0, 8, 11, 3, 7, 1, 9, 2, 10, 4, 6, 6, 0, 11)          # an epoch's order over the 12 items, repeats included
WINDOWS = ((1, 5), (6, 5), (11, 5), (3, 1), (15, 1), (2, 1))            # (row0, B): rows 1-5 repeat item 11, rows 11-15 item 6; row 2 is the empty item


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _arena(F, aligned, seed):
    """12 items of LENGTHS as (F, len) blocks: offsets all multiples of 4 elements, or all odd.  -> host arena, off, len."""
    rng = np.random.RandomState(seed)
    off, at = [], 0
    for n in LENGTHS:
        at = (at + 3) // 4 * 4 if aligned else at | 1
        off.append(at)
        at += F * n + int(rng.randint(0, 6))
    arena = rng.rand(at + 8).astype(np.float32) + 1.0                  # (no zeros: padding is told from data)
    assert all((o % 4 == 0) if aligned else (o % 2 == 1) for o in off)
    return arena, np.asarray(off, np.int64), np.asarray(LENGTHS, np.int32)


def _guarded(n, fill, dtype=torch.float32):
    """A device buffer of n elements between two sentinel guards -> (whole, view of the n elements)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    inner = whole[GUARD:GUARD + n]
    inner.fill_(fill)
    return whole, inner


def _guards_intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "odd"])
@pytest.mark.parametrize("F", [3, 80, 513])
def test_corpus_gather_is_the_numpy_collate(F, aligned):
    arena, off, length = _arena(F, aligned, seed=F)
    abuf, a = _guarded(arena.size, 0.0)
    a.copy_(torch.from_numpy(arena))
    off_d, len_d = torch.from_numpy(off).to(DEV), torch.from_numpy(length).to(DEV)
    rows = np.asarray(TABLE, np.int32)
    rows_d = torch.from_numpy(rows).to(DEV)
    L = _lib.lib()
    ran = clipped = 0
    for row0, B in WINDOWS:
        longest = int(length[rows[row0:row0 + B]].max())
        for width in (longest, longest + 3, longest // 2):
            if width < 1:
                continue                                                 # (an all-empty batch is the host's business: nothing to launch)
            for out_bs in (F * width, F * width + 5):
                n_out = (B - 1) * out_bs + F * width
                obuf, o = _guarded(n_out, float("nan"))
                rc = L.ssv_corpus_gather(_p(a), a.numel(), _p(off_d), _p(len_d), len(LENGTHS), _p(rows_d), rows_d.numel(), row0, _p(o), B, F, width,
                                         out_bs, _stream())
                assert rc == 0, L.ssv_last_error()
                got_all = o.cpu().numpy()
                assert _guards_intact(obuf, n_out) and _guards_intact(abuf, arena.size), (row0, B, width, out_bs)
                want = R.gather_ref(arena, off, length, rows, row0, B, F, width)
                for b in range(B):
                    got = got_all[b * out_bs:b * out_bs + F * width].reshape(F, width)
                    assert not np.isnan(got).any(), (row0, B, width, out_bs, b)
                    assert got.tobytes() == want[b].tobytes(), (row0, B, width, out_bs, b)
                    if b + 1 < B and out_bs > F * width:                 # the slack between two items is nobody's
                        assert np.isnan(got_all[b * out_bs + F * width:(b + 1) * out_bs]).all()
                ran += 1
                clipped += int(width < longest)
    assert ran >= 30 and clipped >= 8
    assert torch.equal(a.cpu(), torch.from_numpy(arena))                 # the corpus is read, never written


@pytest.mark.parametrize("bad", [-1, len(LENGTHS)])
def test_a_row_outside_the_corpus_becomes_nan_and_nothing_else_changes(bad):
    F, width = 80, 70
    arena, off, length = _arena(F, True, seed=9)
    abuf, a = _guarded(arena.size, 0.0)
    a.copy_(torch.from_numpy(arena))
    off_d, len_d = torch.from_numpy(off).to(DEV), torch.from_numpy(length).to(DEV)
    rows = np.asarray([8, 6, bad, 7, 3], np.int32)
    rows_d = torch.from_numpy(rows).to(DEV)
    obuf, o = _guarded(4 * F * width, 5.0)
    _lib.call("ssv_corpus_gather", _p(a), a.numel(), _p(off_d), _p(len_d), len(LENGTHS), _p(rows_d), 5, 1, _p(o), 4, F, width, F * width, _stream())
    got = o.cpu().numpy().reshape(4, F, width)
    assert _guards_intact(obuf, 4 * F * width) and _guards_intact(abuf, arena.size)
    assert np.isnan(got[1]).all()
    good = np.asarray([6, 7, 3], np.int32)
    want = R.gather_ref(arena, off, length, good, 0, 3, F, width)
    assert got[[0, 2, 3]].tobytes() == want.tobytes()


def test_corpus_gather_beyond_two_to_the_31_elements():
    need = 12 << 30
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < need:
        pytest.skip("less than 12 GB of device memory free (%d bytes)" % free)
    F, n_arena = 3, (1 << 31) + (1 << 16)
    arena = torch.empty((n_arena,), dtype=torch.float32, device=DEV)    # 8.6 GB, uninitialised: only the two items are written
    rng = np.random.RandomState(5)
    length = np.asarray([65, 256], np.int32)
    off = np.asarray([(1 << 31) + 1, (1 << 31) + 4096], np.int64)       # one odd, one 16-byte aligned
    items = [rng.rand(F * int(n)).astype(np.float32) + 1.0 for n in length]
    for o, it in zip(off, items):
        arena[int(o):int(o) + it.size].copy_(torch.from_numpy(it))
    rows_d = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    width = 260
    obuf, out = _guarded(3 * F * width, float("nan"))
    off_d, len_d = torch.from_numpy(off).to(DEV), torch.from_numpy(length).to(DEV)
    _lib.call("ssv_corpus_gather", _p(arena), n_arena, _p(off_d), _p(len_d), 2, _p(rows_d), 3, 0, _p(out), 3, F, width, F * width, _stream())
    got = out.cpu().numpy().reshape(3, F, width)
    assert _guards_intact(obuf, 3 * F * width)
    for b, r in enumerate((1, 0, 1)):
        want = np.zeros((F, width), np.float32)
        want[:, :length[r]] = items[r].reshape(F, length[r])
        assert got[b].tobytes() == want.tobytes(), b
    del arena
    torch.cuda.empty_cache()


def test_corpus_gather_ids_pads_with_p():
    lens = np.asarray([1, 2, 185, 186], np.int32)
    rng = np.random.RandomState(2)
    off = np.asarray([3, 9, 20, 300], np.int64)
    ids = rng.randint(1, 32, size=500).astype(np.int32)
    abuf, a = _guarded(ids.size, 0, dtype=torch.int32)
    a.copy_(torch.from_numpy(ids))
    rows = np.asarray([2, 0, 3, 1, 3, 0, 1], np.int32)
    rows_d = torch.from_numpy(rows).to(DEV)
    off_d, len_d = torch.from_numpy(off).to(DEV), torch.from_numpy(lens).to(DEV)
    for row0, B in ((0, 4), (2, 3), (5, 2), (3, 1), (1, 1)):
        longest = int(lens[rows[row0:row0 + B]].max())
        for width in (longest, longest + 3, 300):
            obuf, o = _guarded(B * width, -5, dtype=torch.int64)
            _lib.call("ssv_corpus_gather_ids", _p(a), a.numel(), _p(off_d), _p(len_d), 4, _p(rows_d), rows_d.numel(), row0, _p(o), B, width, _stream())
            got = o.cpu().numpy().reshape(B, 1, width)
            want = R.ids_ref(ids, off, lens, rows, row0, B, width)
            assert bool((obuf[:GUARD] == int(SENTINEL)).all()) and bool((obuf[GUARD + B * width:] == int(SENTINEL)).all())
            assert got.dtype == np.int64 and got.tobytes() == want.tobytes(), (row0, B, width)
    bad_d = torch.tensor([1, 4, -1], dtype=torch.int32, device=DEV)       # outside the corpus: -1 everywhere, never dereferenced
    o = torch.zeros((3, 1, 4), dtype=torch.int64, device=DEV)
    _lib.call("ssv_corpus_gather_ids", _p(a), a.numel(), _p(off_d), _p(len_d), 4, _p(bad_d), 3, 0, _p(o), 3, 4, _stream())
    assert o.cpu().numpy().reshape(3, 4).tolist() == [ids[9:11].tolist() + [0, 0], [-1] * 4, [-1] * 4]


# ---------------------------------------------------------------------------------------------- CorpusSource: resident against cache
def _corpus(tmp_path, n_items=7):
    from test_host_cpu import _make_corpus
    return _make_corpus(str(tmp_path), n_items=n_items, with_cache=True)


def _same_batch(res, ref):
    assert list(res) == list(ref)
    for k in ref:
        assert res[k].is_cuda and not ref[k].is_cuda, k
        assert res[k].dtype == ref[k].dtype and tuple(res[k].shape) == tuple(ref[k].shape), (k, res[k].shape, ref[k].shape)
        assert res[k].is_contiguous() and res[k].cpu().numpy().tobytes() == ref[k].numpy().tobytes(), k


@pytest.mark.parametrize("step,mode", [("train_text2mel", "train"), ("train_ssrn", "train"), ("synthesize", "train"), ("synthesize", "validate")])
def test_resident_batches_are_the_cache_modes_batches(tmp_path, step, mode):
    from spoofsv_amd import harness
    cfg, spec = _corpus(tmp_path)
    ref = harness.CorpusSource(cfg, step, "conditional", mode, 3, spec, seed=3)
    res = harness.CorpusSource(dict(cfg, CORPUS_RESIDENT=True), step, "conditional", mode, 3, spec, seed=3)
    assert ref.resident is None and res.resident is not None and res.resident.nbytes == res.resident.plan.total_bytes
    assert set(res.resident.arenas) == {"train_ssrn": {"mel", "lin"}, "train_text2mel": {"mel", "text", "spk"},
                                        "synthesize": {"mel", "text", "spk"} | ({"lin"} if mode != "validate" else set())}[step]
    for _ in range(2):                                                       # two epochs: the order moves on in step
        a, b = list(res), list(ref)
        assert len(a) == len(b) == 3 and b[-1]["data_0"].shape[0] == 1       # the partial last batch
        for x, y in zip(a, b):
            _same_batch(x, y)
            assert ("data_3" in x) == (step == "synthesize" and mode != "validate")
            if "data_2" in x:                                                # speaker codes: the stacked .npy files, bit for bit
                assert tuple(x["data_2"].shape) == (x["data_0"].shape[0], 200, 1)


def test_speaker_codes_are_the_stacked_npy_files(tmp_path):
    import os
    from spoofsv_amd import harness
    cfg, spec = _corpus(tmp_path)
    res = harness.CorpusSource(dict(cfg, CORPUS_RESIDENT=True), "train_text2mel", "conditional", "validate", 7, spec)      # validate: file order
    (batch,) = list(res)
    want = torch.stack([torch.from_numpy(np.load(os.path.join(cfg["SPK_EMB_DIR"], w[-12:-8] + ".npy"))).view(-1, 1) for w in res.wavlist], 0)
    assert batch["data_2"].dtype == torch.float32 and batch["data_2"].cpu().numpy().tobytes() == want.numpy().tobytes()


def test_prefetcher_gathers_on_the_consuming_thread(tmp_path):
    from spoofsv_amd import harness
    cfg, spec = _corpus(tmp_path)
    dev = torch.device(DEV)
    ref = harness.Prefetcher(harness.BatchSource(cfg, "train_ssrn", 3, spec, seed=1), dev)
    src = harness.BatchSource(dict(cfg, CORPUS_RESIDENT=True), "train_ssrn", 3, spec, seed=1)
    assert src.device_features and not ref.source.device_features
    inner, threads = src.corpus.finish_batch, []

    def recording(hb):
        threads.append(threading.get_ident())
        assert set(hb) == {"_rows", "_row0", "_B"}                          # bookkeeping only crossed the queue
        return inner(hb)
    src.corpus.finish_batch = recording
    res = harness.Prefetcher(src, dev)
    for _ in range(2):
        a, b = list(res), list(ref)
        assert len(a) == len(b) == 3
        for x, y in zip(a, b):
            _same_batch(x, {k: v.cpu() for k, v in y.items()})
    assert len(threads) == 6 and set(threads) == {threading.get_ident()}


# ---------------------------------------------------------------------------------------------- the trainers on both modes
def _train_cfg(tmp_path, **over):
    cfg, spec = _corpus(tmp_path, n_items=5)
    cfg.update(BATCH_SIZE=2, HIDDEN_DIM=32, TEXT_EMB_DIM=16, SSRN_DIM=32, DISC_DIM=16, VAL_EVERY_ITER=1000, MAX_EPOCHS=2, MAX_ITERATIONS=3)
    cfg.update(over)
    return cfg, spec


def _history(step, cfg, spec, tag, stats=None):
    from spoofsv_amd import harness
    torch.manual_seed(0)
    _, hist = harness.ordinary_train(step, "conditional", copy.deepcopy(cfg), spec_dir=spec, current_time=tag, bucket_stats=stats)
    return hist


@pytest.mark.parametrize("step", ["train_text2mel", "train_ssrn"])
def test_ordinary_train_logs_the_cache_modes_losses(tmp_path, step):
    cfg, spec = _train_cfg(tmp_path)
    c1, c2 = _history(step, cfg, spec, "c1"), _history(step, cfg, spec, "c2")
    res = _history(step, dict(cfg, CORPUS_RESIDENT=True), spec, "r")
    allowed = max(abs(a - b) for a, b in zip(c1, c2))                        # what two cache-mode runs show against each other (expected: 0)
    print("cache", c1, "cache again", c2, "resident", res, "allowed", allowed)
    assert len(res) == len(c1) == 3 and all(h == h for h in res)
    assert max(abs(a - b) for a, b in zip(res, c1)) <= allowed


@pytest.mark.parametrize("step,buckets", [("train_text2mel", [[64, 32]]), ("train_ssrn", [32])])
def test_ordinary_train_replays_buckets_on_resident_batches(tmp_path, step, buckets):
    cfg, spec = _train_cfg(tmp_path, MAX_ITERATIONS=5, LENGTH_BUCKETS=buckets)
    c1, c2 = _history(step, cfg, spec, "c1"), _history(step, cfg, spec, "c2")
    st = {}
    res = _history(step, dict(cfg, CORPUS_RESIDENT=True), spec, "r", st)
    allowed = max(abs(a - b) for a, b in zip(c1, c2))
    print("cache", c1, "cache again", c2, "resident", res, "allowed", allowed, st)
    assert st["replays"] > 0 and len(res) == len(c1) == 5
    assert max(abs(a - b) for a, b in zip(res, c1)) <= allowed


@pytest.mark.parametrize("step", ["train_text2mel", "train_ssrn"])
def test_one_adversarial_iteration_prints_the_cache_modes_losses(tmp_path, capsys, step):
    from spoofsv_amd import harness, ops
    cfg, spec = _train_cfg(tmp_path, MAX_ITERATIONS=1)

    def run(c, tag):
        torch.manual_seed(0)
        for ctr in ops._DROP_CTR.values():                                   # the critics' dropout stream starts over, as in a fresh process
            ctr.zero_()                                                      # (a counter that does not exist yet is created at zero)
        capsys.readouterr()
        harness.adversarial_train(step, "conditional", copy.deepcopy(c), spec_dir=spec, current_time=tag)
        return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("training")]
    ref = run(cfg, "c")
    res = run(dict(cfg, CORPUS_RESIDENT=True), "r")
    assert len(ref) == 1 and ref[0].startswith("training G") and "nan" not in ref[0]
    assert res == ref
