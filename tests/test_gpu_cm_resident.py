"""The countermeasure on a resident feature corpus: ssv_corpus_scatter / ssv_corpus_gather round trips in poisoned arenas, the fused head
with a live width against the float64 formulas of tests/_countermeasure_ref.py, the whole classifier in a padded bucket against the
float64 restatement in every arithmetic mode, resident batches against today's batches, the trainer end to end on replayed steps, and a
replayed step against the eager step on identical weights.  Helpers, bars and cached references are those of
tests/test_gpu_countermeasure.py.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest
import torch

import _countermeasure_ref as R
import test_gpu_countermeasure as T0
from test_gpu_countermeasure import precision  # noqa: F401  (the fixture that sets and restores the arithmetic mode)

pytestmark = pytest.mark.gpu
DEV = T0.DEV
POISON = T0.POISON
GUARD = 64
_ptr, _stream, _report = T0._ptr, T0._stream, T0._report


def _poisoned(n):
    return torch.from_numpy(np.full(n, POISON, dtype=np.int32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


# ================================================================================================ 1. scatter and gather
LENGTHS = [37, 0, 1, 130, 3, 4]                   # row starts miss 16-byte alignment whenever F * len is no multiple of 4
TOO_LONG, OUTSIDE = 200, 5


@pytest.mark.parametrize("wider", [False, True], ids=["width_longest", "width_wider"])
@pytest.mark.parametrize("F", [1, 5, 513])
def test_scatter_gather_round_trip_in_a_poisoned_arena(F, wider):
    """Items 1 .. 6 of the table take the six lengths, item 7 is longer than the batch is wide, item 8's block leaves the arena, item 0 is
    not part of the call (item0 = 1).  Blocks lie 3 words apart behind a guard, so starts of every alignment occur."""
    from spoofsv_amd import _lib
    width = max(LENGTHS) + (3 if wider else 0)
    B = len(LENGTHS) + 2
    src_bs = F * width + (4 if wider else 0)
    rng = np.random.default_rng(100 * F + wider)
    src = rng.standard_normal((B, src_bs)).astype(np.float32)
    lens = [2] + LENGTHS + [TOO_LONG, OUTSIDE]
    offs, cur = [], GUARD
    for n in lens[:-1]:
        offs.append(cur)
        cur += F * n + 3
    arena_n = cur + GUARD
    offs.append(arena_n - 2)                                    # F * 5 words from here leave the arena
    arena = _poisoned(arena_n + GUARD)                          # a guard behind the arena the kernel is told of
    src_d = torch.from_numpy(src).to(DEV)
    off_d = torch.tensor(offs, dtype=torch.int64, device=DEV)
    len_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _lib.call("ssv_corpus_scatter", _ptr(src_d), src_bs, B, F, width, _ptr(arena), arena_n, _ptr(off_d), _ptr(len_d), len(lens), 1, _stream())
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    want = np.full(arena_n + GUARD, POISON, dtype=np.int32)
    rows = src[:, :F * width].reshape(B, F, width)
    for b, n in enumerate(LENGTHS):
        want[offs[1 + b]:offs[1 + b] + F * n] = np.ascontiguousarray(rows[b, :, :n]).view(np.int32).ravel()
    assert np.array_equal(got, want), "a fitting block differs from its source, or a skipped item, a gap or a guard was written"
    assert np.array_equal(_bits(src_d), src.view(np.int32)) and len_d.tolist() == lens and off_d.tolist() == offs
    # gather a permutation of the fitting items: the zero-padded batch, bitwise
    perm = [4, 1, 6, 2, 3, 5]
    rows_d = torch.tensor([0] + perm, dtype=torch.int32, device=DEV)
    for gw in (width, width + 5):
        out = _poisoned(len(perm) * F * gw + 8).view(torch.float32)
        _lib.call("ssv_corpus_gather", _ptr(arena.view(torch.float32)), arena_n, _ptr(off_d), _ptr(len_d), len(lens), _ptr(rows_d), rows_d.numel(), 1,
                  _ptr(out), len(perm), F, gw, F * gw, _stream())
        torch.cuda.synchronize()
        exp = np.zeros((len(perm), F, gw), dtype=np.float32)
        for b, i in enumerate(perm):
            exp[b, :, :lens[i]] = rows[i - 1, :, :lens[i]]
        host = out.view(torch.int32).cpu().numpy()
        assert np.array_equal(host[:-8], exp.view(np.int32).ravel()) and np.all(host[-8:] == POISON)


# ================================================================================================ 2. the head with a live width
LEN_SHAPES = [(3, 4, 9), (5, 8, 37), (2, 16, 130)]


def _run_head_len(dev_in, B, C, T, live, out=None):
    from spoofsv_amd import _lib
    x, w, bias, labels, gs = dev_in
    out = out if out is not None else T0._head_outputs(B, C, T)
    _lib.call("ssv_cm_head_fwd_len", _ptr(x), _ptr(w), _ptr(bias), _ptr(labels), R.SLOPE, _ptr(out.t("pred")), _ptr(out.t("amean")), _ptr(out.t("per")),
              _ptr(out.t("loss")), B, C, T, _ptr(live), _stream())
    _lib.call("ssv_cm_head_bwd_len", _ptr(x), _ptr(w), _ptr(bias), _ptr(labels), _ptr(out.t("amean")), _ptr(gs), R.SLOPE, _ptr(out.t("dx")),
              _ptr(out.t("dw")), _ptr(out.t("dbias")), _ptr(out.t("dz")), B, C, T, _ptr(live), _stream())
    return out, ["pred", "amean", "per", "loss", "dx", "dw", "dbias", "dz"]


@pytest.mark.parametrize("shape", LEN_SHAPES, ids=lambda s: "B%d_C%d_T%d" % s)
def test_head_with_live_width_against_float64(shape):
    B, C, T = shape
    gscale = 0.37
    ok = True
    for kind in ("mixed", "sat-"):
        x, w, bias, labels = T0._head_inputs(B, C, T, kind, seed=B * 10000 + C * 100 + T)
        for live in (1, T - 1, T, T + 7):
            Tl = min(live, T)
            xn = x.copy()
            xn[:, :, Tl:] = np.nan
            dev_in = [torch.from_numpy(a.copy()).to(DEV) for a in (xn, w, bias, labels)] + [torch.tensor([gscale], device=DEV)]
            live_d = torch.tensor([live], dtype=torch.int32, device=DEV)
            out, written = _run_head_len(dev_in, B, C, T, live_d)
            torch.cuda.synchronize()
            host = out.host()
            what = "B=%d C=%d T=%d live=%d %s" % (B, C, T, live, kind)
            assert out.guards_intact(host, written), what + ": guard words were written"
            assert np.array_equal(_bits(dev_in[0]), xn.view(np.int32)), what + ": x was written"
            ref = R.head_ref(x[:, :, :Tl], w, bias, labels, R.SLOPE, gscale)
            for name in written:
                assert not np.any(np.isnan(out.get(host, name))), what + ": NaN in " + name
            scal = lambda name, want: float(np.max(np.abs(out.get(host, name) - np.ravel(want)) / np.maximum(1.0, np.abs(np.ravel(want)))))
            for name, want in (("pred", ref.pred), ("per", ref.per), ("loss", ref.loss), ("dw", ref.dw), ("dbias", ref.dbias)):
                ok &= _report("len", what + " " + name, scal(name, want), T0.HEAD_TOL)
            dx = out.get(host, "dx").reshape(B, C, T)
            worst = max(float(np.linalg.norm(dx[b, :, :Tl] - ref.dx[b]) / np.linalg.norm(ref.dx[b])) for b in range(B))
            ok &= _report("len", what + " dx, worst item rel_l2", worst, T0.HEAD_TOL)
            o, n = out.at["dx"]
            assert np.all(host[o:o + n].reshape(B, C, T)[:, :, Tl:] == 0), what + ": dx beyond the live width is not exactly +0"
            if live >= T:                          # the whole row is live: the bits of the dense entries
                dense, _ = T0._run_head(dev_in, B, C, T, gscale)
                torch.cuda.synchronize()
                assert np.array_equal(dense.host(), host), what + ": differs from ssv_cm_head_fwd / _bwd"
    assert ok


def test_head_len_capture_and_two_replays_follow_the_live_width():
    from spoofsv_amd.train import _no_gc
    B, C, T = 5, 8, 65
    x, w, bias, labels = T0._head_inputs(B, C, T, "mixed", seed=78)
    x[:, :, T - 1:] = np.nan
    dev_in = [torch.from_numpy(a.copy()).to(DEV) for a in (x, w, bias, labels)] + [torch.tensor([1.0], device=DEV)]
    live = torch.tensor([T - 1], dtype=torch.int32, device=DEV)
    want = {}
    for v in (T - 1, 1):
        live.fill_(v)
        eager, written = _run_head_len(dev_in, B, C, T, live)
        torch.cuda.synchronize()
        want[v] = eager.host()
    assert not np.array_equal(want[1], want[T - 1])
    out = T0._head_outputs(B, C, T)
    live.fill_(17)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc(), torch.cuda.graph(graph):
        _run_head_len(dev_in, B, C, T, live, out=out)
    torch.cuda.synchronize()
    assert np.all(out.host() == POISON)                      # capturing runs nothing
    for v in (T - 1, 1):
        live.fill_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.host(), want[v]), "the replay with live = %d differs from the eager run" % v
        for name in written:
            out.t(name).view(torch.int32).fill_(POISON)


# ================================================================================================ 3. the whole classifier in a bucket
BUCKET = {"lin": 64, "mel": 40}


@pytest.mark.parametrize("precision", T0.MODES, indirect=True)
@pytest.mark.parametrize("kind", ["mel", "lin"])
def test_whole_classifier_in_a_bucket_vs_float64(kind, precision):
    """The committed dense case (3, 24, 37) gathered into a static buffer of width 64 / 40 and run with ``live``, dropout off: pred, loss
    and every parameter gradient against the float64 restatement ON THE UNPADDED CASE, with the bars of
    test_small_whole_classifier_vs_float64 (max(2e-6, 16 e32) scalars, max(2e-5, 16 e32) gradients; bf16x3 1e-4 and 2e-3)."""
    from spoofsv_amd import countermeasure as C
    sd, x, labels, _ = R.cm_case(kind)
    assert R.kink_margin(sd, kind, x, False) > R.KINK_MARGIN
    want, cpu32 = T0._cached((kind, False), lambda: (R.cm_reference(sd, kind, x, labels, False, torch.float64),
                                                     R.cm_reference(sd, kind, x, labels, False, torch.float32)))
    Fb, dim, B, T = R.CM_SHAPE
    corpus = C.CmResidentCorpus.from_features([x[b] for b in range(B)], labels, kind, batch_size=B, device=DEV)
    W = BUCKET[kind]
    buf = torch.full((B, Fb, W), 7.0, device=DEV)             # the gather writes the padding
    yd = torch.full((B,), -1.0, device=DEV)
    corpus.gather_into(buf, corpus.rows_of(np.arange(B)), 0, yd)
    assert torch.equal(buf[:, :, :T].cpu(), x) and float(buf[:, :, T:].abs().max()) == 0 and torch.equal(yd.cpu(), labels)
    live = torch.tensor([T, C.head_width(kind, T)], dtype=torch.int32, device=DEV)
    disc = (C.CmLinDisc if kind == "lin" else C.CmMelDisc)(Fb, dim)
    disc.load_state_dict(sd)
    disc = disc.to(DEV).eval()
    loss, pred = disc.loss(buf, yd, live)
    loss.backward()
    tag = "%s bucket %d %s" % (kind, W, precision)
    bf = precision == "bf16x3"
    ok = True
    e32 = float((cpu32[0] - want[0]).abs().max() / want[0].abs().max())
    err = float((pred.detach().double().cpu() - want[0]).abs().max() / want[0].abs().max())
    ok &= _report("bucket", "%s pred (cpu32 %.2e)" % (tag, e32), err, 1e-4 if bf else max(2e-6, 16 * e32))
    e32 = abs(cpu32[1] - want[1]) / abs(want[1])
    ok &= _report("bucket", "%s loss (cpu32 %.2e)" % (tag, e32), abs(float(loss.detach()) - want[1]) / abs(want[1]), 1e-4 if bf else max(2e-6, 16 * e32))
    rel_l2 = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())
    for n, p in disc.named_parameters():
        w = want[2][n]
        assert p.grad is not None and p.grad.shape == w.shape, n
        if n in T0._ZERO_GRAD:
            continue
        e32 = rel_l2(cpu32[2][n], w)
        ok &= _report("bucket", "%s grad %s (cpu32 %.2e)" % (tag, n, e32), rel_l2(p.grad.detach(), w), 2e-3 if bf else max(2e-5, 16 * e32))
    assert ok


# ================================================================================================ 4. resident batches are today's batches
CFG = T0.CFG
_SOURCES = {}


def _toy_source(root, spoof_rate=22050):
    """The toy corpus: 12 bona fide wav files, and the spoof class as device waveforms of unequal lengths, 0.6 .. 1.0 s."""
    from spoofsv_amd import countermeasure as C
    bona, spoof_paths = R.write_toy_corpus(root)
    n = len(spoof_paths)
    waves = np.stack([R.toy_wave(i, 0, spoof_rate) for i in range(n)])
    lengths = [int(spoof_rate * (0.6 + 0.4 * i / (n - 1))) for i in range(n)]
    spoof = (torch.from_numpy(waves).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV), spoof_rate)
    return C.CmSource(CFG, bona, spoof, batch_size=T0.E2E_BATCH, seed=0)


@pytest.mark.parametrize("feat", ["lin", "mel"])
def test_resident_batches_are_the_sources_batches(feat, tmp_path):
    from spoofsv_amd import countermeasure as C
    source = _toy_source(str(tmp_path))
    corpus = C.CmResidentCorpus(source, feat)
    key = corpus.key
    assert len(corpus) == 24 and corpus.n_batches() == 3 and corpus.device == source.device and corpus.bytes >= 4 * corpus.used > 0
    assert len(set(corpus.lens[12:].tolist())) > 1               # the spoof items differ in length
    plain = []
    for got, want in zip(corpus.batches(), source.batches()):
        assert set(got) == {key, "data_2"}
        assert got[key].shape == want[key].shape and np.array_equal(_bits(got[key]), _bits(want[key]))      # features and zero padding
        assert np.array_equal(_bits(got["data_2"]), _bits(want["data_2"]))
        plain.append(got[key].cpu())
    assert len(plain) == 3
    block = lambda i: plain[i // 8][i % 8, :, :int(corpus.lens[i])]
    order = C.epoch_order(24, 0, 3)
    assert not np.array_equal(order, np.arange(24))
    for k, got in enumerate(corpus.batches(shuffle=True, epoch=3)):
        idx = order[8 * k:8 * k + 8]
        feats = got[key].cpu()
        assert feats.shape[2] == max(int(corpus.lens[idx].max()), corpus.min_width)
        assert got["data_2"].cpu().tolist() == [1.0 if i < 12 else 0.0 for i in idx]
        for b, i in enumerate(idx):
            n = int(corpus.lens[i])
            assert torch.equal(feats[b, :, :n].view(torch.int32), block(i).view(torch.int32)), (k, b, i)
            assert float(feats[b, :, n:].abs().sum()) == 0
    one = corpus.batch([5, 20, 7])
    assert torch.equal(one[key][1, :, :int(corpus.lens[20])].cpu(), block(20)) and one["data_2"].tolist() == [1.0, 0.0, 1.0]
    # score through the corpus writes the file score writes through the source
    torch.manual_seed(11)
    ckpt = {"model_state_dict": C.build_model(CFG, feat).state_dict()}
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    eer_a, eer_b = C.score(CFG, source, ckpt, a, feat), C.score(CFG, corpus, ckpt, b, feat)
    assert open(a, "rb").read() == open(b, "rb").read() and eer_a == eer_b and len(open(a).read().splitlines()) == 24


# ================================================================================================ 5. end to end
@pytest.mark.parametrize("case", ["lin_paths", "mel_spoof_device_22k"])
def test_resident_replayed_training_end_to_end(case, tmp_path):
    """test_train_resume_and_score_end_to_end's corpus, iteration counts (k = 10 / 18, half before a resume) and bookkeeping, trained from
    the resident corpus with one bucket wider than every batch: every full batch replays behind the masks."""
    from spoofsv_amd import countermeasure as C
    feat, k = ("lin", 10) if case == "lin_paths" else ("mel", 18)
    bona, spoof_paths = R.write_toy_corpus(str(tmp_path))
    if case == "lin_paths":
        spoof = spoof_paths
    else:
        waves = np.stack([R.toy_wave(i, 0, 22050) for i in range(len(spoof_paths))])
        spoof = (torch.from_numpy(waves).to(DEV), torch.full((len(waves),), waves.shape[1], dtype=torch.int32, device=DEV), 22050)
    source = C.CmSource(CFG, bona, spoof, batch_size=T0.E2E_BATCH, seed=0)
    samples = C.CmResidentCorpus._samples(source)
    bucket = int(C.frames_bound(CFG, samples, feat).max()) + 8
    save_dir = str(tmp_path / "ckpt")
    half = k // 2
    torch.manual_seed(T0.E2E_SEED)
    first = C.train(CFG, source, feat, save_dir=save_dir, save_interval=half - 1, max_iterations=half, log=lambda *a: None, resident=True,
                    width_buckets=[bucket], log_interval=3)
    path = os.path.join(save_dir, "%d_iteration.tar.pth" % half)
    assert first["checkpoints"] == [path] and first["global_iteration"] == half and len(first["losses"]) == half
    assert first["captures"] == 1 and first["replays"] > 0 and first["replays"] + first["eager"] == half and first["capture_seconds"] > 0
    assert all(np.isfinite(v) and v > 0 for v in first["losses"])
    ckpt = torch.load(path, map_location="cpu")
    assert set(ckpt) == {"epoch", "global_iteration", "model_state_dict", "optimizer_state_dict"}
    assert ckpt["global_iteration"] == half - 1 and ckpt["epoch"] == first["epoch"] + 1
    assert ckpt["optimizer_state_dict"]["param_groups"][0]["amsgrad"] is True
    assert "max_exp_avg_sq" in ckpt["optimizer_state_dict"]["state"][0]
    assert int(ckpt["optimizer_state_dict"]["state"][0]["step"]) == half          # the capture's warm-up iterations were undone
    second = C.train(CFG, source, feat, save_dir=save_dir, resume=path, save_interval=k - 2, max_iterations=k - half, log=lambda *a: None,
                     resident=True, width_buckets=[bucket])
    assert second["global_iteration"] == k - 1
    final = os.path.join(save_dir, "%d_iteration.tar.pth" % (k - 1))
    assert second["checkpoints"] == [final]
    assert second["captures"] == 1 and second["replays"] > 0 and second["replays"] + second["eager"] == k - half
    assert int(second["optimizer"].state_dict()["state"][0]["step"]) == k
    out = str(tmp_path / "cm_scores" / "scores_t.txt")
    eer = C.score(CFG, source, final, out, feat)
    T0._check_score_file(out, source, C.load_model(CFG, final, feat, DEV), feat, 24)
    print("%s replayed: losses %s ... %s, EER %.3f" % (case, ["%.3f" % v for v in first["losses"][:3]], ["%.3f" % v for v in second["losses"][-3:]], eer))
    assert eer == 0.0
    # resident, eager: no buckets
    corpus = C.CmResidentCorpus(source, feat)
    torch.manual_seed(T0.E2E_SEED)
    third = C.train(CFG, corpus, feat, save_dir=str(tmp_path / "ckpt_eager"), max_iterations=k, log=lambda *a: None)
    assert third["replays"] == 0 and third["captures"] == 0 and third["eager"] == k and len(third["losses"]) == k
    eer = C.score(CFG, corpus, {"model_state_dict": third["model"].state_dict()}, str(tmp_path / "cm_scores" / "scores_e.txt"), feat)
    assert eer == 0.0


# ================================================================================================ 6. a replayed step against the eager step
def test_replayed_step_against_eager_step_on_identical_weights(monkeypatch):
    """A ragged batch (widths 37 .. 64) in a bucket of 80, fp32 arithmetic, dropout off: the gradients the replayed iteration leaves
    against those of the eager iteration on the unpadded batch from the same weights.  The bar is the 2e-5 of the project's fp32-grade
    gradient comparisons; the biases in front of a LayerNorm (zero in exact arithmetic) are left out as everywhere."""
    import spoofsv_amd
    from spoofsv_amd import countermeasure as C
    from spoofsv_amd import critic
    from spoofsv_amd.train import FusedAdamEx
    monkeypatch.setattr(critic, "_P_DROP", 0.0)
    spoofsv_amd.set_precision("fp32")
    Fb, dim = 24, 16
    g = torch.Generator().manual_seed(21)
    widths = [37, 50, 41, 64]
    blocks = [torch.rand(Fb, n, generator=g) for n in widths]
    labels = [1.0, 0.0, 0.0, 1.0]
    corpus = C.CmResidentCorpus.from_features(blocks, labels, "lin", batch_size=4, device=DEV)
    torch.manual_seed(22)
    model = C.CmLinDisc(Fb, dim)
    sd = {n: v.clone() for n, v in model.state_dict().items()}
    model = model.to(DEV).train()
    opt = FusedAdamEx([p for p in model.parameters() if p.requires_grad], capturable=True, **C.ADAM)
    opt.refresh_resident_weights()
    stepper = C.CmBucketedStep(model, opt, corpus, [80])
    idx = np.arange(4)
    rows = corpus.rows_of(idx)
    assert stepper.bucket_of(idx) == 80
    loss = float(stepper.step(rows, 0, idx))
    assert (stepper.replays, stepper.captures, stepper.eager) == (1, 1, 0)
    assert int(opt.state_dict()["state"][0]["step"]) == 1         # one step counted: the warm-up was undone
    got = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}
    stepper.close()
    eager = C.CmLinDisc(Fb, dim)
    eager.load_state_dict(sd)
    eager = eager.to(DEV).train()
    sp = corpus.batch(idx)
    assert sp["data_1"].shape == (4, Fb, 64)
    want_loss, _ = eager.loss(sp["data_1"], sp["data_2"])
    want_loss.backward()
    ok = _report("step", "replayed loss against eager loss", abs(loss - float(want_loss)) / abs(float(want_loss)), 2e-5)
    worst = 0.0
    for n, p in eager.named_parameters():
        if n in T0._ZERO_GRAD:
            continue
        w = p.grad.detach().double().cpu()
        assert float(w.norm()) > 0, n
        err = float((got[n] - w).norm() / w.norm())
        worst = max(worst, err)
        ok &= _report("step", "replayed grad %s against eager" % n, err, 2e-5)
    print("replayed against eager, fp32: worst gradient rel-L2 %.3e" % worst)
    assert ok
