"""Length-masked kernels and the bucketed, replayed training step (train.BucketedTrainStep) against the eager step on the unpadded
batch: a ragged batch padded to a bucket shape must compute what the unpadded batch computes."""
import copy

import pytest
import torch

import spoofsv_amd
from spoofsv_amd import ops, train
from spoofsv_amd.tts import SSRN, melSyn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=["f16x2", "fp32"])
def precision(request):
    prev = spoofsv_amd.set_precision(request.param)
    yield request.param
    spoofsv_amd.set_precision(prev)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _lens(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("live,L", [(1, 64), (97, 128), (157, 192), (321, 325), (325, 325), (400, 325)])
def test_mask_cols_zeroes_exactly_the_tail(live, L):
    x = torch.rand(3, 513, L, device=DEV) + 0.5          # (no entry is 0 before the mask)
    ref = x.clone()
    ops._mask_cols(x, 513 * L, ops.Live(_lens(live)))
    lv = min(live, L)
    assert torch.equal(x[:, :, :lv], ref[:, :, :lv]) and bool((x[:, :, lv:] == 0).all())
    y = torch.rand(2, 256, 2 * L, device=DEV) + 0.5
    ops._mask_cols(y, 256 * 2 * L, ops.Live(_lens(live), 0, 2))
    assert bool((y[:, :, min(2 * live, 2 * L):] == 0).all()) and bool((y[:, :, :min(2 * live, 2 * L)] != 0).all())


@pytest.mark.parametrize("live,L,mult", [(1, 64, 1), (97, 128, 1), (157, 192, 1), (321, 325, 1), (157, 192, 4)])
def test_masked_spec_losses_equal_the_losses_of_the_truncated_batch(live, L, mult):
    C = 513 if mult == 4 else 80
    g = torch.Generator().manual_seed(live)
    y = torch.rand(2, C, mult * L, generator=g).to(DEV)
    gt = torch.rand(2, C, mult * L, generator=g).to(DEV)
    lv = live * mult
    seed = torch.tensor([1.0, 0.5], device=DEV)
    yp = y.clone().requires_grad_(True)
    out = ops.spec_losses_vec(yp, gt, seed, ops.Live(_lens(live), 0, mult))
    out.backward(seed)
    yt = y[:, :, :lv].contiguous().requires_grad_(True)
    ref = ops.spec_losses_vec(yt, gt[:, :, :lv].contiguous())
    ref.backward(seed)
    assert _rel(out, ref) < 1e-5
    assert _rel(yp.grad[:, :, :lv], yt.grad) < 1e-6 and bool((yp.grad[:, :, lv:] == 0).all())
    # the separate backward (no promised seed) gives the same gradient
    yq = y.clone().requires_grad_(True)
    ops.spec_losses_vec(yq, gt, None, ops.Live(_lens(live), 0, mult)).backward(seed)
    assert torch.equal(yq.grad, yp.grad)


def test_masked_guided_attention_loss_uses_the_live_block():
    gaw = train.guided_attention_mat(186, 325, device=DEV)
    a = torch.rand(3, 128, 192, device=DEV)
    ap = a.clone().requires_grad_(True)
    out = ops.guided_att_loss_vec(ap, gaw, ops.Live(_lens(101, 157)))
    out.backward(torch.ones(1, device=DEV))
    at = a[:, :101, :157].contiguous().requires_grad_(True)
    ref = ops.guided_att_loss_vec(at, gaw)
    ref.backward(torch.ones(1, device=DEV))
    assert _rel(out, ref) < 1e-5 and _rel(ap.grad[:, :101, :157], at.grad) < 1e-6
    assert float(ap.grad[:, 101:].abs().sum()) == 0 and float(ap.grad[:, :, 157:].abs().sum()) == 0


@pytest.mark.parametrize("d", [32, 256])
def test_masked_attention_leaves_out_padded_keys_and_frames(d):
    g = torch.Generator().manual_seed(d)
    N, T, Nl, Tl = 128, 192, 101, 157
    kv = torch.randn(2, 2 * d, N, generator=g).to(DEV)
    q = torch.randn(2, d, T, generator=g).to(DEV)
    kv[:, :, Nl:] = 0
    q[:, :, Tl:] = 0
    drq = torch.randn(2, 2 * d, T, generator=g).to(DEV)
    drq[:, :, Tl:] = 0
    kvp, qp = kv.clone().requires_grad_(True), q.clone().requires_grad_(True)
    rq, a = ops.attention_train(kvp, qp, ops.Live(_lens(Nl, Tl)))
    rq.backward(drq)
    kvt = kv[:, :, :Nl].contiguous().requires_grad_(True)
    qt = q[:, :, :Tl].contiguous().requires_grad_(True)
    rqt, at = ops.attention_train(kvt, qt)
    rqt.backward(drq[:, :, :Tl].contiguous())
    assert _rel(a[:, :Nl, :Tl], at) < 1e-5 and _rel(rq[:, :, :Tl], rqt) < 1e-5
    assert float(a[:, Nl:].abs().sum()) == 0 and float(a[:, :, Tl:].abs().sum()) == 0 and float(rq[:, :, Tl:].abs().sum()) == 0
    assert _rel(kvp.grad[:, :, :Nl], kvt.grad) < 1e-5 and _rel(qp.grad[:, :, :Tl], qt.grad) < 1e-5
    assert float(kvp.grad[:, :, Nl:].abs().sum()) == 0 and float(qp.grad[:, :, Tl:].abs().sum()) == 0


@pytest.mark.parametrize("C,live,L", [(256, 97, 128), (512, 157, 192), (256, 1, 64)])
def test_masked_layers_match_the_truncated_input(precision, C, live, L):
    """highwayConv (non-causal, k = 3, dilation 3) and 1x1 conv + LayerNorm + ReLU: output, input gradient and every parameter gradient
    of the masked call on the zero-padded input equal the plain call on the truncated input; the padded columns are exactly 0."""
    torch.manual_seed(C + live)
    from spoofsv_amd.tts import highwayConv
    hc = highwayConv(C, 3, 3).to(DEV)
    w1 = torch.randn(C, C, 1, device=DEV) * 0.05
    b1, g1, be1 = (torch.randn(C, device=DEV) * 0.1 for _ in range(3))
    x = torch.randn(4, C, L, device=DEV)
    x[:, :, live:] = 0
    dy = torch.randn(4, C, L, device=DEV)

    def run(xin, dyin, lv):
        params = [p for p in hc.parameters()] + [w1, b1, g1, be1]
        for p in params:
            p.requires_grad_(True)
            p.grad = None
        xi = xin.clone().requires_grad_(True)
        h = ops.highway_conv1d(xi, hc.conv.weight, hc.conv.bias, hc.ln1.weight, hc.ln1.bias, hc.ln2.weight, hc.ln2.bias, 3, 3, False, lv)
        y = ops.pointwise_conv_ln_act(h, w1, b1, g1, be1, None, 1, lv)
        y.backward(dyin)
        return y.detach(), xi.grad, [p.grad.clone() for p in params]
    ym, dxm, pm = run(x, dy, ops.Live(_lens(live)))
    yt, dxt, pt = run(x[:, :, :live].contiguous(), dy[:, :, :live].contiguous(), None)
    tol = 2e-5
    assert _rel(ym[:, :, :live], yt) < tol and float(ym[:, :, live:].abs().sum()) == 0
    assert _rel(dxm[:, :, :live], dxt) < tol
    for a, b in zip(pm, pt):
        assert _rel(a, b) < tol


# ------------------------------------------------------------------------------------------------ whole steps
def _ragged_t2m(B, N, T, seed, vocab=34):
    mel, text, spk = train.synthetic_text2mel_batch(B, N=N, T=T, seed=seed, vocab=vocab)
    g = torch.Generator().manual_seed(seed + 1)
    for b in range(1, B):                         # items shorter than the batch maximum, padded as the reference's collate pads them
        n = int(torch.randint(N // 2, N, (1,), generator=g))
        t = int(torch.randint(T // 2, T, (1,), generator=g))
        text[b, :, n:] = 0
        mel[b, :, t:] = 0
    return mel.to(DEV), text.to(DEV), spk.to(DEV)


def _ragged_ssrn(B, T, seed, out_bins):
    mel, lin = train.synthetic_ssrn_batch(B, T=T, seed=seed, out_bins=out_bins)
    g = torch.Generator().manual_seed(seed + 1)
    for b in range(1, B):
        t = int(torch.randint(T // 2, T, (1,), generator=g))
        mel[b, :, t:] = 0
        lin[b, :, 4 * t:] = 0
    return mel.to(DEV), lin.to(DEV)


def _pair(make):
    torch.manual_seed(0)
    a = make()
    a.apply(train.init_weights)
    b = make()
    b.load_state_dict(a.state_dict())
    return a.to(DEV).train(), b.to(DEV).train()


class _ArenaGrads:
    """``model`` seen through the gradient arena of a BucketedTrainStep: ``named_parameters`` yields the gradients the last replay wrote
    (on the host), in the form test_gpu_parity's oracle check reads."""

    class _P:
        def __init__(self, g):
            self.grad = g

        def numel(self):
            return self.grad.numel()

    def __init__(self, model, arena):
        self.model, self.arena = model, arena

    def named_parameters(self):
        for k, p in self.model.named_parameters():
            yield k, self._P(self.arena.slot(p).detach().cpu())


def _oracle_record(kind, model, batch, live, gaw):
    """The float64 oracle's forward, losses, kink sides and parameter gradients on the UNPADDED batch (its own maxima ``live``) at the
    model's current weights."""
    from oracle import tts_oracle as TO
    from test_gpu_parity import _oracle_pass
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    cpu = type("Weights", (), {"state_dict": lambda self: sd})()
    if kind == "text2mel":
        mel, text, spk = batch
        N, T = live
        b = (mel[:, :, :T].cpu(), text[:, :, :N].cpu(), spk.cpu())
    else:
        mel, lin = batch
        (T,) = live
        b = (mel[:, :, :T].cpu(), lin[:, :, :4 * T].cpu())
    rec = dict(model=cpu, batch=b, gaw=gaw.cpu() if gaw is not None else None, kind=kind)
    with TO.kink_sides() as sides:
        _, losses, grads = _oracle_pass(rec, torch.float64)
    rec.update(losses64=losses, grads64=grads, kinks64=sides.taps)
    return rec


def _check_run(kind, ma, mb, batches, buckets, precision, gaw=None, loss_tol=2e-5):
    """Bucketed replay on ``ma`` over a batch sequence.  Every iteration: the losses and EVERY parameter gradient of the replay against
    the float64 oracle on the unpadded batch, held on the replay's kink sides (ReLUs, L1; tests/test_gpu_parity.py, 2e-5 rel. L2 in
    both fp32-grade modes); and the losses against the eager HIP step on the unpadded batch with the same weights (``mb`` is set to
    ``ma``'s weights before each iteration, so that the comparison does not carry Adam's amplification of rounding from step to step)."""
    from test_gpu_parity import _check_grads_on_hip_sides
    oa = train.FusedAdam(ma.parameters(), 2e-4, (0.5, 0.9), 1e-6, capturable=True)
    ob = train.FusedAdam(mb.parameters(), 2e-4, (0.5, 0.9), 1e-6)
    bt = train.BucketedTrainStep(kind, ma, oa, buckets, gaw=gaw)
    taps = None
    try:
        for i, batch in enumerate(batches):
            live = bt._need(batch)
            with torch.no_grad():
                for pa, pb in zip(ma.parameters(), mb.parameters()):
                    pb.copy_(pa)
            ob.refresh_resident_weights()
            rec = _oracle_record(kind, ma, batch, live, gaw)
            n = len(rec["kinks64"]) - 1                  # ReLU taps per forward (the last oracle kink is the L1 loss's)
            if taps is None:
                # the first call warms up and captures: the capture's taps (the last n) are tensors of the graph, rewritten by every replay
                ops.RELU_TAP = []
                try:
                    la = [float(v) for v in bt(*batch)]
                    taps = ops.RELU_TAP[-n:]
                finally:
                    ops.RELU_TAP = None
            else:
                la = [float(v) for v in bt(*batch)]
            st = bt.steps[bt.last_bucket]
            T = live[-1] * (4 if kind == "ssrn" else 1)
            sides = [t[..., :ref[0].shape[-1]].cpu() for t, (ref, _, _) in zip(taps, rec["kinks64"][:n])]
            d = (st.pred - st.static[0 if kind == "text2mel" else 1])[..., :T]
            sides.append((d > 0).cpu())
            for x, y in zip(la, rec["losses64"]):
                assert abs(x - y) <= 1e-5 * max(1.0, abs(y)), (i, la, rec["losses64"])
            _check_grads_on_hip_sides(rec, _ArenaGrads(ma, bt.ddp.arena), sides, precision, "bucketed %s iteration %d" % (kind, i),
                                      torch.sign(d).cpu())
            if kind == "text2mel":
                lb = [float(v) for v in train.text2mel_step(mb, ob, *batch, gaw)[:3]]
            else:
                lb = [float(v) for v in train.ssrn_step(mb, ob, *batch)]
            for x, y in zip(la, lb):
                assert abs(x - y) <= loss_tol * max(abs(y), 1e-3), (i, la, lb)
        assert bt.replays == len(batches) and bt.eager == 0
        assert all(v > 0 for v in bt.pool_bytes.values())
        return bt.captures
    finally:
        bt.close()


@pytest.mark.parametrize("hidden", [256, 32])
def test_text2mel_bucketed_replay_matches_oracle_and_eager_unpadded(precision, hidden):
    """Full width (fused attention in the eager step) and a small width (the general attention path): ragged batches at
    (N_b, T_b) = (101, 157), (60, 90), (101, 157) replayed in one (128, 192) bucket -- long, short, long: columns a longer batch
    leaves behind never leak into a shorter one."""
    ma, mb = _pair(lambda: melSyn(34, True, 200, textemb_dim=128 if hidden == 256 else 16, freq_bins=80, hidden_dim=hidden))
    gaw = train.guided_attention_mat(186, 325, device=DEV)
    batches = [_ragged_t2m(8, 101, 157, 1), _ragged_t2m(8, 60, 90, 2), _ragged_t2m(8, 101, 157, 3)]
    assert _check_run("text2mel", ma, mb, batches, [(128, 192)], precision, gaw) == 1


def test_ssrn_bucketed_replay_matches_oracle_and_eager_unpadded(precision):
    ma, mb = _pair(lambda: SSRN(80, 513, 256))
    batches = [_ragged_ssrn(4, 157, 1, 513), _ragged_ssrn(4, 70, 2, 513), _ragged_ssrn(4, 157, 3, 513)]
    assert _check_run("ssrn", ma, mb, batches, [192], precision) == 1


def test_a_second_bucket_keeps_adams_step_count():
    """Replays in one bucket, then a capture of another: Adam's bias correction continues from the device step count (replays advance
    only that one), so the run matches eager training step for step."""
    ma, mb = _pair(lambda: SSRN(80, 65, 32))
    oa = train.FusedAdam(ma.parameters(), 2e-4, (0.5, 0.9), 1e-6, capturable=True)
    ob = train.FusedAdam(mb.parameters(), 2e-4, (0.5, 0.9), 1e-6)
    bt = train.BucketedTrainStep("ssrn", ma, oa, [32, 64])
    try:
        seq = [_ragged_ssrn(2, 30, 1, 65), _ragged_ssrn(2, 28, 2, 65), _ragged_ssrn(2, 31, 3, 65), _ragged_ssrn(2, 60, 4, 65),
               _ragged_ssrn(2, 50, 5, 65), _ragged_ssrn(2, 20, 6, 65)]
        for i, batch in enumerate(seq):
            la = [float(v) for v in bt(*batch)]
            lb = [float(v) for v in train.ssrn_step(mb, ob, *batch)]
            assert int(oa._step_dev.item()) == i + 1 == ob._steps, (i, int(oa._step_dev.item()))
            # (losses: Adam's early, sign-like updates amplify rounding from step to step; a reset bias correction moves them by percent)
            assert all(abs(x - y) <= 1e-3 * max(abs(y), 1e-3) for x, y in zip(la, lb)), (i, la, lb)
        assert (bt.replays, bt.eager, bt.captures) == (6, 0, 2)
        assert float(oa.state_dict()["state"][0]["step"]) == 6
    finally:
        bt.close()


@pytest.mark.parametrize("kind", ["ssrn", "text2mel"])
def test_a_capture_leaves_model_and_optimizer_as_they_were_before_it(kind):
    """After the first bucket's capture and before any replay the warm-up iterations are undone: every parameter equals a never-trained
    twin bitwise, Adam's moments and device step count are 0, and the resident planes are current and byte for byte a fresh split of the
    restored weights."""
    from spoofsv_amd import resident
    if kind == "ssrn":
        ma, mb = _pair(lambda: SSRN(80, 65, 32))
        batch, bucket, gaw = _ragged_ssrn(2, 30, 1, 65), (32,), None
    else:
        ma, mb = _pair(lambda: melSyn(34, True, 200, textemb_dim=16, freq_bins=80, hidden_dim=32))
        batch, bucket, gaw = _ragged_t2m(2, 17, 30, 1), (24, 32), train.guided_attention_mat(186, 325, device=DEV)
    oa = train.FusedAdam(ma.parameters(), 2e-4, (0.5, 0.9), 1e-6, capturable=True)
    bt = train.BucketedTrainStep(kind, ma, oa, [bucket], gaw=gaw)
    try:
        st = bt._capture(bucket, batch)
        assert st.stepper.plan is not None and (bt.captures, bt.replays, bt.eager) == (1, 0, 0)
        for (k, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            assert torch.equal(pa, pb), k
        assert oa.state                                             # (the warm-up created the moments)
        for s in oa.state.values():
            assert not s["exp_avg"].any() and not s["exp_avg_sq"].any()
        assert int(oa._step_dev.item()) == 0 and oa._steps == 0
        convs = [p for p in ma.parameters() if resident.eligible(p)]
        plain = [p for p in convs if not getattr(p, "_ssv_transposed", False)]
        assert plain and all(resident.lookup(p) is not None for p in plain)

        # the planes are those of the RESTORED weights: a fresh split of every weight as it stands now writes the same bytes
        planes = [t.clone() for t in oa._resident._planes]
        resident.invalidate(convs)
        assert all(resident.lookup(p) is None for p in plain)
        oa.refresh_resident_weights()
        torch.cuda.synchronize()
        assert len(planes) == len(convs)
        for p, was, now in zip(oa._resident.params, planes, oa._resident._planes):
            assert torch.equal(was, now), tuple(p.shape)
    finally:
        bt.close()


def test_other_batch_sizes_and_oversized_batches_run_eagerly():
    ma, mb = _pair(lambda: SSRN(80, 65, 32))
    oa = train.FusedAdam(ma.parameters(), 2e-4, (0.5, 0.9), 1e-6, capturable=True)
    ob = train.FusedAdam(mb.parameters(), 2e-4, (0.5, 0.9), 1e-6)
    bt = train.BucketedTrainStep("ssrn", ma, oa, [48], batch_size=2)
    try:
        for batch in [_ragged_ssrn(2, 40, 1, 65), _ragged_ssrn(1, 30, 2, 65), _ragged_ssrn(2, 60, 3, 65), _ragged_ssrn(2, 48, 4, 65)]:
            la = [float(v) for v in bt(*batch)]
            lb = [float(v) for v in train.ssrn_step(mb, ob, *batch)]
            assert all(abs(x - y) <= 2e-5 * max(abs(y), 1e-3) for x, y in zip(la, lb)), (la, lb)
        assert (bt.replays, bt.eager, bt.captures) == (2, 2, 1)
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert _rel(pa.detach(), pb.detach()) < 1e-5
    finally:
        bt.close()


def test_ordinary_train_with_length_buckets_logs_the_eager_losses(tmp_path):
    """ordinary_train on the small on-disk corpus (5 items at B = 2: the last batch is partial) with one bucket that covers it: the
    later full batches replay the first one's capture, the partial batch runs eagerly, and the logged losses are the eager run's."""
    from test_host_cpu import _make_corpus
    from spoofsv_amd import harness
    cfg, spec = _make_corpus(str(tmp_path), n_items=5, with_cache=True)
    cfg.update(BATCH_SIZE=2, HIDDEN_DIM=32, TEXT_EMB_DIM=16, SSRN_DIM=32, VAL_EVERY_ITER=1000, MAX_EPOCHS=2, MAX_ITERATIONS=6)
    for step, buckets in (("train_text2mel", [[64, 32]]), ("train_ssrn", [32])):
        torch.manual_seed(0)
        _, plain = harness.ordinary_train(step, "conditional", copy.deepcopy(cfg), spec_dir=spec, current_time="a")
        torch.manual_seed(0)
        st = {}
        model, hist = harness.ordinary_train(step, "conditional", dict(copy.deepcopy(cfg), LENGTH_BUCKETS=buckets), spec_dir=spec,
                                             current_time="b", bucket_stats=st)
        assert st["captures"] == 1 and st["replays"] >= 2 and st["eager"] >= 1, st
        assert len(hist) == len(plain) == 6
        for a, b in zip(hist, plain):
            assert abs(a - b) <= 1e-5 * abs(b), (hist, plain)
