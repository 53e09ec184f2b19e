"""GPU tests of the wide column-incremental synthesis step (csrc/synth_wide.hip, spoofsv_amd.synth.WideSynthesizer): the layer
kernels against float64, the free run against the golden vectors, the parent's incremental path and the CPU oracle, shared texts,
item independence, and the grouped ``generate_test_utterances``.  Run with `-m gpu` on an MI355X."""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _golden import load, sub, t, rel_err
from oracle import tts_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the project's bars for a forward value against a float64 / oracle evaluation (tests/test_gpu_parity.py, TOLS)
FWD_TOLS = {"fp32": 2e-5, "f16x2": 2e-5, "bf16x3": 1e-4}
MODES = ["f16x2", "bf16x3", "fp32"]


@contextlib.contextmanager
def _mode(name):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(name)
    try:
        yield
    finally:
        spoofsv_amd.set_precision(prev)


def P(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def _planes(*weights):
    """Resident planes of fresh weights in the current arithmetic mode (None per weight in the fp32 mode, which reads the weight)."""
    from spoofsv_amd import _lib, ops, resident
    rw = resident.ResidentWeights(list(weights))
    rw.refresh(ops._stream())
    return rw, [None if _lib.precision() == 0 else resident.lookup(w) for w in weights]


def _ln64(x, g, b):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g.double().view(1, -1, 1) + b.double().view(1, -1, 1)


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("C,B", [(256, 1), (256, 37), (256, 200), (256, 1000), (64, 130)])
def test_highway_wide_stepped_over_a_sequence_vs_float64(C, B, precision):
    """ssv_column_highway_wide stepped over 70 frames, dilations 1, 3, 9, 27, against a float64 evaluation of highwayConv.forward
    (models/TTSModel.py:28-47) on the full sequence; the history holds every input column afterwards; pad columns are zero."""
    from spoofsv_amd import _lib, ops
    with _mode(precision):
        tile = _lib.lib().ssv_column_wide_tile()
        Bw, T = -(-B // tile) * tile, 70
        st = ops._stream()
        for dil in (1, 3, 9, 27):
            torch.manual_seed(3 + dil)
            x = torch.randn(B, C, T, device=DEV)
            w = torch.randn(2 * C, C, 3, device=DEV) * 0.1
            bias = torch.randn(2 * C, device=DEV)
            g1, b1, g2, b2 = (torch.randn(C, device=DEV) for _ in range(4))
            xd = x.double()
            h = torch.nn.functional.conv1d(torch.nn.functional.pad(xd, (2 * dil, 0)), w.double(), bias.double(), dilation=dil)
            sg = torch.sigmoid(_ln64(h[:, :C], g1, b1))
            want = sg * _ln64(h[:, C:], g2, b2) + (1 - sg) * xd                      # (B, C, T)
            rw, (pl,) = _planes(w)
            xw = torch.zeros(T, C, Bw, device=DEV)
            xw[:, :, :B] = x.permute(2, 1, 0)
            hist = torch.full((T, C, Bw), float("nan"), device=DEV)
            outs = torch.full((T, C, Bw), float("nan"), device=DEV)
            tdev = torch.zeros(1, dtype=torch.int32, device=DEV)
            for tt in range(T):
                tdev.fill_(tt)
                _lib.call("ssv_column_highway_wide", P(w), pl, P(bias), P(g1), P(b1), P(g2), P(b2), P(xw[tt]), P(hist), T, P(tdev), dil,
                          P(outs[tt]), B, Bw, C, 3, st)
            torch.cuda.synchronize()
            e = rel_err(outs[:, :, :B].permute(2, 1, 0), want)
            print("highway wide %s C=%d B=%d dilation=%d: %.2e" % (precision, C, B, dil, e))
            assert e < FWD_TOLS[precision], (dil, e)
            assert torch.equal(hist, xw)
            assert not outs[:, :, B:].any()
            del rw


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("Cin,Cout,B,act,with_s", [(80, 256, 37, 1, True), (256, 256, 200, 0, True), (512, 256, 130, 0, False),
                                                   (256, 256, 1000, 1, False), (256, 80, 200, 2, False), (256, 80, 37, 2, True)])
def test_pwln_wide_vs_float64(Cin, Cout, B, act, with_s, precision):
    """ssv_column_pwln_wide, act(LN(W x + bias [+ s])) with the per-item term s (Cout, Bw), against float64; pad columns zero."""
    from spoofsv_amd import _lib, ops
    with _mode(precision):
        tile = _lib.lib().ssv_column_wide_tile()
        Bw = -(-B // tile) * tile
        torch.manual_seed(Cin + Cout + B)
        x = torch.zeros(Cin, Bw, device=DEV)
        x[:, :B] = torch.randn(Cin, B, device=DEV)
        w = torch.randn(Cout, Cin, 1, device=DEV) * 0.1
        bias, g, b = (torch.randn(Cout, device=DEV) for _ in range(3))
        s = None
        if with_s:
            s = torch.zeros(Cout, Bw, device=DEV)
            s[:, :B] = torch.randn(Cout, B, device=DEV)
        rw, (pl,) = _planes(w)
        y = torch.full((Cout, Bw), float("nan"), device=DEV)
        _lib.call("ssv_column_pwln_wide", P(x), P(w), pl, P(bias), P(s), P(g), P(b), P(y), B, Bw, Cin, Cout, act, ops._stream())
        torch.cuda.synchronize()
        pre = w[:, :, 0].double() @ x[:, :B].double() + bias.double().view(-1, 1)
        if with_s:
            pre = pre + s[:, :B].double()
        n = _ln64(pre.t().unsqueeze(-1), g, b)[:, :, 0].t()
        want = torch.relu(n) if act == 1 else torch.sigmoid(n) if act == 2 else n
        e = rel_err(y[:, :B], want)
        print("pwln wide %s %d -> %d B=%d act=%d: %.2e" % (precision, Cin, Cout, B, act, e))
        assert e < FWD_TOLS[precision], e
        assert not y[:, B:].any()


def _load_module_sd(mod, sd):
    mod.load_state_dict({k: v.clone() for k, v in sd.items()})
    return mod.to(DEV)


@pytest.mark.parametrize("precision", MODES)
def test_wide_synthesis_golden_indices_exact(precision):
    """tests/golden/melsyn_eval.npz through free_run_wide: the assertions of test_incremental_synthesis_golden_indices_exact."""
    from spoofsv_amd import synth
    from spoofsv_amd.tts import melSyn
    with _mode(precision):
        g = load("melsyn_eval.npz")
        hidden, temb, B, N = [int(v) for v in g["dims"]]
        m = _load_module_sd(melSyn(34, True, 200, textemb_dim=temb, freq_bins=80, hidden_dim=hidden), sub(g, "sd/"))
        m.eval()
        frames = int(g["steps"]) + 1
        Y, A = synth.free_run_wide(m, t(g["text"], DEV), t(g["spk"], DEV), frames)
        assert torch.equal(A.argmax(1).t().cpu(), t(g["pma"]))       # bit-exact attention indices, every frame
        assert rel_err(Y, t(g["Y"])) < 1e-4
        assert rel_err(A, t(g["A"])) < 1e-4
        Y2, A2 = synth.free_run_wide(m, t(g["text"], DEV), t(g["spk"], DEV), frames)      # replay of the cached graph: same result
        assert torch.equal(Y2, Y) and torch.equal(A2, A)


def _seeded_model(condition, hidden, seed):
    from spoofsv_amd import train
    from spoofsv_amd.tts import melSyn
    torch.manual_seed(seed)
    m = melSyn(34, condition, 200 if condition else None, textemb_dim=16, freq_bins=80, hidden_dim=hidden)
    m.apply(train.init_weights)
    return m.to(DEV).eval()


@pytest.mark.parametrize("condition", [True, False])
@pytest.mark.parametrize("hidden,B,N,frames", [(32, 9, 17, 33), (32, 70, 17, 33), (256, 96, 43, 64)])
def test_wide_synthesis_matches_the_incremental_path(hidden, B, N, frames, condition):
    """free_run_wide against free_run_incremental on the same seeded model: the rule of test_incremental_synthesis_matches_prefix_loop
    (frames before the first top-2 margin <= 1e-4 must agree in arg-max; values within 2e-4 up to there)."""
    from spoofsv_amd import synth
    m = _seeded_model(condition, hidden, 40 + B)
    text = torch.randint(2, 33, (B, 1, N), device=DEV)
    text[:, :, -1] = 1
    spk = (0.04 + 0.05 * torch.rand(B, 200, 1, device=DEV)) if condition else None
    with torch.no_grad():
        Y0, A0 = synth.free_run_incremental(m, text, spk, frames)
        Y1, A1 = synth.free_run_wide(m, text, spk, frames)
    _agree_up_to_the_first_near_tie(Y0, A0, Y1, A1, frames, "wide vs incremental hidden=%d B=%d cond=%s" % (hidden, B, condition))


def _agree_up_to_the_first_near_tie(Y0, A0, Y1, A1, frames, what):
    """Frames before the first top-2 margin <= 1e-4 of (Y0, A0) must agree in arg-max; values within 2e-4 up to there."""
    assert Y1.shape == Y0.shape and A1.shape == A0.shape
    top = A0.topk(2, dim=1).values
    near_tie = ((top[:, 0] - top[:, 1]) <= 1e-4).any(0)
    cut = int(near_tie.nonzero()[0]) if near_tie.any() else frames
    assert cut >= 1
    assert torch.equal(A0.argmax(1)[:, :cut], A1.argmax(1)[:, :cut])
    ey, ea = rel_err(Y1[:, :, :cut + 1], Y0[:, :, :cut + 1]), rel_err(A1[:, :, :cut + 1], A0[:, :, :cut + 1])
    print("%s: cut %d of %d, Y %.2e A %.2e" % (what, cut, frames, ey, ea))
    assert ey < 2e-4 and ea < 2e-4
    if cut == frames:
        assert rel_err(Y1, Y0) < 2e-4 and rel_err(A1, A0) < 2e-4


def test_a_mode_change_recaptures_on_the_cached_synthesizer(monkeypatch):
    """fp32, split-fp16, fp32 again on ONE model object: the three free runs are served by the same cached WideSynthesizer, which
    drops its graph at each mode change (the captured step holds the mode's kernels and plane addresses) and captures again with the
    frame counter at ``frames``, where the run before left it -- the warm-up step of a capture runs at the current frame index, so
    without a reset before it that step would write one frame past Yw and the histories.  The third result is the first bit for bit;
    the second agrees with the first by the rule of test_wide_synthesis_matches_the_incremental_path."""
    from spoofsv_amd import synth
    B, N, frames = 9, 17, 33
    m = _seeded_model(True, 32, 91)
    text = torch.randint(2, 33, (B, 1, N), device=DEV)
    text[:, :, -1] = 1
    spk = 0.04 + 0.05 * torch.rand(B, 200, 1, device=DEV)
    run, seen = synth.WideSynthesizer.run, []

    def spy(self, *args, **kw):
        before = (self.graph, int(self.t))
        out = run(self, *args, **kw)
        seen.append((self,) + before + (self.graph, int(self.t)))
        return out

    monkeypatch.setattr(synth.WideSynthesizer, "run", spy)
    out = []
    for precision in ("fp32", "f16x2", "fp32"):
        with _mode(precision), torch.no_grad():
            out.append(synth.free_run_wide(m, text, spk, frames))
    assert len(seen) == 3 and seen[0][0] is seen[1][0] is seen[2][0]
    assert seen[0][1] is None and seen[0][2] == 0                            # a fresh synthesizer
    for k in (1, 2):
        g_before, t_before, g_after, t_after = seen[k][1:]
        assert g_before is seen[k - 1][3] and g_before is not None            # it came with the graph of the run before ...
        assert t_before == frames == t_after                                  # ... and that run's frame counter,
        assert g_after is not None and g_after is not g_before                # dropped the graph and captured a new one
    (Y0, A0), (Y1, A1), (Y2, A2) = out
    assert torch.equal(Y2, Y0) and torch.equal(A2, A0)
    _agree_up_to_the_first_near_tie(Y0, A0, Y1, A1, frames, "wide f16x2 vs fp32 after a re-capture")


@pytest.mark.parametrize("precision", MODES)
def test_shared_texts_equal_the_expanded_batch(precision):
    """shared_texts = U with S speakers gives the (Y, A) of the expanded (S * U, 1, N) batch: bit-identical in the fp32 mode, within
    2e-4 in the split modes -- an item's operand scale (split-fp16) is that of its 32-column tile, so its values depend on its
    neighbours to rounding, and equality there is to rounding only.  U * N = 136 >= 128 on purpose: the text encoder's convolutions
    take the exact-fp32 kernels below 128 columns in all (csrc/ssv_host.h, use_bf3), so with fewer characters the U shared texts and the
    S * U expanded ones would be ENCODED in two different arithmetics, which is not what this test is about."""
    from spoofsv_amd import synth
    with _mode(precision):
        S, U, N, frames = 5, 8, 17, 33
        m = _seeded_model(True, 32, 77)
        text = torch.randint(2, 33, (U, 1, N), device=DEV)
        text[:, :, -1] = 1
        spk = (0.04 + 0.05 * torch.rand(S, 200, 1, device=DEV)).repeat_interleave(U, dim=0)       # item b: speaker b // U, text b % U
        with torch.no_grad():
            Ys, As = synth.free_run_wide(m, text, spk, frames, shared_texts=U)
            Ye, Ae = synth.free_run_wide(m, text.repeat(S, 1, 1), spk, frames)
        assert tuple(Ys.shape) == (S * U, 80, frames) and tuple(As.shape) == (S * U, N, frames)
        if precision == "fp32":
            assert torch.equal(Ys, Ye) and torch.equal(As, Ae)
        else:
            assert rel_err(Ys, Ye) < 2e-4 and rel_err(As, Ae) < 2e-4


def test_permuting_the_items_permutes_the_outputs_bit_exactly():
    """No cross-item leak (fp32 mode): an item's values do not depend on its column or its neighbours."""
    from spoofsv_amd import synth
    with _mode("fp32"):
        B, N, frames = 45, 17, 33
        m = _seeded_model(True, 32, 78)
        text = torch.randint(2, 33, (B, 1, N), device=DEV)
        text[:, :, -1] = 1
        spk = 0.04 + 0.05 * torch.rand(B, 200, 1, device=DEV)
        perm = torch.randperm(B, device=DEV)
        with torch.no_grad():
            Y0, A0 = synth.free_run_wide(m, text, spk, frames)
            Y1, A1 = synth.free_run_wide(m, text[perm].contiguous(), spk[perm].contiguous(), frames)
        assert torch.equal(Y1, Y0[perm]) and torch.equal(A1, A0[perm])


_ORACLE6 = {}
SENTENCES = ("The birch canoe slid on the smooth planks.", "Glue the sheet to the dark blue background.")
CODES = (0.04, 0.05, 0.06)


def _oracle6():
    """The seeded full-size melSyn of config 2 on the CPU oracle: two Harvard sentences (zero-padded to 44 characters) x three speaker
    codes, item b = speaker b // 2, sentence b % 2, 1 + 325 steps.  Once per session (~30 s on 16 threads)."""
    if _ORACLE6:
        return _ORACLE6
    from spoofsv_amd import harness, train
    from spoofsv_amd.tts import melSyn
    vocab = "PE abcdefghijklmnopqrstuvwxyz-,.?'" + '"'
    ids = [harness.text2id(s, vocab) for s in SENTENCES]
    width = max(len(i) for i in ids)
    assert width == 44
    text = torch.tensor([list(i) + [0] * (width - len(i)) for i in ids], dtype=torch.long).view(2, 1, width)
    spk = torch.cat([torch.full((2, 200, 1), c) for c in CODES], dim=0)
    torch.manual_seed(1234)
    m1 = melSyn(34, True, 200, 128, 80, 256)
    m1.apply(train.init_weights)
    sd1 = {k: v.clone() for k, v in m1.state_dict().items()}
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    with torch.no_grad():
        Yo, Ao, pma_o = TO.synthesize_loop(text.repeat(3, 1, 1), spk, sd1, 325)
    top = torch.topk(Ao, 2, dim=1).values
    _ORACLE6.update(text=text, spk=spk, m1=m1, Yo=Yo, Ao=Ao, pma_o=pma_o, margins=top[:, 0] - top[:, 1])       # margins (B, frames)
    return _ORACLE6


@pytest.mark.parametrize("precision", MODES)
def test_full_size_shared_texts_vs_cpu_oracle(precision):
    """One wide run with shared_texts = 2 (three speaker codes x two sentences, full-size seeded model, all 326 frames) against
    oracle.tts_oracle.synthesize_loop on the expanded batch.  Per item the rule of _config2_check (tests/test_gpu_parity.py):
    attention indices exact up to the first frame whose oracle top-2 margin is <= 1e-3, mel within 1e-3 relative max-norm on the frames
    before it -- and, so that the check cannot pass vacuously, EVERY item must be decisive (margin > 1e-3) on every frame, i.e. the
    comparable prefix is the whole run.  The margins are printed and asserted."""
    from spoofsv_amd import synth
    c = _oracle6()
    frames = 326
    margins = c["margins"]
    print("oracle top-2 margins per item (min over %d frames): %s" % (frames, ["%.2e" % float(v) for v in margins.min(1).values]))
    assert tuple(margins.shape) == (6, frames)
    assert float(margins.min()) > 1e-3, "the oracle is indecisive on a compared frame: the inputs of this test no longer serve"
    with _mode(precision):
        m1 = c["m1"].to(DEV).eval()
        with torch.no_grad():
            Y, A = synth.free_run_wide(m1, c["text"].to(DEV), c["spk"].to(DEV), frames, shared_texts=2)
        m1.cpu()
    assert tuple(Y.shape) == (6, 80, frames)
    pma = A.argmax(1).t().cpu()                                      # (frames, B)
    for b in range(6):
        assert torch.equal(pma[:, b], c["pma_o"][:, b]), (b, int((pma[:, b] != c["pma_o"][:, b]).nonzero()[0]))
        e = rel_err(Y[b], c["Yo"][b])
        print("item %d (%s): mel %.2e over %d frames" % (b, precision, e, frames))
        assert e < 1e-3, (b, e)


def test_generate_test_utterances_in_speaker_groups(tmp_path):
    """generate_test_utterances with speakers_per_batch = 4 (a full group and a remainder of one) against speakers_per_batch = 1
    (today's loop), fp32 mode: the same file names in the same per-speaker order; per file, lengths within one hop of trim_silence
    and, over the common length, waveforms within 2e-2 of the peak (the bar tests/test_gpu_vocoder.py gives two Griffin-Lim runs that
    differ only in rounding).

    Without trained checkpoints generate_test_utterances builds its models BEFORE it seeds the generator (only the parameters that
    train.init_weights touches are seeded; the rest keep their constructor's draw), so two calls see the same models only if they start
    from the same generator state: each call below is preceded by the same torch.manual_seed.  (Measured without that: the per-speaker
    loop against ITSELF differs by 0.7 in the mel spectrogram and 0.82-1.23 of the peak in the waveform.)"""
    from scipy.io import wavfile
    from spoofsv_amd import harness
    cfg = json.load(open(os.path.join(ROOT, "config.json")))
    cfg.update(SRC_ROOT_DIR=str(tmp_path) + os.sep, MAX_TEXT_LEN=24, MAX_FRAME_NUM=40, HIDDEN_DIM=32, TEXT_EMB_DIM=16, SSRN_DIM=32,
               TTS_TEXTS=os.path.join(ROOT, "tts_texts.txt"), GRIFFIN_LIM_ITERS=8, SYNTH_INCREMENTAL=True)
    cfg["STFT"] = {"FFT_LENGTH": 128, "HOP_LENGTH": 32}
    rng = np.random.RandomState(5)
    spk = {"p%d" % (225 + i): (0.04 + 0.05 * rng.rand(200)).astype(np.float32) for i in range(5)}
    texts = ["The birch canoe slid.", "Glue the sheet.", "It's easy to tell the depth of a well."]
    with _mode("fp32"):
        torch.manual_seed(2024)
        one = harness.generate_test_utterances(cfg, "one", eval_utt_num=3, speakers=spk, texts=texts, max_frames=24, speakers_per_batch=1)
        torch.manual_seed(2024)
        four = harness.generate_test_utterances(cfg, "four", eval_utt_num=3, speakers=spk, texts=texts, max_frames=24, speakers_per_batch=4)
    assert list(one) == list(four) == list(spk)
    for name in spk:
        assert [os.path.basename(p) for p in one[name]] == [os.path.basename(p) for p in four[name]] == \
            ["s%s_%03d.wav" % (name[1:], k + 1) for k in range(3)]
        for pa, pb in zip(one[name], four[name]):
            assert os.sep + "four" + os.sep in pb
            (ra, ya), (rb, yb) = wavfile.read(pa), wavfile.read(pb)
            assert ra == rb == cfg["SAMPLING_RATE"]
            assert abs(len(ya) - len(yb)) <= 512, (pa, len(ya), len(yb))
            n = min(len(ya), len(yb))
            assert n > 0
            peak = float(np.abs(ya).max())
            d = float(np.abs(ya[:n] - yb[:n]).max())
            print("%s: %d / %d samples, difference %.2e of the peak" % (os.path.basename(pa), len(ya), len(yb), d / peak))
            assert d <= 2e-2 * peak, (pa, d, peak)
