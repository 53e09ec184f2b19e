"""The spoof countermeasure without a device: the float64 restatement against the reference's own output, the numpy AMSGrad step against
torch, optimizer state interchange, the host logic (protocol lists, score lines, EER) and the argument checks of the new entry points."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import _countermeasure_ref as R
import _golden as G


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------------------------------------ references
def test_restated_lindisc_matches_the_reference_output():
    """tests/golden/countermeasure_lindisc.npz holds linDisc(24, 16).double().eval()(x) of the reference (tools/gen_countermeasure_golden.py).
    Both sides are float64 with the same operation order: 1e-10 leaves orders of magnitude over the roundoff of a few thousand sums."""
    g = G.load("countermeasure_lindisc.npz")
    sd = G.sub(g, "sd.")
    x = G.t(g["x"])
    assert x.shape == (3, 24, 37) and x.dtype == torch.float64 and sd["conv1.weight"].shape == (16, 24, 1)
    with torch.no_grad():
        pred, z, _ = R.cm_forward(x, sd, "lin")
    assert _rel(pred.numpy(), g["y"].reshape(-1)) < 1e-10
    assert float(np.ptp(g["y"])) > 1e-4                     # the fixture's items differ: the input reaches the output


def test_numpy_amsgrad_step_matches_torch_adam():
    """Torch against the restatement, no project code: six float64 steps of torch.optim.Adam(amsgrad=True, weight_decay=1e-4)."""
    rng = np.random.default_rng(3)
    for hp in (R.REF_HP, R.TORCH_DEFAULT):
        for wd, ams in ((1e-4, True), (0.0, True), (1e-4, False)):
            hp32 = [float(np.float32(v)) for v in hp]
            wd32 = float(np.float32(wd))
            p = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(257)))
            opt = torch.optim.Adam([p], lr=hp32[0], betas=(hp32[1], hp32[2]), eps=hp32[3], weight_decay=wd32, amsgrad=ams)
            mine = [p.detach().numpy().copy(), np.zeros(257), np.zeros(257), np.zeros(257)]
            for t in range(1, 7):
                g = rng.standard_normal(257) * 10.0 ** rng.integers(-4, 3, 257)
                p.grad = torch.from_numpy(g.copy())
                opt.step()
                ref = R.adam_ex_step_ref(mine[0], g, mine[1], mine[2], mine[3], *hp, wd, ams, t)
                mine = [ref.p, ref.m, ref.v, ref.vmax]
                st = opt.state[p]
                assert _rel(ref.p, p.detach().numpy()) < 1e-12
                assert _rel(ref.m, st["exp_avg"].numpy()) < 1e-12 and _rel(ref.v, st["exp_avg_sq"].numpy()) < 1e-12
                if ams:
                    assert _rel(ref.vmax, st["max_exp_avg_sq"].numpy()) < 1e-12


def test_committed_classifier_cases_stay_clear_of_the_kinks():
    for kind in ("mel", "lin"):
        sd, x, labels, masks = R.cm_case(kind)
        assert R.kink_margin(sd, kind, x, False) > R.KINK_MARGIN and R.kink_margin(sd, kind, x, masks) > R.KINK_MARGIN, kind
        want = R.cm_reference(sd, kind, x, labels, masks, torch.float64)
        assert all(float(want[2][n].norm()) > 0 for n in want[2] if not n.endswith(("conv1.bias", "conv2.bias", "conv3.bias", "conv4.bias", "hc.conv.bias")))


@pytest.mark.parametrize("case,first", [("lin_paths", 5), ("mel_spoof_22k", 9)])
def test_cpu_trainer_iteration_counts_of_the_end_to_end_test(case, first, tmp_path):
    """The float64 CPU trainer on the toy corpus first reaches EER 0 after 5 (linear features, wav files) and 9 (mel features, spoof class at
    22.05 kHz) iterations: tests/test_gpu_countermeasure.py runs the device trainer for twice as many."""
    import json
    from spoofsv_amd import countermeasure as C
    cfg = dict(json.load(open(os.path.join(os.path.dirname(G.GOLDEN), "..", "config.json"))), DISC_DIM=16)
    bona, spoof = R.write_toy_corpus(str(tmp_path))
    feat = "lin" if case == "lin_paths" else "mel"
    items = R.read_items(spoof) if case == "lin_paths" else [(R.toy_wave(i, 0, 22050), 22050) for i in range(len(spoof))]
    torch.manual_seed(5)
    sd0 = C.build_model(cfg, feat).state_dict()
    got = R.cpu_trainer_first_eer0(cfg, R.read_items(bona), items, sd0, feat, lambda e: C.epoch_order(24, 0, e), 8, 40, C.cm_eer)
    assert got == first


# ------------------------------------------------------------------------------------------------ optimizer interchange
def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3, 1), (7,))]


def _step(opt, params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    opt.step()


def test_fused_adam_ex_state_dict_interchanges_with_torch_adam():
    from spoofsv_amd.countermeasure import ADAM
    from spoofsv_amd.train import FusedAdamEx
    kw = dict(ADAM)
    a = _params(1)
    ta = torch.optim.Adam(a, **kw)
    _step(ta, a, 10)
    _step(ta, a, 11)
    b = _params(1)
    fused = FusedAdamEx(b, **kw)
    assert set(fused.param_groups[0]) == set(ta.param_groups[0])
    assert fused.param_groups[0]["weight_decay"] == 1e-4 and fused.param_groups[0]["amsgrad"] is True
    fused.load_state_dict(copy.deepcopy(ta.state_dict()))        # a copy, as a checkpoint file gives: torch's loader may alias same-device tensors
    assert fused._steps == 2
    assert set(fused.state[b[0]]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    sd = fused.state_dict()
    assert [float(sd["state"][i]["step"]) for i in range(2)] == [2.0, 2.0]
    c = _params(1)
    with torch.no_grad():
        for pc, pa in zip(c, a):
            pc.copy_(pa)
    tc = torch.optim.Adam(c, lr=0.5)                        # other settings: the loaded groups must replace them
    tc.load_state_dict(copy.deepcopy(sd))
    assert tc.param_groups[0]["amsgrad"] is True and tc.param_groups[0]["betas"] == (0.9, 0.98)
    _step(ta, a, 12)
    _step(tc, c, 12)
    for pa, pc in zip(a, c):
        assert torch.equal(pa, pc)
        assert torch.equal(ta.state[pa]["max_exp_avg_sq"], tc.state[pc]["max_exp_avg_sq"])


def test_fused_adam_still_refuses_weight_decay_and_amsgrad():
    from spoofsv_amd.train import FusedAdam, FusedAdamEx
    with pytest.raises(ValueError):
        FusedAdam(_params(2), weight_decay=0.1)
    with pytest.raises(ValueError):
        FusedAdam(_params(2), amsgrad=True)
    with pytest.raises(ValueError):
        FusedAdamEx(_params(2), weight_decay=-1.0)


# ------------------------------------------------------------------------------------------------ host logic
def test_protocol_items_on_a_toy_protocol(tmp_path):
    from spoofsv_amd.countermeasure import protocol_items
    root, anti = str(tmp_path / "data") + "/", str(tmp_path / "anti") + "/"
    os.makedirs(root + "data_path/ordinary")
    os.makedirs(anti + "ASVspoof2019_LA_cm_protocols")
    with open(root + "data_path/ordinary/wav.path.train", "w") as f:
        f.write("".join("/vctk/p%05d.wav \n" % i for i in range(20003)))
    lines = ["LA_0079 LA_T_1000001 - - bonafide", "LA_0079 LA_T_1000002 - A01 spoof", "LA_0080 LA_T_1000003 - A04 spoof", ""]
    with open(anti + "ASVspoof2019_LA_cm_protocols/ASVspoof2019.LA.cm.train.trn.txt", "w") as f:
        f.write("\n".join(lines))
    with open(anti + "ASVspoof2019_LA_cm_protocols/customized_data_t7.txt", "w") as f:
        f.write("s1 s001_001 - - spoof\ns1 s001_002 - - bonafide\n")
    cfg = {"DATA_ROOT_DIR": root, "ANTISPOOF_DIR": anti}
    bona, spoof = protocol_items(cfg, "train", "t7")
    assert len(bona) == 20000 and bona[0] == "/vctk/p00000.wav" and bona[-1] == "/vctk/p19999.wav"
    assert spoof == [anti + "ASVspoof2019_LA_train/flac/LA_T_1000002.flac", anti + "ASVspoof2019_LA_train/flac/LA_T_1000003.flac"]
    bona, spoof = protocol_items(cfg, "dev", "t7", ext=".wav")
    assert bona == ["/vctk/p20000.wav", "/vctk/p20001.wav", "/vctk/p20002.wav"]
    assert spoof == [anti + "t7/flac/s001_001.wav"]


def test_score_lines_byte_for_byte():
    from spoofsv_amd.countermeasure import score_line
    v = torch.tensor([0.5, 0.123456789, 1.0, 3e-12])
    assert score_line(0, 1, v[0].item()) == "LA_D_0000000 - bonafide 0.5\n"
    assert score_line(12, 0, v[1].item()) == "LA_D_0000012 - spoof 0.12345679104328156\n"
    assert score_line(1234567, 1.0, v[2].item()) == "LA_D_1234567 - bonafide 1.0\n"
    assert score_line(3, np.float32(0.0), v[3].item()) == "LA_D_0000003 - spoof " + str(v[3].item()) + "\n"


def test_cm_eer_ties_and_single_class():
    from spoofsv_amd.countermeasure import cm_eer
    assert cm_eer([0.9, 0.8, 0.1, 0.2], [1, 1, 0, 0]) == 0.0
    assert cm_eer([0.1, 0.2, 0.9, 0.8], [1, 1, 0, 0]) == 1.0
    # a score shared by the classes counts against both: FAR = FRR = 1/3 at t = 0.5
    assert cm_eer([0.9, 0.8, 0.5, 0.5, 0.2, 0.1], [1, 1, 1, 0, 0, 0]) == pytest.approx(1 / 3)
    # all tied: FAR = FRR only at t = 0.5 itself, where every trial ties with the threshold and is charged: 1 on both sides
    assert cm_eer([0.5] * 4, [1, 1, 0, 0]) == 1.0
    # one of four bona fide below one of four spoof: 1/4 on both sides between the two
    assert cm_eer([0.9, 0.8, 0.7, 0.3, 0.4, 0.2, 0.1, 0.0], [1, 1, 1, 1, 0, 0, 0, 0]) == pytest.approx(0.25)
    for labels in ([1, 1, 1], [0, 0, 0]):
        with pytest.raises(ValueError):
            cm_eer([0.1, 0.2, 0.3], labels)


# ------------------------------------------------------------------------------------------------ ABI
def test_new_symbols_are_exported():
    import spoofsv_amd.countermeasure as C
    from spoofsv_amd import _lib, ops, train
    L = _lib.lib()
    assert L.ssv_version() == 7
    for name in ("ssv_cm_head_fwd", "ssv_cm_head_bwd", "ssv_adam_ex_multi"):
        assert hasattr(L, name) and name in _lib.parse_header()
    assert ctypes.sizeof(_lib.AdamExChunk) == 48 and [f[0] for f in _lib.AdamExChunk._fields_] == ["p", "g", "m", "v", "vmax", "n"]
    assert callable(ops.cm_head) and issubclass(train.FusedAdamEx, train.FusedAdam)
    for name in ("CmLinDisc", "CmMelDisc", "CmSource", "protocol_items", "train", "score", "cm_eer", "main"):
        assert hasattr(C, name)
    m = C.CmMelDisc(80, 16)
    assert m.ln4.normalized_shape == (8,) and m.conv4.out_channels == 8 and m.pl1.kernel_size == (2,) and m.pl2.kernel_size == (2,)
    lin = C.CmLinDisc(24, 16)
    assert set(lin.state_dict()) == {k[3:] for k in G.load("countermeasure_lindisc.npz") if k.startswith("sd.")}


def test_validation_errors_without_a_device():
    from spoofsv_amd import _lib
    from spoofsv_amd.train import check_adam_ex_rows
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ssv_cm_head_fwd(p, p, p, p, 0.05, p, p, p, p, 2, 17, 3, None) == -1
    assert b"C=17" in L.ssv_last_error()
    assert L.ssv_cm_head_fwd(p, p, p, p, 0.05, p, p, p, p, 2, 4, 0, None) == -1
    assert b"T=0" in L.ssv_last_error()
    assert L.ssv_cm_head_bwd(p, p, p, p, p, p, 0.05, p, p, p, p, 2, 17, 3, None) == -1
    assert b"C=17" in L.ssv_last_error()
    assert L.ssv_cm_head_bwd(p, p, p, p, p, p, 0.05, p, p, p, p, 2, 4, 0, None) == -1
    assert b"T=0" in L.ssv_last_error()
    assert L.ssv_cm_head_fwd(p, p, p, p, 0.05, p, None, p, p, 2, 4, 3, None) == -1          # labels without amean
    assert b"amean" in L.ssv_last_error()
    assert L.ssv_adam_ex_multi(p, 0, 1e-3, 0.9, 0.98, 1e-9, 1e-4, 1, 1, None, None) == -1
    assert b"nchunks=0" in L.ssv_last_error()
    assert L.ssv_adam_ex_multi(p, 1, 1e-3, 0.9, 0.98, 1e-9, -1.0, 1, 1, None, None) == -1
    assert b"weight_decay" in L.ssv_last_error()
    rows = [(16, 32, 48, 64, 80, 5), (160, 320, 480, 640, 0, 7)]
    check_adam_ex_rows(rows, amsgrad=False)
    with pytest.raises(ValueError, match="chunk 1.*vmax"):
        check_adam_ex_rows(rows, amsgrad=True)
    with pytest.raises(ValueError):
        check_adam_ex_rows([(16, 32, 48, 64, 80, 0)], amsgrad=True)
