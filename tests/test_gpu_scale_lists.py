"""The split-fp16 operand scale lists (include/ssv_hip.h, "Operand scales"), kernel by kernel.

Part A -- producers.  Every kernel that leaves a list as a by-product is called through the C ABI in all three arithmetic modes with
the list buffer POISONED (+3e38, negative values, NaN -- nothing a correct run can leave behind), and then
  1. every entry of every item is finite and >= 0 (written or zeroed: no poison survives),
  2. the list's maximum per item EQUALS, bit for bit, max |out(b)| of the tensor the kernel itself wrote (strided outputs: the gap
     between items is filled with 1e30 and must stay untouched),
  3. items are kept apart (item b's output is about 2^(3 b) times item 0's, or at least differs bitwise in its maximum),
  4. two different poisons give bitwise equal lists.
Each case runs with the item's peak placed in the LAST channel and LAST column (ragged tiles, 4-column tails) and with the peak
wherever the random data puts it.  Which kernel form a shape reaches is asserted from the partial-row counts
(ssv_ln_bwd_partial_rows) and, for the forward kernels and the one-launch link backward, from the shape log of a child process.

Part B -- consumers.  The same operands in mode 2 with the list NULL, the 8 pieces of ssv_absmax, one entry per item, lists of 24 /
84 / 256 / 1000 entries whose maximum sits at exactly one position, and the list a real producer wrote: all outputs bitwise equal
(the scale is a function of the maximum's exponent only), per item within the committed 2e-6 bar of float64, binade edges included.

What the header says and what is pinned here:
  * a NaN element is dropped by fmaxf: the list reports the maximum over the item's other elements;
  * ssv_deconv1d_k2s2_fwd writes y_amax in mode 2 only (modes 0 / 1 leave the buffer untouched); with more than y_namax tiles per
    item it runs the product without the list and then ssv_absmax over y -- it works at every length;
  * under a `live` length mask the list is the UNMASKED output's (taken before the mask): >= the masked output's maximum.

Wall time of this file on one MI355X, measured: 14 s in pytest (17 s with interpreter start), the child process of the shape log included."""
import contextlib
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MODES = (0, 1, 2)
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 186, 325, 1300)
POISON = ((3e38, -1.0, NAN), (NAN, -3e38, 7e37, -2.0))
GAP = 8            # floats between the items of a strided output


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L():
    from spoofsv_amd import _lib
    return _lib


@contextlib.contextmanager
def _mode(m):
    lib = _L().lib()
    prev = lib.ssv_set_precision(m)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        lib.ssv_set_precision(prev)


def _poison(B, n, which):
    pat = torch.tensor(POISON[which])
    return pat.repeat(B * n // len(pat) + 1)[:B * n].reshape(B, n).to(DEV).contiguous()


def _spread(B):
    return torch.exp2(3.0 * (torch.arange(B) % 8).float())


def _cdiv(a, b):
    return (a + b - 1) // b


def _na(L):
    return int(_L().lib().ssv_amax_rows(L))


def _out(B, n, strided):
    """(buffer, live view (B, n), batch stride): dense, or items GAP floats apart with 1e30 between them."""
    if not strided:
        buf = torch.full((B, n), NAN, device=DEV)
        return buf, buf, n
    buf = torch.full((B, n + GAP), 1e30, device=DEV)
    return buf, buf[:, :n], n + GAP


def _check(am, live, tag, buf=None, inf_ok=False):
    ok = (am >= 0) & (torch.isfinite(am) | (am == float("inf"))) if inf_ok else (am >= 0) & torch.isfinite(am)
    assert bool(ok.all()), ("an entry was neither written nor zeroed", tag, am[~ok][:8].tolist())
    got, want = am.max(dim=1).values, live.abs().amax(dim=1)
    assert torch.equal(got, want), ("list maximum != max |out| per item", tag, got.tolist()[:8], want.tolist()[:8])
    if buf is not None and buf.shape[1] > live.shape[1]:
        assert bool((buf[:, live.shape[1]:] == 1e30).all()), ("a write between the items", tag)


def _produce(run, B, na, tag, modes=MODES, inf_ok=False, written=lambda mode: True):
    """run(am) launches the producer with list buffer `am` (B, na) and returns (live output (B, n), its buffer or None)."""
    lists = {}
    for mode in modes:
        with _mode(mode):
            got = []
            for which in (0, 1):
                am = _poison(B, na, which)
                live, buf = run(am)
                torch.cuda.synchronize()
                if written(mode):
                    _check(am, live, (tag, "mode", mode, "poison", which), buf, inf_ok)
                else:
                    assert torch.equal(am.nan_to_num(5.0), _poison(B, na, which).nan_to_num(5.0)), (tag, mode, "list touched")
                got.append(am)
            assert torch.equal(got[0].nan_to_num(5.0), got[1].nan_to_num(5.0)) or not written(mode), (tag, mode, "the list depends on what the buffer held")
            lists[mode] = got[0]
    return lists


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _peaked(t, peak, amp=40.0):
    """Items 2^(3 b) apart; peak: the item's maximum in the last channel, last column."""
    B = t.shape[0]
    t = t * _spread(B)[:, None, None]
    if peak:
        t[:, -1, -1] = amp * _spread(B)
    return t


def _ln_params(C, gen, scale=1.0):
    return (torch.rand(C, generator=gen) + 0.5) * scale, torch.randn(C, generator=gen) * 0.3 * scale


def _batch(L, least=3):
    """Enough items for the split-MFMA kernels (B * L >= 128) at every length."""
    return max(least, _cdiv(128, L))


# ---------------------------------------------------------------------------------------------------------------- part A: producers
@pytest.mark.parametrize("namax", [1, 8, 64, 100])
def test_absmax_lists_for_every_piece_count_and_item_size(namax):
    """ssv_absmax: pieces that do not divide the item, fewer elements than pieces (the empty pieces are zeroed), one element, items a
    stride apart (4-byte aligned only), an all-zero item (0), one inf (inf), one NaN (dropped: the maximum of the others)."""
    lib = _L()
    B = 5
    for n in (1, 7, 37, 99, 4099, 80 * 325 + 3):
        gen = _gen(namax, n)
        for bs in (n, n + 5):
            big = torch.full((B, bs), 1e30)
            big[:, :n] = torch.randn(B, n, generator=gen) * _spread(B)[:, None]
            big[1, :n] = 0.0
            big[2, n // 2] = float("inf")
            xd = big.to(DEV)
            run = lambda am: (lib.call("ssv_absmax", P(xd), bs, B, n, P(am), namax, ST()), (xd[:, :n], None))[1]
            lists = _produce(run, B, namax, ("absmax", namax, n, bs), inf_ok=True)
            assert float(lists[2][1].max()) == 0.0 and float(lists[2][2].max()) == float("inf")
            if n > 1:
                big[3, n - 1] = NAN
                xd = big.to(DEV)
                am = _poison(B, namax, 0)
                lib.call("ssv_absmax", P(xd), bs, B, n, P(am), namax, ST())
                torch.cuda.synchronize()
                assert torch.equal(am[3].max(), xd[3, :n - 1].abs().max()), "a NaN element is dropped: the maximum of the others"


def _ln_act_fwd(B, C, L, act, peak, strided):
    lib = _L()
    gen = _gen(1, B, C, L, act, peak)
    x = torch.randn(B, C, L, generator=gen)
    if peak:
        x[:, -1, -1] = 60.0
    gam, bet = _ln_params(C, gen, 4.0)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    stats = torch.empty(B, 2, L, device=DEV)

    def run(am):
        buf, live, bs = _out(B, C * L, strided)
        lib.call("ssv_channel_ln_act_fwd", P(xd), C * L, P(gd), P(bd), P(buf), bs, P(am), P(stats), B, C, L, act, None, 0, ST())
        return live, buf
    return run


@pytest.mark.parametrize("C", [80, 256, 512, 513])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_channel_layernorm_forward_list(C, act):
    """ln_act_fwd_kernel on 16 and 32 channel groups and with 33 channels per thread: one entry per 16-column tile, the last tile
    zeroes the entries past the tiles."""
    for L in LENGTHS + (4100,):
        B = 2 if L > 4000 else 3
        for peak in (True, False):
            _produce(_ln_act_fwd(B, C, L, act, peak, strided=peak), B, _na(L), ("ln_act_fwd", B, C, L, act, peak))


def test_channel_layernorm_forward_list_of_an_all_zero_item():
    lib = _L()
    B, C, L = 3, 256, 65
    x = torch.randn(B, C, L)
    x[1] = 0.0
    xd, gd, bd = x.to(DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)

    def run(am):
        buf, live, bs = _out(B, C * L, False)
        lib.call("ssv_channel_ln_act_fwd", P(xd), C * L, P(gd), P(bd), P(buf), bs, P(am), None, B, C, L, 0, None, 0, ST())
        return live, buf
    lists = _produce(run, B, _na(L), "ln_act_fwd zero item")
    assert float(lists[2][1].max()) == 0.0


def _gate_fwd(B, C, L, peak, strided, special=None):
    lib = _L()
    gen = _gen(2, B, C, L, peak)
    h = torch.randn(B, 2 * C, L, generator=gen)
    x = _peaked(torch.randn(B, C, L, generator=gen), peak)
    if special is not None:
        x[1, C // 2, L // 2] = special
    ps = [p.to(DEV) for p in (*_ln_params(C, gen), *_ln_params(C, gen))]
    hd, xd = h.to(DEV), x.to(DEV)
    stats = torch.empty(B, 4, L, device=DEV)

    def run(am):
        buf, live, bs = _out(B, C * L, strided)
        lib.call("ssv_highway_gate_fwd", P(hd), P(xd), C * L, *[P(p) for p in ps], P(stats), P(buf), bs, P(am), B, C, L, ST())
        return live, buf
    return run


@pytest.mark.parametrize("C", [64, 256, 512])
def test_highway_gate_forward_list(C):
    """ln_gate_fwd_kernel (the critics' gate, and the generator's below the split-MFMA line): items 2^(3 b) apart through the residual."""
    for L in LENGTHS + (4100,):
        B = 2 if L > 4000 else 4
        for peak in (True, False):
            _produce(_gate_fwd(B, C, L, peak, strided=peak), B, _na(L), ("gate_fwd", B, C, L, peak))


def test_highway_gate_forward_list_with_an_inf_and_with_a_nan_element():
    """One inf in the residual: the list says inf.  One NaN: fmaxf drops it -- the list is the maximum over the item's other elements."""
    B, C, L = 3, 256, 65
    _produce(_gate_fwd(B, C, L, False, False, special=float("inf")), B, _na(L), "gate_fwd inf", inf_ok=True)
    run = _gate_fwd(B, C, L, False, False, special=NAN)
    am = _poison(B, _na(L), 0)
    live, _ = run(am)
    torch.cuda.synchronize()
    assert int(torch.isnan(live[1]).sum()) == 1 and bool(torch.isfinite(am).all()) and bool((am >= 0).all())
    assert torch.equal(am.max(dim=1).values, live.abs().nan_to_num(0.0).amax(dim=1))


def _highway_fwd(B, C, L, k, dilation, causal, peak, strided, keep=None):
    lib = _L()
    gen = _gen(3, B, C, L, k, dilation, peak)
    x = _peaked(torch.randn(B, C, L, generator=gen), peak)
    w = torch.randn(2 * C, C, k, generator=gen) / (C * k) ** 0.5
    bias = torch.randn(2 * C, generator=gen) * 0.1
    ps = [p.to(DEV) for p in (*_ln_params(C, gen), *_ln_params(C, gen))]
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    h, stats = torch.empty(B, 2 * C, L, device=DEV), torch.empty(B, 4, L, device=DEV)
    nb = lib.query("ssv_highway_conv1d_fwd_workspace", B, C, L, k)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    if keep is not None:
        keep.update(x=xd, w=wd, bias=bd, ps=ps, h=h, stats=stats, cpu=(x, w, bias))

    def run(am, x_amax=None, x_namax=0):
        buf, live, bs = _out(B, C * L, strided)
        lib.call("ssv_highway_conv1d_fwd", P(xd), C * L, P(x_amax), x_namax, P(wd), None, P(bd), *[P(p) for p in ps], P(h), P(stats), P(buf), bs,
                 P(am), B, C, L, k, dilation, int(causal), P(ws), nb, ST())
        return live, buf
    return run


@pytest.mark.parametrize("C", [80, 256, 512])
def test_highway_convolution_forward_list(C):
    """ssv_highway_conv1d_fwd: the streaming kernel (split modes, C % 64 == 0: entry 4 * tile + channel quarter, ragged last tile and
    4-column tails) and the reducing kernel (mode 0, C = 80, B * L < 128)."""
    for L in LENGTHS + (4100,):
        for B in ((2,) if L > 4000 else (_batch(L), 2)):
            for peak in (True, False):
                _produce(_highway_fwd(B, C, L, 3, 1 if L < 100 else 3, L % 2 == 0, peak, strided=peak), B, _na(L), ("highway_fwd", B, C, L, peak))


def _pw_fwd(B, Cin, Cout, L, act, peak, strided, keep=None):
    lib = _L()
    gen = _gen(4, B, Cin, Cout, L, act, peak)
    x = _peaked(torch.randn(B, Cin, L, generator=gen), peak)
    w = torch.randn(Cout, Cin, 1, generator=gen) / Cin ** 0.5
    bias = torch.randn(Cout, generator=gen) * 0.1
    gam, bet = _ln_params(Cout, gen, 3.0)
    xd, wd, bd, gd, btd = [t.to(DEV) for t in (x, w, bias, gam, bet)]
    pre, stats = torch.empty(B, Cout, L, device=DEV), torch.empty(B, 2, L, device=DEV)
    nb = lib.query("ssv_pointwise_conv_ln_act_fwd_workspace", Cin, Cout)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    if keep is not None:
        keep.update(x=xd, w=wd, bias=bd, gamma=gd, beta=btd, pre=pre, stats=stats)

    def run(am, x_amax=None, x_namax=0):
        buf, live, bs = _out(B, Cout * L, strided)
        lib.call("ssv_pointwise_conv_ln_act_fwd", P(xd), Cin * L, P(x_amax), x_namax, P(wd), None, P(bd), None, P(gd), P(btd), P(pre), P(stats),
                 P(buf), bs, P(am), B, Cin, Cout, L, act, P(ws), nb, ST())
        return live, buf
    return run


@pytest.mark.parametrize("Cin,Cout", [(128, 256), (256, 513), (64, 80)])
def test_link_forward_list(Cin, Cout):
    """ssv_pointwise_conv_ln_act_fwd: gemm_pwln_kernel (dense y, split modes: one entry per 64-column tile, 256 and 513 LayerNorm rows)
    and the product followed by ln_act_fwd_kernel (a strided y, mode 0, B * L < 128)."""
    for L in LENGTHS + (4100,):
        for B in ((2,) if L > 4000 else (_batch(L), 2)):
            for strided in (False, True):
                _produce(_pw_fwd(B, Cin, Cout, L, (L + B) % 3, not strided, strided), B, _na(L), ("pw_fwd", B, Cin, Cout, L, strided))


def _deconv_fwd(B, Cin, Cout, L, peak, strided, keep=None):
    lib = _L()
    gen = _gen(5, B, Cin, Cout, L, peak)
    x = _peaked(torch.randn(B, Cin, L, generator=gen), peak)
    w = torch.randn(Cin, Cout, 2, generator=gen) / Cin ** 0.5
    bias = torch.randn(Cout, generator=gen) * 0.1
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    nb = lib.query("ssv_deconv1d_k2s2_fwd_workspace", Cin, Cout)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    if keep is not None:
        keep.update(x=xd, w=wd, bias=bd, cpu=(x, w, bias))

    def run(am, x_amax=None, x_namax=0, namax=64):
        buf, live, bs = _out(B, Cout * 2 * L, strided)
        lib.call("ssv_deconv1d_k2s2_fwd", P(xd), Cin * L, P(x_amax), x_namax, P(wd), None, P(bd), P(buf), bs, P(am), namax if am is not None else 0,
                 B, Cin, Cout, L, P(ws), nb, ST())
        return live, buf
    return run


DECONV_LENGTHS = LENGTHS + (650, 1301, 1792, 1793, 2048, 2600, 4096)


@pytest.mark.parametrize("Cin,Cout", [(256, 256), (64, 80)])
def test_deconvolution_forward_list(Cin, Cout):
    """ssv_deconv1d_k2s2_fwd, 64 entries: the row-pair epilogue (one entry per tile, the last tile zeroes the rest) up to 64 tiles per item;
    beyond that -- sequences longer than the timed 1300 frames -- the entry runs the product without the list and then ssv_absmax over y:
    it WORKS at every length, and y is bitwise what the call without a list gives.  The list is written in mode 2 only (pinned).
    The tile picker (pick_nnb) weighs the batch: at B = 32 and 512 rows it takes 128 x 112 tiles, 4 * ceil(L / 112) per item -- 48 at the
    timed L = 1300, 64 at L = 1792 (the largest count the list holds), 68 at L = 1793; at B = 2 it takes small tiles and long items
    already exceed the list (test_deconvolution_cases_lie_on_both_sides_of_the_64_tile_limit reads the counts from the shape log)."""
    for L in DECONV_LENGTHS:
        for B in ((1, 2) if L > 1301 else (_batch(L), 2)) + ((32,) if L in (325, 1300, 1792, 1793) else ()):
            for peak in (True, False):
                run = _deconv_fwd(B, Cin, Cout, L, peak, strided=peak)
                _produce(run, B, 64, ("deconv_fwd", B, Cin, Cout, L, peak), written=lambda mode: mode == 2)
        with _mode(2):
            run = _deconv_fwd(2, Cin, Cout, L, True, False)
            y0 = run(None)[0].clone()
            y1 = run(_poison(2, 64, 0))[0]
            torch.cuda.synchronize()
            assert torch.equal(y0, y1), ("deconv: y differs with and without the list", L)


def _gate_ref(h, x, g1, b1, g2, b2):
    C = x.shape[1]
    ln = lambda t, g, b: F.layer_norm(t.permute(0, 2, 1), (C,), g, b, 1e-5).permute(0, 2, 1)
    s = torch.sigmoid(ln(h[:, :C], g1, b1))
    return s * ln(h[:, C:], g2, b2) + (1 - s) * x


def _rl2(a, b):
    return float((a.detach().double().cpu() - b).norm() / b.norm())


def _expected_gate_bwd_rows(B, C, L):
    """The form the issue names for each shape, as a tile count: persistent (C = 256, B <= 256: one row per workgroup), wide tiles
    (C = 512 from L = 64 on: 32 columns; C = 128 from L = 1024 on: 64 columns), else 16 columns."""
    if C == 256 and B <= 256:
        return "pers", B * min(256 // B, _cdiv(L, 16))
    if C == 512 and L >= 64:
        return "wide", B * _cdiv(L, 32)
    if C == 128 and L >= 1024:
        return "wide", B * _cdiv(L, 64)
    return "tile16", B * _cdiv(L, 16)


def _highway_bwd(B, C, L, k, dilation, causal, peak, with_ref=False):
    """Forward through the C ABI (h, stats), then ssv_highway_conv1d_bwd_data with and without the list."""
    lib = _L()
    keep = {}
    fwd = _highway_fwd(B, C, L, k, dilation, causal, False, False, keep)
    fwd(None)
    gen = _gen(6, B, C, L, peak)
    dy = _peaked(torch.randn(B, C, L, generator=gen), peak)
    dyd = dy.to(DEV)
    nb = lib.query("ssv_highway_conv1d_bwd_data_workspace", B, C, L, k)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    nblk = lib.query("ssv_ln_partial_rows", B, L)
    out = {}

    def run(am):
        dx, dh = torch.full((B, C, L), NAN, device=DEV), torch.full((B, 2 * C, L), NAN, device=DEV)
        part = torch.full((nblk, 6 * C), NAN, device=DEV)
        lib.call("ssv_highway_conv1d_bwd_data", P(dyd), C * L, P(keep["x"]), C * L, P(keep["w"]), None, *[P(p) for p in keep["ps"]], P(keep["h"]),
                 P(keep["stats"]), P(dx), C * L, P(dh), P(am), P(part), B, C, L, k, dilation, int(causal), P(ws), nb, ST())
        out["dx"], out["part"] = dx, part
        return dh.reshape(B, -1), None
    ref = None
    if with_ref:
        x, w, bias = keep["cpu"]
        ins = [t.double().requires_grad_(True) for t in (x, w, bias, *[p.cpu() for p in keep["ps"]])]
        pad = dilation * (k - 1)
        xin = F.pad(ins[0], (pad, 0)) if causal else F.pad(ins[0], (pad // 2, pad // 2))
        _gate_ref(F.conv1d(xin, ins[1], ins[2], dilation=dilation), ins[0], *ins[3:]).backward(dy.double())
        ref = {"dx": ins[0].grad, "pg": torch.cat([ins[3].grad, ins[4].grad, ins[5].grad, ins[6].grad, ins[2].grad])}
    return run, out, ref


GATE_BWD_SHAPES = [(1, 256), (32, 256), (5, 256), (3, 512), (3, 128), (3, 80)]


@pytest.mark.parametrize("B,C", GATE_BWD_SHAPES)
def test_highway_backward_list_of_dh(B, C):
    """ssv_highway_conv1d_bwd_data (dh_amax): the persistent kernel (C = 256: B = 1 -- as many workgroups as 16-column tiles, up to the
    256 entries of L = 4096 --, B = 32, and B = 5 where 51 workgroups share 82 tiles), the wide kernels (C = 512, L >= 64; C = 128,
    L >= 1024: entry VEC * tile, the entries between zeroed), the 16-column kernel (C = 512, L < 64; C = 80)."""
    lib = _L().lib()
    for L in LENGTHS + (4096,):
        if B == 32 and L not in (17, 65, 325):
            continue
        form, rows = _expected_gate_bwd_rows(B, C, L)
        assert lib.ssv_ln_bwd_partial_rows(1, B, C, L, 1) == rows, ("the intended kernel form is not the one the dispatch takes", form, B, C, L)
        for peak in (True, False):
            run, _, _ = _highway_bwd(B, C, L, 3, 1, False, peak)
            _produce(run, B, _na(L), ("highway_bwd", form, B, C, L, peak))


@pytest.mark.parametrize("B,C,L", [(1, 256, 325), (32, 256, 65), (5, 256, 1300), (3, 512, 186), (3, 512, 63), (3, 128, 1300), (3, 80, 325)])
def test_highway_backward_gradients_with_and_without_the_list_vs_float64(B, C, L):
    """The partial-row count changes with the list (ssv_ln_bwd_partial_rows(.., with_amax)): dx and the summed parameter gradients of
    both calls against float64 autograd of the reference's expression, at the bar of test_gpu_accuracy (3e-6)."""
    lib = _L().lib()
    for mode in (0, 2):
        with _mode(mode):
            run, out, ref = _highway_bwd(B, C, L, 3, 3, True, False, with_ref=True)
            for with_list in (1, 0):
                run(_poison(B, _na(L), 0) if with_list else None)
                torch.cuda.synchronize()
                rows = lib.ssv_ln_bwd_partial_rows(1, B, C, L, with_list)
                pg = out["part"][:rows].double().sum(0).cpu()
                assert bool(torch.isfinite(pg).all()), "a partial row nobody wrote"
                assert _rl2(out["dx"], ref["dx"]) < 3e-6, (mode, with_list, _rl2(out["dx"], ref["dx"]))
                for i in range(5):
                    a, b = pg[i * C:(i + 1) * C] if i < 4 else pg[4 * C:], ref["pg"][i * C:(i + 1) * C] if i < 4 else ref["pg"][4 * C:]
                    assert float((a - b).norm() / b.norm()) < 3e-6, (mode, with_list, i)


def _pw_bwd(B, Cin, Cout, L, act, peak, resident_w):
    lib = _L()
    from spoofsv_amd import resident
    keep = {}
    _pw_fwd(B, Cin, Cout, L, act, False, False, keep)(None)
    gen = _gen(7, B, Cin, Cout, L, peak)
    dyd = _peaked(torch.randn(B, Cout, L, generator=gen), peak).to(DEV)
    nb = lib.query("ssv_pointwise_conv_ln_act_bwd_data_workspace", B, Cin, Cout, L)
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    nblk = lib.query("ssv_ln_partial_rows", B, L)
    rw = None
    if resident_w:                       # the one-launch form reads the transposed weight's resident planes (written in the mode in force)
        rw = resident.ResidentWeights([keep["w"]])
        rw.refresh(torch.cuda.current_stream().cuda_stream)

    def run(am):
        dx, dpre = torch.full((B, Cin, L), NAN, device=DEV), torch.full((B, Cout, L), NAN, device=DEV)
        part = torch.full((nblk, 3 * Cout), NAN, device=DEV)
        lib.call("ssv_pointwise_conv_ln_act_bwd_data", P(dyd), Cout * L, P(keep["w"]), resident.lookup(keep["w"]) if rw else None, P(keep["gamma"]),
                 P(keep["beta"]), P(keep["pre"]), P(keep["stats"]), P(dx), Cin * L, None, P(dpre), P(am), P(part), B, Cin, Cout, L, act, P(ws), nb, ST())
        run.rw = rw
        return dpre.reshape(B, -1), None
    return run


@pytest.mark.parametrize("Cin,Cout", [(128, 256), (256, 512), (256, 513), (64, 80)])
def test_link_backward_list_of_dpre(Cin, Cout):
    """ssv_pointwise_conv_ln_act_bwd_data (dpre_amax): the one-launch pwln_bwd_kernel (<= 256 LayerNorm rows, resident planes, split modes:
    it writes entry 4 * tile and ZEROES entries 4 * tile + 1 .. 3 itself -- asserted), ln_act_bwd_wide (512 / 513 rows, L >= 64: entry
    4 * tile, rest zeroed) and the 16-column kernel."""
    lib = _L().lib()
    from spoofsv_amd import resident
    for L in LENGTHS + (4100,):
        B = 2 if L > 4000 else _batch(L)
        wide = Cout > 256 and L >= 64
        assert lib.ssv_ln_bwd_partial_rows(0, B, Cout, L, 1) == B * _cdiv(L, 64 if wide else 16), (B, Cout, L)
        for mode in MODES:
            fused = mode >= 1 and Cout <= 256 and L >= 16
            try:
                with _mode(mode):
                    run = _pw_bwd(B, Cin, Cout, L, (L + 1) % 3, L % 2 == 1, resident_w=Cout <= 256 and mode >= 1)
                    lists = _produce(run, B, _na(L), ("pw_bwd", B, Cin, Cout, L), modes=(mode,))
                    if fused or wide:
                        assert float(lists[mode].reshape(B, -1, 4)[:, :, 1:].abs().max()) == 0.0, "entries 4 * tile + 1 .. 3 are zeroed"
            finally:
                resident.invalidate()


# ---- which kernel form a shape reaches: the shape log of a child process (the log is written when the process ends) ------------------
FORMS = [
    # (label, kernel name prefix, note)
    ("ln_act C=80", "ln_act_fwd_kernel<8, 16>", "B=3 C=80 L=65"), ("ln_act C=256", "ln_act_fwd_kernel<16, 16>", "B=3 C=256 L=65"),
    ("ln_act C=512", "ln_act_fwd_kernel<16, 32>", "B=3 C=512 L=65"), ("ln_act C=513", "ln_act_fwd_kernel<33, 16>", "B=3 C=513 L=65"),
    ("gate C=64", "ln_gate_fwd_kernel<4, 16>", "B=4 C=64 L=65"), ("gate C=256", "ln_gate_fwd_kernel<16, 16>", "B=4 C=256 L=65"),
    ("gate C=512", "ln_gate_fwd_kernel<16, 32>", "B=4 C=512 L=65"),
    ("highway stream", "ln_gate_fwd_stream_kernel", "B=2 C=256 L=65"), ("highway stream 512", "ln_gate_fwd_stream_kernel", "B=2 C=512 L=4100"),
    ("highway stream L=1", "ln_gate_fwd_stream_kernel", "B=128 C=256 L=1"),
    ("highway reducing C=80", "ln_gate_fwd_kernel<8, 16>", "B=2 C=80 L=65"), ("highway reducing small", "ln_gate_fwd_kernel<16, 16>", "B=2 C=256 L=17"),
    ("link fused 256", "gemm_pwln_kernel<", "B=2 M=256 N=65 K=128 k=1 +LN"), ("link fused 513", "gemm_pwln_kernel<", "B=2 M=513 N=1300 K=256 k=1 +LN"),
    ("link product + LN", "ln_act_fwd_kernel<16, 16>", "B=2 C=256 L=186"),
    ("gate bwd pers", "ln_gate_bwd_pers_kernel<8, 32>", "B=5 C=256 L=1300"), ("gate bwd wide 512", "ln_gate_bwd_wide_kernel<8, 2>", "B=3 C=512 L=64"),
    ("gate bwd wide 128", "ln_gate_bwd_wide_kernel<2, 4>", "B=3 C=128 L=1300"), ("gate bwd 16 col", "ln_gate_bwd_kernel<16, 32>", "B=3 C=512 L=63"),
    ("gate bwd C=80", "ln_gate_bwd_kernel<8, 16>", "B=3 C=80 L=325"),
    ("link bwd one launch", "pwln_bwd_kernel<", "B=2 Cin=128 N=65 Cout=256"), ("link bwd wide 512", "ln_act_bwd_wide_kernel<8, 4>", "B=2 C=512 L=65"),
    ("link bwd wide 513", "ln_act_bwd_wide_kernel<9, 4>", "B=2 C=513 L=65"), ("link bwd 16 col", "ln_act_bwd_kernel<", "B=3 C=513 L=63"),
]


def _probe_main():
    """Child process (SSV_SHAPE_LOG set): one mode-2 launch per entry of FORMS, through the same helpers the tests use."""
    from spoofsv_amd import resident
    am = lambda B, L: _poison(B, _na(L), 0)
    for C in (80, 256, 512, 513):
        _ln_act_fwd(3, C, 65, 1, True, True)(am(3, 65))
    for C in (64, 256, 512):
        _gate_fwd(4, C, 65, True, True)(am(4, 65))
    for (B, C, L) in ((2, 256, 65), (2, 512, 4100), (128, 256, 1), (2, 80, 65), (2, 256, 17)):
        _highway_fwd(B, C, L, 3, 1, False, True, True)(am(B, L))
    _pw_fwd(2, 128, 256, 65, 1, True, False)(am(2, 65))
    _pw_fwd(2, 256, 513, 1300, 1, True, False)(am(2, 1300))
    _pw_fwd(2, 128, 256, 186, 1, True, True)(am(2, 186))
    for (B, C, L) in ((5, 256, 1300), (3, 512, 64), (3, 128, 1300), (3, 512, 63), (3, 80, 325)):
        _highway_bwd(B, C, L, 3, 1, False, True)[0](am(B, L))
    _pw_bwd(2, 128, 256, 65, 1, True, True)(am(2, 65))
    resident.invalidate()
    _pw_bwd(2, 256, 512, 65, 1, True, False)(am(2, 65))
    _pw_bwd(2, 256, 513, 65, 1, True, False)(am(2, 65))
    _pw_bwd(3, 256, 513, 63, 1, True, False)(am(3, 63))
    for L in DECONV_LENGTHS:
        _deconv_fwd(32, 256, 256, L, True, False)(_poison(32, 64, 0))
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def shape_log():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "shapes.tsv")
        env = dict(os.environ, SSV_SHAPE_LOG=path, SSV_PRECISION="f16x2")
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_scale_lists as t; t._probe_main()" % (root, os.path.join(root, "tests"))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return [(f[0], f[1], f[4]) for f in rows if len(f) >= 5]


@pytest.mark.parametrize("label,kernel,note", FORMS, ids=[f[0] for f in FORMS])
def test_the_shapes_above_reach_the_kernel_form_they_are_meant_for(shape_log, label, kernel, note):
    """A later retune of the dispatch must not silently empty a case of part A: every form is looked up in the library's own shape log."""
    assert any(k.startswith(kernel) and (n == note or n.startswith(note + " ")) for k, _, n in shape_log), (label, [r for r in shape_log if note.split()[1] in r[2]][:6])


def test_deconvolution_cases_lie_on_both_sides_of_the_64_tile_limit(shape_log):
    """Tiles per item of the deconvolution's product (M = 512 rows, B = 32) at DECONV_LENGTHS: well below 64, exactly 64 (the largest count
    the picker's 128 x 112 tile yields within the list), and above it (where the launch logged is the retry without the list)."""
    tiles = {}
    for k, grid, n in shape_log:
        if k.startswith("gemm_nn_bf3") and n.startswith("B=32 M=512 N=") and " K=256 k=1" in n:
            tiles[int(n.split("N=")[1].split()[0])] = int(grid.split("x")[0]) // (512 if "bf3w" in k else 256)
    assert set(tiles) == {L for L in DECONV_LENGTHS if 32 * L >= 128}, sorted(tiles)
    assert min(tiles.values()) <= 8 and tiles[1792] == 64 and tiles[1793] > 64 and max(tiles.values()) > 64, tiles
    assert tiles[1300] <= 64, "the timed length takes the list from the product's epilogue"


# ---- the lists as tags of ops.* results ------------------------------------------------------------------------------------------------
def _ops_case(name, B, L, live=None):
    from spoofsv_amd import ops
    gen = _gen(8, B, L, len(name))
    C = 128
    x = _peaked(torch.randn(B, C, L, generator=gen), True).to(DEV)
    if name == "highway":
        w, bias = (torch.randn(2 * C, C, 3, generator=gen) / 20).to(DEV), torch.zeros(2 * C, device=DEV)
        ps = [p.to(DEV) for p in (*_ln_params(C, gen), *_ln_params(C, gen))]
        return lambda: ops.highway_conv1d(x, w, bias, *ps, 3, 1, False, live)
    if name == "link":
        w, bias = (torch.randn(256, C, 1, generator=gen) / 11).to(DEV), torch.zeros(256, device=DEV)
        g, b = [p.to(DEV) for p in _ln_params(256, gen, 3.0)]
        return lambda: ops.pointwise_conv_ln_act(x, w, bias, g, b, None, 1, live)
    if name == "deconv":
        w, bias = (torch.randn(C, C, 2, generator=gen) / 11).to(DEV), torch.zeros(C, device=DEV)
        return lambda: ops.deconv1d_k2s2(x, w, bias, live)
    return lambda: ops.shift_right(x)


@pytest.mark.parametrize("name", ["highway", "link", "deconv", "shift_right"])
def test_ops_results_carry_their_list_as_a_tag(name):
    """ops.highway_conv1d / pointwise_conv_ln_act / deconv1d_k2s2 tag their result in mode 2 from B * L >= 128 on, ops.shift_right always:
    the tag satisfies 1-2, ops.amax_of returns that very buffer, and after an in-place change of y a freshly computed, correct list."""
    from spoofsv_amd import ops
    for (B, L) in ((3, 65), (2, 325), (1, 2600), (3, 17)):
        with _mode(2), torch.no_grad():
            y = _ops_case(name, B, L)()
            torch.cuda.synchronize()
            tag = getattr(y, "_ssv_amax", None)
            if name != "shift_right" and B * L < 128:
                assert tag is None, "below the split-MFMA line the result carries no tag"
            else:
                assert tag is not None and ops.amax_of(y) is tag[0]
                _check(tag[0], y.reshape(B, -1), (name, B, L))
            _check(ops.amax_of(y), y.reshape(B, -1), (name, B, L, "amax_of"))
            y.mul_(2.0)
            am = ops.amax_of(y)
            torch.cuda.synchronize()
            assert tag is None or am is not tag[0], "a stale list after an in-place change"
            _check(am, y.reshape(B, -1), (name, B, L, "after mul_"))
        for mode in (0, 1):
            with _mode(mode), torch.no_grad():
                y = _ops_case(name, B, L)()
                assert name == "shift_right" or getattr(y, "_ssv_amax", None) is None


@pytest.mark.parametrize("name", ["highway", "link", "deconv"])
def test_lists_under_a_length_mask_are_those_of_the_unmasked_output(name):
    """the lists are taken before the mask -- bitwise the list of the unmasked call, hence >= the masked output's maximum
    (an over-estimate by the padded columns' values; the peak of these inputs sits in the LAST column, which the mask removes)."""
    from spoofsv_amd import ops
    B, L = 3, 200
    lens = torch.tensor([150], dtype=torch.int32, device=DEV)
    with _mode(2), torch.no_grad():
        y0 = _ops_case(name, B, L)()
        y1 = _ops_case(name, B, L, ops.Live(lens, 0, 2 if name == "deconv" else 1))()
        torch.cuda.synchronize()
        cut = 300 if name == "deconv" else 150
        assert torch.equal(y1[:, :, :cut], y0[:, :, :cut]) and float(y1[:, :, cut:].abs().max()) == 0.0
        assert torch.equal(y1._ssv_amax[0], y0._ssv_amax[0])
        assert bool((y1._ssv_amax[0].max(dim=1).values >= y1.reshape(B, -1).abs().amax(dim=1)).all())


# ---------------------------------------------------------------------------------------------------------------- part B: consumers
POSITIONS = (0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 65)


def _crafted_lists(amax, gen):
    """Lists of 24 / 84 / 256 / 1000 entries whose per-item maximum sits at exactly one position; every other entry a smaller positive value."""
    B = amax.numel()
    for n in (24, 84, 256, 1000):
        for p in sorted({q for q in POSITIONS + (n - 1,) if q < n}):
            # (at least 2^6 below the maximum: a consumer that misses position p sees another binade, hence another scale)
            lst = amax.cpu()[:, None] * 2.0 ** -6 * (0.05 + 0.9 * torch.rand(B, n, generator=gen))
            lst[:, p] = amax.cpu()
            yield "crafted n=%d p=%d" % (n, p), lst.to(DEV).contiguous()


def _operand(B, C, L, seed):
    """An operand that a real producer wrote, with the producer's own list: the highway gate's output, items 2^(3 b) apart."""
    run = _gate_fwd(B, C, L, seed % 2 == 0, False)
    am = _poison(B, _na(L), 0)
    live, _ = run(am)
    torch.cuda.synchronize()
    return live.reshape(B, C, L).clone(), am


def _all_lists(x, producer_list, seed):
    lib = _L()
    B = x.shape[0]
    n = x[0].numel()
    am8 = torch.empty(B, 8, device=DEV)
    lib.call("ssv_absmax", P(x), n, B, n, P(am8), 8, ST())
    amax = x.reshape(B, -1).abs().amax(dim=1)
    yield "NULL", None
    yield "absmax 8", am8
    yield "one per item", amax.reshape(B, 1).contiguous()
    if producer_list is not None:
        yield "producer", producer_list
    yield from _crafted_lists(amax, _gen(9, seed))


def _consume(call, x, producer_list, seed, tag):
    """call(list or None, entries per item) -> tuple of output tensors; all lists give bitwise equal outputs."""
    first = None
    for name, lst in _all_lists(x, producer_list, seed):
        outs = call(lst, lst.shape[1] if lst is not None else 0)
        torch.cuda.synchronize()
        if first is None:
            first = [o.clone() for o in outs]
        else:
            for i, (a, b) in enumerate(zip(outs, first)):
                assert torch.equal(a, b), (tag, name, "output", i, "differs from the NULL-list call", float((a - b).abs().max()))
    return first


def _conv_ref(x, w, dy, k, d, causal):
    pad = d * (k - 1)
    xd, wd = x.double().cpu().requires_grad_(True), w.double().cpu().requires_grad_(True)
    xin = F.pad(xd, (pad, 0)) if causal else F.pad(xd, (pad // 2, pad // 2))
    yd = F.conv1d(xin, wd, None, dilation=d)
    yd.backward(dy.double().cpu())
    return yd.detach(), xd.grad, wd.grad


def _per_item(got, ref, tag, tol=2e-6):
    assert bool(torch.isfinite(got).all()), (tag, "inf / NaN in the output")
    for b in range(ref.shape[0]):
        e = _rl2(got[b], ref[b])
        assert e <= tol, (tag, "item", b, e)


CONV_CASES = [(4, 128, 256, 186, 1, 1, False), (3, 64, 128, 325, 3, 27, True), (3, 256, 513, 200, 1, 1, False), (4, 128, 128, 65, 3, 1, False)]


@pytest.mark.parametrize("B,Cin,Cout,L,k,d,causal", CONV_CASES)
def test_convolution_products_do_not_depend_on_the_partition_of_their_lists(B, Cin, Cout, L, k, d, causal):
    """ssv_conv1d_fwd (k = 1, k = 3 with the 54-column halo, the 513-row tail), ssv_conv1d_bwd_data and ssv_conv1d_bwd_weight with every
    list of _all_lists: bitwise equal outputs, and per item -- items 2^(3 b) apart, so a consumer that took item 0's list for all would
    overflow or lose the small items -- within 2e-6 of float64 (the committed per-product bar)."""
    lib = _L()
    with _mode(2):
        x, xl = _operand(B, Cin, L, L)
        gen = _gen(10, B, Cin, Cout, L)
        w = (torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5).to(DEV)
        dy = _peaked(torch.randn(B, Cout, L, generator=gen), True).to(DEV)
        nbf = lib.query("ssv_conv1d_fwd_workspace", Cin, Cout, k)
        nbd = lib.query("ssv_conv1d_bwd_data_workspace", Cin, Cout, k)
        nbw = lib.query("ssv_conv1d_bwd_weight_workspace", B, Cin, Cout, L, k)
        wsf, wsd, wsw = [torch.empty(max(n, 256), dtype=torch.uint8, device=DEV) for n in (nbf, nbd, nbw)]

        def fwd(lst, n):
            y = torch.full((B, Cout, L), NAN, device=DEV)
            lib.call("ssv_conv1d_fwd", P(x), Cin * L, P(lst), n, P(w), None, None, None, P(y), Cout * L, None, B, Cin, Cout, L, k, d, int(causal), P(wsf), nbf, ST())
            return (y,)

        def bwd_data(lst, n):
            dx = torch.full((B, Cin, L), NAN, device=DEV)
            lib.call("ssv_conv1d_bwd_data", P(dy), Cout * L, P(lst), n, P(w), None, None, P(dx), Cin * L, B, Cin, Cout, L, k, d, int(causal), P(wsd), nbd, ST())
            return (dx,)
        am_x8, am_dy8 = torch.empty(B, 8, device=DEV), torch.empty(B, 8, device=DEV)
        lib.call("ssv_absmax", P(x), Cin * L, B, Cin * L, P(am_x8), 8, ST())
        lib.call("ssv_absmax", P(dy), Cout * L, B, Cout * L, P(am_dy8), 8, ST())

        def bwd_weight_x(lst, n):
            dw = torch.full((Cout, Cin, k), NAN, device=DEV)
            lib.call("ssv_conv1d_bwd_weight", P(dy), Cout * L, P(am_dy8), 8, P(x), Cin * L, P(lst if lst is not None else am_x8), n or 8, P(dw),
                     B, Cin, Cout, L, k, d, int(causal), P(wsw), nbw, ST())
            return (dw,)

        def bwd_weight_dy(lst, n):
            dw = torch.full((Cout, Cin, k), NAN, device=DEV)
            lib.call("ssv_conv1d_bwd_weight", P(dy), Cout * L, P(lst if lst is not None else am_dy8), n or 8, P(x), Cin * L, P(am_x8), 8, P(dw),
                     B, Cin, Cout, L, k, d, int(causal), P(wsw), nbw, ST())
            return (dw,)

        def bwd_weight_null(lst, n):
            dw = torch.full((Cout, Cin, k), NAN, device=DEV)
            lib.call("ssv_conv1d_bwd_weight", P(dy), Cout * L, None, 0, P(x), Cin * L, None, 0, P(dw), B, Cin, Cout, L, k, d, int(causal), P(wsw), nbw, ST())
            return (dw,)
        yref, dxref, dwref = _conv_ref(x, w, dy, k, d, causal)
        tag = (B, Cin, Cout, L, k, d, causal)
        y = _consume(fwd, x, xl, L, ("conv1d_fwd",) + tag)[0]
        _per_item(y, yref, ("conv1d_fwd",) + tag)
        dx = _consume(bwd_data, dy, None, L + 1, ("conv1d_bwd_data",) + tag)[0]
        _per_item(dx, dxref, ("conv1d_bwd_data",) + tag)
        dw = _consume(bwd_weight_x, x, xl, L + 2, ("conv1d_bwd_weight x list",) + tag)[0]
        dw2 = _consume(bwd_weight_dy, dy, None, L + 3, ("conv1d_bwd_weight dy list",) + tag)[0]
        dw0 = bwd_weight_null(None, 0)[0]
        torch.cuda.synchronize()
        assert torch.equal(dw, dw2) and torch.equal(dw, dw0), "the weight gradient with NULL lists differs from the one with lists"
        assert _rl2(dw, dwref) <= 2e-6, _rl2(dw, dwref)


def test_batched_weight_gradient_does_not_depend_on_the_partition_of_its_lists():
    """ssv_conv1d_bwd_weight_multi: the job table stores WHOLE lists with total entry counts (B * entries per item)."""
    lib = _L()
    B, Cin, Cout, L, k = 4, 128, 256, 200, 3
    with _mode(2):
        x, xl = _operand(B, Cin, L, 3)
        gen = _gen(11, B, L)
        dy = _peaked(torch.randn(B, Cout, L, generator=gen), True).to(DEV)
        am_dy = torch.empty(B, 8, device=DEV)
        lib.call("ssv_absmax", P(dy), Cout * L, B, Cout * L, P(am_dy), 8, ST())
        nb = lib.query("ssv_conv1d_bwd_weight_multi_workspace", 1, B, Cin, Cout, L, k)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        sh = (ctypes.c_int * 3)()
        lib.call("ssv_conv_shifts", k, 3, 0, sh)

        def run(lst, n):
            if lst is None:
                lst = xl
            dw = torch.full((Cout, Cin, k), NAN, device=DEV)
            table = (lib.WgradJob * 1)()
            t = table[0]
            t.dy, t.x, t.dw, t.part, t.pgrads = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), None, None
            t.shift[0], t.shift[1], t.shift[2] = sh[0], sh[1], sh[2]
            t.dy_amax, t.x_amax, t.dy_namax, t.x_namax = am_dy.data_ptr(), lst.data_ptr(), am_dy.numel(), lst.numel()
            tdev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
            lib.call("ssv_conv1d_bwd_weight_multi", P(tdev), 1, Cout * L, Cin * L, B, Cin, Cout, L, k, 6, 0, 0, P(ws), nb, ST())
            torch.cuda.synchronize()
            return (dw,)
        dw = _consume(run, x, xl, 5, "bwd_weight_multi")[0]
        assert _rl2(dw, _conv_ref(x, torch.zeros(Cout, Cin, k), dy, k, 3, False)[2]) <= 2e-6


def test_highway_link_and_deconvolution_do_not_depend_on_the_partition_of_their_lists():
    """ssv_highway_conv1d_fwd, ssv_pointwise_conv_ln_act_fwd, ssv_deconv1d_k2s2_fwd / _bwd: y (and h, pre, dx, dw) bitwise equal for every list."""
    lib = _L()
    B, C, L = 4, 128, 186
    with _mode(2):
        x, xl = _operand(B, C, L, 7)
        keep = {}
        hw = _highway_fwd(B, C, L, 3, 3, False, False, False, keep)
        keep["x"].copy_(x)
        _consume(lambda lst, n: (hw(None, lst, n)[0].clone(), keep["h"].clone()), x, xl, 1, "highway_conv1d_fwd")
        keep = {}
        pw = _pw_fwd(B, C, 256, L, 1, False, False, keep)
        keep["x"].copy_(x)
        _consume(lambda lst, n: (pw(None, lst, n)[0].clone(), keep["pre"].clone()), x, xl, 2, "pointwise_conv_ln_act_fwd")
        keep = {}
        dc = _deconv_fwd(B, C, C, L, False, False, keep)
        keep["x"].copy_(x)
        y = _consume(lambda lst, n: (dc(None, lst, n)[0].clone(),), x, xl, 3, "deconv1d_k2s2_fwd")[0].reshape(B, C, 2 * L)
        yref = F.conv_transpose1d(x.double().cpu(), keep["w"].double().cpu(), keep["bias"].double().cpu(), stride=2)
        _per_item(y, yref, "deconv1d_k2s2_fwd")
        dy = _peaked(torch.randn(B, C, 2 * L, generator=_gen(12)), True).to(DEV)
        nb = lib.query("ssv_deconv1d_k2s2_bwd_workspace", B, C, C)
        ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)

        def bwd(lst, n):
            dx, dw, db = torch.full((B, C, L), NAN, device=DEV), torch.full((C, C, 2), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
            lib.call("ssv_deconv1d_k2s2_bwd", P(dy), C * 2 * L, P(lst), n, P(x), C * L, P(keep["w"]), P(dx), C * L, P(dw), P(db), B, C, C, L, P(ws), nb, ST())
            return dx, dw, db
        dx = _consume(bwd, dy, None, 4, "deconv1d_k2s2_bwd")[0]
        xr = x.double().cpu().requires_grad_(True)
        F.conv_transpose1d(xr, keep["w"].double().cpu(), None, stride=2).backward(dy.double().cpu())
        _per_item(dx, xr.grad, "deconv1d_k2s2_bwd dx")


@pytest.mark.parametrize("k2", [-20, 0, 14, 15, 16, 40])
@pytest.mark.parametrize("below", [False, True])
def test_binade_edges_of_the_power_of_two_scale(k2, below):
    """Operands whose maximum is exactly 2^k or 2^k (1 - 2^-24) (ssv_pow2_scale reads the exponent field: the two sides of a binade edge
    get scales a factor 2 apart): forward, data gradient and weight gradient stay within 2e-6 of float64, no inf."""
    lib = _L()
    B, Cin, Cout, L, k = 3, 128, 256, 186, 3
    edge = 2.0 ** k2 * ((1.0 - 2.0 ** -24) if below else 1.0)
    gen = _gen(13, k2 + 100, below)
    x = (torch.randn(B, Cin, L, generator=gen) * 0.25).clamp(-0.9, 0.9) * 2.0 ** k2
    dy = (torch.randn(B, Cout, L, generator=gen) * 0.25).clamp(-0.9, 0.9) * 2.0 ** k2
    x[:, 5, L - 1] = edge
    dy[:, Cout - 1, 0] = -edge
    assert float(x.abs().max()) == edge and float(dy.abs().max()) == edge
    w = torch.randn(Cout, Cin, k, generator=gen) * 0.05
    yref, dxref, dwref = _conv_ref(x, w, dy, k, 3, False)
    from spoofsv_amd import ops
    with _mode(2):
        xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        y = ops.conv1d(xg, wg, None, k, 3, False)
        y.backward(dy.to(DEV))
        torch.cuda.synchronize()
        _per_item(y.detach(), yref, ("fwd", k2, below))
        _per_item(xg.grad, dxref, ("dgrad", k2, below))
        assert bool(torch.isfinite(wg.grad).all()) and _rl2(wg.grad, dwref) <= 2e-6, (k2, below, _rl2(wg.grad, dwref))
