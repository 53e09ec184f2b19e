"""The optimizer tail of a training step against plain references (tests/_optimizer_tail_ref.py): ssv_adam_multi and FusedAdam per element and per
moment against a float64 step from the device's own state, the resident planes of ssv_conv_pack_multi bitwise against the documented layout,
their consumers on ragged shapes, and ssv_sum_slabs.  Run with `-m gpu` on an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import _optimizer_tail_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROJECT = (2e-4, 0.5, 0.9, 1e-6)                    # config.json
TORCH_DEFAULT = (1e-3, 0.9, 0.999, 1e-8)
POISON = -0x21524111                                # int32 pattern 0xDEADBEEF: a finite float, -6.26e18
GUARD = 8                                           # guard words between carved tensors
MODES = ("f16x2", "bf16x3", "fp32")
# tests/test_gpu_parity.py TOLS: (forward, backward) max-norm relative error of the conv kernels per arithmetic mode
CONV_TOLS = {"f16x2": (2e-5, 3e-4), "bf16x3": (1e-4, 5e-4)}


@pytest.fixture
def precision(request):
    import spoofsv_amd
    prev = spoofsv_amd.set_precision(request.param)
    yield request.param
    spoofsv_amd.set_precision(prev)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.detach().view(torch.int32).cpu().numpy()


# ================================================================================================ a. ssv_adam_multi through the raw ABI
class _Carved:
    """One flat poisoned device buffer per role (p, g, m, v) with tensors carved out of it: ``specs`` = [(n, (ap, ag, am, av), glued)], the
    start of a tensor's role r rounded up to 16 bytes behind the guard words and then moved by a_r floats; ``glued`` puts the tensor directly
    behind the previous one in every role, no guard, as the gradient arena packs a group."""

    def __init__(self, specs, seed, t):
        self.specs = specs
        cur = [GUARD] * 4
        self.off = []
        for n, al, glued in specs:
            o = []
            for r in range(4):
                s = cur[r] if glued else (cur[r] + GUARD + 3) // 4 * 4 + al[r]
                o.append(s)
                cur[r] = s + n
            self.off.append(o)
        self.size = (max(cur) + 2 * GUARD + 3) // 4 * 4              # whole 16-byte units: the four roles' rows start aligned
        rng = np.random.default_rng(seed)
        host = np.full((4, self.size), POISON, dtype=np.int32).view(np.float32)
        self.mask = np.zeros((4, self.size), dtype=bool)                   # True: belongs to a tensor
        tot = sum(n for n, _, _ in specs)
        floor = lambda a: np.where(a == 0, 0.0, np.sign(a) * np.maximum(np.abs(a), 1e-15))      # non-zero inputs stay >= 1e-15: no flush-to-zero tested
        scale = np.array([1e-12, 1e-6, 1.0, 1e4])[rng.integers(0, 4, tot)]
        p = floor(rng.standard_normal(tot))
        g = floor(rng.standard_normal(tot) * scale)
        g[rng.choice(tot, min(100, tot // 2), replace=False)] = 0.0
        if t > 1:
            m = floor(0.3 * rng.standard_normal(tot) * scale)
            v = np.maximum((rng.standard_normal(tot) * scale) ** 2, 1e-15)
            z = rng.choice(tot, min(50, tot // 2), replace=False)
            m[z] = 0.0
            v[z] = 0.0
        else:
            m, v = np.zeros(tot), np.zeros(tot)
        at = 0
        for (n, _, _), o in zip(specs, self.off):
            for r, a in enumerate((p, g, m, v)):
                host[r, o[r]:o[r] + n] = a[at:at + n].astype(np.float32)
                self.mask[r, o[r]:o[r] + n] = True
            at += n
        self.buf = torch.from_numpy(host.copy()).to(DEV)
        assert self.buf.data_ptr() % 16 == 0 and (self.size * 4) % 16 == 0         # so that the offsets decide every pointer's alignment
        self.before = host

    def rows(self, chunk=32768):
        """The chunk table as FusedAdam._build writes it: every tensor cut into pieces of ``chunk`` elements."""
        rows, owner = [], []
        base = [self.buf[r].data_ptr() for r in range(4)]
        for i, ((n, _, _), o) in enumerate(zip(self.specs, self.off)):
            for c in range(0, n, chunk):
                rows.append([base[r] + 4 * (o[r] + c) for r in range(4)] + [min(chunk, n - c)])
                owner.append(i)
        return rows, owner

    def gather(self, host, r):
        return np.concatenate([host[r, o[r]:o[r] + n] for (n, _, _), o in zip(self.specs, self.off)])


def _launch_adam(rows, hp, step, step_dev):
    from spoofsv_amd import _lib
    assert ctypes.sizeof(_lib.AdamChunk) == 40
    table = torch.from_numpy(np.array(rows, dtype=np.int64)).to(DEV)
    rc = _lib.lib().ssv_adam_multi(_ptr(table), len(rows), *[float(x) for x in hp], step, None if step_dev is None else _ptr(step_dev), _stream())
    torch.cuda.synchronize()
    return rc


def _check_adam(c, hp, t, what):
    """After a launch on ``c``: every element of p', m', v' within the bounds of a float64 step from the state before the launch; guard words and
    g bitwise unchanged.  Returns the worst fractions of the bounds (p, m, v, update part of p)."""
    after = c.buf.cpu().numpy()
    ref = R.adam_step_ref(c.gather(c.before, 0), c.gather(c.before, 1), c.gather(c.before, 2), c.gather(c.before, 3), *hp, t)
    fr = R.adam_fractions(c.gather(after, 0), c.gather(after, 2), c.gather(after, 3), ref)
    ends = np.cumsum([n for n, _, _ in c.specs])
    where = lambda i: "element %d (tensor %d of %d elements)" % (i, int(np.searchsorted(ends, i, side="right")),
                                                                 c.specs[int(np.searchsorted(ends, i, side="right"))][0])
    print("%s: fraction of the bound used p %.3f (update part %.3f) m %.3f v %.3f" % (what, fr[0][0], fr[3][0], fr[1][0], fr[2][0]))
    for name, (f, i) in zip(("p", "exp_avg", "exp_avg_sq"), fr[:3]):
        assert f <= 1.0, "%s: %s misses its bound by a factor %.3g at %s" % (what, name, f, where(i))
    a, b = after.view(np.int32), c.before.view(np.int32)
    assert np.array_equal(a[1], b[1]), what + ": the gradient buffer was written"
    for r, name in ((0, "p"), (2, "exp_avg"), (3, "exp_avg_sq")):
        assert np.array_equal(a[r][~c.mask[r]], b[r][~c.mask[r]]), "%s: guard words of %s were written" % (what, name)
    return [f for f, _ in fr]


SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 1028, 2049, 32767, 32768]
ALIGNS = [tuple((a >> r) & 1 for r in range(4)) for a in range(16)]          # every combination of 0 / 1 float per role; 15 of 16 are misaligned


def _single_specs():
    return [(n, al, False) for n in SIZES for al in ALIGNS]


@pytest.mark.parametrize("hp", [PROJECT, TORCH_DEFAULT], ids=["project", "torch_default"])
@pytest.mark.parametrize("t", [1, 2, 3, 10, 1000, 100000])
def test_adam_multi_every_size_and_alignment_in_one_table(hp, t):
    """One chunk per (size, alignment): the sizes straddle the scalar tail, the single-vector loop and the two-in-flight loop (n > 1024); one
    misaligned pointer of the four must send its chunk down the scalar path with the same result."""
    c = _Carved(_single_specs(), seed=100 + t, t=t)
    rows, _ = c.rows()
    assert len(rows) == len(SIZES) * 16
    assert _launch_adam(rows, hp, t, None) == 0
    _check_adam(c, hp, t, "lr=%g t=%d, %d chunks" % (hp[0], t, len(rows)))


@pytest.mark.parametrize("n", SIZES)
def test_adam_multi_single_chunk_launches(n):
    """The same sizes as launches of ONE chunk, all four pointers aligned and then the gradient alone misaligned."""
    for al in ((0, 0, 0, 0), (0, 1, 0, 0)):
        c = _Carved([(n, al, False)], seed=n, t=7)
        rows, _ = c.rows()
        assert len(rows) == 1 and rows[0][1] % 16 == 4 * al[1]
        assert _launch_adam(rows, PROJECT, 7, None) == 0
        _check_adam(c, PROJECT, 7, "n=%d align=%s" % (n, al))


MULTI = [(2 * 32768 + 5, (0, 0, 0, 0), False),      # three chunks, the last of 5 elements
         (513, (0, 0, 0, 0), False),                # a bias ...
         (256 * 3, (0, 0, 0, 0), True),             # ... and the weight directly behind it: misaligned by one float in every role
         (1, (0, 0, 0, 0), False),
         (40000, (0, 0, 0, 1), False)]              # two chunks, exp_avg_sq alone misaligned


@pytest.mark.parametrize("hp", [PROJECT, TORCH_DEFAULT], ids=["project", "torch_default"])
@pytest.mark.parametrize("t", [1, 10])
def test_adam_multi_chunk_table_of_many_tensors(hp, t):
    c = _Carved(MULTI, seed=7 + t, t=t)
    rows, owner = c.rows()
    assert len(rows) == 8 and [r[4] for r in rows[:3]] == [32768, 32768, 5]
    assert rows[3][0] % 16 == 0 and all(rows[4][r] % 16 == 4 for r in range(4))          # 513 floats behind an aligned start
    assert _launch_adam(rows, hp, t, None) == 0
    _check_adam(c, hp, t, "multi-tensor table, lr=%g t=%d" % (hp[0], t))


def test_adam_multi_step_source():
    """With step_dev the count is *step_dev + 1, whatever the host passes, and the counter advances by exactly one per call; without it and
    with step = 0 the call is refused."""
    specs = [(1025, (0, 0, 0, 0), False), (37, (1, 0, 0, 0), False)]
    step_dev = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    for call, host_step in enumerate((1000, 0, 1)):                        # deliberately not the device's count
        t = 3 + call
        c = _Carved(specs, seed=50 + call, t=t)
        assert _launch_adam(c.rows()[0], PROJECT, host_step, step_dev) == 0
        assert int(step_dev.item()) == t
        _check_adam(c, PROJECT, t, "step_dev call %d (host step %d)" % (call, host_step))
    c = _Carved(specs, seed=60, t=2)
    from spoofsv_amd import _lib
    assert _launch_adam(c.rows()[0], PROJECT, 0, None) == -1               # SSV_BAD_SHAPE
    assert b"adam_multi" in _lib.lib().ssv_last_error()
    assert np.array_equal(_bits(c.buf), c.before.view(np.int32))           # and nothing ran


# ================================================================================================ b. FusedAdam
PARAM_SIZES = (33, 513, 32769, 70001)


def _arena_params(seed):
    """Four parameters whose gradients are consecutive unaligned views of one flat buffer, the gradient arena's layout."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in PARAM_SIZES]
    flat = torch.zeros(sum(PARAM_SIZES), device=DEV)
    assert flat.data_ptr() % 16 == 0
    at = 0
    for p in params:
        p.grad = flat[at:at + p.numel()].view_as(p)
        at += p.numel()
    assert [p.grad.data_ptr() % 16 for p in params] == [0, 4, 8, 12]
    return params, flat


def _fresh_grads(flat, rng):
    n = flat.numel()
    g = rng.standard_normal(n) * np.array([1e-12, 1e-6, 1.0, 1e4])[rng.integers(0, 4, n)]
    g = np.sign(g) * np.maximum(np.abs(g), 1e-15)
    g[rng.choice(n, 100, replace=False)] = 0.0
    flat.copy_(torch.from_numpy(g.astype(np.float32)))              # in place: the views the parameters hold see the new values


def _state(params, opt):
    cat = lambda ts: np.concatenate([t.detach().cpu().numpy().ravel() for t in ts])
    return (cat(params), cat([opt.state[p]["exp_avg"] for p in params]) if opt.state else None,
            cat([opt.state[p]["exp_avg_sq"] for p in params]) if opt.state else None)


def _check_fused(params, opt, flat, before, t, what):
    p0, m0, v0 = before
    ref = R.adam_step_ref(p0, flat.cpu().numpy(), m0, v0, *PROJECT, t)
    p1, m1, v1 = _state(params, opt)
    fr = R.adam_fractions(p1, m1, v1, ref)
    print("%s: fraction of the bound used p %.3f (update part %.3f) m %.3f v %.3f" % (what, fr[0][0], fr[3][0], fr[1][0], fr[2][0]))
    for name, (f, i) in zip(("p", "exp_avg", "exp_avg_sq"), fr[:3]):
        assert f <= 1.0, "%s: %s misses its bound by a factor %.3g at flat element %d" % (what, name, f, i)


@pytest.mark.parametrize("precision", MODES, indirect=True)
def test_fused_adam_six_steps_per_element_and_per_moment(precision):
    from spoofsv_amd.train import FusedAdam
    params, flat = _arena_params(11)
    opt = FusedAdam(params, PROJECT[0], PROJECT[1:3], PROJECT[3])
    rng = np.random.default_rng(12)
    n = flat.numel()
    before = (_state(params, opt)[0], np.zeros(n), np.zeros(n))
    for t in range(1, 7):
        _fresh_grads(flat, rng)
        opt.step()
        _check_fused(params, opt, flat, before, t, "FusedAdam step %d" % t)
        before = _state(params, opt)
    sd = opt.state_dict()["state"]
    assert [float(sd[i]["step"]) for i in range(4)] == [6.0] * 4


def test_fused_adam_capturable_replays_a_captured_step():
    """The step captured on one stream (no parallel branches): every replay advances the device counter and applies the gradients that are in
    the buffer at that moment."""
    from spoofsv_amd.train import FusedAdam, _no_gc
    params, flat = _arena_params(21)
    opt = FusedAdam(params, PROJECT[0], PROJECT[1:3], PROJECT[3], capturable=True)
    rng = np.random.default_rng(22)
    n = flat.numel()
    before = (_state(params, opt)[0], np.zeros(n), np.zeros(n))
    _fresh_grads(flat, rng)
    opt.step()                                                  # eager: builds the chunk table, the moments and the device counter
    _check_fused(params, opt, flat, before, 1, "capturable, eager step 1")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc(), torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    before = _state(params, opt)
    assert int(opt._step_dev.item()) == 1                       # capturing runs nothing
    for replay in range(3):
        _fresh_grads(flat, rng)
        graph.replay()
        torch.cuda.synchronize()
        t = 2 + replay
        assert int(opt._step_dev.item()) == t
        _check_fused(params, opt, flat, before, t, "capturable, replay %d" % replay)
        before = _state(params, opt)
    sd = opt.state_dict()["state"]
    assert [float(sd[i]["step"]) for i in range(4)] == [4.0] * 4
    p1, m1, v1 = before
    assert np.array_equal(np.concatenate([sd[i]["exp_avg"].cpu().numpy().ravel() for i in range(4)]), m1)
    assert np.array_equal(np.concatenate([sd[i]["exp_avg_sq"].cpu().numpy().ravel() for i in range(4)]), v1)


# ================================================================================================ c. ssv_conv_pack_plan + ssv_conv_pack_multi
PLANE_POISON = 0xA7
ZERO_WEIGHT = R.PACK_SHAPES.index((8, 8, 1))
SPIKE_WEIGHT = R.PACK_SHAPES.index((34, 128, 1))


def _layout(mode):
    return "f16x2" if mode == "f16x2" else "bf16x3"            # outside split-fp16 the planes are bf16 halves (include/ssv_hip.h)


def _pack_weights(seed):
    """Amplitudes 2^5 apart from weight to weight (a scale shared between two weights shows), one weight all zeros, one with a single element
    2^20 above the rest (the rest then sits deep in the fp16-subnormal range of the lo halves)."""
    rng = np.random.default_rng(seed)
    ws = []
    for i, (co, ci, k) in enumerate(R.PACK_SHAPES):
        w = rng.uniform(0.5, 1.0, (co, ci, k)) * rng.choice([-1.0, 1.0], (co, ci, k)) * 2.0 ** (5 * (i - 5))
        if i == ZERO_WEIGHT:
            w[:] = 0.0
        if i == SPIKE_WEIGHT:
            w.ravel()[1234] *= 2.0 ** 20
        ws.append(w.astype(np.float32))
    return ws


class _Packed:
    def __init__(self, weights):
        from spoofsv_amd import _lib
        L = _lib.lib()
        n = len(weights)
        self.w = [torch.from_numpy(w.copy()).to(DEV) for w in weights]
        shapes = [tuple(w.shape) for w in weights]
        self.bytes = [int(L.ssv_conv_pack_bytes(*s)) for s in shapes]
        self.planes = [torch.full((b,), PLANE_POISON, dtype=torch.uint8, device=DEV) for b in self.bytes]
        vp = ctypes.c_void_p
        ci = lambda j: (ctypes.c_int * n)(*[s[j] for s in shapes])
        self.jobs = (_lib.PackJob * (2 * n))()
        self.nblocks = L.ssv_conv_pack_plan(n, (vp * n)(*[t.data_ptr() for t in self.w]), (vp * n)(*[t.data_ptr() for t in self.planes]),
                                            ci(0), ci(1), ci(2), self.jobs)
        assert self.nblocks > 0, L.ssv_last_error()
        self.jobs_dev = torch.from_numpy(np.frombuffer(bytes(self.jobs), dtype=np.uint8).copy()).to(DEV)
        self.ws_bytes = int(L.ssv_conv_pack_multi_workspace(2 * n))
        self.ws = torch.zeros(max(self.ws_bytes, 256), dtype=torch.uint8, device=DEV)

    def refresh(self):
        from spoofsv_amd import _lib
        _lib.call("ssv_conv_pack_multi", _ptr(self.jobs_dev), len(self.jobs), self.nblocks, _ptr(self.ws), self.ws_bytes, _stream())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.planes]


def _check_job(buf, off, job, w, mode, what):
    """One job's bytes in the weight's buffer ``buf`` (numpy uint8) against the reference; returns its inverse scale."""
    n = R.plane_elems(job)
    hi = buf[off:off + 2 * n].view(np.uint16)
    lo = buf[off + R.lo_offset(job):off + R.lo_offset(job) + 2 * n].view(np.uint16)
    rhi, rlo, inv = R.pack_planes_ref(w, job, mode)
    sc = R.pow2_scale(np.abs(w).max())[0] if mode == "f16x2" else None
    t, m, k = R._grid(job)
    idx = R.plane_index(t, m, k, job)
    x = w.ravel()[m * job.sm + k * job.sk + t]
    # the arbiter first: the planes reconstruct the weight to the format's accuracy
    worst = R.reconstruction_excess(x, hi[idx], lo[idx], mode, sc)
    assert worst <= 1.0, "%s: reconstruction misses its bound by %.3g" % (what, worst)
    bad = np.flatnonzero(hi != rhi)
    assert bad.size == 0, "%s: %d hi entries differ, first at 2-byte index %d: %#x, expected %#x" % (what, bad.size, bad[0], hi[bad[0]], rhi[bad[0]])
    bad = np.flatnonzero(lo != rlo)
    if bad.size:
        sub = np.abs(rlo[bad].view(np.float16).astype(np.float32)) < 2.0 ** -14
        assert False, "%s: %d lo entries differ (%d of them at fp16-subnormal halves), first at 2-byte index %d: %#x, expected %#x" % (
            what, bad.size, int(sub.sum()), bad[0], lo[bad[0]], rlo[bad[0]])
    return inv


def _check_buffers(pk, bufs, weights, mode):
    for i, (shape, w) in enumerate(zip(R.PACK_SHAPES, weights)):
        jobs_ref, total = R.plan_jobs_ref(*shape)
        assert total == pk.bytes[i], (shape, total, pk.bytes[i])
        tail = bufs[i][total - 256:]
        kept = np.ones(256, dtype=bool)
        for tr, (jr, off) in enumerate(jobs_ref):
            j = pk.jobs[2 * i + tr]
            # the planned job is the documented one, at the documented place in the buffer
            assert (j.M, j.K, j.Kpad, j.KT, j.sm, j.sk) == tuple(jr) and j.w == pk.w[i].data_ptr(), (shape, tr)
            assert j.planes - pk.planes[i].data_ptr() == off and j.inv_out - pk.planes[i].data_ptr() == total - 256 + 128 * tr, (shape, tr)
            inv = _check_job(bufs[i], off, jr, w, mode, "weight %d %s, %s job, %s" % (i, shape, "transposed" if tr else "forward", mode))
            if mode == "f16x2":
                got = tail[128 * tr:128 * tr + 4].view(np.float32)[0]
                assert got == inv, "weight %d %s job %d: inverse scale %g, expected %g" % (i, shape, tr, got, inv)
                kept[128 * tr:128 * tr + 4] = False
        assert np.all(tail[kept] == PLANE_POISON), "weight %d %s: the trailing block was written outside the inverse scales" % (i, shape)
        end = jobs_ref[1][1] + 2 * R.lo_offset(jobs_ref[1][0])
        assert end == total - 256
    firsts = [pk.jobs[q].first_block for q in range(len(pk.jobs))]
    assert firsts == sorted(firsts) and firsts[0] == 0 and firsts[-1] < pk.nblocks


@pytest.mark.parametrize("precision", MODES, indirect=True)
def test_pack_multi_planes_are_the_documented_bytes(precision):
    mode = _layout(precision)
    weights = _pack_weights(31)
    pk = _Packed(weights)
    bufs = pk.refresh()
    _check_buffers(pk, bufs, weights, mode)
    # a second refresh after one weight changed in place: that weight's planes follow, every other buffer keeps its bytes
    i = R.PACK_SHAPES.index((17, 33, 3))
    weights[i] = (weights[i] * np.float32(-1.37) + np.float32(2.0 ** -3)).astype(np.float32)
    pk.w[i].copy_(torch.from_numpy(weights[i]))
    again = pk.refresh()
    for q in range(len(weights)):
        assert np.array_equal(again[q], bufs[q]) == (q != i), q
    _check_buffers(pk, again, weights, mode)


# ================================================================================================ d. consumers on ragged shapes
def _conv_ref(x, w, bias, d):
    """float64 'same' convolution, y(b,o,t) = bias[o] + sum_{c,j} w[o,c,j] x(b,c,t + (j-j0) d)."""
    B, Cin, L = x.shape
    k = w.shape[2]
    y = np.zeros((B, w.shape[0], L)) + bias[None, :, None]
    for j in range(k):
        s = (j - (k - 1) // 2) * d
        xs = np.zeros_like(x)
        lo, hi = max(0, -s), min(L, L - s)
        xs[:, :, lo:hi] = x[:, :, lo + s:hi + s]
        y += np.einsum("oc,bct->bot", w[:, :, j], xs)
    return y


def _conv_bwd_data_ref(dy, w, d):
    B, Cout, L = dy.shape
    k = w.shape[2]
    dx = np.zeros((B, w.shape[1], L))
    for j in range(k):
        s = (j - (k - 1) // 2) * d
        ds = np.zeros_like(dy)
        lo, hi = max(0, s), min(L, L + s)
        ds[:, :, lo:hi] = dy[:, :, lo - s:hi - s]
        dx += np.einsum("oc,bot->bct", w[:, :, j], ds)
    return dx


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _conv_both_ways(w, bias, x, dy, k, d, planes):
    """(y, dx) of ssv_conv1d_fwd / ssv_conv1d_bwd_data through the raw ABI with w_packed = ``planes`` (None: the call splits the weight)."""
    from spoofsv_amd import _lib
    B, Cin, L = x.shape
    Cout = w.shape[0]
    y = torch.full((B, Cout, L), float("nan"), device=DEV)
    dx = torch.full((B, Cin, L), float("nan"), device=DEV)
    nb = _lib.query("ssv_conv1d_fwd_workspace", Cin, Cout, k)
    ws = torch.zeros(max(nb, 256), dtype=torch.uint8, device=DEV)
    _lib.call("ssv_conv1d_fwd", _ptr(x), Cin * L, None, 0, _ptr(w), planes, _ptr(bias), None, _ptr(y), Cout * L, None, B, Cin, Cout, L, k, d, 0,
              _ptr(ws), nb, _stream())
    nb = _lib.query("ssv_conv1d_bwd_data_workspace", Cin, Cout, k)
    ws2 = torch.zeros(max(nb, 256), dtype=torch.uint8, device=DEV)
    _lib.call("ssv_conv1d_bwd_data", _ptr(dy), Cout * L, None, 0, _ptr(w), planes, None, _ptr(dx), Cin * L, B, Cin, Cout, L, k, d, 0,
              _ptr(ws2), nb, _stream())
    torch.cuda.synchronize()
    return y, dx


RAGGED = [(17, 33, 3, 1), (513, 40, 1, 1), (40, 513, 3, 3)]


# L = 37: the shape the trainer's short tail batches have; at B L < 128 these entry points take the exact-fp32 kernels whatever the mode.
# L = 70: the same layers on the split-MFMA path, where the planes are what the product reads.
@pytest.mark.parametrize("L", [37, 70])
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"], indirect=True)
def test_resident_planes_on_ragged_shapes_serve_their_consumers(precision, L):
    from spoofsv_amd import _lib, resident
    from spoofsv_amd.train import FusedAdam
    mode = _layout(precision)
    fwd_tol, bwd_tol = CONV_TOLS[precision]
    B = 2
    g = torch.Generator().manual_seed(41)
    convs = [torch.nn.Parameter((torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5).to(DEV)) for co, ci, k, _ in RAGGED]
    Ci, Co = 40, 33
    wt = resident.mark_transposed(torch.nn.Parameter((torch.randn(Ci, Co, 2, generator=g) / Ci ** 0.5).to(DEV)))
    params = convs + [wt]
    opt = FusedAdam(params, 1e-3)
    opt.refresh_resident_weights()

    def consumers():
        out = []
        for w, (co, ci, k, d) in zip(convs, RAGGED):
            gg = torch.Generator().manual_seed(co)
            x, dy, bias = torch.randn(B, ci, L, generator=gg).to(DEV), torch.randn(B, co, L, generator=gg).to(DEV), torch.randn(co, generator=gg).to(DEV)
            planes = resident.lookup(w)
            assert planes is not None
            y0, dx0 = _conv_both_ways(w.detach(), bias, x, dy, k, d, None)
            y1, dx1 = _conv_both_ways(w.detach(), bias, x, dy, k, d, planes)
            what = "conv %s L=%d %s" % ((co, ci, k, d), L, precision)
            assert torch.equal(y0, y1), what + ": forward differs between resident planes and the per-call split"
            assert torch.equal(dx0, dx1), what + ": data gradient differs between resident planes and the per-call split"
            wn, xn, dyn = w.detach().cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64), dy.cpu().numpy().astype(np.float64)
            e = _rel(y1.cpu().numpy(), _conv_ref(xn, wn, bias.cpu().numpy().astype(np.float64), d))
            assert e < fwd_tol, (what, "forward", e)
            e = _rel(dx1.cpu().numpy(), _conv_bwd_data_ref(dyn, wn, d))
            assert e < bwd_tol, (what, "data gradient", e)
            out += [y1, dx1]
        # the transposed convolution: planes of the 1x1 weight w.view(Cin, 2 Cout, 1)
        gg = torch.Generator().manual_seed(5)
        x, bias = torch.randn(B, Ci, L, generator=gg).to(DEV), torch.randn(Co, generator=gg).to(DEV)
        planes = resident.lookup(wt.view(Ci, 2 * Co, 1))
        assert planes is not None
        ys = []
        for pl in (None, planes):
            y = torch.full((B, Co, 2 * L), float("nan"), device=DEV)
            nb = _lib.query("ssv_deconv1d_k2s2_fwd_workspace", Ci, Co)
            ws = torch.zeros(max(nb, 256), dtype=torch.uint8, device=DEV)
            _lib.call("ssv_deconv1d_k2s2_fwd", _ptr(x), Ci * L, None, 0, _ptr(wt), pl, _ptr(bias), _ptr(y), Co * 2 * L, None, 0, B, Ci, Co, L,
                      _ptr(ws), nb, _stream())
            torch.cuda.synchronize()
            ys.append(y)
        assert torch.equal(ys[0], ys[1]), "deconv L=%d %s: forward differs between resident planes and the per-call split" % (L, precision)
        yr = np.einsum("coj,bct->botj", wt.detach().cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64)).reshape(B, Co, 2 * L)
        yr += bias.cpu().numpy().astype(np.float64)[None, :, None]
        e = _rel(ys[1].cpu().numpy(), yr)
        assert e < fwd_tol, ("deconv", L, precision, e)
        return out + [ys[1]]

    first = consumers()
    # one optimizer step: the re-split is ordered behind the update on the stream, so the planes are those of the UPDATED weights
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    torch.cuda.synchronize()
    rw = opt._resident
    assert [id(p) for p in rw.params] == [id(p) for p in params]
    for p, buf in zip(params, rw._planes):
        shape = resident.pack_shape(p)
        jobs_ref, total = R.plan_jobs_ref(*shape)
        assert total == buf.numel()
        host, w = buf.cpu().numpy(), p.detach().cpu().numpy().reshape(shape)
        for tr, (jr, off) in enumerate(jobs_ref):
            inv = _check_job(host, off, jr, w, mode, "after FusedAdam.step: weight %s, job %d, %s" % (shape, tr, mode))
            if mode == "f16x2":
                assert host[total - 256 + 128 * tr:total - 252 + 128 * tr].view(np.float32)[0] == inv
    second = consumers()
    assert not any(torch.equal(a, b) for a, b in zip(first, second))


# ================================================================================================ e. ssv_sum_slabs
def test_sum_slabs_against_float64_reproducible_and_in_bounds():
    from spoofsv_amd import _lib
    rng = np.random.default_rng(51)
    for n in (1, 255, 257, 1000):
        for Z in (1, 3, 4, 5, 33):
            for stride in (n, n + 3):
                host = np.full(Z * stride, np.nan, dtype=np.float32)                 # NaN in the stride gaps: a read of one shows
                x = (rng.standard_normal((Z, n)) * 10.0 ** rng.integers(-3, 4, (Z, n))).astype(np.float32)
                for z in range(Z):
                    host[z * stride:z * stride + n] = x[z]
                slabs = torch.from_numpy(host).to(DEV)
                outs = []
                for _ in range(2):
                    out = torch.from_numpy(np.full(n + GUARD, POISON, dtype=np.int32)).to(DEV)
                    _lib.call("ssv_sum_slabs", _ptr(slabs), _ptr(out), n, Z, stride, _stream())
                    torch.cuda.synchronize()
                    outs.append(out.cpu().numpy())
                what = "n=%d Z=%d stride=%d" % (n, Z, stride)
                assert np.array_equal(outs[0], outs[1]), what + ": two calls differ"
                assert np.all(outs[0][n:] == POISON), what + ": out was written past n"
                got = outs[0][:n].view(np.float32).astype(np.float64)
                x64 = x.astype(np.float64)
                assert np.all(np.abs(got - x64.sum(0)) <= Z * R.U * np.abs(x64).sum(0)), what
                assert np.array_equal(_bits(slabs), host.view(np.int32)), what + ": the slabs were written"
