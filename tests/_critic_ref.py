"""References for the operator tests of the WGAN-GP critics (tests/test_critic_ref_cpu.py, tests/test_gpu_critic_ops.py): the
functionals the tests differentiate twice, in a form that runs on float64 CPU tensors and on the HIP operators alike; the case
tables; a numpy Philox4x32-10 that mirrors csrc/critic.hip's use of it; and a restatement of the critic's forward that also returns
the inputs of its three leaky-ReLUs.  No device, no HIP: everything here runs in the CPU suite."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of float32

# ------------------------------------------------------------------------------------------- A: conv1d_dd, second order
# (B, Cin, Cout, L, k, dilation, causal) and the kernels each row is chosen to reach in a split arithmetic mode: does the forward / data
# gradient run the split-MFMA kernel (ssv_host.h use_bf3: B * L >= 128 and both channel counts >= SSV_MIN_SPLIT_CHANNELS), does the
# weight gradient (api_conv.hip wgrad_bf3_runs: B * L >= 256 on top of the channel rule).  tests/test_critic_ref_cpu.py holds the
# table to ops._tiny_conv / ops._bf3_shape / the library's own predicate.
CONV_SHAPES = [
    # shape                              fwd/dgrad split  wgrad split  spread operands too
    ((2, 80, 128, 131, 1, 1, False),     True,            True,        True),       # melDisc.conv1: B * L = 262 just over 256, ragged L
    ((2, 128, 256, 131, 3, 1, False),    True,            True,        True),       # hc.conv
    ((2, 128, 64, 131, 1, 1, False),     True,            True,        False),      # conv2
    ((1, 513, 128, 300, 1, 1, False),    True,            True,        True),       # linDisc.conv1: reduction length no multiple of 32, B = 1
    ((2, 32, 32, 64, 3, 1, False),       True,            False,       False),      # on both thresholds: 32 channels, B * L = 128
    ((2, 32, 32, 63, 3, 1, False),       False,           False,       False),      # just under: everything fp32, no lists
    ((2, 64, 16, 131, 1, 1, False),      False,           False,       False),      # conv3: a "tiny" convolution inside a split-mode run
    ((3, 40, 48, 100, 3, 3, True),       True,            True,        False),      # causal and dilated
]
CONV_CASES = [(s, "unit") for s, _, _, _ in CONV_SHAPES] + [(s, "spread") for s, _, _, sp in CONV_SHAPES if sp]
CONV_NAMES = ("y", "gx", "gw", "gb", "d_gy", "d_x", "d_w")
CONV_PER_ITEM = ("y", "gx", "d_gy", "d_x")           # tensors with a batch axis: compared per item


def conv_operands(shape, kind):
    """float32 operands (x, w, bias, gy, vx, vw) of one case.  "spread": batch items of gy and vx scaled by 2^-20, 1, 2^12 (cycled) and
    rows of x by 2^-8 .. 2^4 -- what the penalty's coefficient does to the operands of the second pass."""
    B, Cin, Cout, L, k, d, causal = shape
    gen = torch.Generator().manual_seed(1000 * Cin + 10 * L + k + d + (kind == "spread"))
    x = torch.randn(B, Cin, L, generator=gen)
    w = torch.randn(Cout, Cin, k, generator=gen) * 0.05
    bias = torch.randn(Cout, generator=gen) * 0.1
    gy = torch.randn(B, Cout, L, generator=gen)
    vx = torch.randn(B, Cin, L, generator=gen)
    vw = torch.randn(Cout, Cin, k, generator=gen) * 0.05
    if kind == "spread":
        item = torch.tensor([2.0 ** -20, 1.0, 2.0 ** 12])[torch.arange(B) % 3].view(B, 1, 1)
        gy, vx = gy * item, vx * item
        x = x * torch.exp2(torch.randint(-8, 5, (B, Cin, 1), generator=gen).float())
    return x, w, bias, gy, vx, vw


def conv64(x, w, bias, k, d, causal):
    """The reference convolution: F.conv1d with explicit zero padding ("same", or all on the left when causal)."""
    pad = d * (k - 1)
    return F.conv1d(F.pad(x, (pad, 0) if causal else (pad // 2, pad // 2)), w, bias, dilation=d)


def conv_second_order(conv, operands, k, d, causal):
    """The bilinear functional of part A on ``conv(x, w, bias, k, d, causal)``; returns the seven tensors of CONV_NAMES, detached."""
    x, w, bias, gy, vx, vw = [t.detach().clone().requires_grad_(True) for t in operands]
    y = conv(x, w, bias, k, d, causal)
    gx, gw, gb = torch.autograd.grad(y, (x, w, bias), gy, create_graph=True)
    d_gy, d_x, d_w = torch.autograd.grad((gx, gw), (gy, x, w), (vx, vw))
    return {n: t.detach() for n, t in zip(CONV_NAMES, (y, gx, gw, gb, d_gy, d_x, d_w))}


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())


def worst_rel_l2(got, want, per_item):
    """Relative L2 error: the worst batch item when ``per_item``, the whole tensor otherwise."""
    if not per_item:
        return rel_l2(got, want)
    return max(rel_l2(got[b], want[b]) for b in range(want.shape[0]))


# ------------------------------------------------------------------------------------------- B: LayerNorm / gate, second order
LN_SHAPES = [(3, 128, 325), (2, 64, 41), (2, 16, 20), (2, 4, 7), (1, 8, 5), (2, 256, 33), (2, 33, 17)]
GATE_SHAPES = [(3, 128, 325), (2, 16, 41), (2, 64, 7), (1, 256, 19), (2, 24, 33)]
# operand kinds: unit-variance randn; columns whose variance is comparable to eps = 1e-5 (scales 3e-3 and 1e-2); batch-strided
# activations (channel slices of a tensor twice as wide, unit variance)
LN_KINDS = {"unit": 1.0, "var_9e-6": 3e-3, "var_1e-4": 1e-2, "strided": 1.0}


def ln_ref(x, g, b):
    mu = x.mean(1, keepdim=True)
    d = x - mu
    return d * torch.rsqrt((d * d).mean(1, keepdim=True) + 1e-5) * g.view(1, -1, 1) + b.view(1, -1, 1)


def gate_ref(h, x, g1, b1, g2, b2):
    C = x.shape[1]
    s = torch.sigmoid(ln_ref(h[:, :C], g1, b1))
    return s * ln_ref(h[:, C:], g2, b2) + (1 - s) * x


def ln_operands(shape, kind):
    """float64 (x, gamma, beta, gy, v); the kind's scale applies to x."""
    B, C, L = shape
    gen = torch.Generator().manual_seed(B * 1000 + C)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, g, b, gy, v = mk(B, C, L), mk(C), mk(C), mk(B, C, L), mk(B, C, L)
    return x * LN_KINDS[kind], g, b, gy, v


def gate_operands(shape, kind):
    """float64 (h, x, g1, b1, g2, b2, gy, vh, vx); the kind's scale applies to h and x."""
    B, C, L = shape
    gen = torch.Generator().manual_seed(B * 1000 + C + 7)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    h, x, g1, b1, g2, b2, gy = mk(B, 2 * C, L), mk(B, C, L), mk(C), mk(C), mk(C), mk(C), mk(B, C, L)
    vh, vx = mk(B, 2 * C, L), mk(B, C, L)
    return h * LN_KINDS[kind], x * LN_KINDS[kind], g1, b1, g2, b2, gy, vh, vx


def ln_second_order(ln, x, g, b, gy, v):
    """Forward, the three first-order gradients, and the gradient of <v, dx> with respect to (gy, x, gamma).  The arguments are leaves that
    require a gradient; returns (first, second): lists of detached tensors."""
    y = ln(x, g, b)
    gx, gg, gb = torch.autograd.grad(y, (x, g, b), gy, create_graph=True)
    second = torch.autograd.grad(gx, (gy, x, g), v)
    return [t.detach() for t in (y, gx, gg, gb)], [t.detach() for t in second]


def gate_second_order(gate, h, x, g1, b1, g2, b2, gy, vh, vx):
    """Forward, the six first-order gradients, and the gradient of <vh, dh> + <vx, dx> (either cotangent may be None) with respect to
    (h, x, g1, b1, g2, b2, gy).  An entry of ``second`` is None where the contraction does not depend on that argument."""
    ts = (h, x, g1, b1, g2, b2, gy)
    y = gate(h, x, g1, b1, g2, b2)
    first = torch.autograd.grad(y, ts[:6], gy, create_graph=True)
    outs, vs = zip(*[(o, v) for o, v in zip(first[:2], (vh, vx)) if v is not None])
    second = torch.autograd.grad(outs, ts, vs, allow_unused=True)
    return [t.detach() for t in (y,) + tuple(first)], [None if t is None else t.detach() for t in second]


# ------------------------------------------------------------------------------------------- C: Philox4x32-10 and the dropout mask
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123): ``counter`` four and ``key`` two uint32 values or arrays; returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _LOW for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                      # 32 x 32 -> 64 bit products
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def dropout_threshold(p):
    """uint32(p * 2^32) with p rounded to float32 first, as the kernel receives it."""
    return int(float(np.float32(p)) * 4294967296.0)


def dropout_drops(n, p, seed, call):
    """Boolean array (n,): element 4 * i4 + q is dropped iff word q of Philox(counter = (i4 lo, i4 hi, call lo, call hi),
    key = (seed, 0x5f3759df)) is below the threshold."""
    i4 = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((i4 & _LOW, i4 >> np.uint64(32), call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF), (seed, 0x5F3759DF))
    return (np.stack(words, axis=1).reshape(-1)[:n] < np.uint32(dropout_threshold(p)))


def act_dropout_ref(x, slope, p, seed, call):
    """(d, y) of ssv_act_dropout_fwd for a float32 numpy array x, bit for bit: d = (x > 0 ? 1 : slope) * keep, y = x * d, all in float32,
    keep = 0 or 1 / (1 - p)."""
    x = np.asarray(x, dtype=np.float32)
    keep = np.ones(x.shape, dtype=np.float32)
    if p > 0:
        inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        keep = np.where(dropout_drops(x.size, p, seed, call), np.float32(0.0), inv).astype(np.float32).reshape(x.shape)
    d = np.where(x > 0, np.float32(1.0), np.float32(slope)).astype(np.float32) * keep
    return d, x * d


# ------------------------------------------------------------------------------------------- C: penalty and pool
GP_SHAPES = [(3, 592), (2, 65536), (2, 65539), (70, 300), (1, 1)]      # across the 65,536-element chunk, past 64 samples, the smallest
POOL_SHAPES = [(3, 16, 36, 4), (3, 16, 37, 4), (3, 16, 39, 4), (2, 5, 37, 37), (3, 64, 8, 8), (1, 1, 1, 1)]      # (B, C, L, k): L % k = 0, 1, k - 1; k = L


def gp_operand(B, n):
    """float32 (B, n) penalty input.  With room for them, item 0 is exactly zero (torch's norm has gradient 0 there) and item 1 has norm
    exactly 1 (four entries of 0.5), also in float32."""
    g = torch.randn(B, n, generator=torch.Generator().manual_seed(B * 7 + n))
    if B >= 3 and n >= 8:
        g[0] = 0.0
        g[1] = 0.0
        g[1, [0, 3, n // 2, n - 1]] = 0.5
    return g


def gp_ref(g, lam):
    """mean_b lam (||g_b|| - 1)^2 and its gradient in float64."""
    g = g.double().requires_grad_(True)
    loss = torch.mean(lam * (torch.norm(g, p=2, dim=1) - 1) ** 2)
    (dg,) = torch.autograd.grad(loss, g)
    return loss.detach(), dg


def gp_bound(g, n):
    """Worst-case relative error of one item's loss term and gradient coefficient in float32.  The sum of n squares (all terms >= 0, so the
    bound is relative): a thread adds ceil(min(n, 65536) / 256) terms in sequence, then 8 tree levels, then the chunks in sequence;
    squaring and the square root add 2 u.  (nrm - 1) amplifies the norm's relative error by nrm / |nrm - 1|; a few more roundings for
    the square, lam, the division by B nrm and the product with g."""
    terms = -(-min(n, 65536) // 256) + 8 + -(-n // 65536)
    nrm = g.double().norm(dim=1)
    nrm = nrm[(nrm > 0) & (nrm != 1)]
    amp = float((nrm / (nrm - 1).abs()).max()) if nrm.numel() else 1.0
    return (2 * (0.5 * terms + 2) * amp + 6) * U32


# ------------------------------------------------------------------------------------------- D: the whole critic
CRITIC_CASES = {"mel": (80, 32, (4, 80, 40)), "lin": (65, 32, (3, 65, 64))}       # freq_bins, DISC_DIM, (B, F, T)
# Seeds of (weights, inputs, masks), chosen on the CPU so that in float64 no leaky-ReLU input of the three critic calls lies within
# KINK_MARGIN of its tensor's rms from zero, in eval mode and with the masks: an fp32 kernel and the reference then take the same side
# of every kink.  tests/test_critic_ref_cpu.py asserts it.
CRITIC_SEEDS = {"mel": 32, "lin": 2}
KINK_MARGIN = 1e-4


def critic_with_kink_inputs(x, sd, kind, masks=False):
    """oracle.critic_oracle.critic restated so that it also returns the inputs of the three leaky-ReLUs.  ``masks``: False (eval) or the
    three scaled keep masks of this call."""
    pools = {"mel": (4, 2), "lin": (8, 4)}[kind]
    masks = list(masks) if masks is not False else None
    drop = (lambda t: t) if masks is None else (lambda t: t * masks.pop(0))

    def ln(t, name):
        w = sd[name + ".weight"]
        return F.layer_norm(t.permute(0, 2, 1), (w.shape[0],), w, sd[name + ".bias"], 1e-5).permute(0, 2, 1)

    conv = lambda t, name, padding=0: F.conv1d(t, sd[name + ".weight"], sd[name + ".bias"], padding=padding)
    x = drop(ln(conv(x, "conv1"), "ln1"))
    h = conv(x, "hc.conv", 1)
    c = h.shape[1] // 2
    s = torch.sigmoid(ln(h[:, :c], "hc.ln1"))
    x = drop(s * ln(h[:, c:], "hc.ln2") + (1 - s) * x)
    k1 = ln(F.avg_pool1d(conv(x, "conv2"), pools[0]), "ln2")
    x = drop(F.leaky_relu(k1, 0.05))
    k2 = ln(F.avg_pool1d(conv(x, "conv3"), pools[1]), "ln3")
    k3 = ln(conv(F.leaky_relu(k2, 0.05), "conv4"), "ln4")
    return F.adaptive_avg_pool1d(conv(F.leaky_relu(k3, 0.05), "conv5"), 1), [k1, k2, k3]


def critic_case(kind):
    """The committed case of part D: (float32 state_dict, real, fake, eps, nine float32 masks)."""
    from oracle import critic_oracle as CO
    from spoofsv_amd.critic import linDisc, melDisc
    Fb, dim, (B, _, T) = CRITIC_CASES[kind]
    torch.manual_seed(CRITIC_SEEDS[kind])
    disc = (linDisc if kind == "lin" else melDisc)(Fb, dim)
    sd = {k: v.detach().clone() for k, v in disc.state_dict().items()}
    real, fake, eps = torch.rand(B, Fb, T), torch.rand(B, Fb, T), torch.rand(B)
    masks = []
    CO.critic_losses(fake, real, eps, sd, kind, 10.0, masks=None, drawn=masks)       # (draws the nine masks as nn.Dropout would)
    return sd, real, fake, eps, [m.detach() for m in masks]


def critic_kink_margins(sd, kind, real, fake, eps, masks):
    """min |input| / rms(input) over the leaky-ReLU inputs of the three critic calls (interpolate, ground truth, prediction) in float64."""
    sd = {k: v.double() for k, v in sd.items()}
    c = eps.double().view(-1, 1, 1)
    calls = [c * real.double() + (1 - c) * fake.double(), real.double(), fake.double()]
    worst = float("inf")
    with torch.no_grad():
        for i, x in enumerate(calls):
            m = False if masks is False else [t.double() for t in masks[3 * i:3 * i + 3]]
            for t in critic_with_kink_inputs(x, sd, kind, m)[1]:
                worst = min(worst, float(t.abs().min() / t.pow(2).mean().sqrt()))
    return worst


def critic_reference(sd, kind, real, fake, eps, masks, dtype):
    """(penalty, Wasserstein term, {name: gradient}) of oracle.critic_oracle.critic_losses in ``dtype`` (both losses' gradients summed, as
    a critic iteration accumulates them)."""
    from oracle import critic_oracle as CO
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    m = False if masks is False else [t.to(dtype) for t in masks]
    gp, ld = CO.critic_losses(fake.to(dtype), real.to(dtype), eps.to(dtype), sd, kind, 10.0, masks=m)
    gp.backward()
    ld.backward()
    return float(gp.detach().double()), float(ld.detach().double()), {k: v.grad.detach().double() for k, v in sd.items()}
