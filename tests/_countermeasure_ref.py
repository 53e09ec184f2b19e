"""References for the spoof-countermeasure tests (tests/test_countermeasure_cpu.py, tests/test_gpu_countermeasure.py): a float64 restatement
of the two classifiers of anti_spoofing/discriminator.py on stock torch CPU ops, the loss of anti_spoofing/main_spoof_conv1d.py:87 and
the fused head's gradients as written formulas, one Adam step with L2 weight decay and AMSGrad in float64 numpy with per-element
rounding bounds, and a float64 CPU trainer (features from tests/_corpus_features_ref.py) that fixes the iteration count of the
end-to-end test.  No device, no HIP: everything here runs in the CPU suite.  Nothing under ``spoofsv_amd/`` imports it."""
import collections
import os
import wave as _wave

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                      # unit roundoff of float32
POOLS = {"mel": (2, 2), "lin": (8, 4)}            # discriminator.py:64,68 / :104,108
SLOPE = 0.05
REF_HP = (1e-3, 0.9, 0.98, 1e-9)                   # main_spoof_conv1d.py:52 (lr: torch's default)
TORCH_DEFAULT = (1e-3, 0.9, 0.999, 1e-8)


# ------------------------------------------------------------------------------------------------ the classifiers
def cm_forward(x, sd, kind, masks=False):
    """discriminator.py:76-94 / :115-132 restated on functional ops in x's dtype.  ``masks``: False (eval) or the three scaled keep masks
    (dp1, hc.dp, dp2) of this call.  Returns (pred (B,), z (B,) the logit, [inputs of the three leaky-ReLUs])."""
    pools = POOLS[kind]
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
    x = drop(F.leaky_relu(k1, SLOPE))
    k2 = ln(F.avg_pool1d(conv(x, "conv3"), pools[1]), "ln3")
    k3 = ln(conv(F.leaky_relu(k2, SLOPE), "conv4"), "ln4")
    z = F.adaptive_avg_pool1d(conv(F.leaky_relu(k3, SLOPE), "conv5"), 1).reshape(-1)
    return torch.sigmoid(z), z, [k1, k2, k3]


def bce(z, labels):
    """mean_b -y log(p + 1e-6) - (1 - y) log(q + 1e-6), p = sigmoid(z), q = 1 - p taken as sigmoid(-z): the value of the formula, which
    the subtraction would lose even in float64 beyond z = 37.  Returns (loss, per item)."""
    per = -labels * torch.log(torch.sigmoid(z) + 1e-6) - (1 - labels) * torch.log(torch.sigmoid(-z) + 1e-6)
    return per.mean(), per


def cm_reference(sd, kind, x, labels, masks, dtype):
    """(pred (B,), loss, {name: gradient}) of one training forward / backward in ``dtype``, everything returned as float64."""
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    m = False if masks is False else [t.to(dtype) for t in masks]
    pred, z, _ = cm_forward(x.to(dtype), sd, kind, m)
    loss, _ = bce(z, labels.to(dtype))
    loss.backward()
    return pred.detach().double(), float(loss.detach().double()), {k: v.grad.detach().double() for k, v in sd.items()}


def kink_margin(sd, kind, x, masks):
    """min |input| / rms(input) over the three leaky-ReLU inputs in float64."""
    with torch.no_grad():
        m = False if masks is False else [t.double() for t in masks]
        ks = cm_forward(x.double(), {k: v.double() for k, v in sd.items()}, kind, m)[2]
    return min(float(t.abs().min() / t.pow(2).mean().sqrt()) for t in ks)


def mask_shapes(kind, B, disc_dim, T):
    """Shapes of the three dropout masks of one forward on (B, freq_bins, T) input."""
    return [(B, disc_dim, T), (B, disc_dim, T), (B, 64, T // POOLS[kind][0])]


# ------------------------------------------------------------------------------------------------ the fused head
HeadRef = collections.namedtuple("HeadRef", "pred per loss dx dw dbias z")


def head_ref(x, w, bias, labels, slope, gscale):
    """ssv_cm_head_fwd / _bwd as include/ssv_hip.h states them, float64 numpy from the float32 inputs.  ``labels`` None: pred and z only."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).ravel()
    B, C, T = x.shape
    a = np.where(x > 0, x, float(np.float32(slope)) * x)
    am = a.mean(axis=2)
    z = float(np.asarray(bias, dtype=np.float64).ravel()[0]) + am @ w
    sig = lambda t: np.where(t >= 0, 1.0 / (1.0 + np.exp(-np.abs(t))), np.exp(-np.abs(t)) / (1.0 + np.exp(-np.abs(t))))
    p, q = sig(z), sig(-z)
    if labels is None:
        return HeadRef(p, None, None, None, None, None, z)
    y = np.asarray(labels, dtype=np.float64)
    per = -y * np.log(p + 1e-6) - (1 - y) * np.log(q + 1e-6)
    dz = float(gscale) / B * p * q * (-y / (p + 1e-6) + (1 - y) / (q + 1e-6))
    dx = dz[:, None, None] / T * w[None, :, None] * np.where(x > 0, 1.0, float(np.float32(slope)))
    return HeadRef(p, per, per.mean(), dx, dz @ am, dz.sum(), z)


# ------------------------------------------------------------------------------------------------ Adam with weight decay and AMSGrad
AdamExRef = collections.namedtuple("AdamExRef", "p m v vmax mag step_size denom")


def adam_ex_step_ref(p, g, m, v, vmax, lr, b1, b2, eps, wd, amsgrad, t):
    """torch.optim.Adam's single-tensor step in float64: g' = g + wd p; m' = b1 m + (1-b1) g'; v' = b2 v + (1-b2) g'^2;
    vmax' = max(vmax, v'); denom = sqrt(vmax')/sqrt(1-b2^t) + eps (v' for vmax' without amsgrad, vmax then passes through unchanged);
    p' = p - lr/(1-b1^t) m'/denom.  The hyper-parameters are rounded to float32 first (the ABI takes floats).  Also returns what the
    bounds need: mag = |b1 m| + |(1-b1) g'|, the step size and the denominator."""
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    p, g, m, v, vmax = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v, vmax))
    t = int(t)
    g1 = g + wd * p
    m1 = b1 * m + (1.0 - b1) * g1
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    x1 = np.maximum(vmax, v1) if amsgrad else vmax
    vh = x1 if amsgrad else v1
    step_size = lr / (1.0 - b1 ** t)
    denom = np.sqrt(vh) / np.sqrt(1.0 - b2 ** t) + eps
    return AdamExRef(p - step_size * m1 / denom, m1, v1, x1, np.abs(b1 * m) + np.abs((1.0 - b1) * g1), step_size, denom)


def adam_ex_bounds(ref):
    """Single-step error bounds of the float32 kernel against ``ref``: (tol_p, tol_m, tol_v, tol_vmax), derived as
    ``_optimizer_tail_ref.adam_bounds`` derives its own, one rounding = u = 2^-24 relative.
      g'    one fused multiply-add: relative error u (exact when wd = 0).
      m'    = b1 m + (1-b1) g': the first product carries 1 u, the second 3 u (the float constant 1 - b1, the product, g'), the sum 1 more:
            at most 4 u of mag = |b1 m| + |(1-b1) g'|; tol_m = 5 u mag keeps adam_bounds' one spare.
      v'    = b2 v + (1-b2) g'^2: adam_bounds' 4 u, plus 2 u because g' enters squared: tol_v = 6 u v' (all terms are non-negative, so the
            bound is relative).
      vmax' = max(vmax, v') is exact given v': |max(a, x) - max(a, y)| <= |x - y|, so tol_vmax = tol_v.
      p'    the update s m'/denom: m' 5 u (against mag >= |m'|); denom = sqrt(vh) c + eps with vh within 6 u -> 3 u after the root, then
            the root itself, the product, the float constant c and the sum: 7 u; the float constant eps: 1 u; the division, the product
            with s and the float constant s: 3 u; together 16 u s mag / denom, plus u |p'| for the final subtraction."""
    tol_m = 5 * U * ref.mag
    tol_v = 6 * U * ref.v
    tol_p = U * np.abs(ref.p) + 16 * U * ref.step_size * ref.mag / ref.denom
    return tol_p, tol_m, tol_v, tol_v


def adam_ex_fractions(p1, m1, v1, x1, ref, amsgrad):
    """Worst used fraction of each bound and its index: [(fp, i), (fm, i), (fv, i), (fvmax, i)].  Where a bound is 0 any error counts as
    infinite.  Without amsgrad vmax must pass through bitwise, which the caller checks; its fraction is reported as 0."""
    out = []
    for k, (got, want, tol) in enumerate(zip((p1, m1, v1, x1), (ref.p, ref.m, ref.v, ref.vmax), adam_ex_bounds(ref))):
        if k == 3 and not amsgrad:
            out.append((0.0, 0))
            continue
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err == 0, 0.0, err / tol)
        out.append((float(frac.max()), int(frac.argmax())))
    return out


# ------------------------------------------------------------------------------------------------ end to end: toy corpus, CPU trainer
E2E_RATE, E2E_SECONDS, E2E_FILES = 16000, 1.0, 24


def toy_wave(i, cls, rate=E2E_RATE, seconds=E2E_SECONDS):
    """Item i of class ``cls``: three sinusoids in 200..1400 Hz (class 1) or 4000..6400 Hz (class 0) -- disjoint spectra -- under a
    raised-cosine envelope, peak 0.5, plus noise 50 dB down so that no frame is silent."""
    rng = np.random.default_rng(1000 * cls + i)
    t = np.arange(int(rate * seconds)) / rate
    lo, hi = (200.0, 1400.0) if cls == 1 else (4000.0, 6400.0)
    y = sum(np.sin(2 * np.pi * f * t + ph) for f, ph in zip(rng.uniform(lo, hi, 3), rng.uniform(0, 2 * np.pi, 3)))
    y = y / np.abs(y).max() * 0.5 * (0.6 + 0.4 * np.sin(np.pi * t / t[-1]) ** 2)
    return (y + 1.5e-3 * rng.standard_normal(len(t))).astype(np.float32)


def write_wav16(path, y, rate):
    """16-bit PCM mono with the stdlib ``wave`` module."""
    pcm = np.clip(np.round(np.asarray(y, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with _wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


def write_toy_corpus(root, n_each=E2E_FILES // 2):
    """(bona fide paths, spoof paths): n_each files per class."""
    out = {1: [], 0: []}
    for cls in (1, 0):
        for i in range(n_each):
            path = os.path.join(root, "%s_%02d.wav" % ("bona" if cls else "spoof", i))
            write_wav16(path, toy_wave(i, cls), E2E_RATE)
            out[cls].append(path)
    return out[1], out[0]


def read_items(paths):
    """[(float32 waveform, rate)] of 16-bit wav files, scaled as ``ge2e_harness.read_wav`` scales them."""
    from scipy.io import wavfile
    out = []
    for path in paths:
        sr, y = wavfile.read(path)
        out.append((y.astype(np.float32) / 32768.0, int(sr)))
    return out


def cpu_trainer_first_eer0(cfg, bona, spoof, sd0, feat_type, order, batch_size, max_iterations, eer):
    """The reference's loop (main_spoof_conv1d.py:68-106) in float64 on the CPU with dropout off.  ``bona`` / ``spoof``: [(waveform, rate)];
    features of every item from tests/_corpus_features_ref.py at 16 kHz (its resampler in front for another rate), batches from
    ``order(epoch)`` (the source's own seeded shuffle), zero-padded per batch, ``torch.optim.Adam`` with the reference's settings.  After
    every iteration the whole corpus is scored in eval mode as one batch; returns the first iteration count at which
    ``eer(scores, labels)`` is 0, or None."""
    import _corpus_features_ref as CF
    cfg = dict(cfg, SAMPLING_RATE=E2E_RATE)
    key = "mel" if feat_type == "mel" else "lin"
    feats = [CF.from_file_rate(y, rate, cfg)[0][key] for y, rate in list(bona) + list(spoof)]
    labels = np.array([1.0] * len(bona) + [0.0] * len(spoof))
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.Adam(list(sd.values()), lr=REF_HP[0], betas=REF_HP[1:3], eps=REF_HP[3], weight_decay=1e-4, amsgrad=True)
    batch = lambda idx: torch.from_numpy(CF.collate_pad([feats[i] for i in idx]))
    everything = batch(range(len(feats)))
    it, epoch = 0, 0
    while it < max_iterations:
        o = order(epoch)
        for at in range(0, len(o), batch_size):
            idx = o[at:at + batch_size]
            opt.zero_grad()
            loss, _ = bce(cm_forward(batch(idx), sd, feat_type)[1], torch.from_numpy(labels[idx]))
            loss.backward()
            opt.step()
            it += 1
            with torch.no_grad():
                scores = cm_forward(everything, sd, feat_type)[0].numpy()
            if eer(scores, labels) == 0.0:
                return it
            if it >= max_iterations:
                break
        epoch += 1
    return None


# ------------------------------------------------------------------------------------------------ the small whole classifier
CM_SHAPE = (24, 16, 3, 37)                      # freq_bins, disc_dim, B, T
# Seeds chosen on the CPU so that in float64 no leaky-ReLU input lies within KINK_MARGIN of its tensor's rms from zero, in eval mode and
# with the masks: an fp32 kernel and the reference then take the same side of every kink.  tests/test_countermeasure_cpu.py asserts it.
CM_SEEDS = {"mel": 3, "lin": 0}
KINK_MARGIN = 1e-4


def cm_case(kind, seed=None):
    """The committed case: (float32 state_dict, x (B, freq_bins, T), labels (B,), three float32 masks).  LayerNorm weights and biases and
    the conv biases are spread from their defaults so that each parameter's gradient is a value worth comparing."""
    from spoofsv_amd.countermeasure import CmLinDisc, CmMelDisc
    Fb, dim, B, T = CM_SHAPE
    torch.manual_seed(CM_SEEDS[kind] if seed is None else seed)
    disc = (CmLinDisc if kind == "lin" else CmMelDisc)(Fb, dim)
    with torch.no_grad():
        for name, p in disc.named_parameters():
            if ".ln" in "." + name or name.endswith("bias"):
                p.add_(0.3 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in disc.state_dict().items()}
    x = torch.rand(B, Fb, T)
    labels = torch.tensor([1.0, 0.0, 1.0])
    masks = [(torch.rand(s) >= 0.05).float() / 0.95 for s in mask_shapes(kind, B, dim, T)]
    return sd, x, labels, masks
