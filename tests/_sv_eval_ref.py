"""Float64 numpy restatement of the verification test's device operators: the trial scores of ``ge2e_harness.cossim_eval`` on enrolment
centroids, the threshold sweep of ``ge2e_harness.eer_sweep`` with its table of counts, and the accept rate of ``spoof_rate_at``.
No torch: the tests compare it with the host functions on one side and with the kernels on the other."""
import numpy as np

EPS = 1e-8
THR64 = [0.01 * i + 0.5 for i in range(50)]
THR32 = np.array(THR64, dtype=np.float32)           # what the sweep compares a float32 matrix with


def _cos(a, b):
    """Cosine along the last axis with each norm clamped at EPS (torch.nn.functional.cosine_similarity)."""
    na = np.maximum(np.sqrt((a * a).sum(-1)), EPS)
    nb = np.maximum(np.sqrt((b * b).sum(-1)), EPS)
    return (a * b).sum(-1) / (na * nb)


def scores_ref(enr, ver, V=None):
    """(sim (N, V, N), cent (N, D)) in float64: enr (N, E, D), ver (N, Vs, D) of which the first V rows of every speaker are used."""
    enr, ver = np.asarray(enr, dtype=np.float64), np.asarray(ver, dtype=np.float64)
    V = ver.shape[1] if V is None else V
    ver = ver[:, :V]
    N = ver.shape[0]
    cent = enr.mean(axis=1)
    sim = _cos(ver[:, :, None, :], cent[None, None, :, :])
    loo = (ver.sum(axis=1, keepdims=True) - ver) / (V - 1)
    own = _cos(ver, loo)
    idx = np.arange(N)
    sim[idx, :, idx] = own
    return sim + 1e-6, cent


def sweep_constants(size_1, es1, spoof):
    """(head, tail, den, pos, hden, hpos): the reference's host-side divisions, float and integer where it has them."""
    hden, hpos = float(size_1 / 2 - es1 / 2), size_1 // 2 - es1 // 2
    if spoof:
        half = (size_1 - es1) // 2
        return half, half, float(size_1 - es1), size_1 - es1, hden, hpos
    return 0, 0, hden, hpos, hden, hpos


def counts_ref(sim, thr, head, tail):
    """(nthr, 4) int64: trials with sim > thr (strict, in sim's own dtype) over the matrix, the own column, its first head / last tail rows."""
    sim = np.asarray(sim)
    N, V = sim.shape[0], sim.shape[1]
    idx = np.arange(N)
    own = sim[idx, :, idx]                           # (N, V)
    out = np.zeros((len(thr), 4), dtype=np.int64)
    for t, th in enumerate(np.asarray(thr, dtype=sim.dtype)):
        out[t] = ((sim > th).sum(), (own > th).sum(), (own[:, :head] > th).sum(), (own[:, V - tail:] > th).sum())
    return out


def sweep_ref(sim, size_1, es1, spoof=True):
    """(dict of eer_sweep plus "best" and the per-threshold |FAR - FRR| under "diffs", counts): Python float arithmetic in eer_sweep's operation order."""
    sim = np.asarray(sim)
    N = sim.shape[0]
    head, tail, den, pos, hden, hpos = sweep_constants(size_1, es1, spoof)
    counts = counts_ref(sim, THR64, head, tail)
    best, cur, far_b, frr_b, diffs = 0, 1.0, None, None, []
    for t in range(len(THR64)):
        tot, own = float(counts[t, 0]), float(counts[t, 1])
        far = (tot - own) / (N - 1.0) / den / N
        frr = (N * pos - own) / den / N
        diffs.append(abs(far - frr))
        if t == 0:
            far_b, frr_b = far, frr
        if cur > abs(far - frr):
            cur, best, far_b, frr_b = abs(far - frr), t, far, frr
    out = dict(EER=(far_b + frr_b) / 2, thres=0.01 * best + 0.5, FAR=far_b, FRR=frr_b, best=best, diffs=diffs)
    if spoof:
        out["gt_FRR"] = (N * hpos - float(counts[best, 2])) / hden / N
        out["spoof_rate"] = float(counts[best, 3]) / hden / N
    return out, counts


def accept_rate_ref(stack, thres, eval_num):
    """Per matrix of the float32 stack (nmat, N, V, N): own-speaker trials of the last 2*eval_num rows above float32(thres), as the float32
    quotient count / float(tail) / N."""
    stack = np.asarray(stack, dtype=np.float32)
    N, tail = stack.shape[1], 2 * eval_num
    idx = np.arange(N)
    rates = []
    for m in stack:
        c = np.float32((m[idx, -tail:, idx] > np.float32(thres)).sum())
        rates.append(float(c / np.float32(tail) / np.float32(N)))
    return rates
