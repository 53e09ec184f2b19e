"""Numpy reference of the curve counting (``ssv_sv_score_curve``, ``ssv_score_list_curve_*``) and of curve.py's two rate formulas.
Counts come from ``searchsorted`` over the sorted scores; a literal loop over thresholds is the second opinion (the CPU tests hold the two
together).  No torch: the tests compare it with the golden logs on one side and with the kernels on the other."""
import numpy as np

GE2E_THR = [0.0001 * i + 0.5 for i in range(5000)]
IVECTOR_THR = [-50 + 0.01 * i for i in range(8000)]


def _above(scores, thr):
    """Per threshold the scores with score > thr (strict, both in the scores' dtype; a NaN is above nothing): (K,) int64."""
    scores = np.asarray(scores).reshape(-1)
    thr = np.asarray(thr, dtype=np.float64).astype(scores.dtype)
    s = np.sort(scores[~np.isnan(scores)])
    return (s.size - np.searchsorted(s, thr, side="right")).astype(np.int64)


def _classes(sim, head, tail):
    """The four score sets of one matrix (N, V, N): everything, the own-speaker column, its first head rows, its last tail rows."""
    N, V = sim.shape[0], sim.shape[1]
    idx = np.arange(N)
    own = sim[idx, :, idx]                           # (N, V)
    return sim, own, own[:, :head], own[:, V - tail:]


def stack_counts(stack, thr, head, tail):
    """(nmat, K, 4) int64 for a float32 stack (nmat, N, V, N)."""
    stack = np.asarray(stack, dtype=np.float32)
    return np.stack([np.stack([_above(c, thr) for c in _classes(m, head, tail)], axis=1) for m in stack])


def stack_counts_loop(stack, thr, head, tail):
    stack = np.asarray(stack, dtype=np.float32)
    out = np.zeros((stack.shape[0], len(thr), 4), dtype=np.int64)
    for m, sim in enumerate(stack):
        cl = _classes(sim, head, tail)
        for t, th in enumerate(thr):
            th = np.float32(th)
            for k in range(4):
                out[m, t, k] = int((cl[k] > th).sum())
    return out


def list_counts(scores, cls, thr, nclass):
    """(K, nclass) int64: items of class c above each threshold; a class code >= nclass is counted nowhere."""
    scores, cls = np.asarray(scores), np.asarray(cls)
    return np.stack([_above(scores[cls == c], thr) for c in range(nclass)], axis=1)


def list_counts_loop(scores, cls, thr, nclass):
    scores, cls = np.asarray(scores), np.asarray(cls)
    out = np.zeros((len(thr), nclass), dtype=np.int64)
    for t, th in enumerate(thr):
        th = scores.dtype.type(th)
        for e in range(scores.size):
            if cls[e] < nclass and scores[e] > th:
                out[t, cls[e]] += 1
    return out


def ge2e_rates(head_count, tail_count, N, rows):
    """curve.py:21-22 in its float32 rounding sequence, widened to float64: (spoof_rate, gt_frr)."""
    head, tail = np.asarray(head_count).astype(np.float32), np.asarray(tail_count).astype(np.float32)
    spoof = tail / np.float32(rows) / np.float32(N)
    frr = (np.float32(N * rows) - head) / np.float32(rows) / np.float32(N)
    assert spoof.dtype == np.float32 and frr.dtype == np.float32
    return spoof.astype(np.float64), frr.astype(np.float64)


def ivector_rates(real_count, fake_count, L):
    """curve.py:48-49 in float64: (spoof_rate, gt_frr)."""
    real, fake = np.asarray(real_count, dtype=np.int64), np.asarray(fake_count, dtype=np.int64)
    return fake / L, 1 - real / L


def parse_scores(path, enroll=3, evl=20):
    """(real, fake) float64 arrays of a Kaldi score file by curve.py:32-39's rule, written out on its own."""
    real, fake = [], []
    for line in open(path):
        model, utt, score = line.split()
        if model != utt[:3]:
            continue
        if int(utt[-3:]) > enroll + evl:
            fake.append(float(score))
        else:
            real.append(float(score))
    return np.array(real), np.array(fake)
