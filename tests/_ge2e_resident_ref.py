"""Plain numpy references for GE2E training on a resident corpus: the batch of GE2E/data_load.py:77-85 from a row table, and gradient
clipping per group + the SGD step (GE2E/train_speech_embedder.py:84-86) in float64, with the bounds a float32 evaluation is held to."""
import collections

import numpy as np

U = 2.0 ** -24                          # unit roundoff of float32

ClipSgdRef = collections.namedtuple("ClipSgdRef", "p norms coefs lr")


def gather_ref(corpus, rows):
    """``utters[utter_index]`` then ``np.transpose(.., (0, 2, 1))``, for global rows of the concatenated corpus (U_total, nmels, frames)."""
    return np.ascontiguousarray(np.asarray(corpus)[np.asarray(rows, dtype=np.int64)].transpose(0, 2, 1))


def clip_sgd_ref(groups, lr):
    """``groups``: [(list of (p, g) arrays, max_norm), ...].  Per group: total = sqrt(sum g^2), coef = min(1, max_norm / (total + 1e-6)),
    p' = p - lr * coef * g, all in float64; lr is rounded to float32 first (the ABI takes a float).  Returns per group the list of p',
    and the norms and coefficients."""
    lr = float(np.float32(lr))
    out, norms, coefs = [], [], []
    for pairs, max_norm in groups:
        max_norm = float(np.float32(max_norm))
        total = float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for _, g in pairs)))
        coef = min(1.0, max_norm / (total + 1e-6))
        out.append([np.asarray(p, dtype=np.float64) - lr * coef * np.asarray(g, dtype=np.float64) for p, g in pairs])
        norms.append(total)
        coefs.append(coef)
    return ClipSgdRef(out, norms, coefs, lr)


def clip_sgd_fraction(got, ref_p, g, lr, coef, k):
    """Worst used fraction of the bound ``U |ref| + k U lr coef |g|`` over one tensor, and its index.  k = 4 for the kernel (one rounding
    each for coef, step and the product, plus the subtraction's own share beyond U |ref|), 32 for torch's path, whose float32 tree norm
    over <= 2^22 elements adds about log2 n roundings.  An element whose bound is 0 must be exact: any error there counts as infinite."""
    got, ref_p, g = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref_p, g))
    err = np.abs(got - ref_p)
    tol = U * np.abs(ref_p) + k * U * lr * coef * np.abs(g)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / tol)
    return float(frac.max()), int(frac.argmax())
