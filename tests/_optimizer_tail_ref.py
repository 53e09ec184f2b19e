"""Plain references of the optimizer tail (numpy, float64 / exact bit arithmetic, no torch kernels): one Adam step as the comment above
``adam_multi_kernel`` states it, and the resident hi / lo planes of one ``ssv_pack_job`` in the layout ``pack.hip`` documents."""
import collections

import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ Adam
AdamRef = collections.namedtuple("AdamRef", "p m v mag step_size denom")


def adam_step_ref(p, g, m, v, lr, b1, b2, eps, t):
    """m' = b1 m + (1-b1) g;  v' = b2 v + (1-b2) g^2;  denom = sqrt(v')/sqrt(1-b2^t) + eps;  p' = p - (lr/(1-b1^t)) m'/denom, in float64.
    The hyper-parameters are rounded to float32 first (the ABI takes floats).  Returns p', m', v' and the magnitudes the error bounds
    need: mag = |b1 m| + |(1-b1) g|, the step size and the denominator."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    t = int(t)
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    denom = np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps
    return AdamRef(p - step_size * m1 / denom, m1, v1, np.abs(b1 * m) + np.abs((1.0 - b1) * g), step_size, denom)


def adam_bounds(ref):
    """Single-step error bounds of a float32 evaluation against ``ref`` (tol_p, tol_m, tol_v).  The constants count the kernel's roundings:
    3 for m (two products, one sum), 4 for v, and for p sqrt, mul, add, div, mul, sub plus the two constants converted to float."""
    tol_m = 4 * U * ref.mag
    tol_v = 4 * U * ref.v
    tol_p = U * np.abs(ref.p) + 8 * U * ref.step_size * ref.mag / ref.denom
    return tol_p, tol_m, tol_v


def adam_fractions(p1, m1, v1, ref):
    """Worst used fraction of each bound and the index of the worst element, [(fp, i), (fm, i), (fv, i), (fu, i)].  An element whose bound
    is 0 (m = g = 0) must be exact: any error there counts as infinite.  The rounding of p' itself may use all of the first term of its
    bound, u |p'|, wherever the update is small beside p; fu is the part of the error beyond that term as a fraction of the update's
    term, 8u s mag / denom -- the figure that says how well the UPDATE is computed."""
    out = []
    for got, want, tol in zip((p1, m1, v1), (ref.p, ref.m, ref.v), adam_bounds(ref)):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err == 0, 0.0, err / tol)
        out.append((float(frac.max()), int(frac.argmax())))
    err = np.maximum(np.abs(np.asarray(p1, dtype=np.float64) - ref.p) - U * np.abs(ref.p), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / (8 * U * ref.step_size * ref.mag / ref.denom))
    out.append((float(frac.max()), int(frac.argmax())))
    return out


# ------------------------------------------------------------------------------------------------ planes
PackJobRef = collections.namedtuple("PackJobRef", "M K Kpad KT sm sk")


def align256(n):
    return (n + 255) & ~255


def split_bytes(rows, K, k):
    """Bytes of ONE plane (hi or lo) of a (rows, K) operand with k taps."""
    return align256(2 * k * ((rows + 15) // 16 * 16) * ((K + 31) // 32 * 32))


def plan_jobs_ref(Cout, Cin, k):
    """The forward and the transposed job of a torch-layout (Cout, Cin, k) weight and the byte offset of each job's planes in the weight's buffer
    (include/ssv_hip.h, "Resident pre-split weights"): [(job, offset)] * 2, then the buffer's size.  The two inverse scales sit in the last
    256 bytes, at +0 (forward) and +128 (transposed)."""
    fwd = PackJobRef(Cout, Cin, (Cin + 31) // 32 * 32, k, Cin * k, k)
    tr = PackJobRef(Cin, Cout, (Cout + 31) // 32 * 32, k, k, Cin * k)
    off_tr = 2 * split_bytes(Cout, Cin, k)
    return [(fwd, 0), (tr, off_tr)], off_tr + 2 * split_bytes(Cin, Cout, k) + 256


def plane_elems(job):
    return job.KT * ((job.M + 15) // 16) * (job.Kpad // 32) * 512


def lo_offset(job):
    """Byte offset of the lo plane behind the start of the hi plane."""
    return align256(2 * plane_elems(job))


def plane_index(t, m, k, job):
    """2-byte index of element (tap t, row m, column k) in a plane."""
    MB, NCH = (job.M + 15) // 16, job.Kpad // 32
    return ((((t * MB + m // 16) * NCH + k // 32) * 64 + ((k // 8) % 4) * 16 + m % 16) * 8 + k % 8)


def _grid(job):
    t, m, k = np.meshgrid(np.arange(job.KT), np.arange(job.M), np.arange(job.K), indexing="ij")
    return t.ravel().astype(np.int64), m.ravel().astype(np.int64), k.ravel().astype(np.int64)


def bf16_bits(x):
    """float32 -> bfloat16 bit patterns, round to nearest even (finite inputs)."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def pow2_scale(amax):
    """(sc, inv) = (2^(141-E), 2^(E-141)) as float32, E the biased exponent of ``amax`` clamped to [15, 254]."""
    E = int((np.float32(amax).view(np.uint32) >> 23) & 0xFF)
    E = min(max(E, 15), 254)
    return np.float32(2.0 ** (141 - E)), np.float32(2.0 ** (E - 141))


def split_values(x, mode, sc=None):
    """(hi bits, lo bits) of float32 values ``x`` (uint16 each); f16x2 takes the power-of-two scale ``sc``."""
    x = np.asarray(x, dtype=np.float32)
    if mode == "bf16x3":
        hi = bf16_bits(x)
        return hi, bf16_bits(x - bf16_value(hi))                      # x - hi is exact in float32
    if mode != "f16x2":
        raise ValueError(mode)
    with np.errstate(over="raise"):
        xs = x * np.float32(sc)                                       # exact: a power of two, no underflow in the tests' ranges
        hi = xs.astype(np.float16)                                    # IEEE: round to nearest even, gradual underflow
        lo = (xs - hi.astype(np.float32)).astype(np.float16)          # xs - hi is exact in float32
    return hi.view(np.uint16), lo.view(np.uint16)


def pack_planes_ref(w_flat, job, mode):
    """(hi, lo, inv): the two planes of ``job`` as uint16 arrays of ``plane_elems(job)`` entries each -- their bytes are the device's bytes,
    the lo plane ``lo_offset(job)`` bytes behind the hi plane -- and the inverse scale as float32 (None for bf16x3, which keeps none).
    Element (t, m, k) is w_flat[m*sm + k*sk + t]; padding is zero."""
    w_flat = np.asarray(w_flat, dtype=np.float32).ravel()
    t, m, k = _grid(job)
    x = w_flat[m * job.sm + k * job.sk + t]
    sc = inv = None
    if mode == "f16x2":
        sc, inv = pow2_scale(np.abs(w_flat[: job.M * job.K * job.KT]).max())
    h, l = split_values(x, mode, sc)
    hi = np.zeros(plane_elems(job), dtype=np.uint16)
    lo = np.zeros(plane_elems(job), dtype=np.uint16)
    idx = plane_index(t, m, k, job)
    hi[idx] = h
    lo[idx] = l
    return hi, lo, inv


def planes_value(hi, lo, mode):
    """float64 value hi + lo of plane entries."""
    if mode == "bf16x3":
        return bf16_value(hi).astype(np.float64) + bf16_value(lo).astype(np.float64)
    return np.asarray(hi, dtype=np.uint16).view(np.float16).astype(np.float64) + np.asarray(lo, dtype=np.uint16).view(np.float16).astype(np.float64)


def reconstruction_excess(x, hi, lo, mode, sc=None):
    """Worst |target - (hi+lo)| / bound over the elements: f16x2  2^-22 |x sc| + 2^-25,  bf16x3  2^-16 |x| (normal-range x)."""
    x = np.asarray(x, dtype=np.float64)
    if mode == "f16x2":
        xs = x * float(sc)
        err, tol = np.abs(xs - planes_value(hi, lo, mode)), 2.0 ** -22 * np.abs(xs) + 2.0 ** -25
    else:
        err, tol = np.abs(x - planes_value(hi, lo, mode)), 2.0 ** -16 * np.abs(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / tol)
    return float(frac.max()) if frac.size else 0.0


# The weights of one ssv_conv_pack_multi launch in the GPU test, (Cout, Cin, k): single elements, exact tiles, ragged rows (M % 16), ragged
# columns (K % 8, K % 32), the Cout = 513 layers of the workload (transposed K = 513: K % 8 = 1) and multiples of the tile.
PACK_SHAPES = [(1, 1, 1), (16, 32, 1), (17, 33, 3), (7, 9, 1), (9, 7, 3), (8, 8, 1), (40, 513, 1), (513, 40, 3), (256, 200, 1), (34, 128, 1),
               (64, 64, 3)]
