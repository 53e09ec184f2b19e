#!/usr/bin/env python3
"""The stages of an i-vector extractor EM iteration, the project's kernels beside the same mathematics on torch's stock operators, on one
device at the shape of the recipe's extractor but for its rank and corpus: synthetic statistics drawn from the model, C = 1024, D = 60,
R = 192 (the most the E-step's LDS triangle holds; the sid scripts' default is 400), 2,000 utterances.

  E-step          TotalVariability.estep with M (2 x ssv_ivec_product,  | float32 matmul for Lp and b, the triangle scattered into a dense
                  ssv_ivec_estep)                                       |   float64 (U, R, R), batched linalg.cholesky, cholesky_solve,
                                                                        |   cholesky_inverse, M gathered back to the packed float32 form
  accumulate +    3 x ssv_ivec_product_tn, ssv_ivec_tv_update with a    | float32 matmul for A and Cm (then widened), batched float64
  update          given J                                               |   cholesky + cholesky_solve per Gaussian, @ J
  EM step         TotalVariability.em_step (the two above, sum M, J on  | the two above, J = linalg.cholesky(mean M) on the device, the
                  the host, the planes of the new T)                    |   planes of the new T by einsum

The stock forms are written here for the comparison alone.  Each of their batched factorisation calls is followed by a device
synchronisation: queued back to back, torch's batched cholesky / cholesky_solve / cholesky_inverse returned garbage that changed from run to
run here (each alone, or with a host read between them, is exact to 1e-15), and a comparison against a form that computes something
else measures nothing.  The three waits are inside the stock forms' time.  The forms alternate block by block in ONE process, each timed with device
events around the whole stage after an untimed first call; the figure is the median over the blocks (at least 7).  The outputs are compared
inside the run.  No device: the tool fails, it measures nothing on a CPU.

    python tools/bench_ivector.py [--blocks 7] [--utts 2000] [--out profiles/ivector.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spoofsv_amd import _lib, ivector, ops                                      # noqa: E402

DEV = "cuda:0"
C, D, R, MIN_COUNT = 1024, 60, 192, 10.0
P = R * (R + 1) // 2
F32, F64 = torch.float32, torch.float64


def make_case(U, seed=0):
    """Statistics drawn from the model on the device (set-up, not timed): N_u = frames x a soft max of 3 z over the Gaussians, F_uc =
    N_uc (mu_c + T_c w_u) + sqrt(N_uc var_c) z, centred by ssv_ivec_centre_stats.  Returns (N, Ft, w_ubm, mu, var, T0)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=F64)
    mu, var = 2 * rn(C, D), 0.5 + 1.5 * torch.rand(C, D, generator=g, device=DEV, dtype=F64)
    T_true = 0.3 * var.sqrt()[:, :, None] * rn(C, D, R)
    frames = 80 + 320 * torch.rand(U, 1, generator=g, device=DEV, dtype=F64)
    N = frames * torch.softmax(3 * rn(U, C), dim=1)
    mean = mu[None] + torch.einsum("cdr,ur->ucd", T_true, rn(U, R))
    F = N[:, :, None] * mean + (N[:, :, None] * var[None]).sqrt() * rn(U, C, D)
    w = torch.full((C,), 1.0 / C, dtype=F64, device=DEV)
    T0 = 0.1 * var.sqrt()[:, :, None] * rn(C, D, R)
    N, F = N.float().contiguous(), F.float().contiguous()
    tv = ivector.TotalVariability(T0, w, mu, var)
    return N, ivector.centre_stats(tv, N, F, out=F).view(U, C * D), w, mu, var, T0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ivector.txt"))
    a = ap.parse_args()
    if a.blocks < 7:
        ap.error("--blocks must be at least 7")
    if not torch.cuda.is_available():
        sys.exit("bench_ivector: no ROCm device; nothing is measured on a CPU")
    U = a.utts
    N, Ft, w_ubm, mu, var, T0 = make_case(U)
    tv0 = ivector.TotalVariability(T0, w_ubm, mu, var)
    G, Pk = tv0.planes()
    ti, tj = (t.to(DEV) for t in torch.tril_indices(R, R))
    eye = torch.eye(R, dtype=F64, device=DEV)
    ones = torch.ones((U, 1), dtype=F32, device=DEV)
    kept = {}

    def stock_estep(Pk_, G_):
        Lp, b = N @ Pk_, Ft @ G_
        L = torch.zeros((U, R, R), dtype=F64, device=DEV)
        L[:, ti, tj] = Lp.double()
        Cf = torch.linalg.cholesky(L + torch.tril(L, -1).transpose(1, 2) + eye)
        torch.cuda.synchronize()
        b64 = b.double()
        w = torch.cholesky_solve(b64[:, :, None], Cf)[:, :, 0]
        torch.cuda.synchronize()
        obj = -torch.log(torch.diagonal(Cf, dim1=1, dim2=2)).sum(1) + 0.5 * (b64 * w).sum(1)
        Linv = torch.cholesky_inverse(Cf)
        torch.cuda.synchronize()
        M = (Linv + w[:, :, None] * w[:, None, :])[:, ti, tj].float()
        return w.float(), M, obj

    def stock_update(w, M, J, T):
        A, Cm, Nc = (N.T @ M).double(), (Ft.T @ w).double().view(C, D, R), N.double().sum(0)
        Af = torch.zeros((C, R, R), dtype=F64, device=DEV)
        Af[:, ti, tj] = A
        Cf = torch.linalg.cholesky(Af + torch.tril(Af, -1).transpose(1, 2))
        torch.cuda.synchronize()
        Tn = torch.cholesky_solve(Cm.transpose(1, 2).contiguous(), Cf)
        torch.cuda.synchronize()
        Tn = Tn.transpose(1, 2) @ J
        return torch.where((Nc < MIN_COUNT)[:, None, None], T, Tn)

    def ours_e():
        kept["oe"] = tv0.estep(N, Ft, want_M=True)

    def stock_e():
        kept["se"] = stock_estep(Pk, G)

    def ours_u():
        e = kept["oe"]
        A = torch.zeros((C, P), dtype=F64, device=DEV)
        Cm = torch.zeros((C * D, R), dtype=F64, device=DEV)
        Nc = torch.zeros((C, 1), dtype=F64, device=DEV)
        ivector.product_tn(N, e.M, A)
        ivector.product_tn(Ft, e.w, Cm)
        ivector.product_tn(N, ones, Nc)
        T = T0.clone()
        _lib.call("ssv_ivec_tv_update", ops._p(A), ops._p(Cm), ops._p(Nc), ops._p(kept["J"]), ops._p(T), C, D, R, MIN_COUNT, ops._stream())
        kept["ou"] = T

    def stock_u():
        w, M, _ = kept["se"]
        kept["su"] = stock_update(w, M, kept["J"], T0)

    def ours_em():
        fresh = ivector.TotalVariability(T0, w_ubm, mu, var)
        fresh.planes()
        kept["oem"] = (fresh.em_step(N, Ft, True, MIN_COUNT), fresh)

    def stock_em():
        Gs = (T0 / var[:, :, None])
        Pks = torch.einsum("cdi,cdj->cij", T0, Gs)[:, ti, tj].float()
        w, M, obj = stock_estep(Pks, Gs.reshape(C * D, R).float())
        Mbar = torch.zeros((R, R), dtype=F64, device=DEV)
        Mbar[ti, tj] = M.double().sum(0) / U
        Tn = stock_update(w, M, torch.linalg.cholesky(Mbar + torch.tril(Mbar, -1).T), T0)
        Gn = Tn / var[:, :, None]
        kept["sem"] = (obj.sum() / U, Tn, Gn.reshape(C * D, R).float(), torch.einsum("cdi,cdj->cij", Tn, Gn)[:, ti, tj].float())

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    ours_e()
    kept["J"] = torch.from_numpy(np.linalg.cholesky(ivector.tri_unpack(ivector.DiagUbm.reduce(kept["oe"].M).cpu().numpy() / U, R))).to(DEV).contiguous()
    forms = [("E-step      ours ", ours_e), ("E-step      stock", stock_e), ("acc+update  ours ", ours_u), ("acc+update  stock", stock_u),
             ("EM step     ours ", ours_em), ("EM step     stock", stock_em)]
    for _, fn in forms:
        fn()                                                             # untimed: code objects, the allocator, the library's algorithm choice
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(a.blocks):
        for name, fn in forms:
            times[name].append(timed(fn))
    oe, (sw, sM, sobj) = kept["oe"], kept["se"]
    d_w = float((oe.w - sw).abs().max() / sw.abs().max())
    d_M = float((oe.M - sM).abs().max() / sM.abs().max())
    d_obj = float(((oe.obj - sobj).abs() / sobj.abs().clamp_min(1.0)).max())
    d_T = float((kept["ou"] - kept["su"]).abs().max() / kept["su"].abs().max())
    d_em = abs(float(kept["oem"][0]) - float(kept["sem"][0])) / abs(float(kept["sem"][0]))
    d_Tem = float((kept["oem"][1].T - kept["sem"][1]).abs().max() / kept["sem"][1].abs().max())
    # both against float64 on the host (LAPACK) for the first 64 utterances, from the same float32 planes
    L64 = torch.zeros((64, R, R), dtype=F64, device=DEV)
    L64[:, ti, tj] = N[:64].double() @ Pk.double()
    L64 = (L64 + torch.tril(L64, -1).transpose(1, 2) + eye).cpu()
    w64 = torch.linalg.solve(L64, (Ft[:64].double() @ G.double()).cpu())
    r_ours, r_stock = (float((t[:64].double().cpu() - w64).abs().max() / w64.abs().max()) for t in (oe.w, sw))
    med = {name: statistics.median(t) for name, t in times.items()}
    flop_e = 2.0 * U * C * P + 2.0 * U * C * D * R
    lines = ["I-vector extractor EM stages: milliseconds per stage, median of %d blocks (min .. max), device events, forms alternating in one process" % a.blocks,
             "U = %d utterances, C = %d, D = %d, R = %d (P = %d); product runs of %d, tiles of %d; %s, torch %s"
             % (U, C, D, R, P, _lib.lib().ssv_ivec_product_run(), _lib.lib().ssv_ivec_product_tile(), torch.cuda.get_device_name(0), torch.__version__), ""]
    for k in range(0, len(forms), 2):
        (n0, _), (n1, _) = forms[k], forms[k + 1]
        for n in (n0, n1):
            t = times[n]
            lines.append("  %-20s %10.3f ms  (%.3f .. %.3f)" % (n, med[n], min(t), max(t)))
        lines.append("  %-20s x%.3g" % ("stock / ours", med[n1] / med[n0]))
    lines += ["",
              "dense arithmetic of the two E-step products (N Pk and Ft G, %.1f GFLOP) over our whole E-step time: %.1f TFLOP/s; the two accumulations "
              "are the same count" % (flop_e / 1e9, flop_e / med[forms[0][0]] / 1e9),
              "agreement (ours against stock, relative to the largest entry): w %.3e, M %.3e, obj %.3e; T after accumulate + update %.3e; "
              "EM step: mean objective %.3e, T %.3e" % (d_w, d_M, d_obj, d_T, d_em, d_Tem),
              "w of the first 64 utterances against a float64 solve on the host: ours %.3e, stock %.3e of the largest entry" % (r_ours, r_stock)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not (d_w < 1e-2 and d_M < 1e-2 and d_obj < 1e-4 and d_T < 1e-3 and d_em < 1e-4 and d_Tem < 1e-3):
        sys.exit("bench_ivector: the forms disagree")


if __name__ == "__main__":
    main()
