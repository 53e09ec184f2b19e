"""Writes tests/golden/countermeasure_lindisc.npz: what the reference's own ``anti_spoofing/discriminator.linDisc`` computes in float64 and
eval mode on a fixed small input -- data only (weights, input, output; a few KB).  Run with the reference checkout at hand:

    python tools/gen_countermeasure_golden.py /path/to/reference

The reference module is imported from the given directory (it needs torch only); nothing of its text is held here.  ``melDisc`` has no
fixture: its ``ln4 = LayerNorm(4)`` behind an 8-channel ``conv4`` raises at the first forward.  Nothing imports this tool: not a test,
not smoke(), not bench.py.

Contents: ``x`` (3, 24, 37) float64, ``y`` (3, 1, 1) float64 = linDisc(24, 16).double().eval()(x), ``sd.<name>`` the state dict.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQ_BINS, DISC_DIM, B, T = 24, 16, 3, 37


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="root of the reference checkout (holds anti_spoofing/discriminator.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "countermeasure_lindisc.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "anti_spoofing"))
    disc = importlib.import_module("discriminator")
    torch.manual_seed(20)
    model = disc.linDisc(FREQ_BINS, DISC_DIM).double().eval()
    with torch.no_grad():
        # the default initialisation leaves every LayerNorm at (1, 0) and the biases small: spread them, so that each parameter matters
        for name, p in model.named_parameters():
            if ".ln" in "." + name or name.endswith("bias"):
                p.add_(0.3 * torch.randn_like(p))
        x = torch.rand(B, FREQ_BINS, T, dtype=torch.float64)
        y = model(x)
    out = {"x": x.numpy(), "y": y.numpy()}
    for k, v in model.state_dict().items():
        out["sd." + k] = v.numpy()
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d bytes, %d arrays, y = %s" % (a.out, os.path.getsize(a.out), len(out), y.view(-1).tolist()))


if __name__ == "__main__":
    main()
