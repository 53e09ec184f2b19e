#!/usr/bin/env python3
"""curve.py's command line on the device: the spoof rate against the FRR of real speech, for a GE2E similarity matrix (5,000 thresholds)
and a Kaldi i-vector score file (8,000), counted in libssv_hip.so (``ge2e_harness.curve``).

    python tools/sv_curve.py --simmat simmat/simmat_e1_b1 --ivector_score scores.txt [--out DIR] [--N 20] [--eval_num 20] [--no-plot]

Writes DIR/curve.npz (spoof_rate_log, gt_frr_log, spoof_rate_log_2, gt_frr_log_2, thresholds, thresholds_2) and, when matplotlib is
installed, DIR/curve.png.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spoofsv_amd import ge2e_harness as GH                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--simmat", type=str, required=True, help="a similarity matrix as ge2e_harness.test saves it")
    ap.add_argument("--ivector_score", type=str, default=None, help="a Kaldi trial-score file (`<model speaker> <utterance> <score>` per line)")
    ap.add_argument("--out", type=str, default=".")
    ap.add_argument("--N", type=int, default=None, help="speakers per matrix (default: the configuration's test N)")
    ap.add_argument("--eval_num", type=int, default=20)
    ap.add_argument("--no-plot", action="store_true")
    a = ap.parse_args()
    cfg = GH.default_config()
    if a.N is not None:
        cfg["test"]["N"] = a.N
    out = GH.curve(cfg, a.simmat, a.ivector_score, out_dir=a.out, eval_num=a.eval_num, plot=False if a.no_plot else None)
    print("wrote %s: %d GE2E points, %d i-vector points" % (os.path.join(a.out, "curve.npz"), len(out["spoof_rate_log"]), len(out["spoof_rate_log_2"])))


if __name__ == "__main__":
    main()
