"""Records the fixture of tests/test_ivector_tv_cpu.py::test_host_trial_logic_is_the_reference_scripts: runs the reference's
kaldi_ivectors/local/split_data_enroll_eval.py and local/produce_trials.py, unmodified, on a tiny utt2spk and keeps what they read and
wrote as text lists under tests/golden/ivector_trials_*.txt.

    python tools/gen_ivector_trials_golden.py --reference <checkout of the reference project>

The utt2spk: 4 speakers in an order that is not sorted, their utterances interleaved, one speaker with fewer than 3 utterances (it
enrols everything and has no eval line) and one with exactly 3."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTT2SPK = ["S07_001 S07", "S02_001 S02", "S07_002 S07", "S11_004 S11", "S02_002 S02", "S07_003 S07", "S02_003 S02", "S05_001 S05", "S07_010 S07",
           "S11_001 S11", "S05_002 S05", "S02_004 S02", "S11_002 S11", "S07_004 S07", "S02_010 S02", "S11_003 S11", "S11_024 S11"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project (holds kaldi_ivectors/local/)")
    a = ap.parse_args()
    local = os.path.join(a.reference, "kaldi_ivectors", "local")
    out = os.path.join(ROOT, "tests", "golden")
    name = lambda part: os.path.join(out, "ivector_trials_%s.txt" % part)
    with open(name("utt2spk"), "w") as f:
        f.write("\n".join(UTT2SPK) + "\n")
    subprocess.run([sys.executable, os.path.join(local, "split_data_enroll_eval.py"), name("utt2spk"), name("enroll"), name("eval")], check=True)
    subprocess.run([sys.executable, os.path.join(local, "produce_trials.py"), name("eval"), name("trials")], check=True)
    for part in ("utt2spk", "enroll", "eval", "trials"):
        print(name(part), len(open(name(part)).read().splitlines()), "lines")


if __name__ == "__main__":
    main()
