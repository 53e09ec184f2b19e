"""Writes the fixtures of the spoof-rate / FRR curves by RUNNING the reference's own ``curve.py`` and
``kaldi_ivectors/ivector_spoofrate.py``, unmodified, from the reference checkout, on tiny seeded inputs:

    python tools/gen_sv_curve_golden.py /path/to/reference

  tests/golden/sv_curve_simmat.npy   the similarity matrix (N = 4, V = 80, N) float32 the script reads (it gets a torch.save'd copy)
  tests/golden/sv_curve_scores.txt   a Kaldi trial-score file: 3 model speakers x 3 utterance speakers x 46 utterances, five decimals
  tests/golden/sv_curve.npz          the script's four logs (spoof_rate_log, gt_frr_log, spoof_rate_log_2, gt_frr_log_2; float64), the
                                     planted thresholds (planted_up, planted_down: indices into the GE2E list) and what
                                     ivector_spoofrate.py prints for the score file (spoofrate_value at spoofrate_thres, with
                                     spoofrate_args = train_spk_num, enroll_utt_num, eval_utt_num)

Data only.  The scripts run through ``runpy`` in a temporary directory with a stand-in ``hparam`` module (hp.test.N = 4) on sys.path,
MPLBACKEND=Agg and sys.argv naming the inputs; curve.py needs matplotlib.  Nothing of their text is held here, and nothing imports this
tool: not a test, not smoke(), not bench.py.
"""
import argparse
import contextlib
import io
import os
import runpy
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, V, ROWS = 4, 80, 40
SPEAKERS, UTTS = ("225", "226", "227"), 46
SPOOFRATE_ARGS, SPOOFRATE_THRES = (105, 0, 23), -3.25        # 414 lines: total_num = 207 // 3 = 69 = 3 * 23; utterances 24 ... 46 spoof


def ge2e_thresholds():
    return [0.0001 * i + 0.5 for i in range(5000)]


def make_simmat(rng):
    """Own-speaker scores spread over the whole threshold range, genuine rows higher than spoofing rows; then, in both halves of the own
    column, scores EQUAL to the float32 rounding of a threshold whose rounding goes up and of one whose rounding goes down (the script's
    `sim > thres` compares in float32: rejected both times) and the next float32 above each (accepted)."""
    sim = (0.35 + 0.3 * rng.rand(N, V, N)).astype(np.float32)
    idx = np.arange(N)
    sim[idx, :ROWS, idx] = (0.62 + 0.36 * rng.rand(N, ROWS)).astype(np.float32)
    sim[idx, ROWS:, idx] = (0.48 + 0.42 * rng.rand(N, V - ROWS)).astype(np.float32)
    thr = ge2e_thresholds()
    up = [i for i, t in enumerate(thr) if float(np.float32(t)) > t]
    down = [i for i, t in enumerate(thr) if float(np.float32(t)) < t]
    planted_up, planted_down = [up[len(up) // 3], up[2 * len(up) // 3]], [down[len(down) // 3], down[2 * len(down) // 3]]
    for k, t_idx in enumerate(planted_up + planted_down):
        t32 = np.float32(thr[t_idx])
        spk = k % N
        for v0 in (3 + k, ROWS + 5 + k):                                # one pair in the genuine half, one in the spoofing half
            sim[spk, v0, spk] = t32
            sim[spk, v0 + 10, spk] = np.nextafter(t32, np.float32(2))
    return sim, planted_up, planted_down


def make_scores(rng):
    """`<model speaker> <utterance> <score>` lines as Kaldi's trial scoring writes them; utterance names <speaker>W<3 digits>.  A few
    own-speaker scores sit on two-decimal values, where the thresholds -50 + 0.01 i lie."""
    lines = []
    for model in SPEAKERS:
        for spk in SPEAKERS:
            for u in range(1, UTTS + 1):
                if model != spk:
                    s = -30.0 + 12.0 * rng.rand()
                elif u <= 23:
                    s = 2.0 + 9.0 * rng.randn()
                else:
                    s = -6.0 + 8.0 * rng.randn()
                if model == spk and u % 7 == 0:
                    s = round(s, 2)
                lines.append("%s %sW%03d %.5f\n" % (model, spk, u, s))
    return lines


@contextlib.contextmanager
def _script_run(argv, cwd):
    old_argv, old_cwd, old_path = sys.argv, os.getcwd(), list(sys.path)
    sys.argv = argv
    os.chdir(cwd)
    sys.path.insert(0, cwd)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            yield buf
    finally:
        sys.argv, sys.path[:] = old_argv, old_path
        os.chdir(old_cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="root of the reference checkout (holds curve.py and kaldi_ivectors/ivector_spoofrate.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    os.environ["MPLBACKEND"] = "Agg"
    rng = np.random.RandomState(1515)
    sim, planted_up, planted_down = make_simmat(rng)
    lines = make_scores(rng)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "hparam.py"), "w") as f:
            f.write("import types\nhparam = types.SimpleNamespace(test=types.SimpleNamespace(N=%d))\n" % N)
        simmat_path, score_path = os.path.join(tmp, "simmat"), os.path.join(tmp, "scores.txt")
        torch.save(torch.from_numpy(sim), simmat_path)
        with open(score_path, "w") as f:
            f.writelines(lines)
        with _script_run(["curve.py", "--simmat", simmat_path, "--ivector_score", score_path], tmp):
            g = runpy.run_path(os.path.join(a.reference, "curve.py"), run_name="__main__")
        train, enroll, evl = SPOOFRATE_ARGS
        argv = ["ivector_spoofrate.py", "-S", score_path, "--thres", repr(SPOOFRATE_THRES), "--train_spk_num", str(train), "--enroll_utt_num", str(enroll),
                "--eval_utt_num", str(evl)]
        with _script_run(argv, tmp) as printed:
            runpy.run_path(os.path.join(a.reference, "kaldi_ivectors", "ivector_spoofrate.py"), run_name="__main__")
    said = printed.getvalue().strip()
    assert said.startswith("Spoof Rate: "), said
    out = {k: np.asarray(g[k], dtype=np.float64) for k in ("spoof_rate_log", "gt_frr_log", "spoof_rate_log_2", "gt_frr_log_2")}
    assert out["spoof_rate_log"].shape == (5000,) and out["spoof_rate_log_2"].shape == (8000,)
    out.update(planted_up=np.array(planted_up), planted_down=np.array(planted_down), spoofrate_value=np.float64(float(said[len("Spoof Rate: "):])),
               spoofrate_thres=np.float64(SPOOFRATE_THRES), spoofrate_args=np.array(SPOOFRATE_ARGS))
    os.makedirs(a.out, exist_ok=True)
    np.savez_compressed(os.path.join(a.out, "sv_curve.npz"), **out)
    np.save(os.path.join(a.out, "sv_curve_simmat.npy"), sim)
    with open(os.path.join(a.out, "sv_curve_scores.txt"), "w") as f:
        f.writelines(lines)
    for name in ("sv_curve.npz", "sv_curve_simmat.npy", "sv_curve_scores.txt"):
        print("wrote %s: %d bytes" % (os.path.join(a.out, name), os.path.getsize(os.path.join(a.out, name))))
    print("GE2E: spoof rate %.4f ... %.4f, FRR %.4f ... %.4f; i-vector: spoof rate %.4f ... %.4f; ivector_spoofrate.py: %s"
          % (out["spoof_rate_log"][0], out["spoof_rate_log"][-1], out["gt_frr_log"][0], out["gt_frr_log"][-1], out["spoof_rate_log_2"][0],
             out["spoof_rate_log_2"][-1], said))


if __name__ == "__main__":
    main()
