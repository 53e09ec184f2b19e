"""Writes tests/golden/dvector_host.npz: what the reference's own ``concat_segs`` and ``align_embeddings`` (GE2E/dvector_create.py:24-36,
:55-73) return on seeded inputs -- data only.  Run on the development machine with the reference checkout at hand:

    python tools/gen_dvector_golden.py --reference /path/to/reference

The script's top level needs librosa, webrtcvad and a config file in the working directory, so it is never imported: the two
``FunctionDef`` nodes are cut out of its syntax tree and compiled on their own (both are pure numpy).  Nothing imports this tool: not a
test, not smoke(), not bench.py.

Contents: ``part_off`` (601,), ``part_start`` / ``part_end`` int16 -- the partition list for n = 1 ... 600 window embeddings, entry n - 1
at [part_off[n - 1], part_off[n]) (read off ``align_embeddings``' output on index-valued rows, see ``partitions_of``);
``align_in_<k>`` / ``align_out_<k>`` float64 for 1, 7 and 40 rows x 256; ``concat_<c>_times`` (k, 2) float64, ``concat_<c>_sr_n`` (2,),
``concat_<c>_tags`` int32 and ``concat_<c>_lens``: the chunks are slices of ``np.arange(n)`` (every sample tagged with its own index),
cut as VAD_segments.py:138-149 cuts them, and the tags are ``concat_segs``' segments laid end to end.
"""
import argparse
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_functions(path, names=("concat_segs", "align_embeddings")):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in keep) == sorted(names), [n.name for n in keep]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def partitions_of(align_embeddings, n):
    """The partition list align_embeddings uses for n rows, read off its output: row i of the input is (i, i^2) in the first two
    columns, so a partition's average (mean of i, mean of i^2) names its first and last row."""
    x = np.zeros((n, 256))
    x[:, 0] = np.arange(n)
    x[:, 1] = np.arange(n) ** 2
    out = align_embeddings(x)
    parts = []
    start = 0
    for m1, m2 in out[:, :2]:
        # consecutive rows start .. end - 1: mean = (start + end - 1) / 2
        end = int(round(2 * m1 - start + 1))
        assert end > start and abs(np.mean(np.arange(start, end) ** 2) - m2) < 1e-6, (n, start, end)
        parts.append((start, end))
        start = end
    assert start == n
    return parts


def vad_chunks(intervals, sr, n):
    """VAD_segments.py:138-149 on (start, end) intervals, with the audio's samples tagged by their index."""
    audio = np.arange(n, dtype=np.int32)
    speech_times, speech_segs = [], []
    for time in intervals:
        start = np.round(time[0], decimals=2)
        end = np.round(time[1], decimals=2)
        j = start
        while j + .4 < end:
            end_j = np.round(j + .4, decimals=2)
            speech_times.append((j, end_j))
            speech_segs.append(audio[int(j * sr):int(end_j * sr)])
            j = end_j
        else:
            speech_times.append((j, end))
            speech_segs.append(audio[int(j * sr):int(end * sr)])
    return speech_times, speech_segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds GE2E/dvector_create.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dvector_host.npz"))
    a = ap.parse_args()
    concat_segs, align_embeddings = reference_functions(os.path.join(a.reference, "GE2E", "dvector_create.py"))
    out = {}
    off, starts, ends = [0], [], []
    for n in range(1, 601):
        parts = partitions_of(align_embeddings, n)
        starts += [p[0] for p in parts]
        ends += [p[1] for p in parts]
        off.append(len(starts))
    out["part_off"] = np.asarray(off, dtype=np.int32)
    out["part_start"] = np.asarray(starts, dtype=np.int16)
    out["part_end"] = np.asarray(ends, dtype=np.int16)
    for k, rows in enumerate((1, 7, 40)):
        x = np.random.default_rng(100 + k).standard_normal((rows, 256))
        out["align_in_%d" % k] = x
        out["align_out_%d" % k] = align_embeddings(x)
    cases = [
        (16000, 20000, [(0.0, 1.1)]),                                         # one interval, three chunks, one run
        (800, 4000, [(0.31, 1.74), (1.74, 2.2), (2.95, 3.3), (3.3, 4.4)]),    # touching intervals join; beyond n clips
        (800, 3000, [(0.5, 0.62)]),                                           # a single short chunk
        (800, 2400, [(0.0, 0.4), (0.8, 1.2), (1.2, 3.5)]),                    # an interval of exactly one chunk length; past the end
        (1000, 9000, None),
        (1000, 9000, None),
    ]
    rng = np.random.default_rng(7)
    for c, (sr, n, intervals) in enumerate(cases):
        if intervals is None:                                                 # seeded: sorted cut points, some intervals touching
            cuts = np.sort(np.round(rng.uniform(0, n / sr + 0.5, size=10), 2))
            intervals = [(cuts[i], cuts[i + 1]) for i in range(0, 9, 1) if rng.random() < 0.6 and cuts[i + 1] > cuts[i]]
            if not intervals:
                intervals = [(cuts[0], cuts[-1])]
        times, segs = vad_chunks(intervals, sr, n)
        res = concat_segs(times, segs)
        out["concat_%d_times" % c] = np.asarray(times, dtype=np.float64).reshape(-1, 2)
        out["concat_%d_sr_n" % c] = np.asarray([sr, n], dtype=np.int64)
        out["concat_%d_tags" % c] = np.concatenate([np.asarray(r, dtype=np.int32) for r in res]) if res else np.zeros(0, np.int32)
        out["concat_%d_lens" % c] = np.asarray([len(r) for r in res], dtype=np.int32)
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d bytes, %d arrays" % (a.out, os.path.getsize(a.out), len(out)))


if __name__ == "__main__":
    main()
