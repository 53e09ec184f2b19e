#!/usr/bin/env python
"""Dump every host-side answer of libssv_hip.so that a caller sizes a buffer or plans a launch by, as JSON: the 31 size_t queries
of include/ssv_hip.h (``*_workspace`` / ``*_bytes``), ssv_conv1d_bwd_weight_multi_ok / _multi_splits, ssv_ln_bwd_partial_rows and the
job table of ssv_conv_pack_plan, for each arithmetic mode, over shapes that sit on both sides of every branch of the host layer.
No GPU is touched.  Two builds answer alike exactly when their dumps are equal:

    python tools/dump_host_queries.py --lib other/libssv_hip.so > a.json
    python tools/dump_host_queries.py > b.json && cmp a.json b.json

tests/golden/host_queries.json is ``--precision 2`` of this tool (tests/test_abi_cpu.py regenerates and compares it): a workspace
size or a plan changes by editing that fixture, not by accident."""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_VARS = ("SSV_NT_FORCE", "SSV_NNB_FORCE", "SSV_LN_GROUPS", "SSV_LN_PERSIST", "SSV_LSTM_MERGE", "SSV_PWLN_BWD")

# Channel counts at the edges of SSV_MIN_SPLIT_CHANNELS (32), M % 128 == 1 (129, 513, 641) and Cout <= 640; (Cin, Cout) pairs of them.
CHANNELS = (16, 32, 80, 129, 256, 513, 640, 641)
CH_PAIRS = ((16, 16), (32, 32), (80, 256), (129, 129), (256, 512), (513, 256), (256, 513), (513, 513), (640, 640), (32, 641), (641, 641))
# B * L on both sides of 128 (124 | 186) and 256 (186 | 256), one column, many columns
BL = ((1, 31), (1, 186), (4, 31), (4, 64), (4, 325), (32, 1), (32, 186), (32, 325))
KS = (1, 3)
LSTM = ((8, 4, 40, 32, 1), (8, 4, 40, 20, 1), (64, 6, 40, 64, 3), (70, 5, 33, 96, 2), (880, 120, 40, 768, 3))      # (Bn, T, F, H, layers); H = 20: H % 8 != 0
# queries whose arguments are none of (B, L, C, Cin, Cout, k, njobs): their cases, by argument names
EXPLICIT = {
    ("B", "d", "N", "T"): ((1, 64, 20, 33), (4, 256, 31, 64), (32, 256, 186, 325)),
    ("B", "N", "T"): ((1, 20, 33), (32, 186, 325)),
    ("Bn", "T", "F", "H", "layers"): LSTM,
    ("Bn", "P"): ((8, 16), (70, 33), (880, 256)),
    ("N", "M", "D"): ((4, 5, 64), (88, 10, 256)),
    ("n",): ((1,), (1000,), (3328000,)),
    ("B", "n"): ((1, 1000), (32, 104000)),
    ("njobs",): ((2,), (20,), (222,)),
}
DOMAIN = {"k": KS, "njobs": (1, 10), "gate": (0, 1), "with_amax": (0, 1)}


def cases(argnames):
    """Argument tuples for a query, from the names of its parameters."""
    names = tuple(argnames)
    if names in EXPLICIT:
        return list(EXPLICIT[names])
    groups = []                                   # (names of the group, its value tuples)
    if "Cin" in names:
        groups.append((("Cin", "Cout"), CH_PAIRS))
    if "C" in names:
        groups.append((("C",), tuple((c,) for c in CHANNELS)))
    if "B" in names and "L" in names:
        groups.append((("B", "L"), BL))
    elif "B" in names:
        groups.append((("B",), ((1,), (4,), (32,))))
    for n in names:
        if n in DOMAIN:
            groups.append(((n,), tuple((v,) for v in DOMAIN[n])))
    covered = [n for g, _ in groups for n in g]
    assert sorted(covered) == sorted(names), (names, covered)
    out = []
    for combo in itertools.product(*(vals for _, vals in groups)):
        d = {}
        for (gnames, _), vals in zip(groups, combo):
            d.update(zip(gnames, vals))
        out.append(tuple(d[n] for n in names))
    return out


def pack_plan(L, PackJob):
    """Job table of ssv_conv_pack_plan for one weight of every (channel pair, k): pointers as the fake addresses given."""
    weights = [(co, ci, k) for (ci, co) in CH_PAIRS for k in KS]
    n = len(weights)
    vp = ctypes.c_void_p
    base, planes = 0x10000000, []
    for co, ci, k in weights:
        planes.append(base)
        base += int(L.ssv_conv_pack_bytes(co, ci, k))
    jobs = (PackJob * (2 * n))()
    nblocks = L.ssv_conv_pack_plan(n, (vp * n)(*[0x1000 * (i + 1) for i in range(n)]), (vp * n)(*planes), (ctypes.c_int * n)(*[w[0] for w in weights]),
                                   (ctypes.c_int * n)(*[w[1] for w in weights]), (ctypes.c_int * n)(*[w[2] for w in weights]), jobs)
    fields = ["w", "planes", "M", "K", "Kpad", "KT", "sm", "sk", "first_block", "inv_out"]
    return {"weights": weights, "nblocks": nblocks, "fields": fields, "jobs": [[getattr(j, f) for f in fields] for j in jobs]}


def collect(precisions=(0, 1, 2)):
    """{str(precision): {query: {"args": [...], "rows": [[args..., answer], ...]}, ..., "ssv_conv_pack_plan": {...}}}.  Leaves the process as it found it."""
    from spoofsv_amd import _lib
    L = _lib.lib()
    protos = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIBPATH)
    # buffer sizes in bytes only: a size_t that counts something else (ssv_fft_tables_floats) is no workspace query
    queries = sorted(n for n, (ret, _, _) in protos.items() if ret is ctypes.c_size_t and n.endswith(("_workspace", "_bytes")))
    assert len(queries) == 31, queries
    queries += ["ssv_conv1d_bwd_weight_multi_ok", "ssv_conv1d_bwd_weight_multi_splits", "ssv_ln_bwd_partial_rows"]
    saved_env = {v: os.environ.pop(v) for v in TUNING_VARS if v in os.environ}
    raw.ssv_reload_tuning()
    prev = L.ssv_get_precision()
    out = {}
    try:
        for p in precisions:
            L.ssv_set_precision(p)
            res = {}
            for q in queries:
                names = protos[q][2]
                fn = getattr(L, q)
                res[q] = {"args": list(names), "rows": [list(a) + [int(fn(*a))] for a in cases(names)]}
            res["ssv_conv_pack_plan"] = pack_plan(L, _lib.PackJob)
            out[str(p)] = res
    finally:
        L.ssv_set_precision(prev)
        os.environ.update(saved_env)
        raw.ssv_reload_tuning()
    return json.loads(json.dumps(out))              # tuples -> lists, as a reader of the file sees them


def render(d):
    """One line per query: small, and a diff names the query that moved."""
    parts = []
    for p in sorted(d):
        lines = ",\n".join("  %s: %s" % (json.dumps(q), json.dumps(d[p][q], separators=(",", ":"))) for q in sorted(d[p]))
        parts.append(" %s: {\n%s\n }" % (json.dumps(p), lines))
    return "{\n%s\n}\n" % ",\n".join(parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", help="another build of libssv_hip.so to ask (default: the package's)")
    ap.add_argument("--precision", type=int, action="append", choices=(0, 1, 2), help="only this arithmetic mode (repeatable; default: all three)")
    a = ap.parse_args()
    if a.lib:
        os.environ["SSV_HIP_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    sys.stdout.write(render(collect(tuple(a.precision or (0, 1, 2)))))


if __name__ == "__main__":
    main()
