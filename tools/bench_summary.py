"""Times of matUtils summary on the device (ugp_summary_attach / _mutations / _roho / _clades) on a synthetic MAT of the sars2
polytomy shape with a few thousand annotated nodes in two columns, beside the front end's own host path (`matutils-amd summarize
--host`: the reference's serial walks) on the same tree written as a .pb, and the bytes/s the occurrence-list sort and the RoHo
kernel reach against the bytes they have to move.

    python tools/bench_summary.py [--nodes 10000000] [--annotated 3000] [--reps 5] [--host-limit 600] [--out profiles/summary_bench.json]

Each call's time is the median of --reps runs after one warm-up run; the calls are synchronous (they end in a stream synchronise).
When `--host -R` does not end within --host-limit seconds at --nodes, the tool goes down the ladder 10M, 3M, 1M, 300k and reports
the largest size at which it does, with the device times at that same size.  Prints one JSON line."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_load  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402

EXE = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
KEY_BITS, RADIX_BITS = 41, 8


def median_s(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def tree(nodes):
    st = gsynth.SynthTree(nodes, n_sites=25000, seed=1, shape="sars2")
    arrays = st.arrays
    par = np.asarray(arrays["parent"], np.int64)
    inner = np.zeros(arrays["n"], bool)
    inner[par[1:]] = True
    return st, arrays, inner


def preorder(par):
    """Depth-first positions from a breadth-first parent array (levels are contiguous, parents ascend)."""
    n = len(par)
    levels, lo, hi = [], 0, 1
    while lo < hi:
        levels.append((lo, hi))
        lo, hi = hi, 1 + int(np.searchsorted(par[1:], hi, "left"))
    size = np.ones(n, np.int64)
    for a, b in reversed(levels[1:]):
        np.add.at(size, par[a:b], size[a:b])
    pre = np.zeros(n, np.int64)
    for a, b in levels[1:]:
        cs = np.cumsum(size[a:b]) - size[a:b]
        first = np.r_[True, par[a + 1:b] != par[a:b - 1]]
        start = np.maximum.accumulate(np.where(first, np.arange(b - a), 0))
        pre[a:b] = pre[par[a:b]] + 1 + cs - cs[start]
    return pre


def columns(arrays, inner, annotated):
    rng = np.random.default_rng(5)
    pool = np.flatnonzero(inner)
    k = min(annotated, len(pool))
    return [np.sort(rng.choice(pool, k, replace=False)), np.sort(rng.choice(pool, max(1, k // 3), replace=False))]


def device(arrays, inner, cols, reps):
    n, m = int(arrays["n"]), len(arrays["mut_pos"])
    cand = inner.copy()
    cand[0] = False
    ncand = int(np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))[cand].sum())
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.summary_attach()
    out = {"nodes": n, "entries": m, "candidates": ncand, "attach_s": round(time.perf_counter() - t0, 4)}
    recs = pl.summary_roho()
    out["mutations_s"] = round(median_s(pl.summary_mutations, reps), 5)
    out["roho_s"] = round(median_s(pl.summary_roho, reps), 5)
    out["clades_s"] = round(median_s(lambda: pl.summary_clades(cols), reps), 5)
    out["distinct_mutations"], out["roho_records"] = len(pl.summary_mutations()), len(recs)
    sort_ms, roho_ms = pl.summary_time(reps)
    # the sort: a histogram pass over the keys, then per digit a read and a write of every (8-byte key, 4-byte entry) pair
    passes = (KEY_BITS + RADIX_BITS - 1) // RADIX_BITS
    sort_bytes = 8 * m + passes * 2 * 12 * m
    # the RoHo kernel per candidate: its entry, the entry's node, parent, list position and run, the child's leaf count, the parent's
    # count of large children and the flag (29 B), plus per record the run bounds, a probe of the run, the median's elements and the
    # 24-byte record (about 72 B)
    roho_bytes = 29 * ncand + 72 * len(recs)
    out["sort"] = {"device_ms": round(sort_ms, 4), "bytes": sort_bytes, "bytes_per_s": round(sort_bytes / (sort_ms / 1e3), 1) if sort_ms else None,
                   "passes": passes}
    out["roho_kernel"] = {"device_ms": round(roho_ms, 4), "bytes": roho_bytes, "bytes_per_s": round(roho_bytes / (roho_ms / 1e3), 1) if roho_ms else None}
    pl.close()
    return out


def table_ms(stderr):
    """The front end's own per-table times."""
    return {what: int(ms) for what, ms in re.findall(r"Writing ([A-Za-z ]+?) to output [^\n]*\nCompleted in (\d+) msec", stderr)}


def front_end(st, arrays, inner, cols, limit):
    """`matutils-amd summarize` with and without --host on the tree written as a .pb and annotated through `annotate -C`."""
    d = tempfile.mkdtemp(prefix="summary_")
    pb, ann = os.path.join(d, "tree.pb"), os.path.join(d, "ann.pb")
    time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
    # the loader names internal nodes node_1 .. in depth-first preorder; leaves are L<j>
    order = np.argsort(preorder(np.asarray(arrays["parent"], np.int64))[inner])
    name = np.zeros(arrays["n"], np.int64)
    name[np.flatnonzero(inner)[order]] = np.arange(1, int(inner.sum()) + 1)
    src = pb
    for c, col in enumerate(cols):
        tsv = os.path.join(d, "c%d.tsv" % c)
        open(tsv, "w").write("".join("clade%d_%d\tnode_%d\n" % (c, i, name[v]) for i, v in enumerate(col)))
        r = subprocess.run([EXE, "annotate", "-i", src, "-o", "ann%d.pb" % c, "-C", tsv, "-d", d], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        src = os.path.join(d, "ann%d.pb" % c)
    os.replace(src, ann)
    out = {}
    fast = ["-m", "m.tsv", "-c", "c.tsv", "-C", "sc.tsv"]
    try:
        for mode, extra in (("device", []), ("host", ["--host"])):
            res = {}
            for what, args in (("tables", fast), ("roho", ["-R", "r.tsv"])):
                t0 = time.perf_counter()
                try:
                    r = subprocess.run([EXE, "summarize", "-i", ann, "-d", os.path.join(d, mode)] + args + extra, capture_output=True, text=True,
                                       timeout=limit)
                except subprocess.TimeoutExpired:
                    res[what] = {"timed_out_after_s": limit}
                    continue
                assert r.returncode == 0, r.stderr[-1000:]
                res[what] = {"wall_s": round(time.perf_counter() - t0, 2), "table_ms": table_ms(r.stderr)}
            out[mode] = res
        same = all(open(os.path.join(d, "device", f), "rb").read() == open(os.path.join(d, "host", f), "rb").read()
                   for f in ("m.tsv", "c.tsv", "sc.tsv", "r.tsv") if os.path.exists(os.path.join(d, "host", f)) and os.path.exists(os.path.join(d, "device", f)))
        out["same_bytes"] = bool(same)
        out["clade_rows"] = open(os.path.join(d, "device", "c.tsv")).read().count("\n") - 1
    finally:
        for root, _, files in os.walk(d, topdown=False):
            for f in files:
                os.remove(os.path.join(root, f))
            os.rmdir(root)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--annotated", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-limit", type=float, default=600.0, help="seconds a --host run may take (0: skip the front end)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"tool": "tools/bench_summary.py", "date": time.strftime("%Y-%m-%d"), "shape": "sars2", "reps": a.reps, "host_limit_s": a.host_limit}
    ladder = [a.nodes] + [s for s in (3_000_000, 1_000_000, 300_000) if s < a.nodes]
    for i, nodes in enumerate(ladder):
        st, arrays, inner = tree(nodes)
        cols = columns(arrays, inner, a.annotated)
        dev = device(arrays, inner, cols, a.reps)
        dev["annotated_nodes"] = [len(c) for c in cols]
        if i == 0:
            out["device"] = dev
        if not a.host_limit:
            break
        fe = front_end(st, arrays, inner, cols, a.host_limit)
        if i == 0:
            out["front_end"] = fe
        if "timed_out_after_s" not in fe["host"]["roho"]:
            if i:
                out["host_roho_largest"] = {"device": dev, "front_end": fe}
            break
        st.close()
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
