"""Samples/s of ugp_relatives_closest / ugp_relatives_within (matUtils extract --closest-relatives / --within-distance on the device)
for every leaf of a synthetic MAT of the sars2 polytomy shape, beside the front end's own host path (`matutils-amd relatives
--host`: the reference's walk, statement by statement) on a small sample of the same leaves.

    python tools/bench_relatives.py [--nodes 10000000] [--host 64] [--reps 3] [--out profile.json]
Wall times are medians of --reps calls after one warm-up call; kernel times are device events around the launches, without the
copy to the host.  Prints one JSON line."""
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

BIG_RING = 100_000
MAX_FILL = 1 << 31   # list entries up to which the fill pass is timed


def leaf_counts(par):
    """Leaves below each node of a BFS-ordered tree (parents are nondecreasing, so each level is one contiguous range)."""
    n = len(par)
    levels, lo, hi = [], 0, 1
    while lo < n:
        levels.append((lo, hi))
        lo, hi = hi, int(np.searchsorted(par[1:], hi)) + 1 if hi < n else n
        if lo >= hi:
            break
    cnt = np.ones(n, np.int64)
    cnt[par[1:]] = 0
    for lo, hi in reversed(levels[1:]):
        np.add.at(cnt, par[lo:hi], cnt[lo:hi])
    return cnt


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def median_wall(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--host", type=int, default=64, help="samples of the host comparison (0: skip)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1, shape="sars2")
    arrays = st.arrays
    n = int(arrays["n"])
    par = np.maximum(np.asarray(arrays["parent"], np.int64), 0)
    nleaf = leaf_counts(par)
    has_kids = np.zeros(n, bool)
    has_kids[par[1:]] = True
    leaves = np.flatnonzero(~has_kids).astype(np.uint32)
    nl = len(leaves)
    rank = np.random.default_rng(7).permutation(n).astype(np.uint32)   # (any permutation costs the same)
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.relatives_attach(rank)
    out = {"nodes": n, "leaves": nl, "attach_s": round(time.perf_counter() - t0, 3), "reps": a.reps, "date": time.strftime("%Y-%m-%d"),
           "tool": "tools/bench_relatives.py"}
    say("attached", out["attach_s"])

    def record(key, wall, n_out, kernel):
        out[key] = {"wall_s": round(wall, 4), "samples_per_s": round(nl / wall, 1), "list_entries": int(n_out)}
        if kernel is not None:
            out[key]["kernel_count_ms"], out[key]["kernel_fill_ms"] = round(kernel[0], 3), round(kernel[1], 3)
        say(key, out[key])

    wall = median_wall(lambda: pl.relatives_closest(leaves, lists=False), a.reps)
    total = pl._rel_n_out
    record("closest_ranks_no_lists", wall, total, None)
    wall = median_wall(lambda: pl.relatives_closest(leaves), a.reps)
    record("closest_lists", wall, total, pl.relatives_time(leaves, False, 0, a.reps))
    for k in (2, 5):
        wall = median_wall(lambda: pl.relatives_within(leaves, k, lists=False), a.reps)
        total = pl._rel_n_out
        # (beyond MAX_FILL entries the fill pass is not timed: "kernel_*" are then absent)
        record("within%d_no_lists" % k, wall, total, pl.relatives_time(leaves, True, k, 1) if total <= MAX_FILL else None)
        if total <= 1 << 28:
            record("within%d_lists" % k, median_wall(lambda: pl.relatives_within(leaves, k), a.reps), total, None)
    pick = np.random.default_rng(5).choice(leaves, min(a.host, nl), replace=False)
    levels = pl.relatives_closest(pick, lists=False)[0]["levels"] if a.host else []
    pl.close()
    if a.host:
        # the samples whose closest-mode climb meets a ring of more than BIG_RING leaves: the levels the device reports, walked here
        n_big = 0
        for v, lv in zip(pick.tolist(), levels.tolist()):
            big = False
            for _ in range(lv):
                p = int(par[v])
                big |= int(nleaf[p] - nleaf[v]) > BIG_RING
                v = p
            n_big += big
        assert n_big >= min(8, len(pick)), "only %d of the host samples hang off a ring of more than %d leaves" % (n_big, BIG_RING)
        d = tempfile.mkdtemp(prefix="relatives_")
        pb, sf = os.path.join(d, "tree.pb"), os.path.join(d, "s.txt")
        time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
        open(sf, "w").write("".join("L%d\n" % j for j in pick))
        exe = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
        fe = {"samples": len(pick), "samples_on_big_rings": n_big}
        for name, opts in (("closest", ["-V", "o.tsv"]), ("within2", ["--within-distance", "o.tsv", "--distance-threshold", "2"])):
            ms, text = {}, {}
            for mode, extra in (("device", []), ("host", ["--host"])):
                r = subprocess.run([exe, "relatives", "-i", pb, "-s", sf, "-d", d] + opts + extra, capture_output=True, text=True)
                assert r.returncode == 0, r.stderr[-1000:]
                ms[mode] = float(re.search(r"Relatives of \d+ samples written in ([0-9.]+) msec", r.stderr).group(1))
                text[mode] = open(os.path.join(d, "o.tsv"), "rb").read()
            assert text["device"] == text["host"], name
            fe[name] = {"host_ms_per_sample": round(ms["host"] / len(pick), 3), "device_run_ms": ms["device"], "bytes": len(text["host"])}
            say(name, fe[name])
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
        out["front_end"] = fe
        # the comparison the figures are for: the host walk scaled to every leaf, beside the device call for every leaf
        out["closest_host_scaled_s"] = round(fe["closest"]["host_ms_per_sample"] * nl / 1e3, 1)
        out["closest_device_ms_per_sample"] = round(out["closest_lists"]["wall_s"] * 1e3 / nl, 6)
        out["within2_host_scaled_s"] = round(fe["within2"]["host_ms_per_sample"] * nl / 1e3, 1)
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
