"""Times of matUtils summary --haplotype on the device (ugp_haplotypes_attach / ugp_haplotype_groups / _sets) on a synthetic MAT of
the sars2 polytomy shape, beside the front end's own host path (`matutils-amd haplotypes --host`: the reference's walk with a
std::map per node) on the same tree written as a .pb.

    python tools/bench_haplotypes.py [--nodes 10000000] [--reps 5] [--host-limit 240] [--out profiles/haplotypes_bench.json]

Each call's time is the median of --reps runs after one warm-up run; the calls are synchronous (they end in a stream synchronise).
The passes (scan, sort, verify) are device times from ugp_haplotype_time.  When `--host` does not end within --host-limit seconds
at --nodes, or is killed for its memory, the tool measures the front end again at 1,000,000 nodes and says so.  Prints one JSON line."""
import argparse
import json
import os
import re
import resource
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
HOST_BYTES = 40 << 30   # address space of the --host run: its maps must not take the machine's memory


def median_s(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def topology(arrays):
    n = int(arrays["n"])
    return {"n": n, "parent": arrays["parent"], "mut_off": np.zeros(n + 1, np.int64), "mut_pos": np.zeros(0, np.int32),
            "mut_ref": np.zeros(0, np.int8), "mut_par": np.zeros(0, np.int8), "mut_nuc": np.zeros(0, np.int8)}


def device(arrays, reps):
    n, m = int(arrays["n"]), len(arrays["mut_pos"])
    pl = Placer(topology(arrays))
    t0 = time.perf_counter()
    pl.haplotypes_attach(arrays)
    out = {"nodes": n, "entries": m, "attach_s": round(time.perf_counter() - t0, 4)}
    groups, info = pl.haplotype_groups()
    out.update(leaves=int(info["n_leaves"]), groups=len(groups), groups_of_several=int((groups["count"] > 1).sum()),
               largest_group=int(groups["count"].max()), largest_set=int(groups["size"].max()), verify_entries_visited=int(info["n_visited"]),
               verify_pairs=int(info["n_leaves"]) - len(groups))
    out["groups_s"] = round(median_s(pl.haplotype_groups, reps), 5)
    scan_ms, sort_ms, verify_ms = pl.haplotype_time(reps)
    out["passes_ms"] = {"scan": round(scan_ms, 4), "sort": round(sort_ms, 4), "verify": round(verify_ms, 4)}
    reps_leaves = np.ascontiguousarray(groups["leaf"])
    off, pos, nuc = pl.haplotype_sets(reps_leaves)
    out["set_entries_of_representatives"] = int(off[-1])
    del pos, nuc
    out["sets_of_representatives_s"] = round(median_s(lambda: pl.haplotype_sets(reps_leaves), max(1, min(reps, 2))), 4)
    pl.close()
    return out


def front_end(st, limit):
    """`matutils-amd haplotypes` with and without --host on the tree written as a .pb."""
    d = tempfile.mkdtemp(prefix="haplotypes_")
    pb = os.path.join(d, "tree.pb")
    time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
    out = {}
    try:
        for mode, extra in (("device", []), ("host", ["--host"])):
            t0 = time.perf_counter()
            try:
                cap = (lambda: resource.setrlimit(resource.RLIMIT_AS, (HOST_BYTES, HOST_BYTES))) if extra else None
                r = subprocess.run([EXE, "haplotypes", "-i", pb, "-H", "hap.tsv", "-d", os.path.join(d, mode)] + extra, capture_output=True, text=True,
                                   timeout=limit, preexec_fn=cap)
            except subprocess.TimeoutExpired:
                out[mode] = {"timed_out_after_s": limit}
                continue
            if r.returncode != 0:
                out[mode] = {"failed_with": r.returncode, "stderr": r.stderr[-300:]}
                continue
            ms = re.search(r"Writing haplotype frequencies[^\n]*\nCompleted in (\d+) msec", r.stderr)
            out[mode] = {"wall_s": round(time.perf_counter() - t0, 2), "table_ms": int(ms.group(1)) if ms else None,
                         "fell_back": "walking it on the host" in r.stderr}
        files = [os.path.join(d, mode, "hap.tsv") for mode in ("device", "host")]
        if all("wall_s" in out[mode] for mode in ("device", "host")):
            out["same_bytes"] = open(files[0], "rb").read() == open(files[1], "rb").read()
        if os.path.exists(files[0]):
            out["table_bytes"] = os.path.getsize(files[0])
    finally:
        for root, _, files in os.walk(d, topdown=False):
            for f in files:
                os.remove(os.path.join(root, f))
            os.rmdir(root)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-limit", type=float, default=240.0, help="seconds a front-end run may take (0: skip the front end)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"tool": "tools/bench_haplotypes.py", "date": time.strftime("%Y-%m-%d"), "shape": "sars2", "reps": a.reps, "host_limit_s": a.host_limit}
    for i, nodes in enumerate([a.nodes] + ([1_000_000] if a.nodes > 1_000_000 else [])):
        st = gsynth.SynthTree(nodes, n_sites=25000, seed=1, shape="sars2")
        dev = device(st.arrays, a.reps)
        if i == 0:
            out["device"] = dev
        if not a.host_limit:
            break
        fe = front_end(st, a.host_limit)
        if i == 0:
            out["front_end"] = fe
        else:
            out["host_walk_at_1m"] = {"device": dev, "front_end": fe}
        st.close()
        if "wall_s" in fe["host"]:
            break
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
