"""Queries/s of ugp_nearest_k (matUtils extract's k nearest samples on the device) on a synthetic MAT of the sars2 polytomy shape,
beside the front end's own host path (`matutils-amd extract --reference-ties`: the literal std::sort per query) on a small
sample of the same queries, and the bytes/s the select passes reach against 5 B x range x passes.

    python tools/bench_nearest.py [--nodes 10000000] [--queries 4096] [--host 8] [--out profile.json]
Prints one JSON line."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import bench_annotate as B  # noqa: E402
from tools import time_load  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402

PASSES = 3   # histogram (one pass when distances are below 2048), count, write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--host", type=int, default=8, help="queries of the host comparison (0: skip)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1, shape="sars2")
    arrays = st.arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"], np.int64)
    has_kids = np.zeros(n, bool)
    has_kids[par[1:]] = True
    leaves = np.flatnonzero(~has_kids)
    nodes = np.random.default_rng(5).choice(leaves, min(a.queries, len(leaves)), replace=False)
    size = B.subtree_sizes(np.maximum(par, 0))
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.nearest_k(nodes[:16], 50)                      # tables (ugp_nearest_attach) + warm-up
    out = {"nodes": int(n), "queries": int(len(nodes)), "attach_and_first_16_s": round(time.perf_counter() - t0, 3), "date": time.strftime("%Y-%m-%d"),
           "tool": "tools/bench_nearest.py"}
    for k in (50, 2000):
        t0 = time.perf_counter()
        _, _, info = pl.nearest_k(nodes, k)
        dt = time.perf_counter() - t0
        rng_sum = int(size[info["anc"][info["count"] > 0]].sum())
        out["k%d" % k] = {"device_s": round(dt, 4), "queries_per_s": round(len(nodes) / dt, 1), "range_positions": rng_sum,
                          "select_bytes_per_s": round(5.0 * rng_sum * PASSES / dt, 1), "ties_open": int((info["n_at_cut"] > 1).sum())}
    pl.close()
    if a.host:
        d = tempfile.mkdtemp(prefix="nearest_")
        pb, sf = os.path.join(d, "tree.pb"), os.path.join(d, "s.txt")
        time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
        open(sf, "w").write("".join("L%d\n" % j for j in nodes[:a.host]))
        exe = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
        for k in (50, 2000):
            ms = {}
            for mode, extra in (("device", []), ("reference_ties", ["--reference-ties"])):
                r = subprocess.run([exe, "extract", "-i", pb, "-s", sf, "-Y", str(k), "-u", "u.txt", "-d", d] + extra, capture_output=True, text=True)
                assert r.returncode == 0, r.stderr[-1000:]
                ms[mode] = float(re.search(r"Nearest-k search of \d+ samples: ([0-9.]+) msec", r.stderr).group(1))
            out["k%d" % k]["front_end"] = {"queries": a.host, "device_ms": ms["device"], "reference_ties_ms": ms["reference_ties"],
                                           "host_s_per_query": round((ms["reference_ties"] - ms["device"]) / 1000 / a.host, 4),
                                           "reference_ties_over_device": round(ms["reference_ties"] / max(ms["device"], 1e-3), 1)}
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
