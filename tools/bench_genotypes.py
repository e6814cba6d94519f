"""Rates of the genotype extraction (matUtils extract -v on the device) on a synthetic MAT of the sars2 polytomy shape:
  (a) select + site table for all leaves -- what `extract -v -n` needs -- in sites/s;
  (b) the rows of 10,000 leaves chosen as one union of nearest-k neighbourhoods: cells/s of ugp_genotype_rows as a caller sees it (with
      the copy to pageable host memory), and the bytes/s of the row kernel alone (device events, no copy) against n_cols bytes per
      row, each written once;
  (c) the front end on (b), `matutils-amd extract -s ... -v`, with and without --host-genotypes (the reference's serial walk), same run.

    python tools/bench_genotypes.py [--nodes 10000000] [--samples 10000] [--out profile.json]
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
from tools import time_load  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return min(ts), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--samples", type=int, default=10_000)
    ap.add_argument("--front-end", type=int, default=1, help="0: skip (c)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1, shape="sars2")
    arrays = st.arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"], np.int64)
    has_kids = np.zeros(n, bool)
    has_kids[par[1:]] = True
    leaves = np.flatnonzero(~has_kids)
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.genotypes_attach()
    out = {"nodes": int(n), "leaves": int(len(leaves)), "attach_s": round(time.perf_counter() - t0, 3), "date": time.strftime("%Y-%m-%d"),
           "tool": "tools/bench_genotypes.py"}
    pl.genotype_select()   # warm-up: workspace allocations
    dt, (n_cols, n_sites) = best(lambda: (pl.genotype_select(), pl.genotype_sites())[0])
    out["all_leaves"] = {"n_cols": n_cols, "n_sites": n_sites, "select_and_sites_s": round(dt, 4), "sites_per_s": round(n_sites / dt, 1),
                         "columns_per_s": round(n_cols / dt, 1)}
    # one neighbourhood union: the 50 nearest of random leaves until `samples` leaves are held
    rng = np.random.default_rng(5)
    seen = np.zeros(n, bool)
    while seen.sum() < a.samples:
        nodes, _, info = pl.nearest_k(rng.choice(leaves, 256, replace=False), 50)
        for row, f in zip(nodes, info):
            seen[row[:min(int(f["count"]), 50)]] = True
    sel = np.flatnonzero(seen)[:a.samples].astype(np.uint32)
    n_cols, n_sites = pl.genotype_select(sel)
    pl.genotype_rows(0, min(n_sites, 8))
    dt, codes = best(lambda: pl.genotype_rows())
    dsel, _ = best(lambda: pl.genotype_select(sel))
    kernel_ms = min(pl.genotype_rows_time(reps=10) for _ in range(3))
    out["neighbourhood"] = {"n_cols": n_cols, "n_sites": n_sites, "select_s": round(dsel, 4), "rows_s": round(dt, 4),
                            "cells_per_s": round(n_cols * n_sites / dt, 1), "row_kernel_ms": round(kernel_ms, 4),
                            "row_kernel_bytes_per_s": round(n_cols * n_sites / (kernel_ms / 1e3), 1),
                            "nonzero_cells": int(np.count_nonzero(codes))}
    pl.close()
    if a.front_end:
        d = tempfile.mkdtemp(prefix="genotypes_")
        pb, sf = os.path.join(d, "tree.pb"), os.path.join(d, "s.txt")
        time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
        open(sf, "w").write("".join("L%d\n" % j for j in sel))
        exe = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
        ms, size = {}, {}
        for mode, extra in (("device", []), ("host_genotypes", ["--host-genotypes"])):
            r = subprocess.run([exe, "extract", "-i", pb, "-s", sf, "-v", mode + ".vcf", "-d", d] + extra, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-1000:]
            ms[mode] = float(re.search(r"VCF of \d+ sites x \d+ samples \(\w+\): ([0-9.]+) msec", r.stderr).group(1))
            size[mode] = os.path.getsize(os.path.join(d, mode + ".vcf"))
        same = open(os.path.join(d, "device.vcf"), "rb").read() == open(os.path.join(d, "host_genotypes.vcf"), "rb").read()
        out["front_end"] = {"device_ms": ms["device"], "host_genotypes_ms": ms["host_genotypes"], "vcf_bytes": size["device"], "identical": bool(same),
                            "host_over_device": round(ms["host_genotypes"] / max(ms["device"], 1e-3), 2)}
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
