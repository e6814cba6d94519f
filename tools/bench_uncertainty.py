"""Samples/s of ugp_uncertainty (matUtils uncertainty on the device) on the 10M-node synthetic MAT, beside the oracle's
literal serial search (one full tree pass per sample, as findEPPs_wrapper runs them) on a handful of samples.

    python tools/bench_uncertainty.py [--nodes 10000000] [--samples 16384] [--oracle 2]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import capi  # noqa: E402
from tests import uncertainty_ref as U  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--oracle", type=int, default=2)
    ap.add_argument("--cap", type=int, default=64)
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1)
    arrays = st.arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"])
    has_kids = np.zeros(n, bool)
    has_kids[par[1:]] = True
    leaves = np.flatnonzero(~has_kids)
    nodes = np.random.default_rng(5).choice(leaves, min(a.samples, len(leaves)), replace=False)
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.uncertainty(nodes[:64], cap=a.cap)          # tables (ugp_uncertainty_attach) + warm-up
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    epps, nsize, _, cnt = pl.uncertainty(nodes, cap=a.cap)
    t_dev = time.perf_counter() - t0
    out = {"nodes": int(n), "samples": int(len(nodes)), "device_s": round(t_dev, 3), "device_samples_per_s": round(len(nodes) / t_dev, 1),
           "attach_and_first_64_s": round(t_first, 3), "mean_epps": round(float(epps.mean()), 3),
           "frac_epps_1": round(float((epps == 1).mean()), 4), "max_tie_count": int(cnt.max())}
    if a.oracle:
        ot = capi.OracleTree(arrays)
        dfs = U.dfs_order(arrays)
        t0 = time.perf_counter()
        for j in nodes[:a.oracle]:
            U.search(ot, arrays, dfs, int(j), U.literal_sample(arrays, int(j)))
        t_or = time.perf_counter() - t0
        out["oracle_serial_samples_per_s"] = round(a.oracle / t_or, 4)
    pl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
