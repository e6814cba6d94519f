"""Branches/s of ugp_ripples (RIPPLES' search on the device) on a synthetic MAT, for the default branch list (non-root nodes with
>= 3 mutations and >= 10 leaves, main.cpp:228-251) under the default options, and (candidate x valid pair) evaluations/s.
Beside it: the serial C oracle's pass 1 alone (mapper2_body over every candidate node, main.cpp:343-377) on a few branches --
a lower bound on the reference's serial work per branch, which then runs two more node passes per breakpoint pair.

    python tools/bench_ripples.py [--nodes 1000000] [--branches 64] [--oracle 2]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import capi  # noqa: E402
from tests import ripples_ref as RR  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--branches", type=int, default=64)
    ap.add_argument("--oracle", type=int, default=2)
    a = ap.parse_args()
    arrays = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1).arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"]).astype(np.int64)
    leaf = np.ones(n, bool)
    leaf[par[1:]] = False
    nl = leaf.astype(np.int64)
    sz = np.ones(n, np.int64)
    for j in range(n - 1, 0, -1):
        nl[par[j]] += nl[j]
        sz[par[j]] += sz[j]
    nmut = np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))
    default = np.flatnonzero((nmut >= 3) & (nl >= 10))
    default = default[default != 0]
    rank = np.arange(n, dtype=np.uint32)   # the synthetic tree's names sort in node order
    br = np.random.default_rng(0).permutation(default)[:a.branches]
    cand = int((sz >= 10).sum())
    pairs = sum(len(RR.valid_pairs([r[0] for r in RR.pruned_sample(arrays, int(b))], 3, 1000, 10 ** 7)) for b in br)
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.ripples(br[:2], rank)           # tables (ugp_ripples_attach) + warm-up
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    ev = pl.ripples(br, rank)
    t_dev = time.perf_counter() - t0
    out = {"nodes": int(n), "default_branches": int(len(default)), "branches": int(len(br)), "candidates": cand,
           "valid_pairs": int(pairs), "events": int(len(ev)), "device_s": round(t_dev, 3),
           "device_branches_per_s": round(len(br) / t_dev, 2), "device_cand_pair_evals_per_s": float("%.4g" % (cand * pairs / t_dev)),
           "attach_and_first_2_s": round(t_first, 3)}
    if a.oracle:
        ot = capi.OracleTree(arrays)
        cl = np.flatnonzero(sz >= 10)
        t0 = time.perf_counter()
        for b in br[:a.oracle]:
            ot.place_list(RR.as_sample(RR.pruned_sample(arrays, int(b))), cl, jidx=cl, compute_scores=True, tie_cap=1 << 16)
        t_or = time.perf_counter() - t0
        out["oracle_serial_pass1_only_s_per_branch"] = round(t_or / a.oracle, 3)
    pl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
