"""Clades/s of matUtils annotate's device work on the 10M-node synthetic MAT: about 2,000 clades whose exemplars lie below
chosen roots (about 500k exemplars), through the library calls so that file I/O does not count -- clade allele counts
(ugp_clade_alleles), the search (packed ugp_tied_nodes_ex in depth-first order; ugp_annotate_search for clades with repeated or
masked rows) and the overlap counts (ugp_clade_descendants for every tie and all of its ancestors).  The CPU leg times the literal
restatement (exemplar walks + the oracle's serial mapper2_body) on a few clades and counts mismatches against the device.

    python tools/bench_annotate.py [--nodes 10000000] [--clades 2000] [--exemplars 250] [--oracle 2]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import capi  # noqa: E402
from tests import annotate_ref as A  # noqa: E402
from tests import uncertainty_ref as U  # noqa: E402
from usher_amd import Placer, QueryBatch  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402


def subtree_sizes(par):
    """Subtree sizes of a BFS-ordered tree (parents are nondecreasing, so each level is one contiguous range)."""
    n = len(par)
    levels, lo, hi = [], 0, 1
    while lo < n:
        levels.append((lo, hi))
        lo, hi = hi, int(np.searchsorted(par[1:], hi)) + 1 if hi < n else n
        if lo >= hi:
            break
    sz = np.ones(n, np.int64)
    for lo, hi in reversed(levels[1:]):
        np.add.at(sz, par[lo:hi], sz[lo:hi])
    return sz


def rows_of(arrays, ent, cnt, k, min_freq=0.8, mask_freq=0.2):
    pos = np.asarray(arrays["mut_pos"])[ent]; ref = np.asarray(arrays["mut_ref"])[ent]; nuc = np.asarray(arrays["mut_nuc"])[ent]
    keys = {}
    for p, r, m, c in zip(pos.tolist(), ref.tolist(), nuc.tolist(), cnt.tolist()):
        keys[(p, r, m)] = keys.get((p, r, m), 0) + c
    rows = []
    for (p, r, m), c in keys.items():
        f = np.float32(c) / np.float32(k)
        if f >= np.float32(min_freq):
            rows.append((p, r, m))
        elif f >= np.float32(mask_freq):
            rows.append((p, r, 15))
    rows.sort()
    return {"pos": np.asarray([t[0] for t in rows], np.int32), "ref": np.asarray([t[1] for t in rows], np.int8),
            "nuc": np.asarray([t[2] for t in rows], np.int8), "is_missing": np.zeros(len(rows), np.int8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--clades", type=int, default=2000)
    ap.add_argument("--exemplars", type=int, default=250)
    ap.add_argument("--oracle", type=int, default=2)
    ap.add_argument("--cap", type=int, default=256)
    a = ap.parse_args()
    arrays = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1).arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"], np.int64)
    par[0] = -1
    sz = subtree_sizes(np.maximum(par, 0))
    pl = Placer(arrays)
    dfs = pl.node_order("dfs").astype(np.int64)
    pre = np.empty(n, np.int64); pre[dfs] = np.arange(n)
    rng = np.random.default_rng(7)
    roots = rng.choice(np.flatnonzero((sz >= 4 * a.exemplars) & (sz <= 40 * a.exemplars)), a.clades, replace=False)
    clades = [dfs[pre[r] + rng.integers(0, sz[r], a.exemplars)] for r in roots]
    t0 = time.perf_counter()
    pl.clade_alleles(clades[:4])                       # tables (ugp_annotate_attach) + warm-up
    t_first = time.perf_counter() - t0

    t0 = time.perf_counter()
    alle = pl.clade_alleles(clades)
    t_alleles = time.perf_counter() - t0
    rows = [rows_of(arrays, e, c, len(cl)) for (e, c), cl in zip(alle, clades)]
    awk = [i for i, r in enumerate(rows) if A.awkward(r)]
    plain = [i for i, r in enumerate(rows) if not A.awkward(r)]
    t0 = time.perf_counter()
    ties = [None] * len(rows)
    if plain:
        tj, _, tc = pl.tied_nodes_ex(QueryBatch([rows[i] for i in plain]), cap=a.cap, order="dfs")
        for i, t in zip(plain, tj):
            ties[i] = np.sort(t)
    if awk:
        _, tj, _ = pl.annotate_search(QueryBatch([rows[i] for i in awk]), cap=a.cap)
        for i, t in zip(awk, tj):
            ties[i] = t
    t_search = time.perf_counter() - t0
    # overlap: every tie and each of its ancestors up to the root, one batched call (the reference's walk, :665-680, stops
    # earlier at its freq / overlap break, so this is an upper bound of its pairs)
    pc, pn = [], []
    for c, t in enumerate(ties):
        for j in t:
            v = int(dfs[j])
            while v >= 0:
                pc.append(c); pn.append(v)
                v = int(par[v])
    t0 = time.perf_counter()
    pl.clade_descendants(clades, pc, pn)
    t_overlap = time.perf_counter() - t0
    total = t_alleles + t_search + t_overlap
    out = {"nodes": int(n), "clades": len(clades), "exemplars": int(sum(len(c) for c in clades)), "awkward_clades": len(awk),
           "overlap_pairs": len(pc), "clades_per_s": round(len(clades) / total, 1), "alleles_s": round(t_alleles, 3),
           "search_s": round(t_search, 3), "overlap_s": round(t_overlap, 3), "attach_and_first_s": round(t_first, 3)}
    if a.oracle:
        ot = capi.OracleTree(arrays)
        mism = 0
        t0 = time.perf_counter()
        for c in range(a.oracle):
            want = A.alleles_literal(arrays, clades[c])
            mism += dict(zip(alle[c][0].tolist(), alle[c][1].tolist())) != want
            wb, wt = A.search(ot, arrays, rows[c], dfs)
            if len(wt) <= a.cap:   # a capped packed list need not be the first cap ties
                mism += wt != ties[c].tolist()
        t_or = time.perf_counter() - t0
        out["oracle_serial_s_per_clade"] = round(t_or / a.oracle, 3)
        out["device_s_per_clade"] = round(total / len(clades), 6)
        out["oracle_mismatches"] = int(mism)
    pl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
