"""The select calls (matUtils extract's -m, -c / -I and -U selectors on the device) on a synthetic MAT of the sars2 polytomy shape,
beside the front end's own host path (`matutils-amd select --host`: the reference's walks, statement by statement) on the same tree.

    python tools/bench_select.py [--nodes 10000000] [--reps 5] [--no-front-end] [--out profile.json]
Wall times are medians of --reps calls after one warm-up call; kernel times are device events around the launches, without the
copy to the host.  The front end's runs are timed as whole processes and by the selection step's own line.  Prints one JSON line."""
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
from tools.bench_relatives import leaf_counts, median_wall, say  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402

LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}


def preorder(par):
    """(subtree sizes, depth-first preorder positions) of a BFS-ordered tree whose children follow their parents' order."""
    n = len(par)
    levels, lo, hi = [], 0, 1
    while lo < n:
        levels.append((lo, hi))
        lo, hi = hi, int(np.searchsorted(par[1:], hi)) + 1 if hi < n else n
        if lo >= hi:
            break
    size = np.ones(n, np.int64)
    for lo, hi in reversed(levels[1:]):
        np.add.at(size, par[lo:hi], size[lo:hi])
    c = np.cumsum(size)
    first = np.searchsorted(par[1:], par, "left") + 1          # the first child of each node's parent
    before = np.zeros(n, np.int64)                              # the subtrees of the earlier siblings
    before[1:] = c[np.arange(n - 1)] - c[first[1:] - 1]
    pre = np.zeros(n, np.int64)
    for lo, hi in levels[1:]:
        pre[lo:hi] = pre[par[lo:hi]] + 1 + before[lo:hi]
    return size, pre


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-front-end", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1, shape="sars2")
    arrays = st.arrays
    n = int(arrays["n"])
    par = np.maximum(np.asarray(arrays["parent"], np.int64), 0)
    nleaf = leaf_counts(par)
    pos, nuc, ref = (np.asarray(arrays[k]) for k in ("mut_pos", "mut_nuc", "mut_ref"))
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.select_attach()
    out = {"nodes": n, "leaves": pl._sel_leaves, "entries": int(len(pos)), "attach_s": round(time.perf_counter() - t0, 3), "reps": a.reps,
           "date": time.strftime("%Y-%m-%d"), "tool": "tools/bench_select.py"}
    say("attached", out["attach_s"])
    nl = pl._sel_leaves
    # queries: the position with the most entries first, then 63 drawn from the entries
    rng = np.random.default_rng(11)
    most = int(np.bincount(pos[pos >= 0]).argmax())
    k0 = int(np.flatnonzero(pos == most)[0])
    pick = np.concatenate([[k0], rng.choice(len(pos), 63, replace=False)])
    qpos, qnuc = pos[pick].astype(np.int32), nuc[pick].astype(np.uint8)
    for m in (1, 64):
        wall = median_wall(lambda: pl.select_mutations(qpos[:m], qnuc[:m]), a.reps)
        mask, counts = pl.select_mutations(qpos[:m], qnuc[:m])
        kernel = pl.select_time(qpos[:m], qnuc[:m], a.reps)
        out["mutations_%d" % m] = {"wall_ms": round(wall * 1e3, 3), "kernel_ms": round(kernel, 4), "selected": int(mask.sum()),
                                   "kernel_ns_per_leaf_query": round(kernel * 1e6 / (nl * m), 4)}
        say("mutations", m, out["mutations_%d" % m])
    nodes = rng.integers(0, n, 2000).astype(np.uint32)
    wall = median_wall(lambda: pl.select_subtrees(nodes), a.reps)
    mask, _ = pl.select_subtrees(nodes)
    out["subtrees_2000"] = {"wall_ms": round(wall * 1e3, 3), "selected": int(mask.sum())}
    wall = median_wall(lambda: pl.select_mrca(mask), a.reps)
    out["mrca"] = {"wall_ms": round(wall * 1e3, 3), "below": pl.select_mrca(mask)[1]}
    say(out["subtrees_2000"], out["mrca"])
    pl.close()
    if not a.no_front_end:
        exe = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
        d = tempfile.mkdtemp(prefix="select_")
        pb, apb = os.path.join(d, "tree.pb"), os.path.join(d, "annotated.pb")
        time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
        # a clade of about 2,000 leaves: internal nodes are named node_<k> in depth-first order of the internal nodes
        size, pre = preorder(par)
        inner = np.flatnonzero(size > 1)
        order = inner[np.argsort(pre[inner])]
        want = 2000   # (the front end builds the induced subtree of the selection, which is slow for large selections)
        v = int(inner[np.argmin(np.abs(nleaf[inner] - want))])
        name = "node_%d" % (int(np.flatnonzero(order == v)[0]) + 1)
        open(os.path.join(d, "nid.tsv"), "w").write("BENCH\t%s\n" % name)
        r = subprocess.run([exe, "annotate", "-i", pb, "-o", apb, "-C", os.path.join(d, "nid.tsv")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        mut = "%s%d%s" % (LETTER[int(ref[k0])], most, LETTER[int(nuc[k0])])
        fe = {"clade_leaves": int(nleaf[v]), "mutation": mut}
        for key, opts in (("m", ["-m", mut]), ("c", ["-c", "BENCH"])):
            text = {}
            for mode, extra in (("device", []), ("host", ["--host"])):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "select", "-i", apb, "-d", d, "-u", "u.txt"] + opts + extra, capture_output=True, text=True)
                run_s = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-1000:]
                step = float(re.search(r"Selection step -%s \(%s\): ([0-9.]+) msec" % (key, mode), r.stderr).group(1))
                text[mode] = open(os.path.join(d, "u.txt"), "rb").read()
                fe["%s_%s" % (key, mode)] = {"run_s": round(run_s, 2), "step_ms": round(step, 2)}
            assert text["device"] == text["host"], key
            fe["%s_samples" % key] = text["host"].count(b"\n")
            say(key, fe)
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
        out["front_end"] = fe
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
