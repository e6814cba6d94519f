"""The mask calls (matUtils mask's -s and -m on the device) on a synthetic MAT of the sars2 polytomy shape, beside the front end's
own host path (`matutils-amd mask --host`: the reference's walks, statement by statement) on the same tree.

    python tools/bench_mask.py [--nodes 10000000] [--reps 5] [--no-front-end] [--out profile.json]
Call times are medians of --reps calls after one warm-up call, copies to and from the host included; pass times are ugp_mask_time:
device events around the passes alone, mean of --reps runs after a warm-up.  `bytes` is what the passes must move at least, from the
shapes (see pass_bytes).  The front end's runs are timed as whole processes, the device path and --host in turn.  Prints one JSON
line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_load  # noqa: E402
from tools.bench_relatives import leaf_counts, median_wall, say  # noqa: E402
from tools.bench_select import LETTER, preorder  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402


def pass_bytes(n, m, tp, n_leaves, names, at_positions):
    """(restricted, mutations): the bytes the passes read and write at least.
    restricted: the difference array cleared, written into by F and read twice (12 n); per node two leaf-rank bounds, the subtree
    end, "has a leaf child" and `full` written (14 n), then `full` of the node and of its parent, the parent, leaf, "has a leaf
    child" and the flag written (9 n); the key table cleared (256 tp); per entry position, node and stored alleles twice, the flag
    twice, the caller's index and the answer (25 m); the names and the bitmap with its prefix counts.
    mutations: the answers cleared (4 m), every entry's position (4 m), and for the entries at a line's position their caller's
    index, answer, node and alleles (13 each)."""
    restricted = 35 * n + 256 * tp + 25 * m + 4 * names + 3 * 12 * (n_leaves // 64 + 1)
    mutations = 8 * m + 13 * at_positions
    return int(restricted), int(mutations)


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
    size, pre = preorder(par)
    pos, nuc, mpar = (np.asarray(arrays[k]) for k in ("mut_pos", "mut_nuc", "mut_par"))
    m, tp = int(len(pos)), int(pos.max()) + 1
    bare = {"n": n, "parent": arrays["parent"], "mut_off": np.zeros(n + 1, np.int64), "mut_pos": np.zeros(0, np.int32),
            "mut_ref": np.zeros(0, np.int8), "mut_par": np.zeros(0, np.int8), "mut_nuc": np.zeros(0, np.int8)}
    pl = Placer(bare)
    t0 = time.perf_counter()
    pl.mask_attach(arrays)
    leaves = np.flatnonzero(size == 1).astype(np.uint32)
    out = {"nodes": n, "leaves": int(len(leaves)), "entries": m, "positions": tp, "attach_s": round(time.perf_counter() - t0, 3), "reps": a.reps,
           "date": time.strftime("%Y-%m-%d"), "tool": "tools/bench_mask.py"}
    say("attached", out["attach_s"])
    rng = np.random.default_rng(13)
    # named sets: 1,000 drawn leaves; every leaf of one large clade and 1,000 drawn leaves; half of all leaves
    inner = np.flatnonzero(size > 1)
    clade = int(inner[np.argmin(np.abs(nleaf[inner] - 100_000))])
    under = leaves[(pre[leaves] >= pre[clade]) & (pre[leaves] < pre[clade] + size[clade])]
    drawn = rng.choice(leaves, 1000, replace=False)
    sets = {"leaves_1000": drawn, "clade_and_1000": np.concatenate([under, drawn]), "half": rng.choice(leaves, len(leaves) // 2, replace=False)}
    for key, named in sets.items():
        named = np.ascontiguousarray(named, np.uint32)
        wall = median_wall(lambda: pl.mask_restricted(named), a.reps)
        roots, masked = pl.mask_restricted(named)
        ms = pl.mask_time(named, reps=a.reps)[0]
        nbytes = pass_bytes(n, m, tp, len(leaves), len(named), 0)[0]
        out["restricted_" + key] = {"names": int(len(named)), "roots": int(len(roots)), "masked": int(masked.sum()), "call_ms": round(wall * 1e3, 3),
                                    "passes_ms": round(ms, 4), "bytes": nbytes, "gb_per_s": round(nbytes / ms / 1e6, 1)}
        say(key, out["restricted_" + key])
    # lines: tree-wide ones first, the position with the most entries among them; every fourth a branch line with two exclusions
    per_pos = np.bincount(pos[pos >= 0])
    most = int(per_pos.argmax())
    pick = np.concatenate([[int(np.flatnonzero(pos == most)[0])], rng.choice(m, 999, replace=False)])
    branch = inner[(nleaf[inner] > 1000) & (nleaf[inner] < 500_000)]
    lpos, lpar, lnuc, lnode, lexcl = [], [], [], [], []
    for i, e in enumerate(pick):
        lpos.append(int(pos[e])); lpar.append(int(mpar[e])); lnuc.append(int(nuc[e]))
        if i % 4 == 3:   # below a branch that holds the entry, but not below two of the branch's descendants
            t = int(branch[rng.integers(len(branch))])
            kids = np.arange(np.searchsorted(par[1:], t, "left") + 1, np.searchsorted(par[1:], t, "right") + 1)   # parents ascend
            lnode.append(t); lexcl.append([int(kids[0]), int(kids[-1])])
        else:
            lnode.append(0); lexcl.append([])
    for k in (1, 64, 1000):
        cols = (lpos[:k], lpar[:k], lnuc[:k], lnode[:k], lexcl[:k])
        wall = median_wall(lambda: pl.mask_mutations(*cols), a.reps)
        first, counts = pl.mask_mutations(*cols)
        ms = pl.mask_time(None, *cols, reps=a.reps)[1]
        nbytes = pass_bytes(n, m, tp, len(leaves), 0, int(per_pos[np.unique(lpos[:k])].sum()))[1]
        out["mutations_%d" % k] = {"removed": int(counts.sum()), "most_entries": int(per_pos[most]), "call_ms": round(wall * 1e3, 3),
                                   "passes_ms": round(ms, 4), "bytes": nbytes, "gb_per_s": round(nbytes / ms / 1e6, 1)}
        say("mutations", k, out["mutations_%d" % k])
    pl.close()
    if not a.no_front_end:
        exe = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
        d = tempfile.mkdtemp(prefix="mask_")
        pb = os.path.join(d, "tree.pb")
        time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
        order = inner[np.argsort(pre[inner])]   # internal nodes are named node_<k> in depth-first order of the internal nodes
        number = np.zeros(n, np.int64)
        number[order] = np.arange(1, len(order) + 1)
        name = lambda v: "node_%d" % number[v] if size[v] > 1 else "L%d" % v
        with open(os.path.join(d, "s.txt"), "w") as f:
            f.write("".join("L%d\n" % v for v in drawn))
        with open(os.path.join(d, "m.tsv"), "w") as f:
            for i in range(64):
                mut = "%s%d%s" % (LETTER[lpar[i]], lpos[i], LETTER[lnuc[i]])
                f.write(mut + "\n" if not lexcl[i] else "%s\t%s\t%s\n" % (mut, name(lnode[i]), ";".join(name(x) for x in lexcl[i])))
        fe = {}
        for key, opts in (("s_1000_names", ["-s", os.path.join(d, "s.txt")]), ("m_64_lines", ["-m", os.path.join(d, "m.tsv")])):
            data = {}
            for mode, extra in (("device", []), ("host", ["--host"])):
                o = os.path.join(d, "out_%s.pb" % mode)
                t0 = time.perf_counter()
                r = subprocess.run([exe, "mask", "-i", pb, "-o", o] + opts + extra, capture_output=True, text=True)
                fe["%s_%s_run_s" % (key, mode)] = round(time.perf_counter() - t0, 2)
                assert r.returncode == 0, r.stderr[-1000:]
                data[mode] = open(o, "rb").read()
                os.remove(o)
                say(key, mode, fe["%s_%s_run_s" % (key, mode)], [l for l in r.stderr.split("\n") if l.startswith(("Masked a total", "Restricted"))])
            assert data["device"] == data["host"], key
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
