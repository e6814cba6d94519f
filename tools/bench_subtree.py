"""The induced subtree on the device (ugp_subtree.hip, `matutils-amd subtree`) on a synthetic MAT of the sars2 polytomy shape, beside
get_subtree on the host (`subtree --host`, and `select`, which builds the subtree that way on both of its paths) on the same tree.

    python tools/bench_subtree.py [--nodes 10000000] [--clade-leaves 2000] [--reps 5] [--no-front-end] [--no-host]
                                  [--caterpillar 1000000] [--out profile.json]
Library: attach, ugp_subtree_nodes + ugp_subtree_entries as whole calls (medians of --reps after a warm-up), and the passes alone
(device events, no copies) for a clade of about --clade-leaves leaves, the samples of `-m` on the position with the most entries, a million
drawn leaves and every leaf.  `bytes` is what the passes must move at least, by the model of pass_bytes(); the rate over the 6.29 TB/s
of a float4 copy is a figure to read, not a bar.  Front end: whole runs and the subtree step's own line.  --no-host leaves out the
runs that build the subtree on the host (minutes, or more than anyone waits, on large selections).  --caterpillar: the passes alone
on a caterpillar that deep with two leaves selected (0: not run).  Prints one JSON line."""
import argparse
import ctypes as C
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
from tools.bench_relatives import leaf_counts, median_wall, say  # noqa: E402
from tools.bench_select import LETTER, preorder  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402
from usher_amd.placement import _ptr  # noqa: E402

COPY_TBS = 6.29   # a float4 copy on this GPU
EXE = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")


def pass_bytes(n, m, kept, gathered, entries):
    """The least the passes move: per node its range end, parent, two flags and two scan values; per entry its node, flag and scan
    value; per gathered entry its key and value written, sorted once in and out, read by the merge with its alleles, and its
    survivor flag and scan value; per merged entry its nine bytes; per kept node its list entry, parent and offset."""
    return n * (4 + 4 + 1 + 1 + 4 + 4) + m * (4 + 1 + 4) + gathered * (12 + 24 + 12 + 1 + 1 + 4) + entries * 9 + kept * 12


def topology(arrays):
    n = int(arrays["n"])
    return {"n": n, "parent": arrays["parent"], "mut_off": np.zeros(n + 1, np.int64), "mut_pos": np.zeros(0, np.int32),
            "mut_ref": np.zeros(0, np.int8), "mut_par": np.zeros(0, np.int8), "mut_nuc": np.zeros(0, np.int8)}


def one_call(pl, n_nodes, sel):
    """ugp_subtree_nodes with the room the front end gives it, then ugp_subtree_entries: (kept, entries, info)."""
    room = min(2 * len(sel), n_nodes)
    kept, par, off = np.empty(room, np.uint32), np.empty(room, np.uint32), np.empty(room, np.uint64)
    nk, ne, got = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    info = np.zeros(1, pl.SUB_INFO)
    pl._ck(pl._L.ugp_subtree_nodes(pl._h, len(sel), _ptr(sel), _ptr(kept), _ptr(par), _ptr(off), room, C.byref(nk), C.byref(ne), _ptr(info)))
    e = max(int(ne.value), 1)
    pos, first, nuc = np.empty(e, np.int32), np.empty(e, np.uint32), np.empty(e, np.uint8)
    pl._ck(pl._L.ugp_subtree_entries(pl._h, _ptr(pos), _ptr(first), _ptr(nuc), int(ne.value), C.byref(got)))
    return int(nk.value), int(ne.value), info[0]


def library(pl, n, m, name, sel, reps):
    sel = np.ascontiguousarray(sel, dtype=np.uint32)
    wall = median_wall(lambda: one_call(pl, n, sel), reps)
    kept, entries, info = one_call(pl, n, sel)
    nodes_ms, merge_ms = pl.subtree_time(sel, reps)
    moved = pass_bytes(n, m, kept, int(info["n_gathered"]), entries)
    rec = {"selected": int(info["n_selected"]), "kept": kept, "gathered": int(info["n_gathered"]), "entries": entries,
           "longest_chain": int(info["longest_chain"]), "disagreements": int(info["n_disagree"]), "call_ms": round(wall * 1e3, 3),
           "nodes_pass_ms": round(nodes_ms, 4), "merge_pass_ms": round(merge_ms, 4), "bytes": moved,
           "fraction_of_copy_rate": round(moved / ((nodes_ms + merge_ms) * 1e-3) / (COPY_TBS * 1e12), 4)}
    say(name, rec)
    return rec


def front_end(sub, pb, d, opts, mode):
    """One run: (whole seconds, the step's own line in ms or None, the bytes of -u and -t)."""
    t0 = time.perf_counter()
    r = subprocess.run([EXE, sub, "-i", pb, "-d", d, "-u", "u.txt", "-t", "t.nh"] + opts + (["--host"] if mode == "host" else []),
                       capture_output=True, text=True)
    run_s = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-1000:]
    step = re.search(r"Selection step subtree \(%s\): ([0-9.]+) msec" % mode, r.stderr)
    files = tuple(open(os.path.join(d, f), "rb").read() for f in ("u.txt", "t.nh"))
    return {"run_s": round(run_s, 2), "step_ms": round(float(step.group(1)), 2) if step else None}, files


def most_entries(arrays):
    pos, nuc, ref = (np.asarray(arrays[k]) for k in ("mut_pos", "mut_nuc", "mut_ref"))
    most = int(np.bincount(pos[pos >= 0]).argmax())
    k0 = int(np.flatnonzero(pos == most)[0])
    return most, int(nuc[k0]), "%s%d%s" % (LETTER[int(ref[k0])], most, LETTER[int(nuc[k0])])


def caterpillar(depth):
    """A spine of `depth` nodes with a side leaf each, one entry on every node but the root: position 1 flips down the spine."""
    n = 3 + 2 * depth
    j = np.arange(n, dtype=np.int64)
    parent = 2 * ((j - 1) // 2) - 1
    parent[0], parent[1], parent[2] = -1, 0, 0
    spine = (j % 2 == 1)
    level = (j + 1) // 2
    pos = np.where(spine, 1, 2).astype(np.int32)
    par = np.where(spine, np.where(level % 2 == 1, 1, 2), 4).astype(np.int8)
    nuc = np.where(spine, np.where(level % 2 == 1, 2, 1), 1).astype(np.int8)
    off = np.maximum(j - 1, 0)
    off = np.append(off, n - 1)
    arrays = {"n": n, "parent": parent, "mut_off": off, "mut_pos": pos[1:], "mut_ref": par[1:], "mut_par": par[1:], "mut_nuc": nuc[1:]}
    return arrays, np.asarray([n - 2, 6], np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-front-end", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--clade-leaves", type=int, default=2000)
    ap.add_argument("--caterpillar", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1, shape="sars2")
    arrays = st.arrays
    n, m = int(arrays["n"]), int(len(arrays["mut_pos"]))
    par = np.maximum(np.asarray(arrays["parent"], np.int64), 0)
    nleaf = leaf_counts(par)
    size, pre = preorder(par)
    leaves = np.flatnonzero(size == 1)
    inner = np.flatnonzero(size > 1)
    clade = int(inner[np.argmin(np.abs(nleaf[inner] - a.clade_leaves))])
    most, most_nuc, mut = most_entries(arrays)
    pl = Placer(arrays)
    pl.select_attach()
    mask, _ = pl.select_mutations(np.asarray([most], np.int32), np.asarray([most_nuc], np.uint8))
    with_mut = pl.select_leaves()[mask]
    t0 = time.perf_counter()
    pl.subtree_attach()
    out = {"nodes": n, "leaves": int(len(leaves)), "entries": m, "attach_s": round(time.perf_counter() - t0, 3), "reps": a.reps,
           "date": time.strftime("%Y-%m-%d"), "tool": "tools/bench_subtree.py", "copy_rate_TBs": COPY_TBS}
    say("attached", out["attach_s"])
    rng = np.random.default_rng(11)
    under = leaves[(pre[leaves] >= pre[clade]) & (pre[leaves] < pre[clade] + size[clade])]
    out["library"] = {"clade_%d" % len(under): library(pl, n, m, "clade", under, a.reps),
                      "mutation_%d" % len(with_mut): library(pl, n, m, "mutation", with_mut, a.reps),
                      "drawn_1000000": library(pl, n, m, "drawn", rng.choice(leaves, min(1_000_000, len(leaves)), replace=False), a.reps),
                      "every_leaf": library(pl, n, m, "every leaf", leaves, a.reps)}
    pl.close()
    if not a.no_front_end:
        d = tempfile.mkdtemp(prefix="subtree_")
        pb, apb = os.path.join(d, "tree.pb"), os.path.join(d, "annotated.pb")
        time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
        order = inner[np.argsort(pre[inner])]   # internal nodes are named node_<k> in depth-first order of the internal nodes
        open(os.path.join(d, "nid.tsv"), "w").write("BENCH\tnode_%d\n" % (int(np.flatnonzero(order == clade)[0]) + 1))
        r = subprocess.run([EXE, "annotate", "-i", pb, "-o", apb, "-C", os.path.join(d, "nid.tsv")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        fe = {"clade_leaves": int(nleaf[clade]), "mutation": mut}
        for key, opts in (("c", ["-c", "BENCH"]), ("m", ["-m", mut])):
            fe["%s_subtree_device" % key], dev = front_end("subtree", apb, d, opts, "device")
            fe["%s_samples" % key] = dev[0].count(b"\n")
            say(key, fe)
            if not a.no_host:
                fe["%s_subtree_host" % key], host = front_end("subtree", apb, d, opts, "host")
                fe["%s_select_device" % key], sel = front_end("select", apb, d, opts, "device")   # get_subtree on the host, as before
                assert dev == host == sel, key
                fe["%s_step_ratio_host_over_device" % key] = round(fe["%s_subtree_host" % key]["step_ms"] / fe["%s_subtree_device" % key]["step_ms"], 1)
                say(key, fe)
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        out["front_end"] = fe
        os.rmdir(d)
    if a.caterpillar:
        try:
            arrays, sel = caterpillar(a.caterpillar)
            pl = Placer(topology(arrays))
            pl.subtree_attach(arrays)
            out["caterpillar"] = dict(library(pl, int(arrays["n"]), int(len(arrays["mut_pos"])), "caterpillar", sel, a.reps), depth=a.caterpillar)
            pl.close()
        except Exception as e:   # a handle that does not take a tree this deep is a finding to write down, not a reason to lose the rest
            out["caterpillar"] = {"depth": a.caterpillar, "error": str(e)[:300]}
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
