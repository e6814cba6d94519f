"""Many induced subtrees in one device call (ugp_subtree_batch.hip, `matutils-amd subtrees`) on a synthetic MAT of the sars2
polytomy shape, beside the only way there was before: a loop of ugp_subtree_nodes + ugp_subtree_entries over the same selections in
the same process.

    python tools/bench_subtrees.py [--nodes 10000000] [--reps 5] [--loop-reps 2] [--no-front-end] [--host-samples 40] [--out profile.json]
Library: (a) the nearest-500 sets of 1,000 drawn leaves, (b) the nearest-50 sets of 10,000 drawn leaves (Placer.nearest_k): the batch
with its two fetches as whole calls (median of --reps after a warm-up), the loop of single calls (median of --loop-reps after a
warm-up), the outputs compared array by array, and the passes alone (device events, no copies) of the batch and, summed over a
stated number of the selections and scaled to all, of the single call.  `windows` is what the batch scans: the selections' window
positions over the tree's nodes.
Front end: (c) `subtrees -m <mutation> -N 500 -t s` and `subtrees -N 2000 -t s` over a 100,000-name -s file, whole runs and the
cover and subtree steps' own lines, on the device; --host is run on the first --host-samples names only and its steps are scaled
by the subtrees made, which is said in the record (get_nearby walks every leaf below the ancestor it stops at, and get_subtree every
pair of a set).  Prints one JSON line; with --out the library part is written as soon as it is measured."""
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
from tools.bench_relatives import median_wall, say  # noqa: E402
from tools.bench_select import preorder  # noqa: E402
from tools.bench_subtree import most_entries  # noqa: E402
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402
from usher_amd.placement import _ptr  # noqa: E402

EXE = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")


def batch_call(pl, off, flat):
    """ugp_subtree_batch and its two fetches: (kept_off, entry_off, kept, parent, ent_off, pos, first, nuc, info)."""
    ns = len(off) - 1
    koff, eoff = np.empty(ns + 1, np.uint64), np.empty(ns + 1, np.uint64)
    info = np.zeros(ns, pl.SUB_BATCH_INFO)
    pl._ck(pl._L.ugp_subtree_batch(pl._h, ns, _ptr(off), _ptr(flat), _ptr(koff), _ptr(eoff), _ptr(info)))
    nk, ne = int(koff[ns]), max(int(eoff[ns]), 1)
    kept, par, ent = np.empty(nk, np.uint32), np.empty(nk, np.uint32), np.empty(nk, np.uint64)
    pos, first, nuc = np.empty(ne, np.int32), np.empty(ne, np.uint32), np.empty(ne, np.uint8)
    got = C.c_uint64(0)
    pl._ck(pl._L.ugp_subtree_batch_nodes(pl._h, _ptr(kept), _ptr(par), _ptr(ent), nk, C.byref(got)))
    pl._ck(pl._L.ugp_subtree_batch_entries(pl._h, _ptr(pos), _ptr(first), _ptr(nuc), int(eoff[ns]), C.byref(got)))
    return koff, eoff, kept, par, ent, pos[:int(eoff[ns])], first[:int(eoff[ns])], nuc[:int(eoff[ns])], info


def single_call(pl, n_nodes, sel):
    """ugp_subtree_nodes with the room the front end gives it, then ugp_subtree_entries."""
    room = min(2 * len(sel), n_nodes)
    kept, par, off = np.empty(room, np.uint32), np.empty(room, np.uint32), np.empty(room, np.uint64)
    nk, ne, got = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    info = np.zeros(1, pl.SUB_INFO)
    pl._ck(pl._L.ugp_subtree_nodes(pl._h, len(sel), _ptr(sel), _ptr(kept), _ptr(par), _ptr(off), room, C.byref(nk), C.byref(ne), _ptr(info)))
    e = int(ne.value)
    pos, first, nuc = np.empty(max(e, 1), np.int32), np.empty(max(e, 1), np.uint32), np.empty(max(e, 1), np.uint8)
    pl._ck(pl._L.ugp_subtree_entries(pl._h, _ptr(pos), _ptr(first), _ptr(nuc), e, C.byref(got)))
    k = int(nk.value)
    return kept[:k], par[:k], off[:k], pos[:e], first[:e], nuc[:e], info[0]


def loop_call(pl, n_nodes, sels):
    return [single_call(pl, n_nodes, s) for s in sels]


def equal(batch, singles):
    koff, eoff, kept, par, ent, pos, first, nuc, info = batch
    for b, (k1, p1, o1, q1, f1, n1, i1) in enumerate(singles):
        k0, k9, e0, e9 = int(koff[b]), int(koff[b + 1]), int(eoff[b]), int(eoff[b + 1])
        same = (np.array_equal(kept[k0:k9], k1) and np.array_equal(par[k0:k9], p1) and np.array_equal(ent[k0:k9] - np.uint64(e0), o1)
                and np.array_equal(pos[e0:e9], q1) and np.array_equal(first[e0:e9], f1) and np.array_equal(nuc[e0:e9], n1)
                and all(int(info[b][f]) == int(i1[f]) for f in ("n_selected", "n_gathered", "n_disagree", "longest_chain", "first_disagree")))
        if not same:
            return False
    return True


def library(pl, n, name, nodes, k, reps, loop_reps, pass_sample, size, pre):
    out, _, ninfo = pl.nearest_k(nodes, k)
    sels = [np.ascontiguousarray(out[i, :min(int(ninfo[i]["count"]), k)]) for i in range(len(nodes))]
    sels = [s for s in sels if len(s)]
    off = np.zeros(len(sels) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in sels])
    flat = np.ascontiguousarray(np.concatenate(sels), dtype=np.uint32)
    batch_s = median_wall(lambda: batch_call(pl, off, flat), reps)
    batch = batch_call(pl, off, flat)
    nodes_ms, merge_ms = pl.subtree_batch_time(sels, reps)
    loop_s = median_wall(lambda: loop_call(pl, n, sels), loop_reps)
    assert equal(batch, loop_call(pl, n, sels)), name
    step = max(1, len(sels) // pass_sample)
    single = np.asarray([pl.subtree_time(s, 2) for s in sels[::step]])
    scale = len(sels) / len(sels[::step])
    windows = int(sum(int(size[int(v)]) for v in batch[8]["lca"]))
    rec = {"selections": len(sels), "k": k, "selected": int(off[-1]), "kept": int(batch[0][-1]), "entries": int(batch[1][-1]),
           "gathered": int(batch[8]["n_gathered"].sum()), "windows": windows, "windows_over_nodes": round(windows / n, 3),
           "largest_window": int(max(int(size[int(v)]) for v in batch[8]["lca"])),
           "batch_call_ms": round(batch_s * 1e3, 3), "loop_call_ms": round(loop_s * 1e3, 3), "loop_over_batch": round(loop_s / batch_s, 2),
           "batch_nodes_pass_ms": round(nodes_ms, 4), "batch_merge_pass_ms": round(merge_ms, 4),
           "loop_passes_ms_scaled": round(float(single.sum()) * scale, 3), "loop_passes_measured_on": len(single), "outputs_equal": True}
    say(name, rec)
    return rec


def front_end(pb, d, opts, mode):
    t0 = time.perf_counter()
    r = subprocess.run([EXE, "subtrees", "-i", pb, "-d", d, "-t", "s"] + opts + (["--host"] if mode == "host" else []), capture_output=True, text=True)
    run_s = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-1000:]
    rec = {"run_s": round(run_s, 2)}
    for step in ("cover", "subtrees"):
        m = re.search(r"Selection step %s \(%s\): ([0-9.]+) msec" % (step, mode), r.stderr)
        rec[step + "_ms"] = round(float(m.group(1)), 2)
    m = re.search(r"(\d+) subtrees of (\d+) samples in (\d+) rounds", r.stderr)
    rec["subtrees"], rec["samples"], rec["rounds"] = int(m.group(1)), int(m.group(2)), int(m.group(3))
    files = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".nw") or f.endswith(".tsv")}
    for f in files:
        os.remove(os.path.join(d, f))
    return rec, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--pass-sample", type=int, default=200, help="single calls whose passes are timed alone, then scaled")
    ap.add_argument("--no-front-end", action="store_true")
    ap.add_argument("--host-samples", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1, shape="sars2")
    arrays = st.arrays
    n, m = int(arrays["n"]), int(len(arrays["mut_pos"]))
    par = np.maximum(np.asarray(arrays["parent"], np.int64), 0)
    size, pre = preorder(par)
    leaves = np.flatnonzero(size == 1)
    pl = Placer(arrays)
    pl.subtree_attach()
    out = {"nodes": n, "leaves": int(len(leaves)), "entries": m, "reps": a.reps, "loop_reps": a.loop_reps, "date": time.strftime("%Y-%m-%d"),
           "tool": "tools/bench_subtrees.py"}
    rng = np.random.default_rng(29)
    out["library"] = {"a_nearest500_of_1000": library(pl, n, "a", rng.choice(leaves, 1000, replace=False), 500, a.reps, a.loop_reps, a.pass_sample, size, pre),
                      "b_nearest50_of_10000": library(pl, n, "b", rng.choice(leaves, 10000, replace=False), 50, a.reps, a.loop_reps, a.pass_sample, size, pre)}
    pl.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out) + "\n")
    if not a.no_front_end:
        d = tempfile.mkdtemp(prefix="subtrees_")
        pb = os.path.join(d, "tree.pb")
        time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
        _, _, mut = most_entries(arrays)
        names = ["L%d" % int(v) for v in rng.choice(leaves, 100_000, replace=False)]   # write_workload names leaf j L<j>
        fe = {"mutation": mut, "host_samples": a.host_samples,
              "host_note": "--host ran on the first host_samples of the device run's samples; *_scaled = its step times * device subtrees / host subtrees"}
        open(os.path.join(d, "s.txt"), "w").write("".join(s + "\n" for s in names))
        for key, opts in (("m_N500", ["-m", mut, "-N", "500"]), ("s100000_N2000", ["-s", os.path.join(d, "s.txt"), "-N", "2000"])):
            fe[key + "_device"], _ = front_end(pb, d, opts + ["-u", "u.txt"], "device")
            say(key, fe)
            used = open(os.path.join(d, "u.txt")).read().split("\n")[:a.host_samples]
            open(os.path.join(d, "h.txt"), "w").write("".join(s + "\n" for s in used if s))
            fe[key + "_host_cut"], _ = front_end(pb, d, ["-s", os.path.join(d, "h.txt"), "-N", opts[-1]], "host")
            scale = fe[key + "_device"]["subtrees"] / max(1, fe[key + "_host_cut"]["subtrees"])
            fe[key + "_host_cover_ms_scaled"] = round(fe[key + "_host_cut"]["cover_ms"] * scale, 1)
            fe[key + "_host_subtrees_ms_scaled"] = round(fe[key + "_host_cut"]["subtrees_ms"] * scale, 1)
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
