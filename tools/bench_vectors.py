"""ugp_vectors (ugp_vectors.hip: the excess and imputed mutations of the placement nodes) on the synthetic MAT of bench.py, beside
the host's node_vecs in `usher-amd -n`.

    python tools/bench_vectors.py [--nodes 10000000] [--pairs 16384,1000000] [--reps 5] [--front-end 10000,1000000]
                                  [--caterpillar 1000000] [--caterpillar-distinct 65536] [--out profiles/vectors_bench.json]
Library: the winners of ugp_place_batch for that many samples; the call from host buffers to host lists (median of --reps after a
warm-up), the two passes alone (device events, no copies; repeated until the window is above half a second), entries and bytes
returned.  --caterpillar: one pair a call on a caterpillar that deep whose one position flips at every level; --caterpillar-distinct:
the same with a position of its own on every level, the shape whose back-mutations the ordering pass ranks by counting (0: not run).
Front end: whole `usher-amd -n` runs with --device-vectors and --host-vectors, alternating, outputs compared; the step is the profile
line's "vectors of the winning node (pass 2)" seconds (on the device path: the one call and nothing else).  Prints one JSON line."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import time_load  # noqa: E402
from tools.bench_relatives import median_wall, say  # noqa: E402
from tools.bench_subtree import caterpillar, topology  # noqa: E402
from usher_amd import Placer, QueryBatch  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402

EXE = os.path.join(ROOT, "usher_amd", "bin", "usher-amd")


def library(pl, batch, nodes, reps, name):
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
    got = pl.vectors(batch, nodes)                       # warm-up, and the room the timed calls need
    tot = pl._vec_totals
    wall = median_wall(lambda: pl.vectors(batch, nodes, ex_cap=tot[0], im_cap=tot[1]), reps)
    c1, f1 = pl.vectors_time(batch, nodes, reps=1)
    inner = max(1, min(2000, int(500.0 / max(c1 + f1, 1e-3)) + 1))   # a window of half a second and more
    count_ms, fill_ms = pl.vectors_time(batch, nodes, reps=inner)
    info = got[0]
    rec = {"pairs": int(len(nodes)), "refused": int(info["refused"].sum()), "excess_entries": tot[0], "imputed_entries": tot[1],
           "branch_entries": int(info["n_branch"].sum()), "bytes_returned": int(8 * (tot[0] + tot[1]) + info.nbytes + 16 * (len(nodes) + 1)),
           "call_ms": round(wall * 1e3, 3), "count_pass_ms": round(count_ms, 4), "fill_pass_ms": round(fill_ms, 4), "pass_reps": inner,
           "pairs_per_s_call": round(len(nodes) / wall, 1)}
    say(name, rec)
    return rec


def front_end(pb, vcf, d, flag):
    out = os.path.join(d, "out_" + flag.strip("-"))
    os.makedirs(out, exist_ok=True)
    t0 = time.perf_counter()
    r = subprocess.run([EXE, "-i", pb, "-v", vcf, "-n", flag, "-d", out], capture_output=True, text=True, env=dict(os.environ, USHER_AMD_PROFILE="1"))
    run_s = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-1000:]
    step = re.search(r"vectors of the winning node \(pass 2\) ([0-9.]+) s", r.stderr)
    loop = re.search(r"per-sample loop ([0-9.]+) s", r.stderr)
    return {"run_s": round(run_s, 3), "vectors_step_s": float(step.group(1)) if step else None, "per_sample_loop_s": float(loop.group(1)) if loop else None}, \
        open(os.path.join(out, "placement_stats.tsv"), "rb").read()


def deep_caterpillar(depth, distinct):
    """ONE pair a call on the deepest spine node of a caterpillar that deep (a pair is a wave: two pairs in a call would follow the
    parent chain side by side and take the time of one): a sample without rows, then one with a row at a spine position.  distinct:
    every spine level has a position of its own, so the sample without rows has `depth` back-mutations to order; else one position
    flips at every level and there is one."""
    arrays, _ = caterpillar(depth)
    n = int(arrays["n"])
    first = 1
    if distinct:
        j = np.arange(1, n, dtype=np.int64)
        spine = j % 2 == 1
        arrays["mut_pos"] = np.where(spine, 10 + (j + 1) // 2, 2).astype(np.int32)
        arrays["mut_ref"] = arrays["mut_par"] = np.where(spine, 1, 4).astype(np.int8)
        arrays["mut_nuc"] = np.where(spine, 2, 1).astype(np.int8)
        first = 11
    pl = Placer(topology(arrays))
    pl.vectors_attach(arrays)
    node = np.asarray([n - 2], np.uint32)
    rec = {"depth": depth, "pairs_per_call": 1}
    for name, smp in (("no_rows", {"pos": [], "ref": [], "nuc": [], "is_missing": []}), ("one_row", {"pos": [first], "ref": [1], "nuc": [4], "is_missing": [0]})):
        batch = QueryBatch([smp])
        pl.vectors(batch, node)   # warm-up
        t0 = time.perf_counter()
        got = pl.vectors(batch, node)
        wall = time.perf_counter() - t0
        count_ms, fill_ms = pl.vectors_time(batch, node, reps=1)
        rec[name] = {"excess_entries": pl._vec_totals[0], "call_ms": round(wall * 1e3, 1), "count_pass_ms": round(count_ms, 2),
                     "fill_pass_ms": round(fill_ms, 2), "set_difference": int(got[0]["set_difference"][0])}
    pl.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--pairs", default="16384,1000000")
    ap.add_argument("--front-end", default="10000,1000000")
    ap.add_argument("--rounds", type=int, default=2, help="whole runs per path and size, alternating")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--caterpillar", type=int, default=1_000_000)
    ap.add_argument("--caterpillar-distinct", type=int, default=65_536)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000 if a.nodes >= 1_000_000 else 1500, seed=1)
    arrays = st.arrays
    out = {"nodes": int(arrays["n"]), "entries": int(len(arrays["mut_pos"])), "reps": a.reps, "date": time.strftime("%Y-%m-%d"),
           "tool": "tools/bench_vectors.py", "library": {}, "front_end": {}}
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.vectors_attach()
    out["attach_s"] = round(time.perf_counter() - t0, 3)
    for n in [int(x) for x in a.pairs.split(",") if x]:
        q = st.queries(n, seed=1017)
        batch = QueryBatch.from_csr(q["ent_off"], q["pos"], q["ref"], q["nuc"], q["is_missing"])
        t0 = time.perf_counter()
        res = pl.place(batch)
        place_s = time.perf_counter() - t0
        out["library"]["winners_%d" % n] = dict(library(pl, batch, res["best_j"], a.reps, "winners %d" % n), rows=int(q["ent_off"][-1]),
                                                place_call_ms=round(place_s * 1e3, 1))
    pl.close()
    sizes = [int(x) for x in a.front_end.split(",") if x]
    if sizes:
        d = tempfile.mkdtemp(prefix="vectors_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        pb = os.path.join(d, "tree.pb")
        L = time_load.host_lib()
        time_load.write_workload(L, st, None, 0, pb, None)
        for n in sizes:
            q = st.queries(n, seed=1005)
            vcf = os.path.join(d, "q%d.vcf" % n)
            time_load.write_workload(L, st, q, n, None, vcf)
            runs = {"--device-vectors": [], "--host-vectors": []}
            same = True
            for _ in range(a.rounds):
                files = []
                for flag in runs:
                    rec, stats = front_end(pb, vcf, d, flag)
                    runs[flag].append(rec)
                    files.append(stats)
                    say("%d %s" % (n, flag), rec)
                same = same and files[0] == files[1]
            out["front_end"]["queries_%d" % n] = {"device_vectors": runs["--device-vectors"], "host_vectors": runs["--host-vectors"],
                                                  "placement_stats_equal": bool(same)}
            os.remove(vcf)
        shutil.rmtree(d, ignore_errors=True)
    st.close()
    for key, depth, distinct in (("caterpillar", a.caterpillar, False), ("caterpillar_distinct", a.caterpillar_distinct, True)):
        if not depth:
            continue
        try:
            out[key] = deep_caterpillar(depth, distinct)
            say(key, out[key])
        except Exception as e:   # a finding to write down, not a reason to lose the rest
            out[key] = {"depth": depth, "error": str(e)[:300]}
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
