"""Times of matUtils summary --translate on the device (ugp_translate_attach / _codons / ugp_translate) on a synthetic MAT of the sars2
polytomy shape, beside the front end's own host path (`matutils-amd translate --host`: the reference's serial do / undo walk) on the
same tree written as a .pb.

    python tools/bench_translate.py [--nodes 10000000] [--reps 5] [--host-limit 600] [--out profiles/translate_bench.json]

The FASTA is random letters with the tree's reference alleles at the positions it mutates; the generator stores the true state above
every mutation as its parent allele, so with + strand genes every coding entry is consistent and the device answers (the tool
asserts that).  The GTF is a few + genes laid out like SARS-CoV-2's: one gene in two CDS lines that overlap by a frame shift, and one
gene inside another in a different frame.  Each time is the median of --reps runs after one warm-up run; the calls are synchronous.
Prints one JSON line."""
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
from usher_amd import Placer  # noqa: E402
from usher_amd import synth as gsynth  # noqa: E402

EXE = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
NUC = "NACMGRSVTWYHKDBN"
GENES = [("ORF1ab", 266, 13483), ("ORF1ab", 13468, 21555), ("S", 21563, 25384), ("N", 28274, 29533), ("ORF9b", 28284, 28577)]


def median_s(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def genome_of(arrays, length):
    g = np.array(list("ACGT"))[np.random.default_rng(7).integers(0, 4, length)]
    pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
    ok = pos > 0
    g[pos[ok] - 1] = np.array(list(NUC))[np.asarray(arrays["mut_ref"]).astype(np.int64)[ok]]
    return "".join(g)


def gtf_text():
    return "".join("ref\tbench\tCDS\t%d\t%d\t.\t+\t0\tgene_id \"%s\"; transcript_id \"%s\";\n" % (a, b, g, g) for g, a, b in GENES)


def codon_table(genome):
    """The + strand loops of build_codon_map: first CDS line of a gene, then its further ones."""
    pos, init, seen = [], [], []
    for gene, _, _ in GENES:
        if gene in seen:
            continue
        seen.append(gene)
        for g, a, b in GENES:
            if g != gene:
                continue
            for p in range(a - 1, b, 3):
                pos.append([p + 1, p + 2, p + 3])
                init.append([ord(c) for c in genome[p:p + 3]])
    return np.asarray(pos, np.int32), np.asarray(init, np.uint8)


def device(arrays, slot_pos, slot_init, reps):
    pl = Placer(arrays)
    t0 = time.perf_counter()
    pl.translate_attach()
    out = {"nodes": int(arrays["n"]), "entries": len(arrays["mut_pos"]), "codons": len(slot_pos), "attach_s": round(time.perf_counter() - t0, 4)}
    t0 = time.perf_counter()
    pl.translate_codons(slot_pos, slot_init)
    out["codons_s"] = round(time.perf_counter() - t0, 4)
    recs, info = pl.translate()
    assert int(info["n_inconsistent"]) == 0 and int(info["n_duplicate"]) == 0, info
    n = len(recs)
    out["records"], out["nodes_with_records"] = n, int(info["n_nodes"])
    out["translate_s"] = round(median_s(lambda: pl.translate(cap=n), reps), 5)       # one call: passes, counts and the records copied to the host
    out["passes_device_ms"] = round(pl.translate_time(reps), 4)
    pl.close()
    return out


def front_end(st, genome, limit):
    d = tempfile.mkdtemp(prefix="translate_")
    pb, fa, gtf = os.path.join(d, "tree.pb"), os.path.join(d, "ref.fa"), os.path.join(d, "genes.gtf")
    time_load.write_workload(time_load.host_lib(), st, None, 0, pb, None)
    open(fa, "w").write(">ref\n" + "\n".join(genome[i:i + 70] for i in range(0, len(genome), 70)) + "\n")
    open(gtf, "w").write(gtf_text())
    out = {}
    try:
        for mode, extra in (("device", []), ("host", ["--host"])):
            t0 = time.perf_counter()
            try:
                r = subprocess.run([EXE, "translate", "-i", pb, "-g", gtf, "-f", fa, "-t", "t.tsv", "-d", os.path.join(d, mode)] + extra,
                                   capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                out[mode] = {"timed_out_after_s": limit}
                continue
            assert r.returncode == 0, r.stderr[-1000:]
            assert "walking it on the host" not in r.stderr, r.stderr[-1000:]
            ms = re.findall(r"Completed in (\d+) msec", r.stderr)
            out[mode] = {"wall_s": round(time.perf_counter() - t0, 2), "table_ms": int(ms[-1]) if ms else None}
        files = [os.path.join(d, mode, "t.tsv") for mode in ("device", "host")]
        if all(os.path.exists(f) for f in files):
            out["same_bytes"] = open(files[0], "rb").read() == open(files[1], "rb").read()
            out["lines"] = open(files[0]).read().count("\n") - 1
    finally:
        for root, _, names in os.walk(d, topdown=False):
            for f in names:
                os.remove(os.path.join(root, f))
            os.rmdir(root)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-limit", type=float, default=600.0, help="seconds a front-end run may take (0: skip the front end)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = gsynth.SynthTree(a.nodes, n_sites=25000, seed=1, shape="sars2")
    genome = genome_of(st.arrays, st.genome_len)
    slot_pos, slot_init = codon_table(genome)
    out = {"tool": "tools/bench_translate.py", "date": time.strftime("%Y-%m-%d"), "shape": "sars2", "reps": a.reps, "host_limit_s": a.host_limit,
           "genes": GENES, "device": device(st.arrays, slot_pos, slot_init, a.reps)}
    if a.host_limit:
        out["front_end"] = front_end(st, genome, a.host_limit)
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
