"""matUtils summary --translate without a GPU: per hand-shaped case the literal restatement of translate.cpp (tests/translate_ref.py)
against the lines the case works out by hand, the fast restatement against the literal one, and `matutils-amd translate --host` byte
for byte against the text rendered from the literal restatement; the same on the survey tree with a generated FASTA and GTF."""
import os
import subprocess

import numpy as np
import pytest

from tests import stdorder
from tests import summary_ref as SR
from tests import test_summary_cpu as SCPU
from tests import translate_cases as TC
from tests import translate_ref as R

BIN = SCPU.BIN
SURVEY_PB = SCPU.SURVEY_PB


def pins_its_rule(case):
    """The case does what it says, on the literal restatement; the fast restatement agrees."""
    T, codons = case.tree(), case.codons()
    info = R.info(T, codons)
    assert R.consistent(T, codons) == case.device, case.rule
    if case.lines is not None:
        assert R.render(T, codons) == R.HEADER + "".join(line + "\n" for line in case.lines), case.rule
    for key, want in case.counts.items():
        if key == "first_inconsistent":
            want = case.entry(*want)
        elif key == "first_duplicate":
            want = case.tags[want]
        assert info[key] == want, (case.rule, key)
    # the fast restatement: the same counts always, the same records where the closed form holds
    F = R.Fast(case.arrays, *R.slot_tables(codons))
    assert F.info == info
    if case.device:
        recs = R.records(T, codons)
        assert F.records == recs and len(recs) == info["n_records"]
        assert len({r[0] for r in recs}) == info["n_nodes"]


def test_the_cases_cover_the_rules():
    from usher_amd import Placer, _lib
    assert Placer.TR_RECORD.itemsize == 28 and Placer.TR_INFO.itemsize == 40            # what records() and info() are shaped after
    assert {"ugp_translate_attach", "ugp_translate_codons", "ugp_translate", "ugp_translate_chunked"} <= set(_lib.SYMBOLS)
    cases = TC.by_name()
    codons = cases["single_slots"].codons()
    assert [(c.gene, c.number) for c in codons[10:17]] == [("B", k) for k in range(7)]       # numbering continues over the CDS lines
    assert [c.init for c in codons[17:21]] == ["TTT", "GGG", "AAA", "CCC"] and codons[17].start == 70 and codons[17].sign == -1
    assert (codons[21].gene, codons[21].start) == ("E", 72) and codons[22].gene == "C"
    pos, init = R.slot_tables(codons)
    assert pos[17].tolist() == [71, 70, 69] and pos[21].tolist() == [73, 74, 75] and bytes(init[17]) == b"TTT"
    # the strict bound of the - loop: a CDS whose walk lands on its start drops that codon
    short = R.build_codon_map(TC.gtf_line("M", 62, 71, "-") + "\n", TC.GENOME)
    assert [c.start for c in short] == [70, 67, 64]
    recs = R.records(cases["two_frames"].tree(), cases["two_frames"].codons())
    assert [r[1] for r in recs] == [1, 22, 2]                                                  # by lowest position, then by index
    recs = R.records(cases["wide65"].tree(), cases["wide65"].codons())
    assert len({r[1] for r in recs if r[0] == 1}) == 43 and sum(e != R.NIL for r in recs if r[0] == 1 for e in r[4]) == 65
    assert TC.n_items(cases["star600"]) == 600 and TC.n_items(cases["caterpillar"]) > 640
    assert max(len(SR.Tree(cases["caterpillar"].arrays).rsearch(v, False)) for v in range(cases["caterpillar"].arrays["n"])) >= 300


# ---- the command-line tool, --host ------------------------------------------------------------------------------------------

def write_inputs(case, d):
    d = str(d)
    pb = SCPU.write_annotated(type("C", (), {"arrays": case.arrays, "ann": [[] for _ in range(case.arrays["n"])]})(), os.path.join(d, "case.pb"))
    with open(os.path.join(d, "ref.fa"), "w", newline="") as f:
        f.write(case.fasta)
    with open(os.path.join(d, "genes.gtf"), "w", newline="") as f:
        f.write(case.gtf)
    return pb, os.path.join(d, "genes.gtf"), os.path.join(d, "ref.fa")


def run(args, ok=True):
    r = subprocess.run([BIN, "translate"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


@pytest.mark.parametrize("case", TC.all_cases(), ids=repr)
def test_host_walk_on_hand_shaped_trees(case, tmp_path):
    pins_its_rule(case)
    pb, gtf, fa = write_inputs(case, tmp_path)
    run(["-i", pb, "-g", gtf, "-f", fa, "-t", "out.tsv", "-d", tmp_path, "--host"])
    # std::sort is not stable: where a node stores a position twice the restatement orders the ties as this library does
    sort = stdorder.StdOrder(tmp_path).sort if case.name.startswith("duplicate") else R._stable
    # the tree as loaded: the .pb names internal nodes its own way, and loading (add_mutation) keeps a node's mutations sorted by
    # position and merges those that share one, so stored disorder and repeated positions reach the library through its ABI only
    T = SCPU.load_model(pb)[0]
    assert T.n == case.arrays["n"]
    assert open(tmp_path / "out.tsv", newline="").read() == R.render(T, case.codons(), sort)


def survey_inputs(d):
    """The survey tree with a FASTA that carries its reference alleles and a GTF of + genes (one with two CDS lines, one
    overlapping pair) and a - gene."""
    from oracle import refio
    from tests import usher_model as UM
    Tm = refio.load_mutation_annotated_tree(SURVEY_PB)
    UM.uncondense_leaves(Tm)
    arrays = refio.tree_to_bfs_arrays(Tm)
    pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
    top = int(pos.max()) + 40
    rng = np.random.default_rng(12)
    genome = rng.choice(list("ACGT"), top)
    for p, r in zip(pos.tolist(), np.asarray(arrays["mut_ref"]).tolist()):
        if p > 0 and 1 <= r <= 15:
            genome[p - 1] = SR.NUC[r]
    fasta = ">survey\n" + "\n".join("".join(genome[i:i + 70]) for i in range(0, top, 70)) + "\n"
    third = top // 3
    gtf = "\n".join([TC.gtf_line("one", 10, third), TC.gtf_line("two", third + 5, third + 304), TC.gtf_line("two", third + 400, 2 * third),
                     TC.gtf_line("over", third - 100, third + 199), TC.gtf_line("rev", 2 * third + 10, top - 3, "-")]) + "\n"
    with open(os.path.join(str(d), "ref.fa"), "w") as f:
        f.write(fasta)
    with open(os.path.join(str(d), "genes.gtf"), "w") as f:
        f.write(gtf)
    return SR.Tree(arrays), R.build_codon_map(gtf, R.build_reference(fasta)), os.path.join(str(d), "genes.gtf"), os.path.join(str(d), "ref.fa")


def test_host_walk_on_the_survey_tree(tmp_path):
    T, codons, gtf, fa = survey_inputs(tmp_path)
    run(["--input-mat", SURVEY_PB, "--input-gtf", gtf, "--input-fasta", fa, "--translate", "t.tsv", "--output-directory", tmp_path / "new",
         "--threads", "2", "--host"])
    got = open(tmp_path / "new" / "t.tsv").read()
    assert got == R.render(T, codons, stdorder.StdOrder(tmp_path).sort)
    assert got.count("\n") > 200 and "rev:" in got and "over:" in got and "two:" in got


def test_options_and_errors(tmp_path):
    case = TC.by_name()["single_slots"]
    pb, gtf, fa = write_inputs(case, tmp_path)
    base = ["-i", pb, "-t", "o.tsv", "-d", tmp_path, "--host"]
    r = run(base + ["-f", fa], ok=False)
    assert r.returncode == 1 and r.stderr == "ERROR: You must specify a GTF file with -g\n"
    r = run(base + ["-g", gtf], ok=False)
    assert r.returncode == 1 and r.stderr == "ERROR: You must specify a FASTA reference file with -f\n"
    r = run(base, ok=False)
    assert r.stderr == "ERROR: You must specify a GTF file with -g\nERROR: You must specify a FASTA reference file with -f\n"
    assert "--input-mat" in run(["-g", gtf, "-f", fa, "-t", "o.tsv"], ok=False).stderr

    def with_gtf(text):
        with open(tmp_path / "bad.gtf", "w") as f:
            f.write(text)
        r = run(base + ["-f", fa, "-g", tmp_path / "bad.gtf"], ok=False)
        assert r.returncode == 1
        return r.stderr.split("\n")[-2]

    assert with_gtf(TC.gtf_line("A", 1, 30).replace("gene_id", "gene_name") + "\n") == "ERROR: GTF file formatted incorrectly. Please see the wiki for details."
    for text in (TC.gtf_line("A", 70, 78), TC.gtf_line("A", 70, 76, "-"), TC.gtf_line("A", 0, 5)):
        with pytest.raises(R.BadInput):
            R.build_codon_map(text + "\n", TC.GENOME)
        msg = with_gtf(text + "\n")
        assert msg.startswith("ERROR") and "past the FASTA" in msg
    short = "\t".join(TC.gtf_line("A", 1, 30).split("\t")[:8])
    for text in (short + "\n", TC.gtf_line("A", 1, 30) + "\nstray words\n"):
        with pytest.raises(R.BadInput):
            R.build_codon_map(text, TC.GENOME)
        assert "fewer than 9 columns" in with_gtf(text)
    r = run(base + ["-g", gtf, "-f", tmp_path / "none.fa"], ok=False)
    assert "Could not open the fasta file" in r.stderr
    assert run(["-h"]).stdout.startswith("Usage: matutils-amd translate")
    for word in ("--input-gtf", "--input-fasta", "--translate", "--output-directory", "--threads", "--host"):
        assert word in run(["--help"]).stdout
    top = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert top.returncode == 0 and "translate --help" in top.stdout
    r = subprocess.run([BIN, "introduce"], capture_output=True, text=True)
    assert r.returncode == 1 and "translate" in r.stderr
