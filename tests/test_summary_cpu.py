"""matUtils summary without a GPU: the literal restatement of summary.cpp (tests/summary_ref.py) against the rows every hand-shaped
case names, the fast restatement against the literal one, and `matutils-amd summarize --host` byte for byte against the files
rendered from the literal restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import refio
from tests import summary_cases as SC
from tests import summary_ref as R
from tests import synth
from tests import usher_model as UM
from tests.host_harness import HOST_LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
SURVEY_PB = os.path.join(ROOT, "tests", "golden", "survey_ref", "global", "global_assignments.pb")
ANNOTATED_PB = os.path.join(ROOT, "tests", "golden", "pb_pinned", "ref_written_annotated.pb")
TABLES = {"samples.tsv": R.render_samples, "clades.tsv": R.render_clades, "mutations.tsv": R.render_mutations,
          "aberrant.tsv": R.render_aberrant, "sample-clades.tsv": R.render_sample_clades, "roho.tsv": R.render_roho}


def same_answers(T, F, columns):
    """The fast restatement against the literal one: RoHo rows, the mutation table, the clade counts."""
    assert R.fast_roho_rows(F, T) == R.roho_records(T)
    assert F.mutations() == R.mutation_records(T)
    lit, fast = R.clade_records(T, columns), F.clades(columns)
    assert len(lit) == len(fast) == len(columns)
    for a, b in zip(lit, fast):
        for x, y in zip(a, b):
            assert [int(v) for v in x] == [int(v) for v in y]


@pytest.mark.parametrize("case", SC.all_cases(), ids=repr)
def test_case_pins_its_rule(case):
    T = R.Tree(case.arrays, case.ann)
    rows = R.roho_records(T)
    have = {(r[0], r[1]): r for r in rows}
    assert len(have) == len(rows)
    tag = case.tags
    for p, m, c, cc, w, med in case.present:     # the rows that exist because of the rule
        assert have.get((tag[p], m)) == (tag[p], m, tag[c], cc, w, med), (case.rule, p, m)
    for p, m in case.absent:                     # and those the rule removes
        assert (tag[p], m) not in have, (case.rule, p, m)
    if case.total is not None:
        assert len(rows) == case.total, case.rule
    same_answers(T, R.Fast(case.arrays), SC.columns(case))


def test_the_cases_cover_the_rules():
    """What the hand-shaped cases hit between them, counted on the literal restatement."""
    cases = {c.name: c for c in SC.all_cases()}
    erased = {n: R.Fast(c.arrays).roho()[1] for n, c in cases.items()}
    for n in ("leaf_grandchild_erases", "erased_under_sibling", "erased_at_last_node_inside", "deep_recurrence", "masked_eraser", "wide65", "wide257"):
        assert erased[n] >= 1, n
    for n in ("leaf_child_does_not_erase", "leaf_sibling_owns_nothing", "other_parent_allele_or_allele", "plain"):
        assert erased[n] == 0, n
    assert erased["first_node_outside"] == 1     # the root's own candidate; P's are not erased
    medians = {c.present[0][5] for c in cases.values() if c.present}
    assert {6, 7, 9, 10} <= medians
    # the mutation table: a run longer than two blocks, keys apart in one field only, nothing but masked entries, a large position
    assert R.mutation_records(R.Tree(cases["star600"].arrays)) == [(100, 1, 2, 601)]
    assert R.mutation_records(R.Tree(cases["par_or_nuc"].arrays)) == [(100, 1, 2, 3), (100, 1, 8, 1), (100, 4, 2, 1)]
    assert R.mutation_records(R.Tree(cases["all_masked"].arrays)) == []
    assert R.mutation_records(R.Tree(cases["big_position"].arrays)) == [(3, 1, 2, 1), (16777216, 1, 2, 2), (16777217, 1, 2, 1), (20000000, 8, 4, 1)]
    assert R.render_mutations(R.Tree(cases["name_order"].arrays)).split("\n")[1:3] == ["A100G\t1", "A23G\t2"]
    # the clade tables
    c = cases["predecessor_not_ancestor_enclosed"]
    T = R.Tree(c.arrays, c.ann)
    (incl, excl, near), = R.clade_records(T, SC.columns(c))
    leaf = T.leaves().index(c.tags["L"])
    assert near[leaf] == 1 and c.ann[1] == ["outer"] and sorted(zip(incl, excl)) == [(2, 2), (3, 1)]
    c = cases["predecessor_not_ancestor_none"]
    T = R.Tree(c.arrays, c.ann)
    (incl, excl, near), = R.clade_records(T, SC.columns(c))
    assert near[T.leaves().index(c.tags["L"])] == R.NONE and near.count(R.NONE) == 2
    c = cases["annotated_leaf"]
    T = R.Tree(c.arrays, c.ann)
    assert "leafclade" not in R.render_clades(T) and "A\t2\t2\n" in R.render_clades(T)
    c = cases["same_name_twice"]
    assert R.render_clades(R.Tree(c.arrays, c.ann)) == "clade\tinclusive_count\texclusive_count\nB\t5\t3\n"
    c = cases["three_columns"]
    T = R.Tree(c.arrays, c.ann)
    assert "c0" not in R.render_clades(T) and "c0" in R.render_sample_clades(T)
    c = cases["none_as_a_name"]
    T = R.Tree(c.arrays, c.ann)
    assert R.render_sample_clades(T).count("\treal\n") == 3 and "None\t2\t2\n" in R.render_clades(T)
    c = cases["caterpillar_annotated"]
    T = R.Tree(c.arrays, c.ann)
    assert R.render_sample_clades(T).count("\tNone") == 0 and len(SC.columns(c)[0]) == 41


def random_trees():
    out = []
    for seed, n_leaves in ((1, 90), (2, 250), (3, 400)):
        out.append(("random%d" % n_leaves, synth.make_case(seed, n_leaves=n_leaves, n_queries=1, n_sites=60, genome_len=500)[0]))
    out.append(("polytomy", synth.polytomy_case(5, fanouts=(9, 8, 7), n_queries=1, n_sites=60, genome_len=400)[0]))
    out.append(("caterpillar", synth.caterpillar_case(7, depth=60, muts_per_node=2, n_queries=1, n_sites=100, genome_len=400)[0]))
    return out


def random_columns(arrays, seed):
    rng = np.random.default_rng(seed)
    n = arrays["n"]
    return [sorted(rng.choice(n, max(1, n // d), replace=False).tolist()) for d in (7, 40)]


@pytest.mark.parametrize("name,arrays", random_trees(), ids=lambda v: v if isinstance(v, str) else "")
def test_fast_against_literal_on_synthetic_trees(name, arrays):
    same_answers(R.Tree(arrays), R.Fast(arrays), random_columns(arrays, 11))


def test_synthetic_trees_yield_records_and_erasures():
    recs = erased = 0
    for _, arrays in random_trees():
        r, e = R.Fast(arrays).roho()
        recs += len(r)
        erased += e
    assert recs > 0 and erased > 0, (recs, erased)


# ---- the command-line tool, --host ------------------------------------------------------------------------------------------

def load_model(pb):
    """(Tree of the restatement, condensed nodes, condensed leaves) of a .pb, uncondensed as summary_main does."""
    T = refio.load_mutation_annotated_tree(pb)
    cn, cl = len(T.condensed_nodes), len(T.condensed_leaves)
    UM.uncondense_leaves(T)
    arrays = refio.tree_to_bfs_arrays(T)
    ann = [list(n.clade_annotations) for n in T.breadth_first_expansion()]
    return R.Tree(arrays, ann), cn, cl


def write_annotated(case, path):
    """The case as a .pb through the product's own writer (uh_write_pb_annotated beside uh_write_pb_arrays)."""
    L = C.CDLL(HOST_LIB)
    P = C.c_void_p
    L.uh_write_pb_annotated.argtypes = [C.c_uint64, P, P, P, P, P, P, P, P, P, C.c_char_p]
    a = case.arrays
    par = np.asarray(a["parent"]).astype(np.int64)
    keep = [np.where(par < 0, 0xFFFFFFFF, par).astype(np.uint32), np.asarray(a["mut_off"]).astype(np.uint64), np.asarray(a["mut_pos"]).astype(np.int32),
            np.asarray(a["mut_ref"]).astype(np.uint8), np.asarray(a["mut_par"]).astype(np.uint8), np.asarray(a["mut_nuc"]).astype(np.uint8)]
    keep = [np.ascontiguousarray(k) for k in keep]
    names = (C.c_char_p * a["n"])(*[s.encode() for s in a["names"]])
    flat = [s.encode() for v in case.ann for s in v]
    anns = (C.c_char_p * max(len(flat), 1))(*flat)
    off = np.zeros(a["n"] + 1, np.uint64)
    off[1:] = np.cumsum([len(v) for v in case.ann])
    assert L.uh_write_pb_annotated(a["n"], *[k.ctypes.data_as(P) for k in keep], names, off.ctypes.data_as(P), anns, str(path).encode()) == 0
    return str(path)


def run(args, ok=True):
    r = subprocess.run([BIN, "summarize"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


def same_roho(got, want):
    """Every field as text but single_roho: six printed digits and float rounding against the restatement's arithmetic."""
    g, w = got.split("\n"), want.split("\n")
    assert len(g) == len(w) and g[0] == w[0] and g[-1] == w[-1] == ""
    for a, b in zip(g[1:-1], w[1:-1]):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb) == 8 and fa[:6] == fb[:6] and fa[7] == fb[7] == "", (a, b)
        x, y = float(fa[6]), float(fb[6])
        assert abs(x - y) <= max(1e-6, 1e-5 * abs(y)), (a, b)


def check_tables(pb, out, extra=()):
    """All six tables of one run against the restatement; returns the model and the texts read."""
    T, cn, cl = load_model(pb)
    run(["-i", pb, "-A", "-R", "roho.tsv", "-C", "sample-clades.tsv", "-d", out] + list(extra))
    texts = {}
    for name, render in TABLES.items():
        got = texts[name] = open(os.path.join(str(out), name)).read()
        if name == "roho.tsv":
            same_roho(got, render(T))
        else:
            assert got == render(T), name
    return T, texts


def test_host_tables_on_the_survey_tree(tmp_path):
    T, texts = check_tables(SURVEY_PB, tmp_path, ["--host"])
    assert texts["roho.tsv"].count("\n") > 5 and texts["mutations.tsv"].count("\n") > 300


def test_host_tables_on_the_annotated_tree(tmp_path):
    T, texts = check_tables(ANNOTATED_PB, tmp_path, ["--host"])
    assert R.num_annotations(T) >= 1 and texts["clades.tsv"].count("\n") > 1 and "\tNone" in texts["sample-clades.tsv"] + "\tNone"


CLI_CASES = ["later_child_owns", "twice_on_one_child", "leaf_grandchild_erases", "masked_eraser", "owner_between_even", "wide65", "caterpillar",
             "name_order", "same_name_twice", "annotated_leaf", "annotated_root", "three_columns", "no_annotated_ancestor",
             "predecessor_not_ancestor_enclosed", "predecessor_not_ancestor_none", "fewer_annotations", "none_as_a_name", "caterpillar_annotated"]


@pytest.mark.parametrize("name", CLI_CASES)
def test_host_tables_on_hand_shaped_trees(name, tmp_path):
    case = {c.name: c for c in SC.all_cases()}[name]
    pb = write_annotated(case, tmp_path / "case.pb")
    T, texts = check_tables(pb, tmp_path, ["--host"])
    assert T.n == case.arrays["n"]
    if case.total:
        assert texts["roho.tsv"].count("\n") >= 1 + case.total


def test_options(tmp_path):
    for opt in (["-t", "x.tsv"], ["--translate", "x.tsv"], ["-g", "a.gtf"], ["-f", "a.fa"], ["-E"], ["--expanded-roho"], ["-H", "h.tsv"], ["-N", "n.tsv"]):
        r = run(["-i", SURVEY_PB, "-d", tmp_path, "--host"] + opt, ok=False)
        assert r.returncode == 1 and r.stderr.count("\n") == 1 and "not supported" in r.stderr and opt[0] in r.stderr
    r = run(["--host", "-s", "s.tsv", "-d", tmp_path], ok=False)
    assert r.returncode == 1 and "--input-mat" in r.stderr
    assert run(["-h"]).stdout.startswith("Usage: matutils-amd summarize")
    for word in ("--translate", "--expanded-roho", "--haplotype", "--node-stats", "--host"):
        assert word in run(["--help"]).stdout
    for word in ("introduce", "summary"):       # the reference's own spelling stays refused; the message names the one that runs
        r = subprocess.run([BIN, word], capture_output=True, text=True)
        assert r.returncode == 1 and "summarize" in r.stderr
    # -A names its four files; long names; a directory that does not exist yet
    d = tmp_path / "new"
    run(["--input-mat", SURVEY_PB, "--get-all-basic", "--output-directory", d, "--host"])
    assert sorted(os.listdir(d)) == ["aberrant.tsv", "clades.tsv", "mutations.tsv", "samples.tsv"]
    run(["--input-mat", SURVEY_PB, "--samples", "a.tsv", "--clades", "b.tsv", "--sample-clades", "c.tsv", "--mutations", "d.tsv", "--aberrant", "e.tsv",
         "--calculate-roho", "f.tsv", "--threads", "3", "--output-directory", d, "--host"])
    for a, b in (("a", "samples"), ("b", "clades"), ("d", "mutations"), ("e", "aberrant")):
        assert open(d / (a + ".tsv")).read() == open(d / (b + ".tsv")).read()


def test_basic_counts_and_mutation_stats(tmp_path):
    for pb in (SURVEY_PB, ANNOTATED_PB):
        T, cn, cl = load_model(pb)
        r = run(["-i", pb, "--host"])
        assert r.stdout == R.render_basic(T, cn, cl)
        r = run(["-i", pb, "--host", "-M"])      # -M prints to stdout and is no table: the basic counts follow
        assert r.stdout == R.render_mut_stats(T) + R.render_basic(T, cn, cl)
        r = run(["-i", pb, "--host", "-M", "-s", "s.tsv", "-d", tmp_path])
        assert r.stdout == R.render_mut_stats(T)
