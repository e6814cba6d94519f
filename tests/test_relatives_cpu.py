"""Per-sample relatives without a GPU: the literal restatement of get_closest_samples (tests/relatives_ref.py) against the closed
form on random, polytomy, caterpillar and hand-shaped trees with every node as target, the ABI surface of the ugp_relatives calls,
the argument errors of `matutils-amd relatives`, and `relatives --host` byte for byte against the text rendered from the literal
restatement on the survey tree."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import relatives_cases as RC
from tests import relatives_ref as R
from tests import synth
from usher_amd import Placer, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
PB = os.path.join(ROOT, "tests", "golden", "survey_ref", "global", "global_assignments.pb")


def _trees():
    out = {"random%d" % s: synth.make_case(s, n_leaves=nl, n_queries=1, n_sites=60, genome_len=400, p_masked=pm,
                                           mut_counts=mc)[0]
           for s, nl, pm, mc in ((81, 60, 0.2, (0, 0, 1, 1, 1, 2, 3)), (82, 140, 0.4, (0, 0, 0, 0, 1, 2)), (83, 100, 0.1, (0, 0, 0, 0, 0, 0, 0, 0, 1)))}
    out["polytomy"] = synth.polytomy_case(84, fanouts=(6, 9, 5), n_queries=1, genome_len=3000, n_sites=200)[0]
    out["caterpillar"] = synth.caterpillar_case(85, depth=40, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=300)[0]
    out.update(RC.hand_cases())
    return out


TREES = _trees()


@pytest.mark.parametrize("name", list(TREES))
def test_literal_equals_closed_form(name):
    arrays = TREES[name]
    if name.startswith("random"):
        assert (np.asarray(arrays["mut_pos"]) < 0).sum() > 0
    T = R.Tree(arrays)
    rank = np.random.default_rng(5).permutation(arrays["n"])
    F = R.Fast(arrays, rank)
    top = int(F.cumb.max()) + 1
    for v in range(arrays["n"]):
        assert R.literal(T, v, False, 0, rank) == F.closest(v), (v, "closest")
        for k in (0, 1, 2, 5, top):
            assert R.literal(T, v, True, k) == F.within(v, k), (v, k)
    assert F.closest(0)["levels"] == 0 and F.within(0, top)["count"] == 0   # the root has no relatives


def test_hand_cases_do_what_they_say():
    arrays, t, want = RC.append_across_levels()
    r = R.literal(R.Tree(arrays), t, False)
    assert (r["nodes"], r["dist"], r["levels"]) == (want, 2, 3)
    arrays, t, want = RC.replace_at_deeper_level()
    r = R.literal(R.Tree(arrays), t, False)
    assert (r["nodes"], r["dist"], r["levels"]) == (want, 1, 2)
    arrays = RC.chain()
    assert all(R.literal(R.Tree(arrays), v, False)["count"] == 0 for v in range(arrays["n"]))
    assert R.literal(R.Tree(RC.two_nodes()), 1, False) == {"nodes": [], "dist": 0, "count": 0, "levels": 1, "best": R.NONE}
    arrays = RC.all_zero()
    T = R.Tree(arrays)
    leaves = [v for v in range(arrays["n"]) if T.is_leaf(v)]
    for v in leaves:   # every other leaf ties, and the climb reaches the root
        r = R.literal(T, v, False)
        assert sorted(r["nodes"]) == [u for u in leaves if u != v] and r["dist"] == 0
    arrays = RC.caterpillar()
    assert max(R.literal(R.Tree(arrays), v, False)["levels"] for v in range(arrays["n"])) > 100
    arrays = RC.no_leaf_sibling()
    T = R.Tree(arrays)
    assert T.is_leaf(3) and [T.is_leaf(c) for c in T.kids[T.par[3]]] == [True, False]
    assert R.literal(T, 3, False)["nodes"] == [8]   # two levels down the internal sibling: nothing is pruned


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    names = ("ugp_relatives_attach", "ugp_relatives_closest", "ugp_relatives_within", "ugp_relatives_closest_chunked",
             "ugp_relatives_within_chunked")
    for name in names:
        assert re.search(r"\bint %s\(ugp_mat \*mat" % name, hdr) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    m = re.search(r"typedef struct ugp_rel_info \{(.*?)\} ugp_rel_info;", hdr, re.S)
    fields = [f.strip() for f in re.search(r"uint32_t ([\w, ]+);", m.group(1)).group(1).split(",")]
    assert tuple(fields) == Placer.REL_INFO.names == ("dist", "count", "levels", "best") and Placer.REL_INFO.itemsize == 16
    assert int(re.search(r"#define UGP_REL_BLOCK (\d+)", hdr).group(1)) == Placer.REL_BLOCK
    # no handle: an error code, not a crash
    L = _lib.lib()
    assert L.ugp_relatives_attach(None, None, None) == -1
    assert L.ugp_relatives_closest(None, 1, None, None, None, None, 0, None) == -1
    assert L.ugp_relatives_within(None, 1, None, 2, None, None, None, 0, None) == -1
    assert L.ugp_relatives_closest_chunked(None, 1, None, None, None, None, 0, None, 3) == -1
    assert L.ugp_relatives_within_chunked(None, 1, None, 2, None, None, None, 0, None, 3) == -1


def test_name_ranks_follow_unsigned_bytes():
    names = ["node_10", "node_9", "Zeta", "alpha", "node_100", "éclair", "a", "B|2020", "B.1", "~last"]
    rank = Placer.name_ranks(names)
    assert sorted(rank.tolist()) == list(range(len(names)))
    by_rank = [names[j] for j in np.argsort(rank)]
    assert by_rank == ["B.1", "B|2020", "Zeta", "a", "alpha", "node_10", "node_100", "node_9", "~last", "éclair"]
    assert rank[0] < rank[1] and rank[4] < rank[1]   # "node_10" < "node_100" < "node_9": no numeric order


# ---- the command-line tool --------------------------------------------------------------------------------------------------

def run(args, ok=True):
    r = subprocess.run([BIN, "relatives"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


@pytest.fixture(scope="module")
def survey():
    from oracle import refio
    from tests import usher_model as UM
    Tm = refio.load_mutation_annotated_tree(PB)
    UM.uncondense_leaves(Tm)
    arrays = refio.tree_to_bfs_arrays(Tm)
    T = R.Tree(arrays)
    names = arrays["names"]
    leaves = [v for v in range(T.n) if T.is_leaf(v)]   # get_leaves_ids: breadth-first
    return T, names, leaves


def render_closest(T, names, samples, break_ties):
    out = []
    for v in samples:
        r = R.literal(T, v, False)
        if not r["nodes"]:
            continue
        rel = [names[u] for u in r["nodes"]]
        # std::string::operator< compares unsigned bytes
        out.append("%s\t%s\t%d\n" % (names[v], min(rel, key=lambda s: s.encode()) if break_ties else ",".join(rel), r["dist"]))
    return "".join(out)


def render_within(T, names, samples, k):
    out = []
    for v in samples:
        rel = [names[u] for u in R.literal(T, v, True, k)["nodes"]]
        out.append(names[v] + ("\t" + ",".join(rel) if rel else "") + "\n")
    return "".join(out)


def test_host_walk_on_the_survey_tree(survey, tmp_path):
    T, names, leaves = survey
    run(["-i", PB, "-V", "closest.tsv", "-d", tmp_path, "--host"])
    got = open(tmp_path / "closest.tsv", newline="").read()
    assert got == render_closest(T, names, leaves, False) and got.count("\n") > 100 and "," in got
    run(["--input-mat", PB, "--closest-relatives", "one.tsv", "--break-ties", "--output-directory", tmp_path / "new", "--threads", "2", "--host"])
    got = open(tmp_path / "new" / "one.tsv", newline="").read()
    assert got == render_closest(T, names, leaves, True) and "," not in got
    # both files in one run; thresholds 0 and 3
    run(["-i", PB, "-V", "c.tsv", "--within-distance", "w0.tsv", "-d", tmp_path, "--host"])
    assert open(tmp_path / "c.tsv", newline="").read() == render_closest(T, names, leaves, False)
    w0 = open(tmp_path / "w0.tsv", newline="").read()
    assert w0 == render_within(T, names, leaves, 0)
    run(["-i", PB, "--within-distance", "w3.tsv", "--distance-threshold", "3", "-d", tmp_path, "--host"])
    w3 = open(tmp_path / "w3.tsv", newline="").read()
    assert w3 == render_within(T, names, leaves, 3)
    assert w3.count("\n") == len(leaves) and len(w3) > len(w0) and any("\t" not in line for line in w3.split("\n")[:-1])


def test_host_walk_on_a_shuffled_subset(survey, tmp_path):
    T, names, leaves = survey
    rng = np.random.default_rng(6)
    pick = [int(v) for v in rng.permutation(leaves)[:40]] + [int(v) for v in rng.permutation([v for v in range(1, T.n) if not T.is_leaf(v)])[:5]]
    pick = [pick[i] for i in rng.permutation(len(pick))]
    with open(tmp_path / "s.txt", "w") as f:
        f.write("".join(names[v] + "\n" for v in pick))
    run(["-i", PB, "-s", tmp_path / "s.txt", "-V", "c.tsv", "-q", "--within-distance", "w.tsv", "--distance-threshold", "2", "-d", tmp_path, "--host"])
    assert open(tmp_path / "c.tsv", newline="").read() == render_closest(T, names, pick, True)
    assert open(tmp_path / "w.tsv", newline="").read() == render_within(T, names, pick, 2)


def test_options_and_errors(tmp_path):
    r = run(["-i", PB, "-d", tmp_path, "--host"], ok=False)
    assert r.returncode == 1 and r.stderr == "ERROR: No output files requested!\n"
    assert "--input-mat" in run(["-V", "o.tsv"], ok=False).stderr
    assert "needs a value" in run(["-i", PB, "-V"], ok=False).stderr
    assert "bad value" in run(["-i", PB, "--within-distance", "w.tsv", "--distance-threshold", "two"], ok=False).stderr
    assert "bad value" in run(["-i", PB, "--within-distance", "w.tsv", "--distance-threshold", "-1"], ok=False).stderr
    assert "bogus" in run(["-i", PB, "-V", "o.tsv", "--bogus"], ok=False).stderr
    assert "x.pb" in run(["-i", "/nonexistent/x.pb", "-V", "o.tsv", "-d", tmp_path, "--host"], ok=False).stderr
    with open(tmp_path / "s.txt", "w") as f:
        f.write("no_such_sample\n")
    r = run(["-i", PB, "-s", tmp_path / "s.txt", "-V", "o.tsv", "-d", tmp_path, "--host"], ok=False)
    assert r.returncode == 1 and "ERROR: no_such_sample is not present in the tree!" in r.stderr
    assert run(["-h"]).stdout.startswith("Usage: matutils-amd relatives")
    for word in ("--samples", "--closest-relatives", "--break-ties", "--within-distance", "--distance-threshold", "--output-directory",
                 "--threads", "--device", "--host"):
        assert word in run(["--help"]).stdout
    top = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert top.returncode == 0 and "relatives --help" in top.stdout
    r = subprocess.run([BIN, "introduce"], capture_output=True, text=True)
    assert r.returncode == 1 and "relatives" in r.stderr
    # extract goes on refusing the four options
    for opt in (["-V", "o.tsv"], ["-q"], ["--within-distance", "o.tsv"], ["--distance-threshold", "2"]):
        r = subprocess.run([BIN, "extract", "-i", PB, "-u", "x.txt", "-d", str(tmp_path)] + opt, capture_output=True, text=True)
        assert r.returncode == 1 and "not supported by matutils-amd extract" in r.stderr
