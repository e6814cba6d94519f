"""matUtils summary --haplotype without a GPU: the literal restatement of count_haplotypes / write_haplotype_table
(tests/haplotypes_ref.py) against the table every hand-shaped case names, the closed form Fast against the literal walk, and
`matutils-amd haplotypes --host` byte for byte against the text rendered from the literal walk."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import refio
from tests import haplotypes_cases as HC
from tests import haplotypes_ref as R
from tests import summary_ref as SR
from tests import test_summary_cpu as SCPU
from tests import usher_model as UM
from usher_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
SURVEY_PB, ANNOTATED_PB = SCPU.SURVEY_PB, SCPU.ANNOTATED_PB
CASES = {c.name: c for c in HC.hand_cases()}
ABI = ("ugp_haplotypes_attach", "ugp_haplotype_groups", "ugp_haplotype_groups_hashed", "ugp_haplotype_sets", "ugp_haplotype_sets_chunked",
       "ugp_haplotype_time")


def fast_equals_literal(arrays):
    T, F = SR.Tree(arrays), R.Fast(arrays)
    assert (F.n_duplicate, F.first_duplicate) == R.duplicates(T)
    if F.n_duplicate:
        return T, F
    assert F.group_records() == R.group_records(T)
    leaves = T.leaves()
    assert F.leaf_sets(leaves) == R.leaf_sets(T, leaves)
    off, pos, nuc = F.sets_csr(leaves[::-1])
    want = R.leaf_sets(T, leaves[::-1])
    assert off.tolist() == np.r_[0, np.cumsum([len(s) for s in want])].tolist()
    assert list(zip(pos.tolist(), nuc.tolist())) == [pr for s in want for pr in s]
    return T, F


@pytest.mark.parametrize("case", HC.hand_cases(), ids=repr)
def test_case_pins_its_rule(case):
    T = case.tree()
    if case.text is not None:
        assert R.render(T) == R.HEADER + case.text, case.rule
    groups = R.group_records(T)
    assert sum(g[1] for g in groups) == len(T.leaves()) and len({g[0] for g in groups}) == len(groups)
    assert R.render(T).count("\n") == 1 + len(groups)
    T, F = fast_equals_literal(case.arrays)
    assert (F.n_duplicate == 0) == case.device
    if not case.device:
        assert R.duplicates(T) == (1, case.tags["D"])


def test_the_cases_cover_the_rules():
    g = {n: R.group_records(c.tree()) for n, c in CASES.items()}
    assert len(g["all_distinct"]) == 70 and len(g["star_shared"]) == 1 and g["star_shared"][0][1] == 700
    assert len(g["caterpillar600"]) == 600 and all(x[1] == 2 for x in g["caterpillar600"]) and max(x[2] for x in g["caterpillar600"]) > 256
    assert sorted(x[2] for x in g["set_sizes"]) == [0, 63, 64, 65, 300]
    assert g["no_mutations"] == [(g["no_mutations"][0][0], 4, 0)] and g["single_node"] == [(0, 1, 0)]
    # the two equal leaves of different_histories lie under different children of the root
    c = CASES["different_histories"]
    T = c.tree()
    _, of_leaf = R.node_sets(T)
    same = [l for l in T.leaves() if of_leaf[l] == ((100, 4),)]
    assert len(same) == 2 and len({T.rsearch(l, True)[-2] for l in same}) == 2
    # the masked entries of masked_entries sit on the root, on an inner node and on a leaf
    a = CASES["masked_entries"].arrays
    owners = np.repeat(np.arange(a["n"]), np.diff(a["mut_off"]))[a["mut_pos"] < 0]
    T = CASES["masked_entries"].tree()
    assert 0 in owners and any(T.is_leaf(v) for v in owners) and any(v and not T.is_leaf(v) for v in owners)


def random_trees():
    return SCPU.random_trees()


def test_synthetic_trees_have_shared_haplotypes():
    """Before they are used as a yardstick: groups of more than one leaf, and groups whose members have different parents (so they
    lie in different subtrees of some node and no sibling rule alone would find them)."""
    multi = spread = 0
    for _, arrays in random_trees():
        F = R.Fast(arrays)
        parent = np.asarray(arrays["parent"])[F.leaf_bfs]
        multi += int((F.group_count > 1).sum())
        for g in np.flatnonzero(F.group_count > 1):
            spread += len(set(parent[F.group_of_rank == g].tolist())) > 1
    assert multi > 20 and spread > 5, (multi, spread)


@pytest.mark.parametrize("name,arrays", random_trees(), ids=lambda v: v if isinstance(v, str) else "")
def test_fast_against_literal_on_synthetic_trees(name, arrays):
    fast_equals_literal(arrays)


@pytest.mark.parametrize("name", ["star255", "star257", "caterpillar257", "segment_edge_small"])
def test_fast_against_literal_on_the_edge_builders(name):
    """The builders the device tests scale up, at a size the literal walk takes."""
    root = {"star255": lambda: HC.star(254, every=5), "star257": lambda: HC.star(256, every=0), "caterpillar257": lambda: HC.caterpillar(85, every=4),
            "segment_edge_small": lambda: HC.N((), [HC.N(["A100C"], [HC.N(["G200T"] if i % 3 == 0 else []) for i in range(7)]), HC.N(),
                                                   HC.N(["A100G"], [HC.N(), HC.N(["G200T"])])])}[name]()
    arrays, _ = HC.build(root)
    T, F = fast_equals_literal(arrays)
    assert len(F.group_records()) > 1 or name == "star257"


# ---- the command-line tool, --host ------------------------------------------------------------------------------------------

def run(args, ok=True):
    r = subprocess.run([BIN, "haplotypes"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


def load_model(pb):
    T = refio.load_mutation_annotated_tree(pb)
    UM.uncondense_leaves(T)
    return SR.Tree(refio.tree_to_bfs_arrays(T))


@pytest.mark.parametrize("pb", [SURVEY_PB, ANNOTATED_PB], ids=["survey", "annotated"])
def test_host_table_on_the_fixtures(pb, tmp_path):
    r = run(["-i", pb, "-H", "hap.tsv", "-d", tmp_path, "--host"])
    want = R.render(load_model(pb))
    assert open(tmp_path / "hap.tsv").read() == want and want.count("\n") > 3
    err = r.stderr.split("\n")
    assert err[0] == "Loading input MAT file %s." % pb
    assert err[1] == "Writing haplotype frequencies to output %s" % os.path.join(os.path.realpath(tmp_path), "hap.tsv")
    assert re.fullmatch(r"Completed in \d+ msec ", err[2]) and err[3:] == ["", ""]


@pytest.mark.parametrize("case", HC.cli_cases(), ids=repr)
def test_host_table_on_hand_shaped_trees(case, tmp_path):
    pb = SCPU.write_annotated(case, tmp_path / "case.pb")
    assert R.render(load_model(pb)) == R.render(case.tree())      # the case survives the file unchanged
    run(["-i", pb, "-H", "hap.tsv", "-d", tmp_path, "--host"])
    got = open(tmp_path / "hap.tsv").read()
    assert got == R.render(case.tree())
    if case.text is not None:
        assert got == R.HEADER + case.text


def test_options(tmp_path):
    r = run(["-H", "h.tsv", "--host"], ok=False)
    assert r.returncode == 1 and "--input-mat" in r.stderr and "Usage: matutils-amd haplotypes" in r.stderr
    r = run(["-i", SURVEY_PB, "--host"], ok=False)
    assert r.returncode == 1 and "--haplotype" in r.stderr
    r = run(["-i", SURVEY_PB, "-H"], ok=False)
    assert r.returncode == 1 and "-H needs a value" in r.stderr
    r = run(["-i", SURVEY_PB, "-H", "h.tsv", "--bogus"], ok=False)
    assert r.returncode == 1 and "unknown option --bogus" in r.stderr
    r = run(["-i", tmp_path / "missing.pb", "-H", "h.tsv", "-d", tmp_path, "--host"], ok=False)
    assert r.returncode == 1 and "ERROR" in r.stderr
    for h in ("-h", "--help"):
        out = run([h]).stdout
        assert out.startswith("Usage: matutils-amd haplotypes") and "--haplotype" in out and "--host" in out
    # long names, -T, a directory that does not exist yet
    d = tmp_path / "new"
    r = run(["--input-mat", SURVEY_PB, "--haplotype", "long.tsv", "--output-directory", d, "--threads", "3", "--host"])
    assert "Creating output directory." in r.stderr and os.listdir(d) == ["long.tsv"]
    run(["-i", SURVEY_PB, "-H", "short.tsv", "-d", d, "--host"])
    assert open(d / "long.tsv").read() == open(d / "short.tsv").read()
    # the tool names the subcommand where it lists what it runs; summarize keeps refusing -H
    r = subprocess.run([BIN, "nonsense"], capture_output=True, text=True)
    assert r.returncode == 1 and "haplotypes" in r.stderr
    assert "matutils-amd haplotypes --help" in subprocess.run([BIN, "--help"], capture_output=True, text=True).stdout
    r = subprocess.run([BIN, "summarize", "-i", SURVEY_PB, "-H", "h.tsv", "--host"], capture_output=True, text=True)
    assert r.returncode == 1 and "not supported" in r.stderr


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    L = _lib.lib()
    for name in ABI:
        assert re.search(r"\bint %s\(ugp_mat \*mat" % name, hdr) and name in _lib.SYMBOLS
        assert hasattr(L, name)
    for word in ("ugp_hp_group", "ugp_hp_info", "n_collisions", "first_duplicate"):
        assert word in hdr
    # no handle: an error code, not a crash
    assert L.ugp_haplotypes_attach(None, None) == -1 and L.ugp_haplotype_groups(None, None, 0, None, None) == -1
    assert L.ugp_haplotype_groups_hashed(None, None, 0, None, None, 128) == -1
    assert L.ugp_haplotype_sets(None, None, 0, None, None, None, 0, None) == -1
    assert L.ugp_haplotype_sets_chunked(None, None, 0, None, None, None, 0, None, 1) == -1
    assert L.ugp_haplotype_time(None, 1, None, None, None) == -1
