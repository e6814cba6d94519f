"""The sample selectors without a GPU: the closed form of tests/select_ref.py against the literal restatement on every hand-shaped
case and on the annotated fixture (every (position, allele) that occurs and each position's other three alleles), the ABI surface
of the ugp_select calls, and `matutils-amd select --host` byte for byte against the restated chain of extract_main."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import refio
from tests import select_cases as SC
from tests import select_ref as R
from tests import usher_model as UM
from usher_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
PB = os.path.join(ROOT, "tests", "golden", "pb_pinned", "ref_written_annotated.pb")
CASES = SC.all_cases()


def literal_mask(T, F, names, good):
    """The names the literal functions return as a mask by leaf rank."""
    rank = {names[int(v)]: r for r, v in enumerate(F.lbfs)}
    mask = np.zeros(F.n_leaves, bool)
    for s in good:
        mask[rank[s]] = True
    assert len(set(good)) == len(good)
    return mask


def check_closed_form(arrays, T, F):
    names = T_names(arrays)
    pos, nuc = SC.queries(arrays)
    mask, counts = F.mutations(pos, nuc)
    union = np.zeros(F.n_leaves, bool)
    for q, (p, a) in enumerate(zip(pos.tolist(), nuc.tolist())):
        one = literal_mask(T, F, names, R.mutation_samples(T, p, a))
        assert int(counts[q]) == int(one.sum()), (p, a)
        assert np.array_equal(F.mutations([p], [a])[0], one), (p, a)
        union |= one
    assert np.array_equal(mask, union)
    for nodes in SC.node_sets(arrays):
        mask, counts = F.subtrees(nodes)
        want = set()
        for i, v in enumerate(nodes):
            ids = R.get_leaves_ids(T, names[int(v)])
            assert int(counts[i]) == len(ids)
            want.update(ids)
        assert np.array_equal(mask, literal_mask(T, F, names, sorted(want)))
    for leaves_set in SC.leaf_sets(arrays):
        mask = literal_mask(T, F, names, [names[v] for v in leaves_set])
        node, below = F.mrca(mask)
        assert names[node] == R.get_mrca(T, [names[v] for v in leaves_set]), leaves_set
        assert below == len(R.get_mrca_samples(T, [names[v] for v in leaves_set]))


def T_names(arrays):
    return list(arrays.get("names") or ["n%d" % j for j in range(arrays["n"])])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_closed_form_equals_literal(case):
    check_closed_form(case.arrays, R.tree_from_arrays(case.arrays), R.Fast(case.arrays))


def test_cases_do_what_they_say():
    by = SC.by_name()
    # the owner chain: the leaves hanging below A>T>A>T read T, A, T, A from the nearest owner; any-owner would give all of them both
    c = by["owner_chain"]
    T = R.tree_from_arrays(c.arrays)
    t, a = R.mutation_samples(T, 10, 8), R.mutation_samples(T, 10, 1)
    assert len(t) == 2 and len(a) == 3 and not set(t) & set(a)
    assert len(R.mutation_samples_any_owner(T, 10, 8)) == 5 and len(R.mutation_samples_any_owner(T, 10, 1)) == 4
    # two entries on one node: the first counts
    c = by["two_entries"]
    T = R.tree_from_arrays(c.arrays)
    x = c.tags["x"]
    kids = [n.identifier for n in T.get_node("n%d" % x).children]
    assert kids[0] in R.mutation_samples(T, 7, 2) and kids[0] not in R.mutation_samples(T, 7, 4)
    assert kids[1] in R.mutation_samples(T, 7, 8) and kids[1] not in R.mutation_samples(T, 7, 2)
    # the reference allele selects only leaves under a back-mutation
    c = by["caterpillar"]
    T = R.tree_from_arrays(c.arrays)
    n_leaves = len(UM.get_leaves(T))
    back = R.mutation_samples(T, 1, 1)
    assert 0 < len(back) < n_leaves and len(back) + len(R.mutation_samples(T, 1, 2)) == n_leaves - 1   # all but the leaf beside v1
    # masked entries own nothing
    T = R.tree_from_arrays(by["masked"].arrays)
    assert R.mutation_samples(T, -1, 1) == [] and not R.Fast(by["masked"].arrays).mutations([-1, -7], [1, 1])[0].any()
    assert len(R.mutation_samples(T, 7, 2)) == 2 and len(R.mutation_samples(T, 7, 4)) == 2
    # a set inside one polytomy
    c = by["polytomy"]
    T = R.tree_from_arrays(c.arrays)
    poly = T.get_node("n%d" % c.tags["poly"])
    some = [n.identifier for n in poly.children][2:7:2]
    assert R.get_mrca(T, some) == poly.identifier and len(R.get_mrca_samples(T, some)) == 9
    assert R.Fast(by["no_mutations"].arrays).tp == 0


# ---- the fixture ---------------------------------------------------------------------------------------------------------------

class Model:
    def __init__(self):
        self.T = refio.load_mutation_annotated_tree(PB)
        UM.uncondense_leaves(self.T)
        self.arrays = refio.tree_to_bfs_arrays(self.T)
        self.names = self.arrays["names"]
        self.F = R.Fast(self.arrays)
        self.leaves = R.get_leaves_ids(self.T)
        self.clades = {}
        for n in self.T.depth_first_expansion():
            for c in n.clade_annotations:
                if c != "":
                    self.clades.setdefault(c, n)

    def newick(self, samples):
        S = UM.get_subtree(self.T, samples)
        return refio.get_newick_string(S, S.root, True, True) + "\n"


@pytest.fixture(scope="module")
def model():
    return Model()


def test_fixture_is_what_the_tests_need(model):
    T = model.T
    assert len(model.names) == 586 and len(model.leaves) == 422
    ann = [n for n in T.depth_first_expansion() if any(c != "" for c in n.clade_annotations)]
    assert len(ann) == 68 and sum(n.is_leaf() for n in ann) == 41 and (np.asarray(model.arrays["mut_pos"]) < 0).sum() == 23
    # 11083: nested owners of different alleles -- the nearest-owner and the any-owner reading differ
    near, anyo = R.mutation_samples(T, 11083, 8), R.mutation_samples_any_owner(T, 11083, 8)
    assert set(near) < set(anyo) and 0 < len(near) < len(model.leaves)


def test_fixture_every_position_and_allele(model):
    T, F, names = model.T, model.F, model.names
    leaves = UM.get_leaves(T)
    pos = np.asarray(model.arrays["mut_pos"])
    seen = 0
    for p in sorted(set(int(x) for x in pos if x >= 0)):
        decide = [R.deciding_allele(n, p) for n in leaves]
        there = set(int(a) for a in np.asarray(model.arrays["mut_nuc"])[pos == p])
        for a in sorted(there | {1, 2, 4, 8}):
            want = literal_mask(T, F, names, [n.identifier for n, d in zip(leaves, decide) if d == a])
            mask, counts = F.mutations([p], [a])
            assert np.array_equal(mask, want) and int(counts[0]) == int(want.sum()), (p, a)
            seen += 0 < want.sum() < len(leaves)
    assert seen > 100
    for nodes in SC.node_sets(model.arrays) + [np.asarray([model.names.index(n.identifier)], np.uint32) for n in model.clades.values()]:
        mask, counts = F.subtrees(nodes)
        want = set()
        for v in nodes:
            want.update(R.get_leaves_ids(T, names[int(v)]))
        assert np.array_equal(mask, literal_mask(T, F, names, sorted(want)))
    for ls in SC.leaf_sets(model.arrays):
        node, below = F.mrca(literal_mask(T, F, names, [names[v] for v in ls]))
        assert names[node] == R.get_mrca(T, [names[v] for v in ls])


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    for name in ("ugp_select_attach", "ugp_select_leaves", "ugp_select_mutations", "ugp_select_mutations_chunked", "ugp_select_subtrees",
                 "ugp_select_subtrees_chunked", "ugp_select_mrca", "ugp_select_time"):
        assert re.search(r"\bint %s\(ugp_mat \*mat" % name, hdr) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    L = _lib.lib()   # no handle: an error code, not a crash
    assert L.ugp_select_attach(None, None) == -1 and L.ugp_select_leaves(None, None, None) == -1
    assert L.ugp_select_mutations(None, 0, None, None, None, None) == -1 and L.ugp_select_subtrees(None, 0, None, None, None) == -1
    assert L.ugp_select_mrca(None, None, None, None) == -1 and L.ugp_select_time(None, 0, None, None, 1, None) == -1


# ---- the command-line tool -------------------------------------------------------------------------------------------------------

def run(args, ok=True, sub="select"):
    r = subprocess.run([BIN, sub] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert ok is None or (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


def warnings_of(stderr):
    return [line + "\n" for line in stderr.split("\n") if line.startswith("WARNING:")]


def option_sets(model):
    """(name, command-line options, arguments of R.chain) for every selection the tests run; the clades and nodes are the fixture's."""
    T = model.T
    inner = [(c, n) for c, n in model.clades.items() if not n.is_leaf() and 3 < len(UM.get_leaves(T, n)) < 150]
    leafc = [c for c, n in model.clades.items() if n.is_leaf()]
    assert inner and leafc, "at least one clade root is a leaf"
    c1, c2 = inner[0][0], inner[-1][0]
    node = next(n for n in T.depth_first_expansion() if not n.is_leaf() and not n.is_root() and 5 < len(UM.get_leaves(T, n)) < 60).identifier
    return [
        ("clade", ["-c", c1], dict(clade=c1)),
        ("two_clades", ["-c", c1 + "," + c2], dict(clade=c1 + "," + c2)),
        ("leaf_clade", ["-c", leafc[0]], dict(clade=leafc[0])),
        ("unknown_beside_known", ["-c", "no_such_clade," + c1], dict(clade="no_such_clade," + c1)),
        ("mutation_T", ["-m", "G11083T"], dict(mutation="G11083T")),
        ("mutation_G", ["-m", "T11083G"], dict(mutation="T11083G")),
        ("two_mutations", ["-m", "G11083T,C14408T"], dict(mutation="G11083T,C14408T")),
        ("internal", ["-I", node], dict(internal=node)),
        ("internal_unknown", ["-I", "no_such_node"], dict(internal="no_such_node")),
        ("match", ["-H", ".*2020.*"], dict(match=".*2020.*")),
        ("mrca", ["-c", leafc[0] + "," + leafc[1], "-U"], dict(clade=leafc[0] + "," + leafc[1], from_mrca=True)),
        ("prune", ["-c", c1, "-p"], dict(clade=c1, prune=True)),
        ("chained", ["-c", c1 + "," + c2, "-a", "1", "-p"], dict(clade=c1 + "," + c2, max_parsimony=1, prune=True)),
    ]


def check_run(model, tmp_path, name, opts, kw, extra=(), samples=None):
    out = tmp_path / name
    args = ["-i", PB, "-d", out, "-u", "u.txt", "-t", "t.nh"] + list(opts) + list(extra)
    if samples is not None:
        (tmp_path / (name + ".txt")).write_text("".join(s + "\n" for s in samples))
        args += ["-s", tmp_path / (name + ".txt")]
        kw = dict(kw, samples=samples)
    try:
        want, warns = R.chain(model.T, **kw)
    except R.NoSamples as e:
        r = run(args, ok=False)
        assert r.returncode == 1 and r.stderr.endswith(str(e)) and not os.path.exists(out / "u.txt"), name
        return None
    r = run(args)
    assert warnings_of(r.stderr) == warns, name
    assert "No samples fulfill" not in r.stderr
    if not want:   # nothing selected: the whole tree
        want = model.leaves
    assert open(out / "u.txt", newline="").read() == "".join(s + "\n" for s in want), name
    if len(want) <= 150:
        assert open(out / "t.nh", newline="").read() == model.newick(want), name
    return want


def test_host_chain_on_the_fixture(model, tmp_path):
    n_leaves, partial = len(model.leaves), 0
    for name, opts, kw in option_sets(model):
        want = check_run(model, tmp_path, name, opts, kw, ["--host"])
        assert want is not None, name
        partial += name.startswith("mutation") and 0 < len(want) < n_leaves
        if name == "internal_unknown":
            assert want == model.leaves   # the quirk: nothing selected
    assert partial >= 1
    # long option names
    c1 = option_sets(model)[0][1][1]
    check_run(model, tmp_path, "long", ["--clade", c1, "--prune", "--threads", "2"], dict(clade=c1, prune=True), ["--host"])
    check_run(model, tmp_path, "long2", ["--mutation", "G11083T", "--from-mrca", "--match", ".*"], dict(mutation="G11083T", match=".*", from_mrca=True), ["--host"])


def test_host_chain_after_a_sample_file(model, tmp_path):
    """-s before each selector: the file's order is kept and the selector intersects."""
    rng = np.random.default_rng(8)
    some = [model.leaves[i] for i in rng.permutation(len(model.leaves))[:200]]
    ends = 0
    for name, opts, kw in option_sets(model):
        want = check_run(model, tmp_path, "s_" + name, opts, kw, ["--host"], samples=some)
        ends += want is None
    assert ends < len(option_sets(model)) - 5


def test_messages(model, tmp_path):
    base = ["-i", PB, "-d", tmp_path, "-u", "u.txt", "--host"]
    r = run(base + ["-c", "no_such_clade"], ok=False)
    assert r.returncode == 1 and r.stderr.endswith("WARNING: Clade no_such_clade is not detected in the input tree!\n" +
                                                   "Selection step -c (host): " + r.stderr.split("Selection step -c (host): ")[1].split("\n")[0] + "\n" + R.NONE_LEFT)
    c1 = option_sets(model)[0][1][1]
    r = run(base + ["-c", "no_such_clade," + c1])
    assert r.stderr.count("WARNING:") == 1 and "WARNING: Clade no_such_clade is not detected in the input tree!\n" in r.stderr
    r = run(base + ["-m", "A1C"], ok=False)
    assert "WARNING: No samples with mutation A1C found in tree!\n" in r.stderr and r.stderr.endswith(R.NONE_LEFT)
    r = run(base + ["-H", "no such name"], ok=False)
    assert r.stderr.endswith(R.NONE_LEFT)
    r = run(base + ["-H", ".*", "-p"], ok=False)   # everything selected, inverted: the tree is left empty
    assert r.stderr.endswith(R.NONE_LEFT_PRUNE)
    run(base + ["-p"])                             # nothing selected, inverted: every leaf is outside the empty set
    assert open(tmp_path / "u.txt").read().split("\n")[:-1] == model.leaves


def test_argument_errors(tmp_path):
    base = ["-i", PB, "-d", tmp_path, "--host"]
    table = [
        (["-c", "x"], "No output files requested"),
        (["-u", "u.txt", "-c"], "needs a value"),
        (["-u", "u.txt", "-m"], "needs a value"),
        (["-u", "u.txt", "-I"], "needs a value"),
        (["-u", "u.txt", "-H"], "needs a value"),
        (["-u", "u.txt", "-e"], "needs a value"),
        (["-u", "u.txt", "-e", "two"], "bad value"),
        (["-u", "u.txt", "-e", "-1"], "bad value"),
        (["-u", "u.txt", "-m", "11083T"], "mutation_from_string"),
        (["-u", "u.txt", "-m", "G11083T,G5"], "mutation_from_string"),
        (["-u", "u.txt", "-m", "G11083Tx"], "mutation_from_string"),
        (["-u", "u.txt", "-H", "(["], "bad regular expression"),
        (["-u", "u.txt", "-U"], "needs a selection"),
        (["-u", "u.txt", "--bogus"], "unknown option --bogus"),
    ]
    for opts, word in table:
        r = run(base + opts, ok=False)
        assert r.returncode == 1 and word in r.stderr, (opts, r.stderr[-500:])
    assert "--input-mat" in run(["-u", "u.txt", "-c", "x"], ok=False).stderr
    # out of scope: refused with extract's message
    for opt in (["--max-mutation-density", "0.1"], ["-z", "5"], ["-W", "5"], ["-Z"], ["-r", "2"], ["-L", "w.txt"], ["-S", "p.txt"], ["-C", "p.txt"],
                ["-A", "p.txt"], ["-j", "o.json"], ["-N", "5"], ["-X", "5"], ["-x", "5"], ["-y", "n"], ["-R"], ["-M", "m.tsv"], ["-V", "c.tsv"]):
        r = run(base + ["-u", "u.txt"] + opt, ok=False)
        assert r.returncode == 1 and "not supported by matutils-amd extract" in r.stderr, opt
    help_ = run(["--help"])
    text = help_.stdout + help_.stderr
    assert text.startswith("Usage: matutils-amd select")
    for word in ("--clade", "--mutation", "--get-internal-descendents", "--match", "--max-epps", "--from-mrca", "--prune", "--host",
                 "depth-first order", "leaves only", "std::regex_match"):
        assert word in text, word
    top = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert top.returncode == 0 and "select --help" in top.stdout and "relatives --help" in top.stdout
    r = subprocess.run([BIN, "introduce"], capture_output=True, text=True)
    assert r.returncode == 1 and "select" in r.stderr and "relatives" in r.stderr and "summarize" in r.stderr


def test_extract_goes_on_refusing(tmp_path):
    for opt in (["-c", "x"], ["-m", "G11083T"], ["-I", "node_3"], ["-H", ".*"], ["-e", "1"], ["-U"], ["-p"], ["--host"]):
        r = subprocess.run([BIN, "extract", "-i", PB, "-u", "x.txt", "-d", str(tmp_path)] + opt, capture_output=True, text=True)
        assert r.returncode == 1 and not os.path.exists(tmp_path / "x.txt"), opt
        if opt != ["--host"]:
            assert "not supported by matutils-amd extract" in r.stderr, opt
