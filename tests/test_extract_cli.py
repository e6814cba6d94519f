"""`matutils-amd extract` end to end on a survey tree against a restatement of extract_main's steps for its options: -k and -Y
through tests/nearest_ref.py (canonical ties; --reference-ties: the reference's std::sort order), the three filters restated
from select.cpp, the -u / -t / -o files against tests/usher_model.py's get_subtree, and the written .pb through the pinned reader."""
import os
import subprocess

import pytest

from oracle import refio
from tests import nearest_ref as R
from tests import stdorder
from tests import usher_model as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
PB = os.path.join(ROOT, "tests", "golden", "survey_ref", "global", "global_assignments.pb")


def _run(args, tmp_path):
    r = subprocess.run([BIN, "extract", "-i", PB, "-d", str(tmp_path)] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


class Model:
    def __init__(self):
        self.T = refio.load_mutation_annotated_tree(PB)
        UM.uncondense_leaves(self.T)
        self.arrays = refio.tree_to_bfs_arrays(self.T)
        self.names = self.arrays["names"]
        self.index = {s: j for j, s in enumerate(self.names)}
        self.RT = R.Tree(self.arrays)
        self.pre = R.Fast(self.arrays).pre
        self.leaves = [n.identifier for n in UM.get_leaves(self.T)]

    def nearby(self, name, k, sorter=None):
        return [self.names[v] for v in R.literal(self.RT, self.index[name], k, sorter)["nodes"]]

    def parsimony(self, samples, m):
        return [s for s in (samples or self.leaves) if len(self.T.get_node(s).mutations) <= m]

    def steppers(self, samples, m):
        return [s for s in (samples or self.leaves) if all(len(a.mutations) <= m for a in UM._rsearch(self.T.get_node(s), True))]

    def paths(self, samples, m):
        keep = set(samples)
        out = []
        for n in self.T.depth_first_expansion():
            if n.is_leaf() and sum(len(a.mutations) for a in UM._rsearch(n, True) if not a.is_root()) <= m and (not samples or n.identifier in keep):
                out.append(n.identifier)
        return out

    def dfs_sorted(self, names):
        return sorted(set(names), key=lambda s: self.pre[self.index[s]])

    def newick(self, samples):
        S = UM.get_subtree(self.T, samples)
        return refio.get_newick_string(S, S.root, True, True) + "\n"


@pytest.fixture(scope="module")
def model():
    return Model()


def _lines(path):
    return open(path).read().splitlines()


def test_filters_alone(model, tmp_path):
    lens = sorted(len(model.T.get_node(s).mutations) for s in model.leaves)
    a = lens[len(lens) // 2]
    plen = sorted(sum(len(x.mutations) for x in UM._rsearch(model.T.get_node(s), True) if not x.is_root()) for s in model.leaves)
    p = plen[len(plen) // 2]
    for flag, fn, v in (("-a", model.parsimony, a), ("-b", model.steppers, max(a, 2)), ("-P", model.paths, p)):
        want = fn([], v)
        assert 0 < len(want) < len(model.leaves), (flag, v, len(want))
        _run([flag, str(v), "-u", "u.txt", "-t", "t.nh"], tmp_path)
        assert _lines(tmp_path / "u.txt") == want, flag
        if len(want) <= 150:
            assert open(tmp_path / "t.nh").read() == model.newick(want), flag
    some = model.leaves[::3]
    (tmp_path / "s.txt").write_text("\n".join(some) + "\n")
    _run(["-s", str(tmp_path / "s.txt"), "-a", str(a), "-P", str(p + 1), "-u", "u2.txt"], tmp_path)
    assert _lines(tmp_path / "u2.txt") == model.paths(model.parsimony(some, a), p + 1)
    longest = max(model.leaves, key=lambda s: len(model.T.get_node(s).mutations))
    (tmp_path / "one.txt").write_text(longest + "\n")
    r = subprocess.run([BIN, "extract", "-i", PB, "-d", str(tmp_path), "-s", str(tmp_path / "one.txt"), "-a", "0", "-u", "u3.txt"], capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR: No samples fulfill selected criteria. Change arguments and try again" in r.stderr


def test_whole_tree_without_selection(model, tmp_path):
    _run(["-u", "u.txt", "-t", "t.nh"], tmp_path)
    assert _lines(tmp_path / "u.txt") == model.leaves
    assert open(tmp_path / "t.nh").read() == refio.get_newick_string(model.T, model.T.root, True, True) + "\n"


@pytest.mark.gpu
def test_nearest_k_outputs(model, tmp_path):
    s = model.leaves[len(model.leaves) // 3]
    want = model.nearby(s, 25)
    assert len(want) == 25
    _run(["-k", s + ":25", "-u", "u.txt", "-t", "t.nh", "-o", "o.pb"], tmp_path)
    assert _lines(tmp_path / "u.txt") == want
    assert open(tmp_path / "t.nh").read() == model.newick(want)
    # the written .pb through the pinned reader: the induced subtree, condensed as the reference saves it
    got = refio.load_mutation_annotated_tree(str(tmp_path / "o.pb"))
    S = UM.get_subtree(model.T, want)
    UM.condense_leaves(S)
    # (a .pb stores its newick without internal names: the loader numbers them again)
    norm = lambda T: (refio.get_newick_string(T, T.root, False, True),
                      [(n.identifier if n.is_leaf() else None, [(m.position, m.ref_nuc, m.par_nuc, m.mut_nuc) for m in n.mutations])
                       for n in T.depth_first_expansion()],
                      sorted((k, tuple(v)) for k, v in T.condensed_nodes.items()))
    assert norm(got) == norm(S)
    # -k with -s: the -s samples that are among the nearest, in the file's order
    mix = [want[7], model.leaves[0], want[2], model.leaves[-1], want[20]]
    (tmp_path / "s.txt").write_text("\n".join(mix) + "\n")
    _run(["-k", s + ":25", "-s", str(tmp_path / "s.txt"), "-u", "u2.txt"], tmp_path)
    assert _lines(tmp_path / "u2.txt") == [x for x in mix if x in set(want)]
    # no ancestor with more than k leaves: the reference's assert
    r = subprocess.run([BIN, "extract", "-i", PB, "-d", str(tmp_path), "-k", "%s:%d" % (s, len(model.leaves)), "-u", "u3.txt"], capture_output=True, text=True)
    assert r.returncode != 0 and "the nearest-k selection is empty" in r.stderr
    r = subprocess.run([BIN, "extract", "-i", PB, "-d", str(tmp_path), "-k", "no_such_sample:3", "-u", "u3.txt"], capture_output=True, text=True)
    assert r.returncode != 0 and "ERROR: no_such_sample is not present in the tree!" in r.stderr


@pytest.mark.gpu
def test_select_nearest_with_samples(model, tmp_path):
    some = model.leaves[5::41]
    (tmp_path / "s.txt").write_text("\n".join(some) + "\n")
    want = model.dfs_sorted(x for s in some for x in model.nearby(s, 6))
    _run(["-s", str(tmp_path / "s.txt"), "-Y", "6", "-u", "u.txt", "-t", "t.nh"], tmp_path)
    assert _lines(tmp_path / "u.txt") == want
    assert open(tmp_path / "t.nh").read() == model.newick(want)
    # after a filter, as the reference orders its steps
    _run(["-s", str(tmp_path / "s.txt"), "-b", "3", "-Y", "4", "-u", "u2.txt"], tmp_path)
    assert _lines(tmp_path / "u2.txt") == model.dfs_sorted(x for s in model.steppers(some, 3) for x in model.nearby(s, 4))


@pytest.mark.gpu
def test_reference_ties(model, tmp_path):
    so = stdorder.StdOrder(tmp_path)
    # a sample whose cut runs through equal distances, where the two orders pick different sets
    pick = None
    for s in model.leaves:
        for k in (4, 9, 30):
            r = R.literal(model.RT, model.index[s], k)
            if r["count"] and r["n_at_cut"] > sum(1 for d in r["dist"][int(model.RT.nleaves[r["last_anc"]]):] if d == r["cut_dist"]):
                if sorted(model.nearby(s, k)) != sorted(model.nearby(s, k, so)):
                    pick = (s, k)
                    break
        if pick:
            break
    assert pick, "no query on this tree separates the two tie orders"
    s, k = pick
    _run(["-k", "%s:%d" % (s, k), "-u", "u.txt", "--reference-ties"], tmp_path)
    assert _lines(tmp_path / "u.txt") == model.nearby(s, k, so)
    _run(["-k", "%s:%d" % (s, k), "-u", "u2.txt"], tmp_path)
    assert _lines(tmp_path / "u2.txt") == model.nearby(s, k)
    some = model.leaves[3::57]
    (tmp_path / "s.txt").write_text("\n".join(some) + "\n")
    _run(["-s", str(tmp_path / "s.txt"), "-Y", "9", "-u", "u3.txt", "--reference-ties"], tmp_path)
    assert _lines(tmp_path / "u3.txt") == model.dfs_sorted(x for q in some for x in model.nearby(q, 9, so))
