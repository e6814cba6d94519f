"""`matutils-amd annotate` against the restatement of annotate_main / assignLineages (tests/annotate_ref.py): the -u and -D files
byte for byte, and the output .pb (decoded by refio.parse_parsimony_pb through refio's loader) against the restated tree --
newick, per-node mutations, condensed table and clade annotations -- in the -c, -M, -P and -C modes and in combinations, with -l
on and off, on a survey tree and on a pinned tree that already carries annotations."""
import os
import subprocess

import numpy as np
import pytest

from oracle import refio
from tests import annotate_ref as A
from tests import stdorder
from tests import usher_model as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
SYN = os.path.join(ROOT, "tests", "golden", "survey_ref", "syn", "tree.pb")
PINNED = os.path.join(ROOT, "tests", "golden", "pb_pinned", "ref_written_annotated.pb")


def _run(args, cwd):
    return subprocess.run([BIN, "annotate"] + args, cwd=str(cwd), capture_output=True, text=True, timeout=600)


def _load(path):
    T = refio.load_mutation_annotated_tree(path)
    if T.condensed_nodes:
        UM.uncondense_leaves(T)
    return T


def _norm(T):
    nodes = [(n.identifier, [(m.position, m.ref_nuc, m.par_nuc, m.mut_nuc) for m in n.mutations], list(n.clade_annotations))
             for n in T.depth_first_expansion()]
    return refio.get_newick_string(T, T.root, True, True), nodes, sorted((k, tuple(v)) for k, v in T.condensed_nodes.items())


def _files(T, tmp_path, seed):
    """Clade files drawn from the tree: -c exemplars below chosen roots, -M root-path mutation sets (one inherits another), -P
    mutation paths, -C node ids."""
    rng = np.random.default_rng(seed)
    dfs = T.depth_first_expansion()
    inner = [n for n in dfs if not n.is_leaf() and 4 <= T.get_num_leaves(n) <= 80]
    chosen = [inner[int(k)] for k in rng.choice(len(inner), min(8, len(inner)), replace=False)]
    leaves = [n for n in dfs if n.is_leaf()]
    names = []
    for k, c in enumerate(chosen[:5]):
        below = [n for n in T.depth_first_expansion(c) if n.is_leaf()]
        ex = [below[int(i)] for i in rng.integers(0, len(below), min(len(below), 15))] + [leaves[int(rng.integers(len(leaves)))]]
        names += ["cl%d\t%s" % (k, n.identifier) for n in ex]
    names.append("cl0\tno_such_sample")
    muts = []
    for k, c in enumerate(chosen[5:7] + chosen[:1]):
        state = {}
        for a in reversed(UM._rsearch(c, True)):
            for m in a.mutations:
                if m.position > 0:
                    state[m.position] = (m.ref_nuc, m.mut_nuc)
        s = ["%s%d%s" % (refio.get_nuc(r), p, refio.get_nuc(x)) for p, (r, x) in sorted(state.items()) if r != x]
        muts.append("M%d\t%s" % (k, ",".join(s)))
    first = muts[0].split("\t")[1].split(",")[0]
    muts.append("M9\tM0 > " + first)   # inherits M0's set
    muts.append("cl1\t" + muts[1].split("\t")[1])   # -M takes precedence over -c
    paths = []
    for k, c in enumerate(chosen[2:4] + chosen[6:]):
        nodes = list(reversed(UM._rsearch(c, True)))[1:]
        paths.append("P%d\t%s" % (k, " > ".join(",".join(m.get_string() for m in n.mutations) for n in nodes)))
    paths.append("cl2\t")   # the root: -P takes precedence over -c and -M
    nid = ["N0\t%s" % chosen[0].identifier, "N1\t%s" % chosen[1].identifier, "N2\t%s" % chosen[0].identifier]
    out = {}
    for key, lines in (("c", names), ("M", muts), ("P", paths), ("C", nid)):
        p = tmp_path / ("%s.tsv" % key)
        p.write_text("".join(ln + "\n" for ln in lines))
        out[key] = (str(p), lines)
    return out


def _check(tree, clear, modes, tmp_path):
    so = stdorder.StdOrder(tmp_path)
    files = _files(_load(tree), tmp_path, 5)
    args = ["-i", tree, "-o", "out.pb", "-d", str(tmp_path / "o")]
    for m in modes:
        args += ["-" + m, files[m][0]]
    if "C" not in modes:
        args += ["-u", "u.tsv", "-D", "d.tsv"]
    if clear:
        args.append("-l")
    r = _run(args, tmp_path)
    if tree == PINNED and not clear:
        # this file's nodes carry 0 or 1 annotations: appending one more leaves them ragged
        assert r.returncode == 1 and "different numbers of clade annotations" in r.stderr
        with pytest.raises(ValueError):
            A._init(_load(tree), False)
        return
    assert r.returncode == 0, r.stderr[-3000:]
    T = _load(tree)
    if "C" in modes:
        assert A.assign_from_nids(T, files["C"][1], clear) is None
    else:
        u, d = A.assign_lineages(T, so, names_lines=files["c"][1] if "c" in modes else None,
                                 muts_lines=files["M"][1] if "M" in modes else None,
                                 paths_lines=files["P"][1] if "P" in modes else None, clear=clear)
        assert (tmp_path / "o" / "u.tsv").read_text() == u
        assert (tmp_path / "o" / "d.tsv").read_text() == d
    UM.condense_leaves(T)
    got = refio.load_mutation_annotated_tree(str(tmp_path / "o" / "out.pb"))
    assert _norm(got) == _norm(T)
    assert any(n.clade_annotations[-1] for n in got.depth_first_expansion())


@pytest.mark.parametrize("tree", [SYN, PINNED])
@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("modes", [("P",), ("C",)])
def test_paths_and_node_ids(tree, clear, modes, tmp_path):
    """-P and -C never open a device."""
    _check(tree, clear, modes, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("tree", [SYN, PINNED])
@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("modes", [("c",), ("M",), ("c", "M"), ("c", "M", "P")])
def test_annotate_matches_the_restatement(tree, clear, modes, tmp_path):
    if tree == PINNED and clear:
        # this file carries a multi-allelic mutation: the device tree takes one-hot alleles only, and the tool says so
        files = _files(_load(tree), tmp_path, 5)
        args = ["-i", tree, "-o", "out.pb", "-l"] + sum((["-" + m, files[m][0]] for m in modes), [])
        r = _run(args, tmp_path)
        assert r.returncode == 1 and "not one-hot" in r.stderr and not os.path.exists(tmp_path / "out.pb")
        return
    _check(tree, clear, modes, tmp_path)


def test_messages_and_exit_codes(tmp_path):
    """Argument and file errors, all reached before a device is opened."""
    files = _files(_load(SYN), tmp_path, 6)
    r = _run(["-i", SYN, "-o", "o.pb", "-c", files["c"][0], "-C", files["C"][0]], tmp_path)
    assert r.returncode == 1 and "must specify either --clade-to-nid" in r.stderr
    r = _run(["-i", SYN, "-o", "o.pb"], tmp_path)
    assert r.returncode == 1 and "must specify either --clade-to-nid" in r.stderr
    bad = tmp_path / "bad.tsv"
    bad.write_text("A\tnode_1\textra\n")
    r = _run(["-i", SYN, "-o", "o.pb", "-C", str(bad)], tmp_path)
    assert r.returncode == 1 and "Incorrect format for clade to node id assignment file" in r.stderr
    bad.write_text("A\tno_such_node\n")
    r = _run(["-i", SYN, "-o", "o.pb", "-C", str(bad)], tmp_path)
    assert r.returncode == 1 and "ERROR: Node id no_such_node not found!" in r.stderr
    bad.write_text("A\tC100T\nA\tC200T\n")
    r = _run(["-i", SYN, "-o", "o.pb", "-M", str(bad)], tmp_path)
    assert r.returncode == 1 and "ERROR: clade A is defined on multiple lines" in r.stderr and "Encountered errors" in r.stderr
    bad.write_text("A\tx\ty\n")
    r = _run(["-i", SYN, "-o", "o.pb", "-c", str(bad)], tmp_path)
    assert r.returncode == 1 and "Incorrect format for clade assignment file" in r.stderr
    r = _run(["-o", "o.pb", "-C", str(bad)], tmp_path)
    assert r.returncode == 1 and "input-mat" in r.stderr
