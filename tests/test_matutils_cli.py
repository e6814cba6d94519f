"""matutils-amd uncertainty on a MAT of the reference's own test data: -e / -o byte for byte against files rendered from the
oracle's literal search and the literal neighborhood (the MAT uncondensed as host/mat.cpp and the reference do), CRLF in
the sample file, and the exit on an unknown sample."""
import os
import subprocess

import numpy as np
import pytest

from oracle import refio
from tests import uncertainty_ref as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
MAT = os.path.join(ROOT, "tests", "golden", "survey_ref", "syn", "tree.pb")


def _uncondensed(path):
    """Tree::uncondense_leaves (mutation_annotated_tree.cpp:1334-1382) on the oracle's tree."""
    T = refio.load_mutation_annotated_tree(path)
    for name, leaves in list(T.condensed_nodes.items()):
        n = T.get_node(name)
        if n is None:
            continue
        par = n.parent if n.parent is not None else n
        k = len(leaves)
        if k > 1 and n.mutations:
            del T.all_nodes[n.identifier]
            n.identifier = T.new_internal_node_id()
            T.all_nodes[n.identifier] = n
            for s in leaves:
                T.create_node(s, n)
        elif k > 1:
            del T.all_nodes[n.identifier]
            n.identifier = leaves[0]
            T.all_nodes[n.identifier] = n
            for s in leaves[1:]:
                T.create_node(s, par, n.branch_length)
        elif k == 1:
            del T.all_nodes[n.identifier]
            n.identifier = leaves[0]
            T.all_nodes[n.identifier] = n
    T.condensed_nodes = {}
    T.condensed_leaves = set()
    return T


def test_uncertainty_files_byte_for_byte(tmp_path):
    T = _uncondensed(MAT)
    arrays = refio.tree_to_bfs_arrays(T)
    names = arrays["names"]
    par = np.asarray(arrays["parent"])
    leaves = np.setdiff1d(np.arange(arrays["n"]), par[1:])
    rng = np.random.default_rng(3)
    picks = [int(j) for j in rng.choice(leaves, 60, replace=False)] + [int(j) for j in rng.choice(np.unique(par[1:])[1:], 5, replace=False)]
    sf = tmp_path / "samples.txt"
    sf.write_bytes("".join(names[j] + "\r\n" for j in picks).encode())
    e, o = tmp_path / "epps.tsv", tmp_path / "placements.tsv"
    r = subprocess.run([BIN, "uncertainty", "-i", MAT, "-s", str(sf), "-e", str(e), "-o", str(o), "-T", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Processing %d samples" % len(picks) in r.stderr and "Completed in" in r.stderr
    want = U.expected(arrays, picks)
    assert any(nb > 1 for nb, _, _ in want)
    we, wo = U.render(names, par, U.dfs_order(arrays), picks, want)
    assert e.read_text() == we
    assert o.read_text() == wo


def test_unknown_sample_exits_1(tmp_path):
    sf = tmp_path / "samples.txt"
    sf.write_text("no_such_sample\n")
    r = subprocess.run([BIN, "uncertainty", "-i", MAT, "-s", str(sf), "-e", str(tmp_path / "e.tsv")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    assert "ERROR: Sample missing in input MAT!" in r.stderr and "no_such_sample" in r.stderr
