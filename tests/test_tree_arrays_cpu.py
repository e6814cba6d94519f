"""uh::TreeArrays, the one place a host tree becomes the breadth-first arrays of the C ABI, through the round trip the placement
tests stand on: arrays written with uh_write_pb_arrays come back from uh_pb_to_arrays (a copy out of a TreeArrays) as they were
written, on the trees at which the shared loop can go wrong.  (tests/test_pb_pinned.py checks the same call on real trees.)"""
import ctypes as C

import numpy as np
import pytest

from tests import pb_cases
from tests.host_harness import HOST_LIB

A, Cc, G, T = 1, 2, 4, 8


def tree(parent, muts):
    """Breadth-first arrays of a tree given per node as [(position, ref, par, nuc), ...] sorted by position."""
    flat = [m for node in muts for m in node]
    col = lambda k, t: np.array([m[k] for m in flat], t)
    return {"n": len(parent), "parent": np.array(parent, np.int64), "mut_off": np.cumsum([0] + [len(m) for m in muts]).astype(np.int64),
            "mut_pos": col(0, np.int32), "mut_ref": col(1, np.int8), "mut_par": col(2, np.int8), "mut_nuc": col(3, np.int8)}


ONE_NODE = tree([-1], [[]])   # N = 1: no file holds it (below); tools/tree_arrays_check.cpp builds its TreeArrays from a Tree
CASES = {
    "three_nodes_no_entry": tree([-1, 0, 0], [[], [], []]),                                   # no entry at all: the padding path
    "root_only": tree([-1, 0, 0], [[(5, A, A, G), (9, Cc, Cc, T)], [], []]),
    "empty_node_between": tree([-1, 0, 0, 0], [[], [(3, A, A, Cc)], [], [(7, G, G, T), (8, T, T, A)]]),   # mut_off repeats
    "last_node_last_entries": tree([-1, 0, 0, 1, 1], [[], [(2, A, A, T)], [(4, Cc, Cc, G)], [(6, G, G, A)], [(10, T, T, Cc), (11, A, A, G)]]),
}
KEYS = ("parent", "mut_off", "mut_pos", "mut_ref", "mut_par", "mut_nuc")


def read_back(path):
    L = C.CDLL(HOST_LIB)
    L.uh_pb_to_arrays.argtypes = [C.c_char_p] + [C.c_void_p] * 8
    counts = (C.c_uint64 * 2)()
    assert L.uh_pb_to_arrays(path.encode(), counts, None, None, None, None, None, None, None) == 0   # the sizing call: counts only
    n, m = int(counts[0]), int(counts[1])
    # one element more than the counts say, preset: a copy that runs past mut_off[N] entries (the padding entry) would show
    got = [np.full(n + 1, -7, np.int64), np.full(n + 2, -7, np.int64), np.full(m + 1, -7, np.int32), np.full(m + 1, -7, np.int8),
           np.full(m + 1, -7, np.int8), np.full(m + 1, -7, np.int8)]
    counts2 = (C.c_uint64 * 2)()
    assert L.uh_pb_to_arrays(path.encode(), counts2, *[a.ctypes.data_as(C.c_void_p) for a in got], None) == 0
    assert (int(counts2[0]), int(counts2[1])) == (n, m)
    assert all(a[-1] == -7 for a in got)
    return (n, m), dict(zip(KEYS, [a[:-1] for a in got]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_arrays_come_back_as_written(name, tmp_path):
    want = CASES[name]
    path = str(tmp_path / "t.pb")
    pb_cases.write_pb_arrays(want, path)
    counts, got = read_back(path)
    assert counts == (want["n"], len(want["mut_pos"]))
    for k in KEYS:
        assert got[k].tolist() == want[k].tolist(), k


def test_a_single_node_is_no_tree_to_the_loader(tmp_path, capfd):
    """N = 1 with no entry never reaches the arrays through a file: its newick string is a bare leaf, which load_mat() refuses as
    the reference's parser does (mutation_annotated_tree.cpp:415-508: a leaf outside every bracket).  The call says so and
    leaves the counts alone."""
    path = str(tmp_path / "one.pb")
    pb_cases.write_pb_arrays(ONE_NODE, path)
    L = C.CDLL(HOST_LIB)
    L.uh_pb_to_arrays.argtypes = [C.c_char_p] + [C.c_void_p] * 8
    counts = (C.c_uint64 * 2)(77, 77)
    assert L.uh_pb_to_arrays(path.encode(), counts, None, None, None, None, None, None, None) == 1
    assert (int(counts[0]), int(counts[1])) == (77, 77)
    assert "incorrect Newick format" in capfd.readouterr().err
