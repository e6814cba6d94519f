"""Nearest-k without a GPU: the restatements of tests/nearest_ref.py against each other (canonical and the reference's tie order,
per-leaf walks and numpy tables), the ABI surface of ugp_nearest_k, and the argument errors of `matutils-amd extract`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import nearest_cases as NC
from tests import nearest_ref as R
from tests import stdorder, synth
from usher_amd import Placer, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATUTILS = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
PB = os.path.join(ROOT, "tests", "golden", "survey_ref", "global", "global_assignments.pb")


def _small_trees():
    yield synth.make_case(71, n_leaves=120, n_queries=1, n_sites=60, genome_len=400, p_masked=0.1)[0]
    yield synth.polytomy_case(72, fanouts=(6, 9, 5), n_queries=1, genome_len=3000, n_sites=200)[0]
    yield synth.caterpillar_case(73, depth=40, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=300)[0]
    yield NC.tie_tree()[0]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_two_tie_orders_agree_up_to_the_cut(which, tmp_path):
    arrays = list(_small_trees())[which]
    T, F = R.Tree(arrays), R.Fast(arrays)
    so = stdorder.StdOrder(tmp_path)
    L = int(T.nleaves[0])
    differ = 0
    for node in range(0, arrays["n"], 1 if arrays["n"] <= 300 else 5):
        for k in (1, 2, 7, 25, L - 1, L, L + 5):
            if k <= 0:
                continue
            a, b = R.literal(T, node, k), R.literal(T, node, k, sorter=so)
            assert a == F.query(node, k), (node, k)
            for f in ("count", "anc", "last_anc", "cut_dist", "n_at_cut"):
                assert a[f] == b[f], (node, k, f)
            if k >= L:
                assert a["count"] == 0 and a["anc"] == R.NONE
                continue
            nl = int(T.nleaves[a["last_anc"]])
            assert sorted(a["nodes"][:nl]) == sorted(b["nodes"][:nl])
            assert a["dist"][nl:] == b["dist"][nl:] == sorted(a["dist"][nl:])
            strict = lambda r: sorted(v for v, d in zip(r["nodes"][nl:], r["dist"][nl:]) if d < r["cut_dist"])
            assert strict(a) == strict(b)
            taken_at_cut = sum(1 for d in a["dist"][nl:] if d == a["cut_dist"])
            if a["n_at_cut"] == taken_at_cut:
                assert sorted(a["nodes"][nl:]) == sorted(b["nodes"][nl:])
            else:
                differ += sorted(a["nodes"][nl:]) != sorted(b["nodes"][nl:])
    if which == 3:
        assert differ, "the reference's order never chose another set: the case does not test the tie rule"


def test_reference_rules_kept():
    T = R.Tree(NC.tie_tree()[0])
    leaf = NC.tie_tree()[1]
    r = R.literal(T, leaf, 100)
    assert (r["last_anc"], r["anc"], r["n_at_cut"], r["count"]) == (int(T.par[leaf]), 1, 480, 100)
    # a leaf is a candidate of its own search: is_ancestor starts at the parent
    r = R.literal(T, leaf, 1)
    assert r["nodes"] == [leaf] and r["count"] == 1
    r = R.literal(T, leaf, 19)
    assert r["anc"] == int(T.par[leaf]) and r["nodes"][0] == leaf and r["nodes"].count(leaf) == 2
    # a node with more than k leaves of its own: all of them
    r = R.literal(T, 1, 10)
    assert r["anc"] == r["last_anc"] == 1 and r["count"] == 500


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    for name in ("ugp_nearest_attach", "ugp_nearest_k", "ugp_nearest_k_chunked"):
        assert re.search(r"\bint %s\(ugp_mat \*mat" % name, hdr) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    m = re.search(r"typedef struct ugp_nearest_info \{(.*?)\} ugp_nearest_info;", hdr, re.S)
    fields = re.findall(r"uint32_t (\w+);", m.group(1))
    assert tuple(fields) == Placer.NEAREST_INFO.names and Placer.NEAREST_INFO.itemsize == 4 * len(fields)
    # no handle: an error code, not a crash
    L = _lib.lib()
    assert L.ugp_nearest_k(None, 1, None, None, 1, None, None, None) == -1
    assert L.ugp_nearest_attach(None, None) == -1


def _extract(*args):
    return subprocess.run([MATUTILS, "extract"] + list(args), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,msg", [
    (["-u", "x.txt"], "input-mat"),
    (["-i", PB], "ERROR: No output files requested!"),
    (["-i", PB, "-u", "x.txt", "-k", "nocolon"], "ERROR: Invalid formatting of -k argument. Requires input in the form of 'sample_id:k'"),
    (["-i", PB, "-u", "x.txt", "-k", "s:0"], "ERROR: Invalid neighborhood size. Please choose a positive nonzero integer."),
    (["-i", PB, "-u", "x.txt", "-K", "f.txt:5"], "not supported by matutils-amd"),
    (["-i", PB, "-u", "x.txt", "-c", "B.1"], "not supported by matutils-amd"),
    (["-i", PB, "-u", "x.txt", "-j", "o.json"], "not supported by matutils-amd"),
    (["-i", PB, "-u", "x.txt", "--closest-relatives", "o.tsv"], "not supported by matutils-amd"),
    (["-i", "/nonexistent/x.pb", "-u", "x.txt"], "x.pb"),
    (["-i", PB, "-u", "x.txt", "--bogus"], "bogus"),
])
def test_extract_argument_errors(args, msg, tmp_path):
    r = _extract(*(args + ["-d", str(tmp_path)]))
    assert r.returncode != 0 and msg in r.stderr, (r.returncode, r.stderr[-500:])


@pytest.mark.parametrize("L", [70, 131])
def test_sort_tree_is_what_the_size_edges_need(L):
    """The generator of the sort's size edges at a size the per-leaf walk takes: every need from 1 to L - 2, the numpy restatement
    against the literal one, and the shape the device test relies on."""
    arrays, q, P = NC.sort_tree(L)
    T, F = R.Tree(arrays), R.Fast(arrays)
    assert int(T.nleaves[P]) == L and int(T.par[q]) == P and not T.kids[q]
    keys = [int(T.nmut[c]) for c in T.kids[P]]
    assert keys == [(L - i) % 64 + 1 for i in range(L)] and keys != sorted(keys) and len(set(keys)) == min(L, 64)   # unsorted, with ties
    for need in range(1, L - 1):
        want = F.query(q, need + 1)
        assert want == R.literal(T, q, need + 1), need
        assert (want["anc"], want["last_anc"], want["count"]) == (P, q, need + 1) and want["nodes"][0] == q
        assert want["dist"][1:] == sorted(keys)[:need]                      # the need smallest keys, the leaf's own among them
        if keys[0] < want["cut_dist"]:                                      # a candidate of its own search: listed twice
            assert want["nodes"].count(q) == 2
    assert F.query(q, L)["anc"] == 0                                        # one more climbs past P
