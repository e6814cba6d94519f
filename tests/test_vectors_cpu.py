"""ugp_vectors' closed form (tests/vectors_ref.py) against the literal mapper2_body of the oracle (OracleTree.node_vecs): every
(sample, node) of every case of tests/vectors_cases.py, 200 seeded random trees, the winners of OracleTree.place, and the header's
declarations against the ctypes table."""
import os
import re

import numpy as np
import pytest

from oracle import capi
from tests import vectors_cases as VC
from tests import vectors_ref as VR
from usher_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", VC.cases(), ids=lambda c: c["name"])
def test_closed_form_is_the_oracle_on_every_pair(case):
    ot, T = capi.OracleTree(case["arrays"]), VR.Tables(case["arrays"])
    n = int(case["arrays"]["n"])
    refused = 0
    for s, smp in enumerate(case["samples"]):
        for j in range(n):
            mine = VR.vectors(T, smp, j)
            assert mine["refused"] == (1 if j in case["refused"] else 0), (case["name"], s, j)
            if mine["refused"]:
                refused += 1
                assert mine["excess"] == [] and mine["imputed"] == []
                continue
            assert VR.agrees(mine, VR.oracle_answer(ot, smp, j)), (case["name"], s, j, mine, VR.oracle_answer(ot, smp, j))
    assert (refused > 0) == (case["name"] == "twice")
    assert all(0 <= s < len(case["samples"]) and 0 <= j < n for s, j in case["pairs"])


def test_the_cases_name_their_edges():
    by = {c["name"]: c for c in VC.cases()}
    T = {k: VR.Tables(c["arrays"]) for k, c in by.items()}
    for name in ("caterpillar", "caterpillar_flip"):
        nodes = sorted({j for _, j in by[name]["pairs"]})
        cum = lambda j: sum(1 for _ in _path_entries(T[name], j))
        assert sorted({cum(j) for j in nodes}) == sorted(VC.PATH_COUNTS)
    assert sorted(len(s["pos"]) for s in by["rows"]["samples"]) == [0, 1, 63, 64, 65, 70, 257]
    assert all(by["rows"]["samples"][-1]["is_missing"])
    assert sum(T["polytomy"].leaf) == 129
    # loop 1 passes a row on the node with descending entries, and both imputed lists and part 3 are exercised
    got = [VR.vectors(T[c["name"]], c["samples"][s], j) for c in VC.cases() for s, j in c["pairs"]]
    assert any(g["imputed"] for g in got) and any(len(g["excess"]) > g["n_branch"] + 1 for g in got)
    assert {(g["has_unique"], g["eligible"]) for g in got} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    bits = {bin(a & 15).count("1") for c in VC.cases() for s in c["samples"] for a, m in zip(s["nuc"], s["is_missing"]) if not m}
    assert bits == {1, 2, 3, 4}


def _path_entries(T, j_bfs):
    v = T.bfs2dfs[j_bfs]
    while v != VR.NIL:
        yield from range(T.moff[v], T.moff[v + 1])
        v = T.dpar[v]


def random_case(seed):
    """A random tree of up to 300 nodes in breadth-first order: masked entries, no position twice on a node, and samples with missing
    rows and ambiguous alleles at and around the tree's positions."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 301))
    parent = [-1] + sorted(int(rng.integers(0, max(1, j))) for j in range(1, n))
    parent = [-1] + [min(p, j - 1) for j, p in enumerate(parent[1:], 1)]
    npos = int(rng.integers(3, 40))
    muts = []
    for j in range(n):
        ents = []
        for p in rng.permutation(npos)[:int(rng.integers(0, 5))]:
            p = 10 + 3 * int(p)
            ents.append((p, VC.ONEHOT[int(rng.integers(0, 4))]))
        if rng.random() < 0.15:
            ents.insert(int(rng.integers(0, len(ents) + 1)), (-1, VC.ONEHOT[int(rng.integers(0, 4))], VC.ONEHOT[int(rng.integers(0, 4))]))
        muts.append(ents)
    samples = []
    for _ in range(3):
        rows = []
        for p in range(9, 10 + 3 * npos):
            u = rng.random()
            if u < 0.25:
                rows.append((p, None if rng.random() < 0.2 else int(rng.integers(1, 16))))
        samples.append(VC.sample(rows))
    return VC.case("random%d" % seed, parent, muts, samples)


def test_closed_form_is_the_oracle_on_random_trees():
    pairs = 0
    for seed in range(200):
        c = random_case(seed)
        ot, T = capi.OracleTree(c["arrays"]), VR.Tables(c["arrays"])
        n = int(c["arrays"]["n"])
        rng = np.random.default_rng(1000 + seed)
        for s, smp in enumerate(c["samples"]):
            for j in (range(n) if s == 0 else rng.integers(0, n, 30)):
                mine = VR.vectors(T, smp, int(j))
                assert not mine["refused"]
                assert VR.agrees(mine, VR.oracle_answer(ot, smp, int(j))), (seed, s, int(j))
                pairs += 1
    assert pairs > 30000


def test_winners_are_eligible_and_score_the_best():
    for c in VC.cases()[:5] + [random_case(s) for s in range(20)]:
        ot, T = capi.OracleTree(c["arrays"]), VR.Tables(c["arrays"])
        for smp in c["samples"]:
            w = ot.place(smp)
            for j in [w["best_j"]] + [int(t) for t in w["ties"]]:
                mine = VR.vectors(T, smp, j)
                if mine["refused"]:
                    continue
                assert mine["eligible"] == 1 and mine["set_difference"] == w["best"], (c["name"], j)


def test_header_declares_what_the_binding_lists():
    text = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    declared = set(re.findall(r"^int (ugp_vectors\w*)\(", text, re.M))
    assert declared == {k for k in _lib.SYMBOLS if k.startswith("ugp_vectors")} == {"ugp_vectors_attach", "ugp_vectors", "ugp_vectors_chunked",
                                                                                     "ugp_vectors_time"}
    for name in declared:   # and the argument counts agree
        args = re.search(r"^int " + name + r"\((.*?)\);", text, re.M | re.S).group(1)
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S)
        assert len(args.split(",")) == len(_lib.SYMBOLS[name][1]), name
