"""The fixtures of tests/dense_cases.py have the properties tests/test_dense_edges_gpu.py relies on -- shown with the oracle
alone, so that a fixture that stops meeting one fails here instead of letting the GPU test pass vacuously.  CPU only."""
import os
import re

import numpy as np
import pytest

from oracle import capi
from tests import annotate_ref as A
from tests import dense_cases as D
from tests import uncertainty_ref as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "usher_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_follow_the_sources():
    """KSEG / KBLOCK / BATCH are literals in dense_cases.py; the sizes tested follow the sources through this guard."""
    dense = _text("ugp_dense.hpp")
    assert re.search(r"constexpr uint32_t kBlock = (\d+);", dense).group(1) == str(D.KBLOCK)
    assert re.search(r"constexpr uint32_t kSeg = (\d+);", dense).group(1) == str(D.KSEG)
    unc = _text("ugp_uncertainty.hip")
    assert re.search(r"constexpr uint64_t kDiffBudget = 1ull << (\d+);", unc).group(1) == "31"
    m = re.search(r"bmax = std::max<uint64_t>\(1, std::min<uint64_t>\((\d+), kDiffBudget / \(4ull \* N\)\)\);", unc)
    assert m and m.group(1) == str(D.BATCH)
    for arrays in (D.bushy(), D.big_comb("chain")):   # the trees are small enough for full batches
        assert (1 << 31) // (4 * arrays["n"]) >= D.BATCH
    assert D.SIZE_EDGES == (D.KSEG - 1, D.KSEG, D.KSEG + 1, D.KSEG + D.KBLOCK - 1, D.KSEG + D.KBLOCK, 2 * D.KSEG, 2 * D.KSEG + 1)


@pytest.mark.parametrize("variant", ["plain", "root", "chain"])
def test_big_combs_tie_thousands_in_every_segment(variant):
    arrays = D.big_comb(variant)
    ot, dfs = capi.OracleTree(arrays), U.dfs_order(arrays)
    hub = 2 if variant == "chain" else 0
    j = int(np.flatnonzero(np.asarray(arrays["parent"]) == hub)[0]) + 4
    nb, ties = D.search_ties(ot, arrays, dfs, j)
    assert nb == len(ties) >= 5000 and D.segments(ties) == [0, 1, 2]
    c0, c1, caps = D.cap_edges(ties)
    assert c0 > 2 and c1 > 2 and len(ties) - c0 - c1 > 2 and len(set(caps)) == len(caps) and caps == sorted(caps)
    if variant == "plain":
        assert j == 5 and (nb, ties[:3], ties[-1]) == (5713, [12, 19, 26], 39996)
    c, dc, deepest = D.lca_and_depths(arrays, dfs, ties)
    if variant == "chain":   # the common ancestor is the hub, and the second hub's leaves lie two levels below it
        assert c == hub and dc == 2 and deepest == dc + 2
        assert arrays["mut_off"][hub + 1] - arrays["mut_off"][1] == 3   # mutations on the chain
    else:
        assert c == 0
    # annotate's one-row query
    best, at = A.search(ot, arrays, D.big_comb_rows(variant), dfs)
    c0, c1, caps = D.cap_edges(at)
    assert len(at) >= 5000 and D.segments(at) == [0, 1, 2] and c0 > 2 and c1 > 2 and len(set(caps)) == len(caps)
    if variant == "root":
        pos = arrays["mut_pos"][:arrays["mut_off"][1]]
        assert len(pos) == 3 and (pos < 0).sum() == 1 and 103 in pos.tolist()
        assert D.root_branch(arrays, 0, ot, dfs) == "kept" and D.search_ties(ot, arrays, dfs, 0) == (1, [0])
    else:
        assert D.root_branch(arrays, 0, ot, dfs) == "empty"


@pytest.mark.parametrize("N", D.SIZE_EDGES)
def test_size_edge_combs(N):
    for root in ((), D.COMB_ROOT):
        arrays = D.comb(N - 1, root=root)
        assert arrays["n"] == N and len(arrays["parent"]) == N and arrays["mut_off"][-1] == N - 1 + len(root)
        ot, dfs = capi.OracleTree(arrays), U.dfs_order(arrays)
        assert dfs.tolist() == list(range(N))
        for p in (1, N - 1):
            nb, ties = D.search_ties(ot, arrays, dfs, p)
            assert nb > 2000 and ties[0] <= 14 and N - 1 - ties[-1] <= 14   # ties from one end of the tree to the other


def test_bushy_tree_and_its_samples():
    arrays = D.bushy()
    n = arrays["n"]
    assert n == 33139 and (n + D.KSEG - 1) // D.KSEG == 3
    nodes = D.bushy_nodes()
    assert len(nodes) == 9000 == len(set(nodes.tolist())) and 0 in nodes
    assert len(nodes) > 2 * D.BATCH and (len(nodes) - 2 * D.BATCH) % 64 != 0
    internal = np.unique(np.asarray(arrays["parent"])[1:])
    assert np.isin(internal, nodes).all()
    ot, dfs = capi.OracleTree(arrays), U.dfs_order(arrays)
    want = D.expected(arrays, nodes[:300], ot, dfs)
    span = [w for w in want if w[0] > 1 and len(D.segments(w[2])) > 1]
    assert len(span) >= 15 and any(len(D.segments(w[2])) == 3 for w in span)
    deep = [w for w in span if (lambda c, dc, deepest: deepest >= dc + 2)(*D.lca_and_depths(arrays, dfs, w[2]))]
    assert len(deep) >= 15                                # k_tiewrite's walk to the child of the common ancestor
    assert len({w[1] for w in want}) >= 5                 # neighborhood sizes vary
    assert any(w[0] == 0 for w in want) and any(w[0] == 1 for w in want)
    # the shortcut of D.expected for large tie sets is the literal pair loop
    for nb, ns, ties in want:
        if nb > 1:
            assert D.neighborhood_top2(arrays, [int(dfs[t]) for t in ties]) == ns


def test_neighborhood_top2_is_the_literal_loop_on_a_chain_comb():
    arrays = D.comb(60, chain=2, sub=30)
    ot, dfs = capi.OracleTree(arrays), U.dfs_order(arrays)
    some = 0
    for j in range(arrays["n"]):
        nb, ties = D.search_ties(ot, arrays, dfs, j)
        if nb > 1:
            bfs = [int(dfs[t]) for t in ties]
            assert D.neighborhood_top2(arrays, bfs) == U.neighborhood_literal(arrays, bfs) == U.neighborhood_closed(arrays, bfs)
            some += 1
    assert some >= 50


@pytest.mark.parametrize("branch,spec", [(b, s) for b in ("kept", "joined", "below") for s in D.ROOT_CASES[b]])
def test_pinned_root_cases_reach_their_branch(branch, spec):
    """'kept': the device's `m == kNone || m > init` branch; 'joined': its `m == init` branch (shift = 1).  Both are reachable:
    the root's rows are its own mutations, its initial bound is 2 * root_muts + 1, and in about one random tree in 300 no
    candidate scores below that."""
    arrays = D.root_case(spec)
    assert arrays["mut_off"][1] == spec[2] and (np.asarray(arrays["mut_pos"]) < 0).any()
    ot, dfs = capi.OracleTree(arrays), U.dfs_order(arrays)
    nb, ties = D.search_ties(ot, arrays, dfs, 0)
    if branch == "kept":
        assert D.root_branch(arrays, 0, ot, dfs) == "kept" and (nb, ties) == (1, [0])
    elif branch == "joined":
        assert D.root_branch(arrays, 0, ot, dfs) == "joined" and nb == len(ties) > 1 and ties[0] == 0 and ties[1] > 0
    else:
        got = {D.root_branch(arrays, j, ot, dfs) for j in range(arrays["n"])}
        assert got == {"below"}, got
    rng = np.random.default_rng(spec[0])
    root_pos = [int(p) for p in arrays["mut_pos"][:spec[2]] if p >= 0]
    for k in range(8):
        rows = D.root_rows(arrays, rng, k)
        p = rows["pos"].tolist()
        assert A.awkward(rows) and p == sorted(p) and min(p) < 0 and set(root_pos) <= set(p)


def test_each_branch_is_pinned_at_least_twice():
    assert len(D.ROOT_CASES["kept"]) >= 2 and len(D.ROOT_CASES["joined"]) >= 2
    assert {s[2] for b in ("kept", "joined") for s in D.ROOT_CASES[b]} == {1, 2, 3}
    assert 60 <= min(s[1] for b in D.ROOT_CASES for s in D.ROOT_CASES[b]) and max(s[1] for b in D.ROOT_CASES for s in D.ROOT_CASES[b]) == 400
    found = D.find_root_cases([909, 1089], n_leaves=(60,), root_muts=(1,), n_sites=(40,))
    assert found == {"kept": [((909, 60, 1, 40), 0)], "joined": [((1089, 60, 1, 40), 0)]}
