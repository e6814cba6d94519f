"""RIPPLES' search (ripples/main.cpp:300-680): the closed form the device runs (tests/ripples_ref.closed) against the literal
restatement through the oracle's mapper2_body, the top-2 selection claim, and the planted-recombinant fixture."""
import numpy as np
import pytest

from oracle import capi
from tests import ripples_ref as RR
from tests import synth

OPTS = [dict(l=3, r=1000, R=10 ** 7, p=3, n_desc=10), dict(l=1, r=0, R=10 ** 7, p=0, n_desc=1),
        dict(l=1, r=500, R=6000, p=3, n_desc=10), dict(l=3, r=0, R=10 ** 7, p=0, n_desc=1)]


def _trees():
    for seed in range(12):
        yield "planted%d" % seed, RR.planted(seed, n_leaves=120 + 20 * (seed % 4), masked_rows=seed % 3 == 1,
                                               p_masked=0.05 if seed % 4 == 2 else 0.0, iupac=seed % 5 == 3)
    for seed in range(10):
        rng = np.random.default_rng(500 + seed)
        arrays, _, _, _ = synth.random_tree(rng, 60 + 10 * seed, genome_len=4000, n_sites=150, mut_counts=(0, 1, 1, 2, 3, 4),
                                            p_masked=0.08 if seed % 2 else 0.0, root_muts=seed % 3)
        arrays["names"] = ["s%03d_%d" % ((j * 37) % arrays["n"], j) for j in range(arrays["n"])]   # name order != BFS order
        yield "random%d" % seed, arrays
    for seed in range(4):
        arrays, _ = synth.polytomy_case(seed, fanouts=(12, 9, 5), n_queries=1, genome_len=3000, n_sites=120)
        yield "polytomy%d" % seed, arrays
    for seed in range(4):
        arrays, _ = synth.caterpillar_case(seed, depth=40, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=200)
        yield "caterpillar%d" % seed, arrays


def _branches(arrays, rng, k=6):
    n = arrays["n"]
    par = np.asarray(arrays["parent"])
    internal = np.unique(par[1:])
    pick = list(rng.choice(internal, min(k, len(internal)), replace=False)) + list(rng.choice(n, 2, replace=False)) + [0]
    if "recomb_" in " ".join(arrays["names"][-200:]):
        pick += [j for j, s in enumerate(arrays["names"]) if s.startswith("recomb_")]
    return [int(x) for x in pick]


@pytest.mark.parametrize("name,arrays", list(_trees()), ids=lambda v: v if isinstance(v, str) else "")
def test_closed_form_equals_literal(name, arrays):
    rng = np.random.default_rng(len(name))
    br = _branches(arrays, rng)
    ot = capi.OracleTree(arrays)
    opts = OPTS[len(name) % len(OPTS)], OPTS[(len(name) + 1) % len(OPTS)]
    for o in opts:
        assert RR.closed(arrays, br, **o) == RR.literal(arrays, br, ot, **o), (name, o)


def test_planted_recombinant_is_found():
    for seed in range(4):
        arrays = RR.planted(seed)
        X = RR.node_named(arrays, "recomb_%d" % seed)
        ev = RR.literal(arrays, [X])
        assert ev, seed
        assert all(e["donor_count"] + e["acceptor_count"] + 3 <= int(np.diff(arrays["mut_off"])[X]) for e in ev)


def _literal_select(don, acc, nid, B):
    """:577-606: sort by (count, name), truncate to 1000, the first donor with a fitting acceptor."""
    don = sorted(don)[:1000]
    acc = sorted(acc)[:1000]
    for d in don:
        for a in acc:
            if d[1] != a[1] and d[1] != nid and a[1] != nid and d[0] + a[0] <= B:
                return d, a
    return None


def _top3(lst):
    return sorted((c << 32) | r for c, r in lst)[:3]


def _check_select(don, acc, nid, B):
    want = _literal_select(don, acc, nid, B)
    got = RR.select(_top3(don), _top3(acc), nid, B)
    if want is None:
        assert got is None
    else:
        assert got == ((want[0][0] << 32) | want[0][1], (want[1][0] << 32) | want[1][1])


def test_top2_selection_engineered():
    B = 4
    # d1 = a1: the donor pairs with the second acceptor, or the second donor with the first acceptor
    _check_select([(0, 5), (3, 6)], [(0, 5), (5, 7)], nid=99, B=B)
    _check_select([(1, 5), (2, 6)], [(0, 5), (4, 7)], nid=99, B=B)
    _check_select([(2, 5), (3, 6)], [(0, 5), (3, 7)], nid=99, B=B)
    # nid at the head of both lists
    _check_select([(0, 9), (1, 5), (2, 6)], [(0, 9), (1, 5), (3, 7)], nid=9, B=B)
    # a tie in count: the name rank decides, not the node index
    _check_select([(1, 30), (1, 4)], [(1, 30), (1, 4)], nid=99, B=B)
    # nothing fits
    _check_select([(3, 1), (3, 2)], [(2, 1), (2, 3)], nid=99, B=B)


def test_top2_selection_random_long_lists():
    """Lists longer than 1000 and every arrangement of nid / shared nodes: the top-3 rule equals the literal one."""
    rng = np.random.default_rng(7)
    for it in range(400):
        n = int(rng.choice([2, 3, 5, 40, 1500]))
        B = int(rng.integers(0, 6))
        ranks = rng.permutation(4 * n)[:n]
        don = [(int(rng.integers(0, B + 1)), int(r)) for r in ranks if rng.random() < 0.8]
        acc = [(int(rng.integers(0, B + 1)), int(r)) for r in ranks if rng.random() < 0.8]
        nid = int(ranks[int(rng.integers(0, n))]) if rng.random() < 0.5 else -1
        _check_select(don, acc, nid, B)
