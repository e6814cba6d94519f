"""ugp_uncertainty / Placer.uncertainty (matUtils uncertainty, uncertainty.cpp:132-339) against the oracle's literal
mapper2_body fed the UNSORTED sample findEPPs builds, and the literal get_neighborhood_size."""
import numpy as np
import pytest

from oracle import capi
from tests import synth
from tests import uncertainty_ref as U
from usher_amd import Placer

pytestmark = pytest.mark.gpu


def _check(arrays, nodes, cap=4096, chunk_nodes=None):
    pl = Placer(arrays, chunk_nodes=chunk_nodes)
    epps, nsize, ties, cnt = pl.uncertainty(np.asarray(nodes), cap=cap)
    dfs = pl.node_order("dfs").astype(np.int64)
    assert dfs.tolist() == U.dfs_order(arrays).tolist()
    want = U.expected(arrays, nodes, capi.OracleTree(arrays), dfs)
    for i, (nb, ns, wt) in enumerate(want):
        got = (int(epps[i]), int(nsize[i]), ties[i].tolist(), int(cnt[i]))
        assert got == (nb, ns, wt[:cap], nb), (int(nodes[i]), got, (nb, ns, wt[:10]))
    pl.close()
    return want


def _nodes(arrays, n_internal, seed):
    par = np.asarray(arrays["parent"])
    leaves = np.setdiff1d(np.arange(arrays["n"]), par[1:])
    internal = np.setdiff1d(np.unique(par[1:]), [0])
    rng = np.random.default_rng(seed)
    return np.concatenate([leaves, rng.choice(internal, min(n_internal, len(internal)), replace=False)])


@pytest.mark.parametrize("seed,p_masked", [(301, 0.0), (302, 0.03), (303, 0.0)])
def test_every_leaf_and_some_internal_nodes(seed, p_masked):
    arrays, _ = synth.make_case(seed, n_leaves=400, n_queries=1, n_sites=90, p_masked=p_masked)
    want = _check(arrays, _nodes(arrays, 40, seed), chunk_nodes=48)
    assert any(nb > 1 for nb, _, _ in want) and any(nb == 1 for nb, _, _ in want)


def test_literal_order_is_what_is_reproduced():
    """The fixture has samples whose literal and sorted row orders give different searches: the device follows the literal one."""
    arrays, _ = synth.make_case(301, n_leaves=400, n_queries=1, n_sites=90)
    nodes = _nodes(arrays, 0, 0)
    ot = capi.OracleTree(arrays)
    dfs = U.dfs_order(arrays)
    differ = [j for j in nodes
              if U.search(ot, arrays, dfs, int(j), U.literal_sample(arrays, int(j))) !=
              U.search(ot, arrays, dfs, int(j), U.sorted_sample(U.literal_sample(arrays, int(j))))]
    assert len(differ) >= 10, len(differ)
    _check(arrays, np.asarray(differ))


def test_polytomy_and_caterpillar():
    arrays, _ = synth.polytomy_case(7, fanouts=(8, 10, 6), n_queries=1, genome_len=3000, n_sites=200)
    _check(arrays, _nodes(arrays, 30, 7), chunk_nodes=64)
    arrays, _ = synth.caterpillar_case(8, depth=120, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=300)
    _check(arrays, _nodes(arrays, 30, 8), chunk_nodes=32)


def test_small_cap_keeps_neighborhood_and_true_count():
    arrays, _ = synth.polytomy_case(11, fanouts=(6, 12, 8), n_queries=1, genome_len=3000, n_sites=150)
    nodes = _nodes(arrays, 20, 11)
    pl = Placer(arrays)
    full = pl.uncertainty(nodes, cap=arrays["n"])
    small = pl.uncertainty(nodes, cap=2)
    big = [i for i in range(len(nodes)) if full[3][i] > 2]
    assert len(big) >= 5
    assert small[0].tolist() == full[0].tolist() and small[1].tolist() == full[1].tolist() and small[3].tolist() == full[3].tolist()
    for i in range(len(nodes)):
        assert small[2][i].tolist() == full[2][i][:2].tolist()
    pl.close()


def test_empty_sample_and_parent_rule():
    """A leaf whose root path carries no mutation: the reference skips the search; reported as 0 placements, no ties.
    And -o's single-placement rule names the sample's parent, whatever node the search found."""
    arrays, _ = synth.make_case(304, n_leaves=200, n_queries=1, n_sites=60)
    n = arrays["n"]
    assert arrays["mut_off"][1] == 0            # the synthetic root carries no mutation
    arrays = dict(arrays)
    arrays["parent"] = np.append(arrays["parent"], 0)
    arrays["mut_off"] = np.append(arrays["mut_off"], arrays["mut_off"][-1])
    arrays["n"] = n + 1
    pl = Placer(arrays)
    epps, nsize, ties, cnt = pl.uncertainty(np.array([n, 5]), cap=8)
    assert (int(epps[0]), int(nsize[0]), ties[0].tolist(), int(cnt[0])) == (0, 0, [], 0)
    want = U.expected(arrays, [5])
    assert (int(epps[1]), int(nsize[1])) == want[0][:2]
    names = ["n%d" % j for j in range(n + 1)]
    e, o = U.render(names, arrays["parent"], U.dfs_order(arrays), [n], [(0, 0, [])])
    assert o == "placement\tsample\nn%d\tn%d\n" % (n, n)
    _, o = U.render(names, arrays["parent"], U.dfs_order(arrays), [5], [(1, 0, [123])])
    assert o.splitlines()[2] == "n%d\tn5" % arrays["parent"][5]
    pl.close()
