"""The dense searches (Placer.uncertainty, Placer.annotate_search; usher_amd/csrc/ugp_dense.hpp) where their machinery can go
wrong: trees of two and three segments at the segment and block edges, tie lists that cross segments and are cut by `cap` in
every segment, every sample of calls that take several batches, root mutations with the root as a sample (both branches of the
reference's initial bound), a handle's workspaces reused by a smaller call, and the clade counts at the same sizes.  Every field
that comes back is compared with the oracle's literal mapper2_body and the literal get_neighborhood_size
(tests/uncertainty_ref.py, tests/annotate_ref.py); tests/test_dense_cases_cpu.py proves that the fixtures of
tests/dense_cases.py have the properties relied on here."""
import numpy as np
import pytest

from oracle import capi
from tests import annotate_ref as A
from tests import dense_cases as D
from tests import uncertainty_ref as U
from usher_amd import Placer, QueryBatch

pytestmark = pytest.mark.gpu

KSEG, KBLOCK, BATCH = D.KSEG, D.KBLOCK, D.BATCH   # usher_amd/csrc/ugp_dense.hpp, ugp_uncertainty.hip (guarded by the CPU module)


def _unc(pl, nodes, cap):
    epps, nsize, ties, cnt = pl.uncertainty(np.asarray(nodes), cap=cap)
    return [(int(epps[i]), int(nsize[i]), ties[i].tolist(), int(cnt[i])) for i in range(len(nodes))]


def _ann(pl, samples, cap):
    best, ties, cnt = pl.annotate_search(QueryBatch(samples), cap=cap)
    return [(int(best[i]), ties[i].tolist(), int(cnt[i])) for i in range(len(samples))]


def _unc_want(want, cap):
    return [(nb, ns, tl[:cap], nb) for nb, ns, tl in want]


def _ann_want(want, cap):
    return [(b, tl[:cap], len(tl)) for b, tl in want]


def _brief(r):
    return tuple((len(x), x[:6], x[-3:]) if isinstance(x, list) else x for x in r)


def _same(got, want, labels, what):
    assert len(got) == len(want)
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, "%s: %d of %d differ; first: %s got %s want %s" % (
        what, len(bad), len(got), labels[bad[0]], _brief(got[bad[0]]), _brief(want[bad[0]]))


def _tree(arrays):
    return capi.OracleTree(arrays), U.dfs_order(arrays)


# ---- size edges --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("root", [False, True], ids=["plain", "rootmuts"])
@pytest.mark.parametrize("N", D.SIZE_EDGES)
def test_size_edges(N, root):
    """Comb trees of exactly N nodes at the segment and block edges; samples at the first position, around the segment edge, at
    the last position and a random handful (and the root, which has rows only with root mutations); uncertainty and
    annotate_search with one- and two-row queries."""
    arrays = D.comb(N - 1, root=D.COMB_ROOT if root else ())
    assert arrays["n"] == N
    ot, dfs = _tree(arrays)
    rng = np.random.default_rng(N)
    at = [0, 1, KSEG - 1, KSEG, KSEG + 1, 2 * KSEG - 1, 2 * KSEG, N - 1] + rng.integers(1, N, size=5).tolist()
    at = sorted({p for p in at if p < N})
    nodes = [int(dfs[p]) for p in at]
    pl = Placer(arrays)
    assert pl.node_order("dfs").tolist() == dfs.tolist()
    want = D.expected(arrays, nodes, ot, dfs)
    assert max(nb for nb, _, _ in want) > 2000
    _same(_unc(pl, nodes, N), _unc_want(want, N), at, "uncertainty N=%d" % N)
    rows = D.comb_rows(105) + D.comb_rows(100 + (N - 2) % 7) + D.comb_rows(103)   # the last leaf's site; a root mutation's
    aw = D.annotate_expected(arrays, rows, ot, dfs)
    assert min(len(tl) for _, tl in aw) > 2000
    _same(_ann(pl, rows, N), _ann_want(aw, N), list(range(len(rows))), "annotate_search N=%d" % N)
    pl.close()


# ---- ties across segments, and cap -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["plain", "root", "chain"])
def test_comb_ties_cross_segments_and_cap_cuts_in_each(variant):
    """K = 40,000: thousands of ties in each of three segments.  The full list, then `cap` at 1, 2, around the end of segment
    0's and of segment 1's ties and at the total: the oracle's prefix, the true count, epps and neighborhood size unchanged."""
    arrays = D.big_comb(variant)
    N = arrays["n"]
    ot, dfs = _tree(arrays)
    hub = 2 if variant == "chain" else 0
    j = int(np.flatnonzero(np.asarray(arrays["parent"]) == hub)[0]) + 4
    want = D.expected(arrays, [j], ot, dfs)
    pl = Placer(arrays)
    _same(_unc(pl, [j], N), _unc_want(want, N), [j], "uncertainty, full list")
    for cap in D.cap_edges(want[0][2])[2]:
        _same(_unc(pl, [j], cap), _unc_want(want, cap), [j], "uncertainty, cap=%d" % cap)
    rows = [D.big_comb_rows(variant)]
    aw = D.annotate_expected(arrays, rows, ot, dfs)
    _same(_ann(pl, rows, N), _ann_want(aw, N), [0], "annotate_search, full list")
    for cap in D.cap_edges(aw[0][1])[2]:
        _same(_ann(pl, rows, cap), _ann_want(aw, cap), [0], "annotate_search, cap=%d" % cap)
    # the root as a sample, and samples on the chain
    nodes = list(range(hub + 1)) + [N - 1]
    _same(_unc(pl, nodes, 64), _unc_want(D.expected(arrays, nodes, ot, dfs), 64), nodes, "uncertainty, root and chain")
    pl.close()


# ---- every sample, several batches ---------------------------------------------------------------------------------------------

BUSHY_CAP = 512   # above the largest tie set of the bushy tree's samples (373; asserted below), so every list is whole


@pytest.fixture(scope="module")
def bushy_run():
    """One Placer.uncertainty call on the bushy tree with 9,000 nodes: two full batches and a remainder of 808 = 12 * 64 + 40.
    The Placer stays open for test_workspace_reuse."""
    arrays = D.bushy()
    nodes = D.bushy_nodes()
    assert len(nodes) > 2 * BATCH and (len(nodes) - 2 * BATCH) % 64 != 0
    pl = Placer(arrays)
    got = _unc(pl, nodes, BUSHY_CAP)
    yield pl, nodes, got
    pl.close()


def test_every_sample_of_three_batches(bushy_run):
    _, nodes, got = bushy_run
    want = D.bushy_expected()
    assert max(nb for nb, _, _ in want) < BUSHY_CAP
    _same(got, _unc_want(want, BUSHY_CAP), nodes, "9,000 nodes of the bushy tree")


def test_tie_sets_that_span_segments(bushy_run):
    """Every sample of the 9,000 whose oracle tie set spans segments, alone in a call of its own batch layout, with cap at
    exactly the largest count."""
    _, nodes, got = bushy_run
    want = D.bushy_expected()
    span = [i for i, (nb, _, tl) in enumerate(want) if nb > 1 and len(D.segments(tl)) > 1]
    assert len(span) >= 1000
    _same([got[i] for i in span], _unc_want([want[i] for i in span], BUSHY_CAP), nodes[span], "spanning samples, in the big call")
    cap = max(want[i][0] for i in span)
    pl = Placer(D.bushy())
    _same(_unc(pl, nodes[span], cap), _unc_want([want[i] for i in span], cap), nodes[span], "spanning samples, own call")
    pl.close()


@pytest.mark.parametrize("count", [BATCH, BATCH + 1])
def test_calls_of_one_batch_and_one_more(count):
    nodes = D.bushy_nodes()[-count:]
    want = D.bushy_expected()[-count:]
    pl = Placer(D.bushy())
    _same(_unc(pl, nodes, 16), _unc_want(want, 16), nodes, "%d nodes" % count)
    pl.close()


# ---- root mutations --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("branch,spec", [(b, s) for b in ("kept", "joined", "below") for s in D.ROOT_CASES[b]])
def test_root_mutations(branch, spec):
    """Trees whose root carries mutations, every node a sample, the root included: the root's own score, root_muts in the
    initial bound, and (pinned by seed) the two outcomes in which the reference's initial {0} survives."""
    arrays = D.root_case(spec)
    n = arrays["n"]
    assert arrays["mut_off"][1] == spec[2]
    ot, dfs = _tree(arrays)
    nodes = np.arange(n)
    want = D.expected(arrays, nodes, ot, dfs)
    pl = Placer(arrays)
    for cap in (n, 2, 1):
        _same(_unc(pl, nodes, cap), _unc_want(want, cap), nodes, "uncertainty, cap=%d" % cap)
    rng = np.random.default_rng(spec[0])
    rows = [D.root_rows(arrays, rng, k) for k in range(8)]
    assert all(A.awkward(r) for r in rows)
    _same(_ann(pl, rows, n), _ann_want(D.annotate_expected(arrays, rows, ot, dfs), n), list(range(8)), "annotate_search")
    pl.close()


# ---- workspace reuse -------------------------------------------------------------------------------------------------------------

def test_workspace_reuse(bushy_run):
    """On the handle that ran the 9,000-node call: a 3-node call with a smaller cap, an annotate search, uncertainty again.
    Each equals what a fresh handle gives, and the oracle."""
    pl, nodes, _ = bushy_run
    arrays = D.bushy()
    want = D.bushy_expected()
    ot, dfs = _tree(arrays)
    big = [i for i, (nb, _, _) in enumerate(want) if nb > 40][:2] + [int(np.flatnonzero(nodes == 0)[0])]
    rng = np.random.default_rng(77)
    e0 = [int(arrays[k][0]) for k in ("mut_pos", "mut_ref", "mut_nuc")]
    rows = [D.awkward_rows(arrays, rng, k) for k in range(4)] + D.comb_rows(*e0)
    again = list(range(2 * BATCH - 50, 2 * BATCH + 50))
    steps = [("3 nodes, cap 3", lambda p: _unc(p, nodes[big], 3), _unc_want([want[i] for i in big], 3)),
             ("annotate", lambda p: _ann(p, rows, 300), _ann_want(D.annotate_expected(arrays, rows, ot, dfs), 300)),
             ("100 nodes, cap 40", lambda p: _unc(p, nodes[again], 40), _unc_want([want[i] for i in again], 40)),
             ("annotate, cap 1", lambda p: _ann(p, rows, 1), _ann_want(D.annotate_expected(arrays, rows, ot, dfs), 1)),
             ("3 nodes, cap 512", lambda p: _unc(p, nodes[big], BUSHY_CAP), _unc_want([want[i] for i in big], BUSHY_CAP))]
    used = [call(pl) for _, call, _ in steps]
    for (what, call, expect), got in zip(steps, used):
        _same(got, expect, list(range(len(expect))), "reused handle, " + what)
        fresh = Placer(arrays)
        _same(call(fresh), got, list(range(len(got))), "fresh handle, " + what)
        fresh.close()


# ---- clade counts at the same sizes ----------------------------------------------------------------------------------------------

def test_clade_counts_on_three_segments():
    arrays = D.bushy()
    n = arrays["n"]
    dfs = U.dfs_order(arrays)
    rng = np.random.default_rng(5)
    first_last = [int(dfs[0]), int(dfs[n - 1])]
    clades = [list(range(n)), [], first_last, rng.integers(0, n, size=300).tolist(), [], [int(dfs[KSEG])] * 3]
    pl = Placer(arrays)
    got = pl.clade_alleles(clades)
    assert len(got) == len(clades)
    for c, (ent, cnt) in zip(clades, got):
        assert dict(zip(ent.tolist(), cnt.tolist())) == A.alleles_literal(arrays, c)
    targets = [0, int(dfs[n - 1]), int(dfs[KSEG - 1]), int(dfs[KSEG]), int(arrays["parent"][int(dfs[n - 1])])]
    pc = [c for c in range(len(clades)) for _ in targets]
    pn = targets * len(clades)
    d = pl.clade_descendants(clades, pc, pn)
    assert d.tolist() == [A.descendants(arrays, clades[c], v) for c, v in zip(pc, pn)]
    assert d[0] == n - 1 and d[1] == 0
    pl.close()
