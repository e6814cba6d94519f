"""The ugp_subtree calls at the smallest sizes that cross the seams of their three flag scans (ugp_scan.hpp: kSeg items per block):
the selected positions over N nodes, the entries of the nodes with members over the tree's entries, and the survivors over the sorted
gathered entries -- each count at one segment less one, one segment, one more, one segment and one block, two segments and two and
one, with the flags at the seam between the first two segments set ('11') and clear ('00'); a caterpillar deeper than two segments
whose one chain crosses two seams, and a star of one segment and one leaf with every second leaf selected.  The oracle is the closed
form of tests/subtree_ref.py; tests/test_subtree_cpu.py runs the same generators small against the literal walk."""
import numpy as np
import pytest

from tests import subtree_cases as SC
from tests import subtree_ref as R
from tests import summary_cases as SMC
from tests.scan_edge_cases import EDGES, KBLOCK, KSEG
from usher_amd import Placer

pytestmark = pytest.mark.gpu
assert EDGES == (KSEG - 1, KSEG, KSEG + 1, KSEG + KBLOCK - 1, KSEG + KBLOCK, 2 * KSEG, 2 * KSEG + 1)


def check(arrays, sel):
    want = R.closed_form(arrays, sel)
    pl = Placer(SMC.topology(arrays))
    pl.subtree_attach(arrays)
    got = pl.subtree_nodes(sel)
    assert R.same(got, want, pl.subtree_owner(np.arange(int(arrays["n"]), dtype=np.uint32)))
    pl.close()
    return want


@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("N", EDGES)
def test_node_counts(N, variant):
    arrays, sel = SC.seam_selection(N, variant, KSEG)
    assert arrays["n"] == N
    want = check(arrays, sel)
    assert len(want["kept"]) > len(sel) and want["info"]["n_gathered"] > 100


@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("K", EDGES)
def test_kept_and_entry_counts(K, variant):
    arrays, sel = SC.entry_star(K, variant, KSEG)
    want = check(arrays, sel)
    gone = 2 if variant == "00" and K > KSEG else 1 if variant == "00" and K == KSEG else 0
    assert arrays["n"] == K == len(arrays["mut_pos"]) and len(want["kept"]) == K - gone == want["info"]["n_gathered"]


@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("G", EDGES)
def test_gathered_counts(G, variant):
    arrays, sel = SC.cancel_star(G, variant, KSEG)
    want = check(arrays, sel)
    assert want["info"]["n_gathered"] == G and len(want["pos"]) == G - (2 if variant == "00" and G > KSEG else 0)


def test_a_chain_across_two_seams():
    arrays, sel = SC.deep_caterpillar(2 * KSEG + 40)
    want = check(arrays, sel)
    assert len(want["kept"]) == 3 and want["info"]["longest_chain"] == 2 * KSEG + 39 and len(want["pos"]) <= 6


def test_every_second_leaf_of_a_star():
    arrays, sel = SC.half_star(KSEG + 1)
    want = check(arrays, sel)
    assert len(want["kept"]) == 1 + (KSEG + 2) // 2
