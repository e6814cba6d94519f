"""The relatives calls on a SARS-CoV-2-shaped tree of a million nodes against the closed form of tests/relatives_ref.py: 504 leaves
and 8 arbitrary nodes, closest mode and within 2.  The test checks its own inputs first -- rings of more than 100,000 leaves, long
and empty lists, long climbs -- so that it cannot pass on easy samples."""
import numpy as np
import pytest

from tests import relatives_ref as R
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_a_million_nodes():
    st = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2")
    arrays = st.arrays
    n = int(arrays["n"])
    rank = np.random.default_rng(19).permutation(n).astype(np.uint32)
    F = R.Fast(arrays, rank, rings=True)
    nodes = np.random.default_rng(17).choice(F.lbfs, 512, replace=False).astype(np.uint32)
    nodes[:8] = np.random.default_rng(18).integers(0, n, 8)
    closest, big_ring = [], 0
    for v in nodes:
        F.seen = []
        closest.append(F.closest(int(v)))
        big_ring += any((b1 - a1) + (b2 - a2) > 100_000 for a1, b1, a2, b2 in F.seen)
    within = [F.within(int(v), 2) for v in nodes]
    # the inputs are hard enough
    assert big_ring >= 100
    assert max(w["count"] for w in within) > 300
    assert sum(w["count"] == 0 for w in within) >= 1
    assert max(w["levels"] for w in closest) >= 20
    pl = Placer(arrays)
    pl.relatives_attach(rank)
    got = pl.relatives_closest(nodes)
    for i, w in enumerate(closest):
        R.check(got, w, i)
    got = pl.relatives_within(nodes, 2)
    for i, w in enumerate(within):
        R.check(got, w, i)
    pl.close()
