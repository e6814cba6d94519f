"""The select calls on a SARS-CoV-2-shaped tree of a million nodes against the closed form of tests/select_ref.py: 64 mutation
queries that include the position with the most owners, a position with one owner and an absent one, 1,000 subtree nodes and 3
MRCA sets.  The test checks its own inputs first, so that it cannot pass on easy queries."""
import numpy as np
import pytest

from tests import select_ref as R
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_a_million_nodes():
    st = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2")
    arrays = st.arrays
    n = int(arrays["n"])
    F = R.Fast(arrays)
    rng = np.random.default_rng(23)
    per_pos = np.bincount(F.opos, minlength=F.tp + 1)
    most, single = int(per_pos.argmax()), int(np.flatnonzero(per_pos == 1)[0])
    absent = int(np.flatnonzero(per_pos[1:] == 0)[0]) + 1
    assert per_pos[most] > 100 and per_pos[absent] == 0 and absent < F.tp
    k = int(np.flatnonzero(F.opos == most)[0])
    pos = [most, most, single, absent, F.tp - 1, F.tp, -1] + [int(p) for p in rng.choice(F.opos, 57)]
    nuc = [int(F.onuc[k]), int(F.onuc[k]) ^ 15, int(F.onuc[np.flatnonzero(F.opos == single)[0]]), 1, 1, 1, 1] + [int(a) for a in rng.choice([1, 2, 4, 8], 57)]
    assert len(pos) == 64
    want = F.mutations(pos, nuc)
    assert want[1][0] > 100 and want[1][2] >= 1 and want[1][3] == 0 and 0 < want[0].sum() < F.n_leaves
    nodes = rng.integers(0, n, 1000).astype(np.uint32)
    nodes[:3] = (F.lbfs[0], F.lbfs[-1], F.par[int(F.lbfs[5])])
    want_sub = F.subtrees(nodes)
    assert 0 < want_sub[0].sum() < F.n_leaves and want_sub[1].max() > 100
    sets = []
    for size in (2, 50, 3):
        m = np.zeros(F.n_leaves, bool)
        m[rng.choice(F.n_leaves, size, replace=False)] = True
        sets.append(m)
    sets[2][:] = False
    lo, hi = F.ranks(int(nodes[np.argmax(want_sub[1] * (want_sub[1] < 5000))]))   # a set inside one mid-sized subtree
    sets[2][[lo, hi - 1]] = True
    pl = Placer(arrays)
    assert np.array_equal(pl.select_leaves(), F.lbfs)
    got = pl.select_mutations(pos, nuc)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = pl.select_subtrees(nodes)
    assert np.array_equal(got[0], want_sub[0]) and np.array_equal(got[1], want_sub[1])
    for m in sets:
        assert pl.select_mrca(m) == F.mrca(m)
    assert pl.select_mrca(sets[2])[1] == hi - lo
    pl.close()
