"""The haplotype calls on a SARS-CoV-2-shaped tree of a million nodes against the closed form of tests/haplotypes_ref.py (held
against the literal walk on every small tree by tests/test_haplotypes_cpu.py).  The test checks its own inputs first, so that it
cannot pass on an easy question."""
import numpy as np
import pytest

from tests import haplotypes_ref as R
from tests.test_mask_at_size_gpu import topology
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_a_million_nodes():
    st = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2")
    arrays = st.arrays
    F = R.Fast(arrays)
    S = F.S
    # its own inputs: many shared haplotypes, one shared across children of the root, a leaf that equals the reference
    assert F.n_duplicate == 0 and (F.group_count > 1).sum() > 1000
    under = np.zeros(S.n, np.int64)                       # the child of the root above every node
    for lo, hi in S.levels[1:]:
        under[lo:hi] = np.where(S.par[lo:hi] == 0, np.arange(lo, hi), under[S.par[lo:hi]])
    top = under[F.leaf_bfs]
    gmin, gmax = np.full(len(F.group_count), S.n), np.zeros(len(F.group_count), np.int64)
    np.minimum.at(gmin, F.group_of_rank, top)
    np.maximum.at(gmax, F.group_of_rank, top)
    assert (gmin != gmax).sum() >= 1
    assert (np.diff(F.off) == 0).sum() >= 1 and F.group_size.max() > 30
    pl = Placer(topology(arrays))
    pl.haplotypes_attach(arrays)
    groups, info = pl.haplotype_groups()
    assert np.array_equal(groups["leaf"], F.leaf_bfs[F.group_rank]) and np.array_equal(groups["count"], F.group_count)
    assert np.array_equal(groups["size"], F.group_size) and not groups["pad"].any()
    assert (int(info["n_leaves"]), int(info["n_groups"]), int(info["n_collisions"]), int(info["n_duplicate"])) == (F.n_leaves, len(groups), 0, 0)
    assert int(info["n_visited"]) > 0
    # the sets of 1,000 drawn leaves, the leaves that equal the reference and the largest set among them
    rng = np.random.default_rng(31)
    size = np.diff(F.off)
    drawn = np.concatenate([rng.choice(F.n_leaves, 1000, replace=False), np.flatnonzero(size == 0)[:3], [int(size.argmax())]])
    leaves = F.leaf_bfs[drawn].astype(np.uint32)
    want = F.sets_csr(leaves)
    for chunk in (0, 333):
        got = pl.haplotype_sets(leaves, chunk_leaves=chunk)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), chunk
    t = pl.haplotype_time(reps=2)
    assert min(t) > 0
    pl.close()
