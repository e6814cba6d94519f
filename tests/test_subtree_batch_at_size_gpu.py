"""ugp_subtree_batch on the 1M-node synthetic MAT of the sars2 shape that tests/test_nearest_at_size_gpu.py uses: the nearest-50 and
nearest-500 sets of 256 drawn leaves (Placer.nearest_k) as one batch with the default group budget, and again with a budget that
splits the batch into several groups; every slice must equal the single call on its selection."""
import numpy as np
import pytest

from tests import nearest_ref as NR
from tests import subtree_ref as R
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_batch_against_single_calls_at_size():
    arrays = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2").arrays
    F = NR.Fast(arrays)
    leaves = F.dfs[np.flatnonzero(F.leaf)]
    nodes = np.random.default_rng(23).choice(leaves, 256, replace=False)
    ks = np.where(np.arange(256) % 2 == 0, 50, 500)
    pl = Placer(arrays)
    out, _, info = pl.nearest_k(nodes, ks)
    sels = [out[i, :min(int(info[i]["count"]), int(ks[i]))] for i in range(256)]
    assert all(len(s) for s in sels) and max(len(s) for s in sels) == 500
    pl.subtree_attach()
    want = []
    for s in sels:
        w = pl.subtree_nodes(s)
        w["info"] = {k: int(w["info"][k]) for k in ("n_selected", "n_gathered", "n_disagree", "longest_chain", "first_disagree")}
        want.append(w)
    got = pl.subtree_batch(sels)
    windows = sorted(int(F.dend[F.pre[int(g["info"]["lca"])]]) - int(F.pre[int(g["info"]["lca"])]) for g in got)
    small = windows[len(windows) // 4]
    several = pl.subtree_batch(sels, group_positions=8 * small)   # a quarter of the windows fit eight to a group, the large ones run alone
    assert windows[-1] > 8 * small
    for i in range(256):
        assert R.same(got[i], want[i]), i
        assert R.same(several[i], want[i]), i
        assert int(got[i]["info"]["lca"]) == int(got[i]["kept"][0])
    pl.close()
