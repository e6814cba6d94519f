"""ugp_uncertainty on the 10M-node synthetic MAT (bench.py's tree): a few thousand leaves in one call, a handful of them
checked against the oracle's literal search (each is a full pass over 10M nodes on the host)."""
import numpy as np
import pytest

from oracle import capi
from tests import uncertainty_ref as U
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_uncertainty_at_10m_nodes():
    st = gsynth.SynthTree(10_000_000, n_sites=25000, seed=1)
    arrays = st.arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"])
    has_kids = np.zeros(n, bool)
    has_kids[par[1:]] = True
    leaves = np.flatnonzero(~has_kids)
    rng = np.random.default_rng(17)
    nodes = rng.choice(leaves, 2048, replace=False)
    pl = Placer(arrays)
    epps, nsize, ties, cnt = pl.uncertainty(nodes, cap=256)
    assert (epps == cnt).all() and (epps >= 1).all()
    dfs = pl.node_order("dfs").astype(np.int64)
    ot = capi.OracleTree(arrays)
    check = list(rng.choice(len(nodes), 3, replace=False)) + [int(np.argmax(epps))]
    for i in check:
        j = int(nodes[i])
        nb, tl = U.search(ot, arrays, dfs, j, U.literal_sample(arrays, j))
        ns = U.neighborhood_closed(arrays, [int(dfs[t]) for t in tl]) if nb > 1 else 0
        assert (int(epps[i]), int(nsize[i]), ties[i].tolist()) == (nb, ns, tl[:256]), (j, int(epps[i]), nb)
    pl.close()
