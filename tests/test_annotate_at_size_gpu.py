"""Annotate's device calls on a 1M-node synthetic MAT with a few hundred clades whose exemplars lie below chosen roots: allele
counts against the literal exemplar walk, descendant counts against a numpy range count over the depth-first order, and the
literal search (rows with repeated and masked positions) against the oracle's serial mapper2_body."""
import numpy as np
import pytest

from oracle import capi
from tests import annotate_ref as A
from tools import bench_annotate as B
from usher_amd import Placer, QueryBatch
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_annotate_at_size():
    arrays = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3).arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"], np.int64)
    sz = B.subtree_sizes(np.maximum(par, 0))
    pl = Placer(arrays)
    dfs = pl.node_order("dfs").astype(np.int64)
    pre = np.empty(n, np.int64); pre[dfs] = np.arange(n)
    rng = np.random.default_rng(11)
    roots = rng.choice(np.flatnonzero((sz >= 200) & (sz <= 5000)), 300, replace=False)
    clades = [dfs[pre[r] + rng.integers(0, sz[r], 60)] for r in roots]
    alle = pl.clade_alleles(clades)
    for c in rng.choice(len(clades), 12, replace=False):
        assert dict(zip(alle[c][0].tolist(), alle[c][1].tolist())) == A.alleles_literal(arrays, clades[c]), c
    pc = rng.integers(0, len(clades), 5000)
    pn = np.where(rng.random(5000) < 0.5, roots[pc], rng.integers(0, n, 5000))
    got = pl.clade_descendants(clades, pc, pn)
    want = [int(((pre[clades[c]] > pre[v]) & (pre[clades[c]] < pre[v] + sz[v])).sum()) for c, v in zip(pc, pn)]
    assert got.tolist() == want
    # the literal search on awkward rows built from the clades' counts
    ot = capi.OracleTree(arrays)
    rows = []
    for c in range(len(clades)):
        r = B.rows_of(arrays, alle[c][0], alle[c][1], len(clades[c]), min_freq=0.6, mask_freq=0.05)
        if len(r["pos"]):
            k = len(r["pos"]) // 2
            for key in r:
                r[key] = np.concatenate([r[key][:k + 1], r[key][k:]])   # a repeated position
            r["nuc"][k] = 15
            rows.append(r)
        if len(rows) == 2:
            break
    best, ties, cnt = pl.annotate_search(QueryBatch(rows), cap=4096)
    for i, r in enumerate(rows):
        assert A.awkward(r)
        wb, wt = A.search(ot, arrays, r, dfs)
        assert (int(best[i]), ties[i].tolist(), int(cnt[i])) == (wb, wt[:4096], len(wt))
    pl.close()
