"""ugp_ripples on the paths only large inputs reach: several candidate chunks per branch folded into one slab, the slab-row
clamp and one-candidate LDS tiles (forced on small trees with UGP_RIPPLES_LIMITS and checked against the literal search),
and a 1M-node tree (the same events with and without those limits; the chosen nodes' counts and scores against the oracle's
literal mapper2_body)."""
import numpy as np
import pytest

from oracle import capi
from tests import ripples_ref as RR
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu

SMALL = "4096,4096,64"   # count bytes, slab bytes, LDS ints: many chunks, one slab row, tiles of one candidate


def _events(pl, br, rank, **o):
    return pl.ripples(np.asarray(br), rank, branch_len=o["l"], min_range=o["r"], max_range=o["R"],
                      parsimony_improvement=o["p"], num_descendants=o["n_desc"])


def _dicts(ev):
    return [{k: (bool(e[k]) if k.endswith("sibling") else int(e[k])) for k in RR.KEYS} for e in ev]


@pytest.mark.parametrize("seed", [21, 22])
def test_forced_small_limits_equal_literal(seed, monkeypatch):
    arrays = RR.planted(seed, n_leaves=180, masked_rows=seed == 22)
    X = RR.node_named(arrays, "recomb_%d" % seed)
    br = [X, 0] + RR.default_branches(arrays)[:6]
    pl = Placer(arrays)
    rank = RR.name_ranks(arrays)
    for o in (dict(l=3, r=1000, R=10 ** 7, p=3, n_desc=10), dict(l=1, r=0, R=10 ** 7, p=0, n_desc=1)):
        want = RR.literal(arrays, br, **o)
        monkeypatch.setenv("UGP_RIPPLES_LIMITS", SMALL)
        assert _dicts(_events(pl, br, rank, **o)) == want, o
        monkeypatch.delenv("UGP_RIPPLES_LIMITS")
        assert _dicts(_events(pl, br, rank, **o)) == want, o
        assert want
    pl.close()


def test_one_million_nodes(monkeypatch):
    arrays = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3).arrays
    n = arrays["n"]
    par = np.asarray(arrays["parent"]).astype(np.int64)
    nmut = np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))
    rng = np.random.default_rng(3)
    inner = np.unique(par[1:])
    br = [int(v) for v in rng.choice(inner[nmut[inner] >= 2], 6, replace=False)]
    rank = np.arange(n, dtype=np.uint32)
    pl = Placer(arrays)
    o = dict(l=1, r=0, R=10 ** 7, p=0, n_desc=4)
    ev = _events(pl, br, rank, **o)
    monkeypatch.setenv("UGP_RIPPLES_LIMITS", "%d,%d,%d" % (1 << 22, 1 << 16, 12288))
    again = _events(pl, br, rank, **o)
    monkeypatch.delenv("UGP_RIPPLES_LIMITS")
    assert len(ev) > 0 and ev.tobytes() == again.tobytes()
    # the chosen nodes of a sample of events: counts and pass-1 scores from the oracle's literal mapper2_body
    ot = capi.OracleTree(arrays)
    for e in ev[rng.choice(len(ev), min(6, len(ev)), replace=False)]:
        nid = br[int(e["branch"])]
        rows = RR.pruned_sample(arrays, nid)
        pos = [x[0] for x in rows]
        sample = RR.as_sample(rows)
        sh, el = pos[int(e["i"])], pos[int(e["j"]) - 1]
        for node, cnt, score, donor in ((int(e["donor"]), int(e["donor_count"]), int(e["donor_score"]), True),
                                        (int(e["acceptor"]), int(e["acceptor_count"]), int(e["acceptor_score"]), False)):
            v = ot.node_vecs(sample, node)
            own = RR._muts(arrays, node)
            u = [ep for (ep, _, _, em) in v["excess"] if not (ep >= 0 and any(op == ep and om == em for (op, _, om) in own))]
            nin = sum(1 for x in u if sh <= x <= el)
            assert cnt == (nin if donor else len(u) - nin)
            assert score == v["set_difference"]
    pl.close()
