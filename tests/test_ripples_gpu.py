"""ugp_ripples / Placer.ripples (RIPPLES, ripples/main.cpp:300-680) against the literal restatement through the oracle's
mapper2_body, on planted recombinants and random trees, over a grid of options."""
import numpy as np
import pytest

from oracle import capi
from tests import ripples_ref as RR
from tests import synth
from usher_amd import Placer

pytestmark = pytest.mark.gpu


def _device(pl, arrays, branches, **o):
    ev = pl.ripples(np.asarray(branches), RR.name_ranks(arrays), branch_len=o["l"], min_range=o["r"], max_range=o["R"],
                    parsimony_improvement=o["p"], num_descendants=o["n_desc"])
    return [{k: (bool(e[k]) if k.endswith("sibling") else int(e[k])) for k in RR.KEYS} for e in ev]


def _planted(seed, **kw):
    arrays = RR.planted(seed, **kw)
    return arrays, RR.node_named(arrays, "recomb_%d" % seed)


GRID = [dict(l=l, p=p, n_desc=nd, r=r, R=R) for l in (1, 3) for p in (0, 3) for nd in (1, 10) for (r, R) in ((1000, 10 ** 7),)] + \
       [dict(l=1, p=0, n_desc=1, r=200, R=3000), dict(l=3, p=3, n_desc=10, r=2000, R=9000)]


@pytest.mark.parametrize("seed", [0, 1])
def test_planted_grid(seed):
    arrays, X = _planted(seed, n_leaves=150, masked_rows=seed == 1)
    rng = np.random.default_rng(seed)
    par = np.asarray(arrays["parent"])
    br = [X, 0] + [int(v) for v in rng.choice(np.unique(par[1:]), 5, replace=False)]
    pl = Placer(arrays)
    ot = capi.OracleTree(arrays)
    seen = 0
    for o in GRID:
        want = RR.literal(arrays, br, ot, **o)
        assert _device(pl, arrays, br, **o) == want, o
        seen += len(want)
    assert seen > 0
    pl.close()


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_random_trees_and_masks(seed):
    rng = np.random.default_rng(900 + seed)
    arrays, _, _, _ = synth.random_tree(rng, 150, genome_len=4000, n_sites=160, mut_counts=(0, 1, 1, 2, 3, 4),
                                        p_masked=0.08, root_muts=2)
    arrays["names"] = ["s%03d_%d" % ((j * 37) % arrays["n"], j) for j in range(arrays["n"])]
    br = [int(v) for v in rng.choice(arrays["n"], 12, replace=False)] + [0]
    pl = Placer(arrays)
    for o in (dict(l=1, p=0, n_desc=1, r=0, R=10 ** 7), dict(l=2, p=1, n_desc=4, r=100, R=10 ** 7)):
        assert _device(pl, arrays, br, **o) == RR.literal(arrays, br, **o), o
    pl.close()


def test_sample_file_style_branches_and_edge_cases():
    """A root path with the root itself (-s), branches with M < 2l, with orig < p, and no candidate at all."""
    arrays, X = _planted(2, n_leaves=120, masked_rows=True)
    par = np.asarray(arrays["parent"])
    path = [X]
    while par[path[-1]] >= 0:
        path.append(int(par[path[-1]]))
    off = np.diff(arrays["mut_off"])
    short = [k for k in range(1, arrays["n"]) if 0 < off[k] < 3][:3]
    br = path + short
    pl = Placer(arrays)
    o = dict(l=3, p=3, n_desc=10, r=1000, R=10 ** 7)
    want = RR.literal(arrays, br, **o)
    assert want and _device(pl, arrays, br, **o) == want
    assert _device(pl, arrays, br, **dict(o, n_desc=arrays["n"] + 1)) == []
    assert _device(pl, arrays, br, **dict(o, l=400)) == []
    pl.close()


def test_split_into_calls_does_not_matter():
    arrays, X = _planted(6, n_leaves=160)
    br = [X] + RR.default_branches(arrays)
    pl = Placer(arrays)
    o = dict(l=3, p=3, n_desc=10, r=1000, R=10 ** 7)
    whole = _device(pl, arrays, br, **o)
    parts = []
    for s in range(0, len(br), 3):
        for e in _device(pl, arrays, br[s:s + 3], **o):
            e["branch"] += s
            parts.append(e)
    assert whole == parts and whole == RR.literal(arrays, br, **o)
    pl.close()
