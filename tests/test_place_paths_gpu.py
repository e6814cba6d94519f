"""Which path a placement call takes, at the smallest shapes where a decision of the plan (usher_amd/csrc/ugp_plan.hpp) flips: one
512-sample tile or two, sorted or not, third bound or not, packed or the forced 32-bit walk.  Results equal the literal oracle's on
every path; which path ran shows only in timing(), whose fields are compared with the rule restated here in a few lines of Python.
(A tree this small has fewer chunks than the packed rule wants units, so its group count ends at one group per chunk for every Q:
the doubling and its 4096-unit stop are pinned by tests/test_plan_cpu.py.)

UGP_BOUND3 is set explicitly in every case (the conftest pin is by a hash of the test's name)."""
import functools
import os

import numpy as np
import pytest

from oracle import capi
from tests import synth
from usher_amd import Placer, QueryBatch

pytestmark = pytest.mark.gpu

SIZES = (1, 512, 513, 1300)


def _env(monkeypatch, bound3, knobs=()):
    """Exactly these UGP_* variables: every other one is cleared."""
    for k in list(os.environ):
        if k.startswith("UGP_"):
            monkeypatch.delenv(k)
    monkeypatch.setenv("UGP_BOUND3", str(bound3))
    for k, v in dict(knobs).items():
        monkeypatch.setenv(k, str(v))


@functools.lru_cache(None)
def _case():
    """A ~600-node random tree and 1,300 queries with the oracle's (best, num_best, best_j, has_unique) for each."""
    arrays, queries = synth.make_case(83, n_leaves=400, n_queries=max(SIZES), n_sites=200, n_ambig=(0, 0, 2, 5))
    ot = capi.OracleTree(arrays)
    full = [ot.place(s) for s in queries]
    want = np.array([[w["best"], w["num_best"], w["best_j"], int(w["has_unique"])] for w in full], dtype=np.int64)
    return arrays, queries, want


def _rows(res):
    return np.stack([res["best_set_difference"].astype(np.int64), res["num_best"].astype(np.int64), res["best_j"].astype(np.int64),
                     res["best_has_unique"].astype(np.int64)], 1)


def _groups_packed(n_chunks, tiles512):
    """Units of 16 chunks, doubled in number until there are ~4096 of them or one per chunk."""
    g = max(1, -(-n_chunks // 16))
    while g < n_chunks and g * tiles512 < 4096:
        g = min(n_chunks, g * 2)
    return g


def _groups_lanes(n_chunks, tiles64):
    """~4096 waves: at most one group per chunk, from 8 on a multiple of 8."""
    g = max(1, min(-(-4096 // tiles64), n_chunks))
    return g & ~7 if g >= 8 else g


def _placer(monkeypatch, bound3, knobs=()):
    """A fresh handle under exactly these knobs; a coarse tree however small the tree is."""
    _env(monkeypatch, bound3, {"UGP_COARSE_MIN_NODES": 0, **dict(knobs)})
    pl = Placer(_case()[0], chunk_nodes=24)
    assert pl.info()["n_chunks"] >= 8
    return pl


@pytest.mark.parametrize("bound3", [1, 0])
@pytest.mark.parametrize("Q", SIZES)
def test_packed_path(Q, bound3, monkeypatch):
    _, queries, want = _case()
    placer = _placer(monkeypatch, bound3)
    try:
        n_chunks = placer.info()["n_chunks"]
        got = _rows(placer.place(QueryBatch(queries[:Q])))
        t = placer.timing()
    finally:
        placer.close()
    assert (got == want[:Q]).all(), np.flatnonzero((got != want[:Q]).any(1))[:8]
    tiles512 = -(-Q // 512)
    assert t["packed_path"] == 1 and t["place_launches"] == 1, t
    assert t["n_tiles"] == tiles512, t
    assert t["n_groups"] == _groups_packed(n_chunks, tiles512), (t, n_chunks)
    # the third bound runs for the sorted walk only: more than 512 samples
    assert t["bound3"] == (1 if bound3 == 1 and Q > 512 else 0), t


@pytest.mark.parametrize("Q", SIZES)
def test_forced_32_bit_path(Q, monkeypatch):
    _, queries, want = _case()
    placer = _placer(monkeypatch, 1, {"UGP_FORCE_V1": 1})
    try:
        n_chunks = placer.info()["n_chunks"]
        got = _rows(placer.place(QueryBatch(queries[:Q])))
        t = placer.timing()
    finally:
        placer.close()
    assert (got == want[:Q]).all(), np.flatnonzero((got != want[:Q]).any(1))[:8]
    tiles64 = -(-Q // 64)
    assert t["packed_path"] == 0 and t["place_launches"] == 1, t
    assert t["n_tiles"] == tiles64, t
    assert t["n_groups"] == _groups_lanes(n_chunks, tiles64), (t, n_chunks)
    assert t["bound3"] == 0, t
