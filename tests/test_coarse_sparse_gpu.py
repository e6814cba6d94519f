"""The locality pre-pass from the samples' own rows (k_coarse_sparse, usher_amd/csrc/ugp_coarse.hip) against the walked pre-pass and
the oracles, on the ~600-node tree of tests/test_place_paths_gpu.py: the hook ugp_debug_coarse_pass runs only the pre-pass of an
uploaded batch by the method named; both methods must name the same node at the same cost per sample, and that cost must be the
closed form's best on the coarse tree's own arrays, at a node whose eligible cost it is.  Through place() the answers equal the
literal oracle's whichever pre-pass ran.  Which one a call takes shows in the hook: it refuses "sparse" where the plan does."""
import functools
import os

import numpy as np
import pytest

from oracle import capi
from oracle.closed_form import ClosedFormTree
from tests import synth
from usher_amd import Placer, QueryBatch
from usher_amd.placement import UgpError

pytestmark = pytest.mark.gpu

CAP_EVENTS = 512   # kCoarseSparseMaxEvents (ugp_coarse.hpp)


def _env(monkeypatch, knobs=()):
    for k in list(os.environ):
        if k.startswith("UGP_"):
            monkeypatch.delenv(k)
    monkeypatch.setenv("UGP_BOUND3", "1")
    monkeypatch.setenv("UGP_COARSE_MIN_NODES", "0")
    for k, v in dict(knobs).items():
        monkeypatch.setenv(k, str(v))


@functools.lru_cache(None)
def _case(kind="plain"):
    kw = dict(p_masked=0.04, root_muts=2) if kind == "masked" else {}
    arrays, queries = synth.make_case(83, n_leaves=400, n_queries=1300, n_sites=200, n_ambig=(0, 0, 2, 5), **kw)
    ot = capi.OracleTree(arrays)
    want = np.array([[w["best"], w["num_best"], w["best_j"], int(w["has_unique"])] for w in (ot.place(s) for s in queries)], dtype=np.int64)
    return arrays, queries, want


def _rows(res):
    return np.stack([res["best_set_difference"].astype(np.int64), res["num_best"].astype(np.int64), res["best_j"].astype(np.int64),
                     res["best_has_unique"].astype(np.int64)], 1)


def _coarse_arrays(arrays, kept):
    """The coarse tree (the kept nodes, ascending BFS index; a kept node's parent is kept) as arrays of its own."""
    kept = kept.astype(np.int64)
    idx = {int(j): k for k, j in enumerate(kept)}
    off, sel = [0], []
    for j in kept:
        sel.extend(range(int(arrays["mut_off"][j]), int(arrays["mut_off"][j + 1])))
        off.append(len(sel))
    sel = np.array(sel, dtype=np.int64)
    return {"n": len(kept), "parent": np.array([-1 if j == 0 else idx[int(arrays["parent"][j])] for j in kept], dtype=np.int32),
            "mut_off": np.array(off, dtype=np.uint64), "mut_pos": np.asarray(arrays["mut_pos"])[sel], "mut_ref": np.asarray(arrays["mut_ref"])[sel],
            "mut_nuc": np.asarray(arrays["mut_nuc"])[sel]}


def _max_per_pos(coarse):
    p = np.asarray(coarse["mut_pos"])
    p = p[p >= 0]
    return int(np.bincount(p).max()) if len(p) else 0


def _check_prepass(pl, arrays, queries):
    """Sparse == walked, node for node and cost for cost; both the closed form's best on the coarse arrays."""
    qs = pl.upload(QueryBatch(queries))
    try:
        cw, nw, kept = pl.coarse_pass(qs, "walked")
        cs, ns, kept2 = pl.coarse_pass(qs, "sparse")
    finally:
        pl.free_qset(qs)
    assert kept.tolist() == kept2.tolist() and kept[0] == 0
    assert (cs == cw).all(), np.flatnonzero(cs != cw)[:8]
    assert (ns == nw).all(), (np.flatnonzero(ns != nw)[:8], ns[ns != nw][:8], nw[ns != nw][:8])
    cf = ClosedFormTree(_coarse_arrays(arrays, kept))
    for i, s in enumerate(queries):
        w = cf.place(s, compute_scores=True)
        assert cs[i] == w["best"] and w["scores"][ns[i]] == w["best"], (i, cs[i], ns[i], w["best"])
    return kept


@pytest.mark.parametrize("Q", [513, 1300])
def test_sparse_equals_walked_and_the_oracle(Q, monkeypatch):
    arrays, queries, _ = _case()
    _env(monkeypatch)
    pl = Placer(arrays, chunk_nodes=24)
    try:
        kept = _check_prepass(pl, arrays, queries[:Q])
        assert 64 <= len(kept) < int(arrays["n"])
    finally:
        pl.close()


@pytest.mark.parametrize("phase2", [0, 1])
@pytest.mark.parametrize("Q", [513, 1300])
def test_place_equals_the_oracle_with_either_prepass(Q, phase2, monkeypatch):
    arrays, queries, want = _case()
    _env(monkeypatch, {"UGP_COARSE_PHASE2": 1} if phase2 else {})
    pl = Placer(arrays, chunk_nodes=24)
    try:
        got = _rows(pl.place(QueryBatch(queries[:Q])))
        t = pl.timing()
        assert pl.last_prepass() == ("walked" if phase2 else "sparse")
        qs = pl.upload(QueryBatch(queries[:Q]))
        try:
            if phase2:   # the knob keeps the walked pass: the hook refuses the sparse one
                with pytest.raises(UgpError):
                    pl.coarse_pass(qs, "sparse")
            else:
                pl.coarse_pass(qs, "sparse")
        finally:
            pl.free_qset(qs)
    finally:
        pl.close()
    assert (got == want[:Q]).all(), np.flatnonzero((got != want[:Q]).any(1))[:8]
    assert t["packed_path"] == 1 and t["coarse_ms"] > 0, t


def test_masked_and_root_mutations(monkeypatch):
    arrays, queries, want = _case("masked")
    assert int(arrays["mut_off"][1]) >= 2 and (np.asarray(arrays["mut_pos"]) < 0).any()
    _env(monkeypatch)
    pl = Placer(arrays, chunk_nodes=24)
    try:
        kept = _check_prepass(pl, arrays, queries[:513])
        coarse = _coarse_arrays(arrays, kept)
        assert (np.asarray(coarse["mut_pos"]) < 0).any()   # (the coarse tree has masked mutations of its own)
        got = _rows(pl.place(QueryBatch(queries[:513])))
    finally:
        pl.close()
    assert (got == want[:513]).all(), np.flatnonzero((got != want[:513]).any(1))[:8]


def _long_sample(arrays, coarse, n_rows, rng):
    """A sample of n_rows rows: every position of the coarse tree first (so that its events are many), then positions the tree
    does not have; alleles at random, the reference base as the tree has it."""
    tp = np.asarray(arrays["mut_pos"]); tr = np.asarray(arrays["mut_ref"])
    ref_at = {int(p): int(r) for p, r in zip(tp, tr) if p >= 0}
    cpos = sorted({int(p) for p in np.asarray(coarse["mut_pos"]) if p >= 0})
    free = [p for p in range(1, 2000) if p not in ref_at]
    pos = sorted((cpos + free)[:n_rows])
    assert len(pos) == n_rows
    return {"name": "long", "pos": np.array(pos, dtype=np.int32), "ref": np.array([ref_at.get(p, 1) for p in pos], dtype=np.uint8),
            "nuc": np.array([int(rng.choice([1, 2, 4, 8, 3, 12])) for _ in pos], dtype=np.uint8), "is_missing": np.zeros(n_rows, dtype=np.uint8)}


def test_capacity_edge(monkeypatch):
    """max_rows x (events per position) exactly at the capacity takes the sparse pass, one row more the walked one: the hook refuses
    "sparse" for the second set.  Results equal the oracle either way."""
    arrays, queries, want = _case()
    _env(monkeypatch)
    pl = Placer(arrays, chunk_nodes=24)
    try:
        qs = pl.upload(QueryBatch(queries[:4]))
        _, _, kept = pl.coarse_pass(qs, "walked")
        pl.free_qset(qs)
        coarse = _coarse_arrays(arrays, kept)
        mpp = _max_per_pos(coarse)
        assert mpp >= 2
        rows_at = CAP_EVENTS // mpp   # the largest max_rows the rule admits
        ot = capi.OracleTree(arrays)
        rng = np.random.default_rng(5)
        for n_rows, sparse in ((rows_at, True), (rows_at + 1, False)):
            qq = [_long_sample(arrays, coarse, n_rows, rng)] + list(queries[1:513])
            assert max(len(s["pos"]) for s in qq) == n_rows
            if sparse:
                _check_prepass(pl, arrays, qq)
            else:
                qs = pl.upload(QueryBatch(qq))
                try:
                    with pytest.raises(UgpError):
                        pl.coarse_pass(qs, "sparse")
                finally:
                    pl.free_qset(qs)
            got = _rows(pl.place(QueryBatch(qq)))
            assert pl.last_prepass() == ("sparse" if sparse else "walked")
            w = ot.place(qq[0])
            assert got[0].tolist() == [w["best"], w["num_best"], w["best_j"], int(w["has_unique"])], (n_rows, got[0], w)
            assert (got[1:] == want[1:513]).all(), n_rows
    finally:
        pl.close()


def test_unsorted_rows_get_the_same_error(monkeypatch):
    arrays, queries, want = _case()
    good = QueryBatch(queries[:513])
    smp = int(np.flatnonzero(np.diff(good.ent_off.astype(np.int64)) >= 3)[5])
    e0 = int(good.ent_off[smp])
    pos = good.pos.copy()
    pos[e0], pos[e0 + 1] = pos[e0 + 1], pos[e0]
    ref, nuc, mis = good.ref.copy(), good.nuc.copy(), good.is_missing.copy()
    for a in (ref, nuc, mis):
        a[e0], a[e0 + 1] = a[e0 + 1], a[e0]
    bad = QueryBatch.from_csr(good.ent_off.copy(), pos, ref, nuc, mis)
    seen = []
    for knobs in ({}, {"UGP_COARSE_PHASE2": 1}):
        _env(monkeypatch, knobs)
        pl = Placer(arrays, chunk_nodes=24)
        try:
            with pytest.raises(UgpError) as e1:
                pl.place(bad)
            j = pl.place_async(bad)        # (the whole chain is queued before the row check's verdict is read)
            with pytest.raises(UgpError) as e2:
                pl.job_wait(j)
            seen.append((e1.value.code, str(e1.value), e2.value.code, str(e2.value)))
            assert (_rows(pl.place(good)) == want[:513]).all()
        finally:
            pl.close()
    assert seen[0] == seen[1], seen
    assert seen[0][0] == -2 and seen[0][2] == -2, seen


def test_after_an_update_and_under_a_node_mask_the_walked_pass_serves(monkeypatch):
    from tests import touched_cases as TC
    arrays, queries, want = _case()
    n = int(arrays["n"])
    qq = queries[:513]
    _env(monkeypatch)
    ot = capi.OracleTree(arrays)
    pl = Placer(arrays, chunk_nodes=24)
    try:
        batch = QueryBatch(qq)
        qs = pl.upload(batch)
        _, _, kept = pl.coarse_pass(qs, "sparse")
        # under a node mask: the call equals the oracle over the admitted nodes, and the handle is as it was behind it
        mask = np.ones(n, np.uint8)
        mask[kept[1::3]] = 0              # every third node of the coarse tree (never the root) is no candidate
        allowed = np.flatnonzero(mask).astype(np.int64)
        res = pl.place_ex(batch, order="bfs", node_mask=mask)
        assert pl.timing()["packed_path"] == 1 and pl.last_prepass() == "walked"
        for i in range(0, len(qq), 7):
            w = ot.place_list(qq[i], allowed, jidx=allowed)
            assert (int(res["best_set_difference"][i]), int(res["num_best"][i]), int(res["best_j"][i])) == (w["best"], w["num_best"], w["best_j"]), i
        pl.coarse_pass(qs, "sparse")      # (no mask in force any more)
        assert (_rows(pl.place(batch)) == want[:513]).all() and pl.last_prepass() == "sparse"
        # after one ugp_mat_update that takes a node of the coarse tree out: the sparse pass is refused, the answers are the oracle's
        T, flat_nodes = TC.tree_from_arrays(arrays)
        victim = int(kept[1])
        assert pl.update([TC.record_of(flat_nodes[victim], victim)], []) == 0
        with pytest.raises(UgpError):
            pl.coarse_pass(qs, "sparse")
        pl.free_qset(qs)
        res = pl.place(batch)
        assert pl.last_prepass() == "walked"
        allowed = np.array([j for j in range(n) if j != victim], np.int64)
        for i, s in enumerate(qq):
            w = ot.place_list(s, allowed, jidx=allowed)
            assert (int(res["best_set_difference"][i]), int(res["num_best"][i])) == (w["best"], w["num_best"]), i
            assert int(res["best_j"][i]) != victim
    finally:
        pl.close()


def _no_rows(n):
    return [{"name": "E%d" % i, "pos": np.zeros(0, np.int32), "ref": np.zeros(0, np.uint8), "nuc": np.zeros(0, np.uint8),
             "is_missing": np.zeros(0, np.uint8)} for i in range(n)]


def test_a_batch_without_any_row(monkeypatch):
    """513 samples equal to the reference: the set has no row arrays on the device (a fresh one) or still holds those of the batch
    before it (the handle's own reused set).  Through the hook and through place(), before and after a batch with rows."""
    arrays, queries, want = _case()
    empty = _no_rows(513)
    ot = capi.OracleTree(arrays)
    w = ot.place(empty[0])
    want_empty = np.array([[w["best"], w["num_best"], w["best_j"], int(w["has_unique"])]] * 513, dtype=np.int64)
    _env(monkeypatch)
    pl = Placer(arrays, chunk_nodes=24)
    try:
        _check_prepass(pl, arrays, empty)                                 # a fresh set, the hook
        got = _rows(pl.place(QueryBatch(empty)))                          # the handle's own set, never filled before
        assert pl.last_prepass() == "sparse" and (got == want_empty).all()
        assert (_rows(pl.place(QueryBatch(queries[:1300]))) == want).all()
        got = _rows(pl.place(QueryBatch(empty)))                          # the same set again: it still holds 1,300 samples' rows
        assert pl.last_prepass() == "sparse" and (got == want_empty).all(), np.flatnonzero((got != want_empty).any(1))[:8]
        j1 = pl.place_async(QueryBatch(queries[:513])); j2 = pl.place_async(QueryBatch(empty)); j3 = pl.place_async(QueryBatch(empty))
        assert (_rows(pl.job_wait(j1)) == want[:513]).all()
        assert (_rows(pl.job_wait(j2)) == want_empty).all() and (_rows(pl.job_wait(j3)) == want_empty).all()
        _check_prepass(pl, arrays, empty)
    finally:
        pl.close()
