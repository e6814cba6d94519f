"""Every knob of tests/knob_table.py marked "grid", against the oracle: each sample's (best, num_best, best_j, has_unique)
equals the literal oracle's (small trees) or the C closed form's (trees of 0.3-1M nodes), whatever value the knob has.  Where the
library reports which path ran (timing(): n_groups, bound3, place_launches; pipeline_depth()), that is asserted too.

UGP_BOUND3 is set explicitly in every case (the conftest pin is by a hash of the test's name).  Knobs read when a tree is
flattened or uploaded get a fresh Placer, the others ugp_mat_reload_knobs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import capi
from tests import synth
from usher_amd import Placer, QueryBatch, UgpError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(monkeypatch, bound3, knobs=()):
    """Exactly these UGP_* variables: every other one is cleared."""
    for k in list(os.environ):
        if k.startswith("UGP_"):
            monkeypatch.delenv(k)
    monkeypatch.setenv("UGP_BOUND3", str(bound3))
    for k, v in dict(knobs).items():
        monkeypatch.setenv(k, str(v))


def _rows(res):
    return np.stack([res["best_set_difference"].astype(np.int64), res["num_best"].astype(np.int64), res["best_j"].astype(np.int64),
                     res["best_has_unique"].astype(np.int64)], 1)


def _check(res, want, label):
    got = _rows(res)
    assert got.shape == want.shape, label
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), (label, "%d samples differ, e.g." % len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:4]])


@functools.lru_cache(None)
def _case(name):
    """(arrays, queries, oracle results with ties, oracle rows)
    A: ~9,000-node random tree, 1,300 queries (a partial last 512-sample tile); D: the same tree, >= 128 rows per sample, ~90 N cells;
    B: polytomies (fanouts 30 / 50 / 20: the wide-descent shape)."""
    if name == "A":
        arrays, queries = synth.make_case(71, n_leaves=6000, n_queries=1300, n_sites=500, n_ambig=(0, 0, 2, 5, 30))
    elif name == "D":
        arrays, queries = synth.make_case(71, n_leaves=6000, n_queries=1300, n_sites=500, n_ambig=(260, 300))
        assert min(len(s["pos"]) for s in queries) >= 128 and sum(int(s["is_missing"].sum()) for s in queries) > 50 * len(queries)
    elif name == "B":
        arrays, queries = synth.polytomy_case(47, fanouts=(30, 50, 20), n_queries=900)
    ot = capi.OracleTree(arrays)
    full = [ot.place(s) for s in queries]
    want = np.array([[w["best"], w["num_best"], w["best_j"], int(w["has_unique"])] for w in full], dtype=np.int64)
    return arrays, queries, full, want


def _place_grid(monkeypatch, pl, batch, want, base, grid, label, bound3s=(0, 1)):
    for knobs in grid:
        for b3 in bound3s:
            _env(monkeypatch, b3, {**base, **knobs})
            pl.reload_knobs()
            _check(pl.place(batch), want, (label, knobs, b3))


# ---- seeds ---------------------------------------------------------------------------------------------------------------------

SEED_GRID = ({}, {"UGP_LIGHT_ORDER": 0}, {"UGP_LIGHT_ORDER": 1},
             {"UGP_DESCENT_MAX": 1}, {"UGP_DESCENT_MAX": 2}, {"UGP_DESCENT_MAX": 4096},
             {"UGP_DESCENT_SLACK": 0}, {"UGP_DESCENT_SLACK": 1}, {"UGP_DESCENT_SLACK": 40},
             {"UGP_DESCENT_MAX": 1, "UGP_DESCENT_SLACK": 0}, {"UGP_DESCENT_MAX": 4096, "UGP_DESCENT_SLACK": 40, "UGP_LIGHT_ORDER": 1})


@pytest.mark.parametrize("case", ["A", "B"])
def test_seed_descent_lanes_depth_slack_and_light_order(case, monkeypatch):
    """Both descent kernels (k_descend<16> / <64>) on both tree shapes, truncated and widened descents (their costs are the upper
    bounds the pruning trusts), and both light-unit orders of k_build_units."""
    arrays, queries, _, want = _case(case)
    batch = QueryBatch(queries)
    for lanes in (16, 64):
        base = {"UGP_COARSE_MIN_NODES": 0, "UGP_DESCENT_LANES": lanes}
        _env(monkeypatch, 1, base)
        pl = Placer(arrays, chunk_nodes=300)       # (the lane count is read when the tree is uploaded)
        _place_grid(monkeypatch, pl, batch, want, base, SEED_GRID, (case, lanes))
        pl.close()


def test_no_pad_fix_on_full_and_partial_tiles(monkeypatch):
    arrays, queries, _, want = _case("A")
    base = {"UGP_COARSE_MIN_NODES": 0, "UGP_NO_PAD_FIX": 1}
    _env(monkeypatch, 1, base)
    pl = Placer(arrays, chunk_nodes=300)
    for n in (1, 513, 1300):
        _place_grid(monkeypatch, pl, QueryBatch(queries[:n]), want[:n], base, ({},), ("n", n))
    pl.close()


# ---- tile builders -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["A", "D"])
@pytest.mark.parametrize("no_sort", [False, True])
def test_tile_builders_sorted_and_unsorted(case, no_sort, monkeypatch):
    """UGP_TILE_BUILD 0 / 1 (the scatter builder and the LDS builder) on sorted and unsorted batches of few and of many rows per
    sample, with and without the N-mask tiles, each with the third bound pinned off and on.  The LDS builder has no third bound."""
    arrays, queries, _, want = _case(case)
    batch = QueryBatch(queries)
    base = {"UGP_COARSE_MIN_NODES": 0}
    if no_sort:
        base["UGP_NO_SORT"] = 1
    _env(monkeypatch, 0, base)
    pl = Placer(arrays, chunk_nodes=300)
    for tile_build in (0, 1):
        for nmask in (None, 1):
            for b3 in (0, 1):
                knobs = dict(base, UGP_TILE_BUILD=tile_build)
                if nmask is not None:
                    knobs["UGP_NMASK"] = nmask
                _env(monkeypatch, b3, knobs)
                pl.reload_knobs()
                label = (case, knobs, b3)
                _check(pl.place(batch), want, label)
                t = pl.timing()
                assert t["packed_path"] == 1, label
                if tile_build == 1 or b3 == 0 or no_sort:
                    assert t["bound3"] == 0, label
                else:
                    assert t["bound3"] == 1, label
    pl.close()


# ---- walk scheduling -----------------------------------------------------------------------------------------------------------

WALK_GRID = ({"UGP_GROUPS": 1}, {"UGP_GROUPS": 3}, {"UGP_GROUPS": 1 << 20},
             {"UGP_TARGET_WAVES": 1}, {"UGP_TARGET_WAVES": 7}, {"UGP_WAVES_PER_CU": 1}, {"UGP_WAVES_PER_CU": 2},
             {"UGP_HEAVY_PRIO": 1}, {"UGP_SPLIT_HEAVY": 0}, {"UGP_SPLIT_HEAVY": 1},
             {"UGP_SPLIT_DENSE": 0}, {"UGP_SPLIT_DENSE": 1}, {"UGP_SPLIT_DENSE": 100000}, {"UGP_REFILL_ALL": 1},
             {"UGP_FORK": 1}, {"UGP_FORK": 1, "UGP_NO_FORK": 1},
             {"UGP_WAVES_PER_CU": 1, "UGP_HEAVY_PRIO": 1, "UGP_SPLIT_DENSE": 1, "UGP_REFILL_ALL": 1, "UGP_GROUPS": 3})


@pytest.mark.parametrize("case", ["A", "B"])
def test_walk_scheduling_with_units_cut_at_every_restart(case, monkeypatch):
    arrays, queries, _, want = _case(case)
    batch = QueryBatch(queries)
    base = {"UGP_COARSE_MIN_NODES": 0, "UGP_SPLIT_CYCLES": 1}
    _env(monkeypatch, 0, base)
    pl = Placer(arrays, chunk_nodes=300 if case == "A" else 40)
    n_chunks = pl.info()["n_chunks"]
    assert n_chunks > 3
    for knobs in WALK_GRID:
        for b3 in (0, 1):
            _env(monkeypatch, b3, {**base, **knobs})
            pl.reload_knobs()
            _check(pl.place(batch), want, (case, knobs, b3))
            if "UGP_GROUPS" in knobs:
                assert pl.timing()["n_groups"] == min(n_chunks, knobs["UGP_GROUPS"]), (knobs, pl.timing())
    pl.close()


# ---- per-node scores -----------------------------------------------------------------------------------------------------------

def test_per_node_scores_at_every_block_size(monkeypatch):
    """k_scores_level at block sizes 64..1024 (values round down to a multiple of 64 and clamp): a level wider than 1,024 nodes,
    levels narrower than 64, branches of more than 15 mutations, 70 samples (no multiple of 32)."""
    arrays, queries = synth.make_case(65, n_leaves=6000, n_queries=70, n_sites=150, p_masked=0.04, root_muts=1,
                                      mut_counts=(0, 0, 1, 1, 1, 2, 3, 17, 40), n_ambig=(0, 0, 2, 5, 30))
    par = np.asarray(arrays["parent"])
    depth = np.zeros(arrays["n"], np.int64)
    for j in range(1, arrays["n"]):
        depth[j] = depth[par[j]] + 1
    widths = np.bincount(depth)
    assert widths.max() > 1024 and widths.min() < 64 and np.diff(arrays["mut_off"]).max() > 15
    ot = capi.OracleTree(arrays)
    want = np.stack([ot.place(s, compute_scores=True)["scores"] for s in queries])
    batch = QueryBatch(queries)
    _env(monkeypatch, 0)
    pl = Placer(arrays, chunk_nodes=40)
    for block in (None, 10, 64, 100, 128, 1000, 1024, 5000):
        _env(monkeypatch, 0, {} if block is None else {"UGP_SCORES_BLOCK": block})
        pl.reload_knobs()
        got = pl.scores_per_node(batch)
        assert got.shape == want.shape and (got == want).all(), (block, np.argwhere(got != want)[:5])
    pl.close()


# ---- sub-batches ---------------------------------------------------------------------------------------------------------------

def test_sub_batches_of_a_few_tiles_on_a_tree_of_many_chunks(monkeypatch):
    """UGP_LBEST_GIB=1 on a 1M-node tree of ~250,000 chunks: a sub-batch holds 32 tiles or fewer, so a 5,000-sample call runs as
    three sub-batches and more, the last one partial.  Placements against the closed form, tie lists against the same handle
    in one sub-batch."""
    from usher_amd import synth as gsynth
    st = gsynth.SynthTree(1_000_000, n_sites=8000, seed=5)
    q = st.queries(5000, seed=12, max_subst=3, n_lo=0, n_hi=20, iupac_hi=3)
    batch = QueryBatch.from_csr(q["ent_off"], q["pos"], q["ref"], q["nuc"], q["is_missing"])
    cf = capi.ClosedFormC(capi.OracleTree(st.arrays)).place_csr(q["ent_off"], q["pos"], q["ref"], q["nuc"], q["is_missing"])
    want = np.stack([cf["best"], cf["num_best"], cf["best_j"], cf["has_unique"]], 1).astype(np.int64)
    _env(monkeypatch, 0)
    pl = Placer(st.arrays, chunk_nodes=4)
    n_chunks = pl.info()["n_chunks"]
    sub_tiles = max(8, (1 << 30) // (n_chunks * 128)) & ~7
    n_sub = -(-len(batch) // (sub_tiles * 64))
    assert sub_tiles <= 64 and n_sub >= 3 and len(batch) % (sub_tiles * 64), (n_chunks, sub_tiles)
    whole = pl.place(batch)
    assert pl.timing()["place_launches"] == 1
    _check(whole, want, "one sub-batch")
    ties0, hu0, tc0 = pl.tied_nodes(batch, 4096)
    assert (tc0.astype(np.int64) == want[:, 1]).all() and int(tc0.max()) <= 4096 and int((tc0 > 16).sum()) > 0
    full0 = [dict(zip(t.tolist(), h.tolist())) for t, h in zip(ties0, hu0)]
    for b3 in (0, 1):
        _env(monkeypatch, b3, {"UGP_LBEST_GIB": 1})
        pl.reload_knobs()
        _check(pl.place(batch), want, ("UGP_LBEST_GIB=1", b3))
        assert pl.timing()["place_launches"] == n_sub
        ties, hu, tc = pl.tied_nodes(batch, 4096)
        assert (tc == tc0).all()
        for i in range(len(batch)):
            assert ties[i].tolist() == ties0[i].tolist() and hu[i].tolist() == hu0[i].tolist(), (b3, i)
        ties, hu, tc = pl.tied_nodes(batch, 16)      # (a cap below the count: the true count, `cap` of the tied nodes)
        assert (tc == tc0).all()
        for i in range(len(batch)):
            assert len(ties[i]) == min(16, int(tc0[i])) and all(full0[i].get(int(j)) == bool(h) for j, h in zip(ties[i], hu[i])), (b3, i)
    pl.close()


# ---- pipeline of overlapped calls ----------------------------------------------------------------------------------------------

def test_pipeline_depth_and_shared_waves(monkeypatch):
    """UGP_PIPELINE_DEPTH 2 and 4 (out of range: 1 -> 2, 9 -> 4), each with UGP_SHARED_WAVES unset, 1 and 3: depth + 2 overlapped
    calls on distinct query sets, with no synchronisation between them, each answer against the closed form."""
    import torch
    from usher_amd import synth as gsynth
    st = gsynth.SynthTree(300_000, n_sites=4000, seed=33)
    qs = [st.queries(n, seed=90 + i, max_subst=3, n_lo=0, n_hi=12, iupac_hi=2) for i, n in enumerate((1500, 600, 2600, 40, 1100, 3000))]
    batches = [QueryBatch.from_csr(q["ent_off"], q["pos"], q["ref"], q["nuc"], q["is_missing"]) for q in qs]
    cfc = capi.ClosedFormC(capi.OracleTree(st.arrays))
    want = []
    for q in qs:
        c = cfc.place_csr(q["ent_off"], q["pos"], q["ref"], q["nuc"], q["is_missing"])
        want.append(np.stack([c["best"], c["num_best"], c["best_j"], c["has_unique"]], 1).astype(np.int64))
    stream = torch.cuda.current_stream().cuda_stream
    for depth, want_depth in ((2, 2), (4, 4), (1, 2), (9, 4)):
        _env(monkeypatch, 0, {"UGP_PIPELINE_DEPTH": depth})
        pl = Placer(st.arrays)
        assert pl.pipeline_depth() == want_depth
        if depth in (1, 9):
            pl.close()
            continue
        handles = [pl.upload(b) for b in batches]
        for shared in (None, 1, 3):
            knobs = {"UGP_PIPELINE_DEPTH": depth}
            if shared is not None:
                knobs["UGP_SHARED_WAVES"] = shared
            for b3 in (0, 1):
                _env(monkeypatch, b3, knobs)
                pl.reload_knobs()
                assert pl.pipeline_depth() == want_depth
                order = [k % len(batches) for k in range(depth + 2)]
                bufs = [torch.full((len(batches[i]), 4), -7, dtype=torch.int32, device="cuda") for i in order]
                torch.cuda.synchronize()
                for i, o in zip(order, bufs):
                    pl.place_device_overlapped(handles[i], o.data_ptr(), stream)
                torch.cuda.synchronize()
                for k, (i, o) in enumerate(zip(order, bufs)):
                    got = o.cpu().numpy().astype(np.int64)
                    assert (got == want[i]).all(), (knobs, b3, k, i, np.flatnonzero((got != want[i]).any(1))[:4])
        for h in handles:
            pl.free_qset(h)
        pl.close()


# ---- coarse tree ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knobs", [{"UGP_COARSE_DIV": 2}, {"UGP_COARSE_DIV": 1000}, {"UGP_COARSE_FLOOR": 16}, {"UGP_COARSE_FLOOR": 100000},
                                   {"UGP_COARSE_CHUNK_NODES": 1}, {"UGP_COARSE_CHUNK_NODES": 7}], ids=lambda k: "%s=%s" % next(iter(k.items())))
def test_coarse_tree_shape(knobs, monkeypatch):
    arrays, queries, _, want = _case("A")
    batch = QueryBatch(queries)
    base = {"UGP_COARSE_MIN_NODES": 0, **knobs}
    _env(monkeypatch, 0, base)
    pl = Placer(arrays, chunk_nodes=300)
    _place_grid(monkeypatch, pl, batch, want, base, ({},), knobs)
    pl.close()


# ---- flattening ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["A", "B"])
def test_flattening_without_sibling_records(case, monkeypatch):
    arrays, queries, full, want = _case(case)
    batch = QueryBatch(queries)
    _env(monkeypatch, 1, {"UGP_COARSE_MIN_NODES": 0, "UGP_NO_SIB": 1})
    pl = Placer(arrays, chunk_nodes=48)
    _check(pl.place(batch), want, (case, "UGP_NO_SIB"))
    ties, hu, tc = pl.tied_nodes(batch, 64)
    for i, w in enumerate(full):
        assert int(tc[i]) == w["num_best"], i
        if w["num_best"] <= 64:
            assert ties[i].tolist() == w["ties"].tolist() and hu[i].tolist() == w["ties_has_unique"].tolist(), i
    ot = capi.OracleTree(arrays)
    few = queries[:37]
    got = pl.scores_per_node(QueryBatch(few))
    for i, s in enumerate(few):
        assert got[i].tolist() == ot.place(s, compute_scores=True)["scores"].tolist(), i
    pl.close()


def test_handle_without_update_maps_places_exactly_and_refuses_update(monkeypatch):
    arrays, queries, _, want = _case("A")
    _env(monkeypatch, 1, {"UGP_COARSE_MIN_NODES": 0, "UGP_NO_UPDATE_MAPS": 1})
    pl = Placer(arrays, chunk_nodes=300)
    _check(pl.place(QueryBatch(queries)), want, "UGP_NO_UPDATE_MAPS")
    with pytest.raises(UgpError) as ei:
        pl.update([{"flat_j": 1, "leaf": True, "path": [], "own": []}])
    assert ei.value.code == -2, str(ei.value)
    _check(pl.place(QueryBatch(queries)), want, "UGP_NO_UPDATE_MAPS after the refused update")
    pl.close()


# ---- add mode ------------------------------------------------------------------------------------------------------------------

def test_touched_records_per_block_in_fresh_processes():
    """UGP_TOUCHED_RECS is read once per process: the add-mode parity case of test_add_mode_gpu.py in one child process per value,
    one child at a time."""
    for recs in (1, 64):
        env = {k: v for k, v in os.environ.items() if not k.startswith("UGP_")}
        env.update({"UGP_TOUCHED_RECS": str(recs), "UGP_COARSE_MIN_NODES": "0", "UGP_BOUND3": "1", "PYTHONPATH": ROOT})
        code = "from tests.test_add_mode_gpu import check_flattened_tree_plus_records; check_flattened_tree_plus_records(5, 400, 60, 16)"
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, timeout=900, capture_output=True, text=True)
        assert r.returncode == 0, ("UGP_TOUCHED_RECS=%d" % recs, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- experiments build ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("knobs", [{"UGP_STATS": 1}, {"UGP_STATS": 1, "UGP_SEED_CHECK": 1}, {"UGP_KBEST_EXCLUSIVE": 1}, {"UGP_SEED_PREV": 1}],
                         ids=lambda k: "+".join(sorted(k)))
def test_experiments_build_stays_exact(knobs, monkeypatch):
    """libusher_amd_exp.so: one query set placed twice (UGP_SEED_PREV / UGP_SEED_CHECK act on the second call), both answers exact."""
    import torch
    arrays, queries, _, want = _case("A")
    batch = QueryBatch(queries)
    for b3 in (0, 1):
        _env(monkeypatch, b3, {"UGP_COARSE_MIN_NODES": 0, **knobs})
        pl = Placer(arrays, chunk_nodes=300, experiments=True)
        _check(pl.place(batch), want, (knobs, b3, "host"))
        h = pl.upload(batch)
        stream = torch.cuda.current_stream().cuda_stream
        for k in range(2):
            o = torch.full((len(batch), 4), -7, dtype=torch.int32, device="cuda")
            pl.place_device(h, o.data_ptr(), stream)
            torch.cuda.synchronize()
            got = o.cpu().numpy().astype(np.int64)
            assert (got == want).all(), (knobs, b3, k, np.flatnonzero((got != want).any(1))[:4])
        pl.free_qset(h)
        pl.close()
