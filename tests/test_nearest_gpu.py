"""ugp_nearest_k (Placer.nearest_k) against the restatements of tests/nearest_ref.py, every output field exactly: random,
caterpillar and polytomy trees, ranges at the segment edges of the dense kernels, distances at the radix-digit edges, ties,
chunked batches, masked entries and the error codes."""
import ctypes as C

import numpy as np
import pytest

from tests import nearest_cases as NC
from tests import nearest_ref as R
from tests import synth
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu


def _run(arrays, nodes, ks, literal_every=0, **kw):
    """All (node, k) pairs in one call against the numpy restatement; every literal_every-th also against the per-leaf walk."""
    F = R.Fast(arrays)
    T = R.Tree(arrays) if literal_every else None
    pl = Placer(arrays)
    got = pl.nearest_k(nodes, ks, **kw)
    pl.close()
    infos = []
    for i, (v, k) in enumerate(zip(nodes, np.broadcast_to(ks, (len(nodes),)))):
        want = F.query(int(v), int(k))
        if literal_every and i % literal_every == 0:
            assert want == R.literal(T, int(v), int(k)), (v, k)
        R.check(got, want, i, kw.get("out_stride"))
        infos.append(want)
    return infos


def _all_nodes_all_k(arrays, extra=()):
    T = R.Tree(arrays)
    L = int(T.nleaves[0])
    ks = [k for k in (1, 2, 7, L - 1, L, L + 5) + tuple(extra) if k > 0]
    nodes = np.repeat(np.arange(arrays["n"]), len(ks))
    kk = np.tile(ks, arrays["n"])
    infos = _run(arrays, nodes, kk, literal_every=97, out_stride=max(L, max(ks)))
    for w, k in zip(infos, kk):
        if k >= L:
            assert w["count"] == 0 and w["anc"] == R.NONE   # the reference's empty result
    return infos


@pytest.mark.parametrize("seed,n_leaves", [(1, 130), (2, 700), (3, 1700)])
def test_random_trees(seed, n_leaves):
    arrays = synth.make_case(seed, n_leaves=n_leaves, n_queries=1, n_sites=80, genome_len=600)[0]
    assert 200 <= arrays["n"] <= 3000
    _all_nodes_all_k(arrays)


def test_polytomy_tree():
    arrays = synth.polytomy_case(4, fanouts=(12, 15, 9), n_queries=1, genome_len=3000, n_sites=200)[0]
    assert 200 <= arrays["n"] <= 3000
    _all_nodes_all_k(arrays)


def test_caterpillar_and_root_polytomy():
    arrays = synth.caterpillar_case(5, depth=150, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=300)[0]
    infos = _all_nodes_all_k(arrays, extra=(40,))
    assert any(w["last_anc"] == v for w, v in zip(infos, np.repeat(np.arange(arrays["n"]), 7)) if w["count"])
    assert any(w["anc"] == 0 for w in infos)
    arrays = synth.polytomy_case(6, fanouts=(300,), n_queries=1)[0]
    infos = _all_nodes_all_k(arrays)
    leaf_rows = [w for w, v in zip(infos, np.repeat(np.arange(arrays["n"]), 6)) if v and w["count"]]
    assert leaf_rows and all(w["anc"] == 0 and w["last_anc"] != 0 for w in leaf_rows)


def test_segment_edges():
    arrays, ids = NC.segment_tree()
    par = arrays["parent"]
    F = R.Fast(arrays)
    assert (int(F.pre[ids["c2"]]), int(F.dend[F.pre[ids["c2"]]])) == (NC.SEG, 2 * NC.SEG)
    assert int(F.pre[ids["v"]]) < NC.SEG and int(F.dend[F.pre[ids["v"]]]) > 2 * NC.SEG
    in_c2 = np.flatnonzero(par == ids["c2"])
    in_v = np.flatnonzero(par == ids["v"])
    in_c1 = np.flatnonzero(par == ids["c1"])
    in_c3 = np.flatnonzero(par == ids["c3"])
    lv = len(in_c2) + len(in_v) - 1
    nodes, ks = [], []
    for leaf in (in_c2[0], in_c2[5000], in_c2[-1]):          # anc = c2: one whole segment
        nodes += [leaf] * 3; ks += [1, 50, len(in_c2) - 1]
    for leaf in (in_v[0], in_v[382], in_v[-1], in_c2[77]):   # anc = v: starts in segment 0, ends in segment 2
        nodes += [leaf] * 2; ks += [len(in_c2) + 3, lv - 1]
    for leaf in (in_c2[9], in_v[3]):                         # last_anc = v straddles both edges, anc = w; > 4096 candidates taken
        nodes += [leaf] * 3; ks += [lv, lv + 1, lv + 5000]
    for leaf in (in_c1[0], in_c1[-1], in_c3[0], in_c3[-1]):  # anc = w from both ends, the global sort
        nodes += [leaf] * 2; ks += [len(par[par == par[leaf]]), 20000]
    nodes += [ids["c2"], ids["v"], ids["w"], 0]; ks += [10, 10, 10, 10]   # nodes with more than k leaves of their own
    infos = _run(arrays, np.array(nodes), np.array(ks), out_stride=max(ks))
    assert sum(w["anc"] == ids["c2"] for w in infos) >= 9 and sum(w["last_anc"] == ids["v"] and w["anc"] == ids["w"] for w in infos) == 6
    assert infos[-4]["count"] == len(in_c2) and infos[-1]["count"] > max(ks)


SORT_NEEDS = (1, 2, 3, 4, 5, NC.SORT_LDS - 1, NC.SORT_LDS, NC.SORT_LDS + 1, 2 * NC.SORT_LDS - 1, 2 * NC.SORT_LDS, 2 * NC.SORT_LDS + 1)


def test_sort_size_edges():
    """The sort of one query's candidates at the edges of its two paths: 4096 pairs in LDS and the same network over a global
    scratch for more, padded to a power of two (a pad of one slot at 4095 and 8191, none at 4096 and 8192, the next power at 4097
    and 8193).  The keys come unsorted and with ties (NC.sort_tree).  A second call puts the LDS queries between the global ones, so
    that scratch ranges of different padded length lie side by side in one chunk."""
    arrays, q, P = NC.sort_tree()
    F = R.Fast(arrays)
    want = {need: F.query(q, need + 1) for need in SORT_NEEDS}
    assert all(w["anc"] == P and w["last_anc"] == q and w["count"] == need + 1 for need, w in want.items())
    mixed = (8193, 3, 4097, 1, 4096, 8192, 2, 4095, 8191, 5, 4)
    assert sorted(mixed) == sorted(SORT_NEEDS)
    pl = Placer(arrays)
    for needs in (SORT_NEEDS, mixed):
        ks = np.array(needs, np.uint32) + 1
        for chunk in (1, 3, 0):
            got = pl.nearest_k(np.full(len(needs), q), ks, chunk_queries=chunk)
            assert got[0].shape == (len(needs), max(SORT_NEEDS) + 1)
            for i, need in enumerate(needs):
                R.check(got, want[need], i)
    pl.close()


def test_digit_edges():
    arrays, q, n_p = NC.digit_tree()
    infos = _run(arrays, np.full(n_p + 3, q), np.arange(1, n_p + 4), literal_every=1)
    # k = 1: nothing taken; then one pass (keys below 2^11), three (the digit moved up once), five (beyond 2^22);
    # k = leaves(P) and more climb to the root, k = all leaves is empty
    assert [w["cut_dist"] for w in infos[:n_p - 1]] == [0, 1, 5, 5, 5, 2047, 2048, 2048, 2049, 2100 * 2000 + 7]
    assert [w["n_at_cut"] for w in infos[5:9]] == [1, 2, 2, 1]
    assert [(w["anc"], w["last_anc"], w["cut_dist"]) for w in infos[n_p - 1:n_p + 2]] == [(0, 1, 0), (0, 1, 1), (0, 1, 2)]
    assert infos[n_p + 2]["count"] == 0


def test_ties_are_the_first_in_depth_first_order():
    arrays, leaf = NC.tie_tree()
    infos = _run(arrays, np.array([leaf, leaf, leaf]), np.array([100, 20, 499]), literal_every=1)
    w = infos[0]
    s = int(arrays["parent"][leaf])
    assert w["last_anc"] == s and w["anc"] == 1 and w["n_at_cut"] == 500 - 20
    direct = [int(v) for v in np.flatnonzero(arrays["parent"] == 1) if v != s]
    assert w["nodes"][20:] == direct[:80]


def test_mixed_batch_over_several_chunks():
    arrays = synth.make_case(8, n_leaves=600, n_queries=1, n_sites=80, genome_len=600)[0]
    L = int(R.Tree(arrays).nleaves[0])
    rng = np.random.default_rng(9)
    nodes = rng.integers(0, arrays["n"], 1500)
    ks = np.where(rng.random(1500) < 0.5, rng.integers(1, 6, 1500), rng.integers(1, L + 3, 1500))
    for chunk in (64, 7, 0):   # 0: the default chunk of 1024 queries, still more than one
        _run(arrays, nodes, ks, chunk_queries=chunk)


def test_masked_entries_count():
    arrays = synth.make_case(10, n_leaves=300, n_queries=1, n_sites=80, genome_len=600, p_masked=0.3)[0]
    assert (arrays["mut_pos"] < 0).sum() > 50
    _all_nodes_all_k(arrays)


def test_error_codes_leave_the_output_untouched():
    arrays = synth.make_case(11, n_leaves=100, n_queries=1)[0]
    pl = Placer(arrays)
    pl.nearest_k([1], 1)
    nodes = np.array([3, 4, 5], np.uint32)
    for bad_nodes, ks, stride in ((np.array([3, arrays["n"], 5], np.uint32), [2, 2, 2], 4), (nodes, [2, 0, 2], 4), (nodes, [2, 9, 2], 8)):
        on = np.full((3, stride), 0xABCDEF01, np.uint32); od = on.copy()
        info = np.full(3, 0x5A, np.uint8).repeat(20).view(Placer.NEAREST_INFO)
        ks = np.array(ks, np.uint32)
        rc = pl._L.ugp_nearest_k(pl._h, 3, _ptr(bad_nodes), _ptr(ks), stride, _ptr(on), _ptr(od), _ptr(info))
        assert rc == -1 and pl._L.ugp_last_error()
        assert (on == 0xABCDEF01).all() and (od == 0xABCDEF01).all() and (info.view(np.uint8) == 0x5A).all()
    with pytest.raises(UgpError):
        pl.nearest_k([arrays["n"]], 1)
    pl.close()
