"""Placer.vectors (ugp_vectors) against the literal mapper2_body of the oracle (OracleTree.node_vecs_split: the lists, and n_branch,
eligible and the score each on its own), exactly, on every case of tests/vectors_cases.py: info, both offset arrays and both lists,
on a handle that holds the tree's mutations and on a topology-only one, through every window size, with pairs shuffled and repeated,
under caps, and the errors; nodes of more than 64 entries, root paths whose nodes hold 0 to 70 entries side by side, windows of one
and two tiles of the prefix sums and a pair more or less, and seeded random trees (the picks of vectors_cases.py, whose edges
tests/test_vectors_cpu.py proves); then vectors beside the other families that share a handle's depth-first tables
(tests/shared_tables_cases.py)."""
import numpy as np
import pytest

from oracle import capi
from tests import shared_tables_cases as S
from tests import summary_cases as SMC
from tests import vectors_cases as VC
from tests import vectors_ref as VR
from usher_amd import Placer, QueryBatch, UgpError

pytestmark = pytest.mark.gpu
CASES = VC.cases()
WANT = {}   # case name -> {(sample, node): the oracle's answer}, computed once


def want(case):
    if case["name"] not in WANT:
        ot = capi.OracleTree(case["arrays"])
        WANT[case["name"]] = {(s, j): VR.oracle_answer_split(ot, case["samples"][s], j) for s, j in sorted(set(case["pairs"]))
                              if j not in case["refused"]}
    return WANT[case["name"]]


def bare(case):
    pl = Placer(SMC.topology(case["arrays"]))
    pl.vectors_attach(case["arrays"])
    return pl


def check(case, pl, pairs, **kw):
    """One call over `pairs`; every pair against the oracle, the offsets against the counts."""
    q = QueryBatch(case["samples"])
    got = pl.vectors(q, [j for _, j in pairs], [s for s, _ in pairs], **kw)
    info, ex_off, ex, im_off, im = got
    assert int(ex_off[0]) == 0 and int(im_off[0]) == 0 and int(ex_off[-1]) == len(ex) and int(im_off[-1]) == len(im)
    assert pl._vec_totals == (len(ex), len(im))
    ans = VR.device_answers(info, ex_off, ex, im_off, im)
    w = want(case)
    for (s, j), a in zip(pairs, ans):
        assert a["refused"] == (1 if j in case["refused"] else 0), (case["name"], s, j)
        if a["refused"]:
            assert a["excess"] == [] and a["imputed"] == [] and a["n_branch"] == 0 and a["set_difference"] == 0
        else:
            assert VR.agrees(a, w[(s, j)]), (case["name"], s, j, a, w[(s, j)])
            assert a["excess"][:a["n_branch"]] == w[(s, j)]["excess"][:a["n_branch"]]
            assert VR.agrees_split(a, w[(s, j)]), (case["name"], s, j, a, w[(s, j)])
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_every_pair_on_a_topology_only_handle(case):
    pl = bare(case)
    check(case, pl, case["pairs"])
    pl.close()


def test_every_pair_on_a_handle_with_the_trees_own_mutations():
    """The placement tables refuse masked entries and a position twice on a node: the cases they take run on such a handle too."""
    ran = []
    for case in CASES:
        try:
            pl = Placer(case["arrays"])
        except UgpError as e:
            assert e.code == -2, case["name"]
            continue
        pl.vectors_attach()
        check(case, pl, case["pairs"])
        pl.close()
        ran.append(case["name"])
    assert {"ambiguous", "rewrite", "caterpillar", "caterpillar_flip", "rows", "polytomy"} <= set(ran), ran


@pytest.mark.parametrize("name", ["loop1", "rows", "twice"])
def test_windows_shuffles_and_repeats(name):
    case = next(c for c in CASES if c["name"] == name)
    pl = bare(case)
    pairs = list(case["pairs"])
    n = len(pairs)
    whole = check(case, pl, pairs)
    for chunk in (1, 2, 3, n - 1, n, n + 1, 0):
        got = check(case, pl, pairs, chunk_pairs=chunk)
        assert all(np.array_equal(a, b) for a, b in zip(got, whole)), chunk
    rng = np.random.default_rng(7)
    mixed = [pairs[i] for i in rng.permutation(n)]
    mixed.insert(n // 2, mixed[0])
    check(case, pl, mixed, chunk_pairs=5)
    pl.close()


def test_no_pairs_and_caps():
    case = next(c for c in CASES if c["name"] == "ambiguous")
    pl = bare(case)
    q = QueryBatch(case["samples"])
    info, ex_off, ex, im_off, im = pl.vectors(q, [])
    assert len(info) == 0 and ex_off.tolist() == [0] and im_off.tolist() == [0] and len(ex) == 0 and len(im) == 0
    pairs = case["pairs"]
    nodes, smp = [j for _, j in pairs], [s for s, _ in pairs]
    whole = pl.vectors(q, nodes, smp)
    tot = pl._vec_totals
    assert tot[0] > 2 and tot[1] > 2
    for chunk in (0, 7):
        for cap_ex, cap_im in ((0, 0), (tot[0] - 1, tot[1] - 1), (tot[0], tot[1]), (0, tot[1]), (tot[0], 0)):
            info, ex_off, ex, im_off, im = pl.vectors(q, nodes, smp, chunk_pairs=chunk, ex_cap=cap_ex, im_cap=cap_im)
            assert pl._vec_totals == tot                                                       # the totals are true
            assert np.array_equal(info, whole[0]) and np.array_equal(ex_off, whole[1]) and np.array_equal(im_off, whole[3])   # complete
            assert len(ex) == cap_ex and np.array_equal(ex, whole[2][:cap_ex])                   # the prefix is exact
            assert len(im) == cap_im and np.array_equal(im, whole[4][:cap_im])
    pl.close()


def _raw(pl, q, nodes, samples, info, ex_off, ex, im_off, im):
    import ctypes as C
    from usher_amd.placement import _ptr
    n_ex, n_im = C.c_uint64(77), C.c_uint64(77)
    rc = pl._L.ugp_vectors(pl._h, C.byref(q.desc), len(nodes), _ptr(samples), _ptr(nodes), _ptr(info), _ptr(ex_off), _ptr(ex), len(ex), C.byref(n_ex),
                           _ptr(im_off), _ptr(im), len(im), C.byref(n_im))
    return rc, n_ex.value, n_im.value


def test_errors_write_nothing():
    case = next(c for c in CASES if c["name"] == "loop1")
    q = QueryBatch(case["samples"])
    n = int(case["arrays"]["n"])
    pl = Placer(SMC.topology(case["arrays"]))
    with pytest.raises(UgpError) as e:   # before the attach
        pl.vectors(q, [0])
    assert e.value.code == -1 and "ugp_vectors_attach" in str(e.value)
    with pytest.raises(UgpError) as e:
        pl.vectors_time(q, [0])
    assert e.value.code == -1 and "ugp_vectors_attach" in str(e.value)
    pl.vectors_attach(case["arrays"])
    for nodes, samples in (([1, n], [0, 0]), ([1, 0xFFFFFFFF], [0, 0]), ([1, 2], [0, len(case["samples"])]), ([1, 2], [0xFFFFFFFF, 0])):
        nodes, samples = np.asarray(nodes, np.uint32), np.asarray(samples, np.uint32)
        info = np.full(2, 0x5A, np.uint8).repeat(Placer.VEC_INFO.itemsize).view(Placer.VEC_INFO)
        ex_off, im_off = np.full(3, 99, np.uint64), np.full(3, 99, np.uint64)
        ex, im = np.full(64, 0x5A, np.uint8).view(Placer.VEC_ENTRY), np.full(64, 0x5A, np.uint8).view(Placer.VEC_ENTRY)
        rc, n_ex, n_im = _raw(pl, q, nodes, samples, info, ex_off, ex, im_off, im)
        assert rc == -1 and b"out of range" in pl._L.ugp_last_error()
        assert (n_ex, n_im) == (77, 77) and ex_off.tolist() == [99] * 3 and im_off.tolist() == [99] * 3
        assert (info.view(np.uint8) == 0x5A).all() and (ex.view(np.uint8) == 0x5A).all() and (im.view(np.uint8) == 0x5A).all()
    # without a sample list pair i is sample i: more pairs than samples is out of range too
    with pytest.raises(UgpError) as e:
        pl.vectors(q, [0] * (len(case["samples"]) + 1))
    assert e.value.code == -1
    # unsorted rows: the error of ugp_place_batch
    bad = dict(case["samples"][0])
    bad = {k: (v[::-1].copy() if k != "name" else v) for k, v in bad.items()}
    qb = QueryBatch([bad])
    with pytest.raises(UgpError) as e1:
        pl.place(qb)
    with pytest.raises(UgpError) as e2:
        pl.vectors(qb, [1])
    assert e1.value.code == e2.value.code == -2 and str(e1.value) == str(e2.value) and "not sorted" in str(e2.value)
    check(case, pl, case["pairs"][:7])   # and the handle still answers
    pl.close()


# ---- the steps of 64, the tiles of the prefix sums, random trees --------------------------------------------------------------------

def generated(make, *args):
    """A case of a generator of vectors_cases.py, built once."""
    key = (make.__name__,) + args
    if key not in _GENERATED:
        _GENERATED[key] = make(*args)
        assert not _GENERATED[key]["refused"]
    return _GENERATED[key]


_GENERATED = {}


@pytest.mark.parametrize("pick", VC.WIDE_PICKS, ids=lambda p: "-".join(map(str, p)))
def test_wide_nodes(pick):
    """A node of 63 .. 200 own entries in ascending, descending and shuffled stored order, with a masked entry on and around the
    seam of two steps of 64, as an internal node, as a leaf and as the root: all pairs in one call, and a pair a window."""
    case = generated(VC.wide, *pick)
    pl = bare(case)
    whole = check(case, pl, case["pairs"])
    single = check(case, pl, case["pairs"], chunk_pairs=1)
    assert all(np.array_equal(a, b) for a, b in zip(single, whole))
    pl.close()
    masked = (np.asarray(case["arrays"]["mut_pos"]) < 0).any()
    try:
        pl = Placer(case["arrays"])
    except UgpError as e:   # the placement tables may refuse a masked entry, nothing else here
        assert e.code == -2 and masked, case["name"]
        return
    pl.vectors_attach()
    got = check(case, pl, case["pairs"])
    assert all(np.array_equal(a, b) for a, b in zip(got, whole))
    pl.close()


@pytest.mark.parametrize("pick", VC.RAGGED_PICKS, ids=lambda p: "%d-%s" % (p[0], "".join(map(str, p[1]))))
def test_ragged_paths(pick):
    """Root paths whose nodes hold 0, 1, 2, 3, 7 and 70 entries side by side in one step of 64 lanes, of 2 .. 202 nodes."""
    case = generated(VC.ragged_path, *pick)
    pl = bare(case)
    check(case, pl, case["pairs"])
    pl.close()


def expected_arrays(case, pairs):
    """What Placer.vectors must return for `pairs`, as arrays, from the oracle's answers to the distinct pairs."""
    w = want(case)
    one = {}
    for pr in set(pairs):
        o = w[pr]
        info = np.zeros(1, Placer.VEC_INFO)
        info[0] = (len(o["excess"]), len(o["imputed"]), o["n_branch"], o["set_difference"] - (0 if o["eligible"] else 1), o["has_unique"],
                   o["eligible"], 0, 0)
        ent = lambda l: np.asarray([(p, r, a, n, 0) for p, r, a, n in l], Placer.VEC_ENTRY).reshape(-1)
        one[pr] = (info, ent(o["excess"]), ent(o["imputed"]))
    info, ex, im = (np.concatenate([one[pr][k] for pr in pairs]) for k in range(3))
    off = lambda c: np.concatenate([[0], np.cumsum(c, dtype=np.uint64)]).astype(np.uint64)
    return info, off(info["n_excess"]), ex, off(info["n_imputed"]), im


@pytest.mark.parametrize("both", [False, True], ids=["empty_empty_part3", "both_lists"])
def test_window_seams(both):
    """One tile of k_vec_scan less a pair, one tile, one more, two tiles, two and a pair, in one window: at the seam of the first two
    tiles two pairs without any entry and one with entries of part 3, or three pairs with both lists.  Every returned array against
    the oracle's; the largest count once more in windows of a tile less and more a pair; caps that cut inside the pair on the seam."""
    case = next(c for c in CASES if c["name"] == VC.SEAM_CASE)
    pl = bare(case)
    q = QueryBatch(case["samples"])
    w = want(case)
    for n in VC.SEAM_COUNTS:
        pairs = VC.seam_pairs(n, both)
        nodes, smp = [j for _, j in pairs], [s for s, _ in pairs]
        exp = expected_arrays(case, pairs)
        got = pl.vectors(q, nodes, smp)
        for name, a, b in zip(("info", "ex_off", "excess", "im_off", "imputed"), got, exp):
            assert np.array_equal(a, b), (n, name, np.flatnonzero(a != b)[:4] if len(a) == len(b) else (len(a), len(b)))
        assert pl._vec_totals == (len(exp[2]), len(exp[4]))
        lo = max(0, VC.SEAM_TILE - 3)
        for pr, a in zip(pairs[lo:lo + 6], VR.device_answers(got[0][lo:lo + 6], got[1][lo:lo + 7], got[2], got[3][lo:lo + 7], got[4])):
            assert VR.agrees_split(a, w[pr]), (n, pr)
        if n == VC.SEAM_COUNTS[-1]:
            for chunk in (VC.SEAM_TILE - 1, VC.SEAM_TILE + 1):
                again = pl.vectors(q, nodes, smp, chunk_pairs=chunk)
                assert all(np.array_equal(a, b) for a, b in zip(again, got)), chunk
        if both and n == VC.SEAM_TILE + 1:   # the caps end one entry into the lists of the pair at the head of the second tile
            cap_ex, cap_im = int(exp[1][VC.SEAM_TILE]) + 1, int(exp[3][VC.SEAM_TILE]) + 1
            assert cap_ex < int(exp[1][VC.SEAM_TILE + 1]) and cap_im < int(exp[3][VC.SEAM_TILE + 1])
            cut = pl.vectors(q, nodes, smp, ex_cap=cap_ex, im_cap=cap_im)
            assert pl._vec_totals == (len(exp[2]), len(exp[4]))
            assert np.array_equal(cut[0], exp[0]) and np.array_equal(cut[1], exp[1]) and np.array_equal(cut[3], exp[3])
            assert len(cut[2]) == cap_ex and np.array_equal(cut[2], exp[2][:cap_ex])
            assert len(cut[4]) == cap_im and np.array_equal(cut[4], exp[4][:cap_im])
    pl.close()


def test_random_trees_on_the_device():
    """Every node for every sample of a dozen seeded random trees of up to 150 nodes and 80 entries a node, one call a tree."""
    pairs = part3 = branch = 0
    for pick in VC.RANDOM_PICKS:
        case = generated(VC.random_case, *pick)
        pl = bare(case)
        info = check(case, pl, case["pairs"])[0]
        pl.close()
        pairs += len(info)
        branch += int((info["n_branch"] > 0).sum())
        part3 += int((info["n_excess"] > info["n_branch"] + np.asarray([_part2(case, s, j) for s, j in case["pairs"]])).sum())
    assert pairs >= 4000 and part3 >= 2000 and branch >= 500, (pairs, part3, branch)


def _part2(case, s, j):
    """The entries of part 2 in the oracle's answer: those behind the branch's at the position of a non-missing row of the sample
    (part 3 has entries only where the sample has no row)."""
    smp, o = case["samples"][s], want(case)[(s, j)]
    rows = {int(p) for p, m in zip(smp["pos"], smp["is_missing"]) if not m}
    return sum(1 for p, _, _, _ in o["excess"][o["n_branch"]:] if p in rows)


# ---- beside the families that share the depth-first tables ----------------------------------------------------------------------------

vectors_answer = S.vectors_answer   # the questions and the oracle's answers live beside the other families'


@pytest.mark.parametrize("tree", ("plain", "bare"))
@pytest.mark.parametrize("other", ("uncertainty", "select", "haplotypes"))
def test_beside_the_families_that_share_the_tables(tree, other):
    t = S.trees()[tree]
    B = next(f for f in S.families(t) if f.name == other)
    pl = t.handle()            # vectors first: it builds the depth-first tables and the owners' nodes
    pl.vectors_attach(t.X)
    vectors_answer(t, pl, "alone")
    B.attach(pl, t.X)
    assert B.ask(pl) == B.wanted(), ("after vectors", other)
    vectors_answer(t, pl, ("after", other))
    pl.close()
    pl = t.handle()            # vectors second
    B.attach(pl, t.X)
    assert B.ask(pl) == B.wanted()
    pl.vectors_attach(t.X)
    vectors_answer(t, pl, ("attached after", other))
    assert B.ask(pl) == B.wanted(), ("before vectors", other)
    pl.close()


def _refused(pl, y):
    with pytest.raises(UgpError) as e:
        pl.vectors_attach(y)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value) and "ugp_vectors_attach" in str(e.value)


@pytest.mark.parametrize("tree", ("plain", "bare"))
def test_other_arrays_are_refused(tree):
    t = S.trees()[tree]
    B = next(f for f in S.families(t) if f.name == "select")
    pl = t.handle()
    B.attach(pl, t.X)
    for y in S.YS:             # as a first attach of vectors: the handle has no vector tables afterwards
        _refused(pl, t.Y[y])
        with pytest.raises(UgpError) as e:
            pl.vectors(QueryBatch([]), [])
        assert "ugp_vectors_attach" in str(e.value)
    assert B.ask(pl) == B.wanted()
    pl.vectors_attach(t.X)
    for y in S.YS:             # as a second attach, which would replace the state
        _refused(pl, t.Y[y])
    vectors_answer(t, pl, "after the refused attaches")
    assert B.ask(pl) == B.wanted()
    pl.close()
