"""ugp_subtree_batch (Placer.subtree_batch) on the batches of tests/subtree_batch_cases.py: every slice exactly against
tests/subtree_ref.py and against Placer.subtree_nodes on the same selection alone -- kept nodes, parents within the slice, offsets,
merged entries and the info record with the lowest common ancestor; the windows' relations, the seams of the concatenation at
kBlock and kSeg, the group budget and the launch windows of the _chunked hook, the root path above the lowest common ancestor, the
cap conventions, the error codes, and the two result states side by side."""
import ctypes as C

import numpy as np
import pytest

from tests import subtree_batch_cases as BC
from tests import subtree_cases as SC
from tests import subtree_ref as R
from tests import summary_cases as SMC
from usher_amd import Placer
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu
BATCHES = BC.all_batches()
_oracles = {}


def placer(batch):
    pl = Placer(SMC.topology(batch.arrays))
    pl.subtree_attach(batch.arrays)
    return pl


def oracle(batch, sel):
    """Computed once per (tree, selection) and shared; the literal walk where it is quick, else the closed form."""
    key = (id(batch.arrays), tuple(sel))
    if key not in _oracles:
        _oracles[key] = R.literal(batch.arrays, sel) if len(sel) <= 70 and int(batch.arrays["n"]) <= 2000 else R.closed_form(batch.arrays, sel)
    return _oracles[key]


def check(batch, got, why=None):
    assert len(got) == len(batch.sels)
    lcas = BC.windows(batch)
    for b, (sel, g) in enumerate(zip(batch.sels, got)):
        want = oracle(batch, sel)
        assert R.same(g, want), (batch.name, b, sel[:20], why)
        assert int(g["info"]["n_kept"]) == len(want["kept"]) and int(g["info"]["n_entries"]) == len(want["pos"]), (batch.name, b, why)
        assert int(g["info"]["lca"]) == lcas[b][0] == int(g["kept"][0]), (batch.name, b, why)


@pytest.mark.parametrize("batch", BATCHES, ids=repr)
def test_batches(batch):
    pl = placer(batch)
    check(batch, pl.subtree_batch(batch.sels))
    for b, sel in enumerate(batch.sels):   # each selection as a batch of one, and the single call on it
        one = pl.subtree_batch([sel])
        assert len(one) == 1 and R.same(one[0], oracle(batch, sel)), (b, sel[:20])
        assert R.same(pl.subtree_nodes(sel), oracle(batch, sel)), (b, sel[:20])
    pl.close()


@pytest.mark.parametrize("name", ["rel_mixed", "rel_nested", "path_caterpillar", "path_disagree", "block_255_256_257", "block_every_leaf", "sstar257"])
def test_group_budgets_and_launch_windows(name):
    batch = BC.by_name()[name]
    pl = placer(batch)
    sizes = sorted({w for _, w in BC.windows(batch)})
    budgets = {1, 0}
    for w in sizes:
        budgets |= {max(w - 1, 1), w, w + 1}
    budgets |= {sizes[-1] + sizes[0], sum(w for _, w in BC.windows(batch))}
    for gp in sorted(budgets):
        check(batch, pl.subtree_batch(batch.sels, group_positions=gp), ("group_positions", gp))
    for chunk in (1, 2, 63, 0):
        check(batch, pl.subtree_batch(batch.sels, chunk_items=chunk), ("chunk_items", chunk))
    check(batch, pl.subtree_batch(batch.sels, group_positions=sizes[0], chunk_items=2), "both")
    a, b = pl.subtree_batch_time(batch.sels, reps=2)
    assert a > 0 and b > 0
    check(batch, pl.subtree_batch(batch.sels), "after the timing hook")
    pl.close()


def test_seams_at_the_segment_size():
    batch = BC.segment_seam_batch()
    sizes = [w for _, w in BC.windows(batch)]
    seams = np.cumsum(sizes).tolist()
    assert seams[:3] == [BC.KSEG - 1, BC.KSEG, BC.KSEG + 1] and seams[-1] > 2 * BC.KSEG
    pl = placer(batch)
    check(batch, pl.subtree_batch(batch.sels))
    check(batch, pl.subtree_batch(batch.sels, group_positions=BC.KSEG), "two windows fill a group to kSeg exactly")
    check(batch, pl.subtree_batch(batch.sels, group_positions=BC.KSEG - 1), "the large windows alone")
    rotated = BC.Batch("segment_seams_rotated", batch.arrays, batch.sels[1:] + batch.sels[:1], "the large window last")
    check(rotated, pl.subtree_batch(rotated.sels))
    pl.close()


def test_a_disagreement_astride_the_lca_is_counted_per_selection():
    batch = BC.by_name()["path_disagree"]
    tags = {"b": 3, "l": 4, "m": 5}
    pl = placer(batch)
    got = pl.subtree_batch(batch.sels)   # [l, m], [l], [m, out], [l, m]
    check(batch, got)
    # b's chain (root, a, b) holds both entries; l's whole root path holds them and l's own; m's chain below the root (a, b, m) too
    assert [int(g["info"]["n_disagree"]) for g in got] == [1, 2, 1, 1]
    assert [int(g["info"]["first_disagree"]) for g in got] == [tags["b"], tags["l"], tags["m"], tags["b"]]
    none = pl.subtree_batch([[2], [tags["b"], 2]])   # `out` alone, and b beside it: b's chain (a, b) holds both entries, out's none
    assert [int(g["info"]["n_disagree"]) for g in none] == [0, 1] and int(none[0]["info"]["first_disagree"]) == R.NIL
    assert int(got[0]["kept"][0]) == tags["b"] and int(got[1]["kept"][0]) == tags["l"]
    rev = BC.by_name()["path_reverted"]
    pl2 = placer(rev)
    got = pl2.subtree_batch(rev.sels)
    check(rev, got)
    assert R.strings(rev.arrays, got[0])[int(got[0]["kept"][0])] == [] and int(got[0]["info"]["n_gathered"]) == 3
    chg = BC.by_name()["path_changed"]
    pl3 = placer(chg)
    got = pl3.subtree_batch(chg.sels)
    assert R.strings(chg.arrays, got[0])[int(got[0]["kept"][0])] == ["A5G", "T7A"]
    msk = BC.by_name()["path_masked"]
    pl4 = placer(msk)
    got = pl4.subtree_batch(msk.sels)
    assert R.strings(msk.arrays, got[0])[int(got[0]["kept"][0])] == ["MASKED", "A7T"] and R.strings(msk.arrays, got[1])[int(got[1]["kept"][0])] == ["A7T"]
    for p in (pl, pl2, pl3, pl4):
        p.close()


def _flat(sels):
    off = np.zeros(len(sels) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in sels])
    return off, np.asarray([v for s in sels for v in s], np.uint32)


def test_cap_conventions():
    batch = BC.by_name()["block_255_256_257"]
    pl = placer(batch)
    L, h = pl._L, pl._h
    want = [oracle(batch, s) for s in batch.sels]
    nk, ne = sum(len(w["kept"]) for w in want), sum(len(w["pos"]) for w in want)
    off, flat = _flat(batch.sels)
    ns = len(batch.sels)
    koff, eoff = np.zeros(ns + 1, np.uint64), np.zeros(ns + 1, np.uint64)
    assert L.ugp_subtree_batch(h, ns, _ptr(off), _ptr(flat), _ptr(koff), _ptr(eoff), None) == 0   # info may be NULL
    assert koff.tolist() == np.cumsum([0] + [len(w["kept"]) for w in want]).tolist()
    assert eoff.tolist() == np.cumsum([0] + [len(w["pos"]) for w in want]).tolist()
    kept, par, ent = np.full(nk, 7, np.uint32), np.full(nk, 7, np.uint32), np.full(nk, 7, np.uint64)
    a = C.c_uint64(0)
    assert L.ugp_subtree_batch_nodes(h, _ptr(kept), _ptr(par), _ptr(ent), 0, C.byref(a)) == 0
    assert a.value == nk and (kept == 7).all() and (par == 7).all() and (ent == 7).all()
    assert L.ugp_subtree_batch_nodes(h, None, None, None, 0, C.byref(a)) == 0 and a.value == nk
    cut = len(want[0]["kept"]) + 1   # into the second slice
    assert L.ugp_subtree_batch_nodes(h, _ptr(kept), _ptr(par), _ptr(ent), cut, C.byref(a)) == 0 and a.value == nk
    assert kept[:cut].tolist() == want[0]["kept"].tolist() + want[1]["kept"][:1].tolist() and (kept[cut:] == 7).all()
    assert par[:cut].tolist() == want[0]["parent"].tolist() + [R.NIL] and (par[cut:] == 7).all() and (ent[cut:] == 7).all()
    assert ent[:cut].tolist() == want[0]["ent_off"][:-1].tolist() + [len(want[0]["pos"])]
    pos, first, nuc = np.full(ne, 7, np.int32), np.full(ne, 7, np.uint32), np.full(ne, 7, np.uint8)
    assert L.ugp_subtree_batch_entries(h, _ptr(pos), _ptr(first), _ptr(nuc), 2, C.byref(a)) == 0 and a.value == ne
    assert pos[:2].tolist() == want[0]["pos"][:2].tolist() and (pos[2:] == 7).all() and (first[2:] == 7).all() and (nuc[2:] == 7).all()
    assert L.ugp_subtree_batch_entries(h, None, None, None, 0, C.byref(a)) == 0 and a.value == ne
    assert L.ugp_subtree_batch_entries(h, _ptr(pos), _ptr(first), _ptr(nuc), ne + 5, C.byref(a)) == 0 and a.value == ne
    assert pos.tolist() == [p for w in want for p in w["pos"].tolist()]
    assert L.ugp_subtree_batch_nodes(h, None, None, None, 1, C.byref(a)) == -1 and L.ugp_subtree_batch_nodes(h, None, None, None, 0, None) == -1
    assert L.ugp_subtree_batch_entries(h, None, None, None, 1, C.byref(a)) == -1 and L.ugp_subtree_batch_entries(h, None, None, None, 0, None) == -1
    pl.close()


def test_error_codes_write_nothing():
    batch = BC.by_name()["rel_mixed"]
    n = int(batch.arrays["n"])
    pl = Placer(SMC.topology(batch.arrays))
    L, h = pl._L, pl._h
    off, flat = _flat(batch.sels)
    ns = len(batch.sels)
    koff, eoff = np.full(ns + 1, 7, np.uint64), np.full(ns + 1, 7, np.uint64)
    info = np.zeros(ns, Placer.SUB_BATCH_INFO)
    a, ms = C.c_uint64(7), C.c_double(0)

    def run(k=ns, o=off, f=flat, ko=koff):
        return L.ugp_subtree_batch(h, k, _ptr(o) if o is not None else None, _ptr(f) if f is not None else None,
                                   _ptr(ko) if ko is not None else None, _ptr(eoff), _ptr(info))

    def untouched():
        return (koff == 7).all() and (eoff == 7).all() and not info.view(np.uint8).any() and a.value == 7

    # before the attach: every call names the missing one
    assert run() == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    assert L.ugp_subtree_batch_nodes(h, None, None, None, 0, C.byref(a)) == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    assert L.ugp_subtree_batch_entries(h, None, None, None, 0, C.byref(a)) == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    assert L.ugp_subtree_batch_time(h, ns, _ptr(off), _ptr(flat), 1, C.byref(ms), C.byref(ms)) == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    pl.subtree_attach(batch.arrays)
    # a fetch before any batch, also after a single call
    assert L.ugp_subtree_batch_nodes(h, None, None, None, 0, C.byref(a)) == -1 and b"ugp_subtree_batch" in L.ugp_last_error()
    pl.subtree_nodes(batch.sels[1])
    assert L.ugp_subtree_batch_entries(h, None, None, None, 0, C.byref(a)) == -1 and b"ugp_subtree_batch" in L.ugp_last_error()
    assert untouched()
    # no selections, an empty one, a node out of range, descending offsets, null pointers
    assert run(k=0) == -1 and run(o=None) == -1 and run(f=None) == -1 and run(ko=None) == -1 and untouched()
    empty = off.copy()
    empty[3] = empty[2]
    assert run(o=empty) == -1 and b"empty" in L.ugp_last_error() and untouched()
    down = off.copy()
    down[2], down[3] = off[3], off[2]
    assert run(o=down) == -1 and b"descend" in L.ugp_last_error() and untouched()
    bad = flat.copy()
    bad[-1] = n
    assert run(f=bad) == -1 and b"out of range" in L.ugp_last_error() and untouched()
    assert L.ugp_subtree_batch_time(h, ns, _ptr(off), _ptr(flat), 0, C.byref(ms), C.byref(ms)) == -1
    assert L.ugp_subtree_batch_nodes(h, None, None, None, 0, C.byref(a)) == -1   # none of these made a batch
    # a good batch, then a refused one: the good one's lists stay
    check(batch, pl.subtree_batch(batch.sels))
    assert run(f=bad) == -1
    assert L.ugp_subtree_batch_nodes(h, None, None, None, 0, C.byref(a)) == 0 and a.value == sum(len(oracle(batch, s)["kept"]) for s in batch.sels)
    pl.close()


def test_the_single_call_and_the_batch_keep_their_own_state():
    case = SC.by_name()["sstar65"]
    batch = BC.of_case(case)
    pl = placer(batch)
    L, h = pl._L, pl._h
    few, every = case.sels[0], case.sels[1]
    everyone = np.arange(int(case.arrays["n"]), dtype=np.uint32)
    a = C.c_uint64(0)
    # single, then batch: the single call's entries and owners still answer for `every`
    want = oracle(batch, every)
    got = pl.subtree_nodes(every)
    check(batch, pl.subtree_batch(batch.sels))
    pos = np.zeros(len(want["pos"]), np.int32)
    first, nuc = np.zeros(len(pos), np.uint32), np.zeros(len(pos), np.uint8)
    assert L.ugp_subtree_entries(h, _ptr(pos), _ptr(first), _ptr(nuc), len(pos), C.byref(a)) == 0 and a.value == len(pos)
    got.update(pos=pos, first_entry=first, nuc=nuc)
    assert R.same(got, want, pl.subtree_owner(everyone))
    # batch, then single: the batch's lists still answer for the batch
    one = pl.subtree_batch([few, every])
    assert R.same(pl.subtree_nodes(few), oracle(batch, few), pl.subtree_owner(everyone))
    nk = len(oracle(batch, few)["kept"]) + len(want["kept"])
    kept, par, ent = np.zeros(nk, np.uint32), np.zeros(nk, np.uint32), np.zeros(nk, np.uint64)
    assert L.ugp_subtree_batch_nodes(h, _ptr(kept), _ptr(par), _ptr(ent), nk, C.byref(a)) == 0 and a.value == nk
    assert kept.tolist() == one[0]["kept"].tolist() + one[1]["kept"].tolist() == oracle(batch, few)["kept"].tolist() + want["kept"].tolist()
    assert L.ugp_subtree_batch_entries(h, None, None, None, 0, C.byref(a)) == 0 and a.value == len(oracle(batch, few)["pos"]) + len(want["pos"])
    pl.subtree_attach(case.arrays)   # a second attach drops both
    assert L.ugp_subtree_batch_nodes(h, None, None, None, 0, C.byref(a)) == -1
    pl.close()
