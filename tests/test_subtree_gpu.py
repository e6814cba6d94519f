"""The ugp_subtree calls (Placer.subtree_*) against tests/subtree_ref.py on every hand-shaped case of tests/subtree_cases.py, exactly --
kept nodes, subtree parents, offsets, merged entries, the info record and every node's owner; the launch windows of the _chunked
hook, the cap conventions, the error codes, a second selection on one handle, the attach order with select and mask, and
`matutils-amd subtree` on the device byte for byte against its own --host output."""
import ctypes as C

import numpy as np
import pytest

from tests import select_cases as SLC
from tests import select_ref as SR
from tests import subtree_cases as SC
from tests import subtree_ref as R
from tests import summary_cases as SMC
from tests import test_subtree_cpu as CPU
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu
CASES = SC.all_cases()


def placer(case):
    pl = Placer(SMC.topology(case.arrays))
    pl.subtree_attach(case.arrays)
    return pl


def oracle(case, sel):
    """The literal walk where it is quick, else the closed form (held against the literal walk by tests/test_subtree_cpu.py)."""
    return R.literal(case.arrays, sel) if len(sel) <= 70 else R.closed_form(case.arrays, sel)


def everyone(case):
    return np.arange(int(case.arrays["n"]), dtype=np.uint32)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_cases(case):
    pl = placer(case)
    for sel in case.sels:
        got = pl.subtree_nodes(sel)
        assert R.same(got, oracle(case, sel), pl.subtree_owner(everyone(case))), sel[:20]
    pl.close()


@pytest.mark.parametrize("name", ["all_leaves", "twice_on_one_node", "disagreement", "sstar65", "sstar257", "scaterpillar"])
def test_launch_windows(name):
    case = SC.by_name()[name]
    pl = placer(case)
    for sel in case.sels[:2]:
        want = oracle(case, sel)
        for chunk in (1, 2, 63, 0):
            assert R.same(pl.subtree_nodes(sel, chunk_items=chunk), want, pl.subtree_owner(everyone(case))), (sel[:20], chunk)
    a, b = pl.subtree_time(case.sels[0], reps=2)
    assert a > 0 and b > 0
    assert R.same(pl.subtree_nodes(case.sels[0]), oracle(case, case.sels[0]))   # the handle answers as before
    pl.close()


def test_cap_conventions_and_a_second_selection():
    case = SC.by_name()["sstar65"]
    pl = placer(case)
    few, every = case.sels[0], case.sels[1]
    want = oracle(case, every)
    nk, ne = len(want["kept"]), len(want["pos"])
    got = pl.subtree_nodes(every, cap=0)   # the counts are true, nothing is written
    assert got["n_kept"] == nk and got["n_entries"] == ne and len(got["kept"]) == 0 and len(got["pos"]) == 0
    L, h = pl._L, pl._h
    nodes = np.asarray(every, np.uint32)
    kept, par, off = np.full(nk, 7, np.uint32), np.full(nk, 7, np.uint32), np.full(nk, 7, np.uint64)
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert L.ugp_subtree_nodes(h, len(nodes), _ptr(nodes), _ptr(kept), _ptr(par), _ptr(off), 0, C.byref(a), C.byref(b), None) == 0
    assert (a.value, b.value) == (nk, ne) and (kept == 7).all() and (par == 7).all() and (off == 7).all()
    assert L.ugp_subtree_nodes(h, len(nodes), _ptr(nodes), _ptr(kept), _ptr(par), _ptr(off), 3, C.byref(a), C.byref(b), None) == 0
    assert (a.value, b.value) == (nk, ne) and kept[:3].tolist() == want["kept"][:3].tolist() and (kept[3:] == 7).all() and (off[3:] == 7).all()
    assert par[:3].tolist() == want["parent"][:3].tolist() and off[:3].tolist() == want["ent_off"][:3].tolist()
    pos, first, nuc = np.full(ne, 7, np.int32), np.full(ne, 7, np.uint32), np.full(ne, 7, np.uint8)
    assert L.ugp_subtree_entries(h, _ptr(pos), _ptr(first), _ptr(nuc), 2, C.byref(a)) == 0
    assert a.value == ne and pos[:2].tolist() == want["pos"][:2].tolist() and (pos[2:] == 7).all() and (first[2:] == 7).all() and (nuc[2:] == 7).all()
    assert L.ugp_subtree_entries(h, None, None, None, 0, C.byref(a)) == 0 and a.value == ne
    part = pl.subtree_nodes(every, cap=5)
    assert part["n_kept"] == nk and part["kept"].tolist() == want["kept"][:5].tolist() and part["pos"].tolist() == want["pos"][:5].tolist()
    # a second selection replaces the first for the entries and the owners
    assert R.same(pl.subtree_nodes(few), oracle(case, few), pl.subtree_owner(everyone(case)))
    assert L.ugp_subtree_entries(h, _ptr(pos), _ptr(first), _ptr(nuc), ne, C.byref(a)) == 0 and a.value == len(oracle(case, few)["pos"]) < ne
    assert R.same(pl.subtree_nodes(every), want, pl.subtree_owner(everyone(case)))
    pl.close()


def test_other_arrays_are_refused_and_error_codes():
    case = SC.by_name()["inner_selected"]
    sel = np.asarray(case.sels[0], np.uint32)
    n = int(case.arrays["n"])
    pl = Placer(SMC.topology(case.arrays))
    L, h = pl._L, pl._h
    kept, par, off = np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 7, np.uint64)
    a, b, ms = C.c_uint64(7), C.c_uint64(7), C.c_double(0)
    own = np.full(n, 7, np.uint32)

    def nodes(k=len(sel), s=sel, cap=n, na=a, nb=b, kb=kept):
        return L.ugp_subtree_nodes(h, k, _ptr(s) if s is not None else None, _ptr(kb) if kb is not None else None, _ptr(par), _ptr(off), cap,
                                   C.byref(na) if na is not None else None, C.byref(nb) if nb is not None else None, None)

    # before the attach: every call names the missing one
    assert nodes() == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    assert L.ugp_subtree_entries(h, None, None, None, 0, C.byref(a)) == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    assert L.ugp_subtree_owner(h, len(sel), _ptr(sel), _ptr(own)) == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    assert L.ugp_subtree_time(h, len(sel), _ptr(sel), 1, C.byref(ms), C.byref(ms)) == -1 and b"ugp_subtree_attach" in L.ugp_last_error()
    pl.subtree_attach(case.arrays)
    # after the attach and before a selection: the entries and the owners name the missing call
    assert L.ugp_subtree_entries(h, None, None, None, 0, C.byref(a)) == -1 and b"ugp_subtree_nodes" in L.ugp_last_error()
    assert L.ugp_subtree_owner(h, len(sel), _ptr(sel), _ptr(own)) == -1 and b"ugp_subtree_nodes" in L.ugp_last_error()
    want = R.literal(case.arrays, sel)
    assert R.same(pl.subtree_nodes(sel), want)
    # tables built from other arrays are refused, the state stays
    other = dict(case.arrays)
    other["mut_pos"] = np.asarray(case.arrays["mut_pos"]) + 1
    with pytest.raises(UgpError) as e:
        pl.subtree_attach(other)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    assert R.same(pl.subtree_nodes(sel), want)
    # an allele above 15 is unsupported
    wide = dict(case.arrays)
    wide["mut_nuc"] = np.asarray(case.arrays["mut_nuc"]).copy()
    wide["mut_nuc"][0] = 16
    pl2 = Placer(SMC.topology(case.arrays))
    with pytest.raises(UgpError) as e:
        pl2.subtree_attach(wide)
    assert e.value.code == -2
    pl2.close()
    # no names, a node out of range (nothing is written), null pointers
    a.value = b.value = 7
    assert nodes(k=0) == -1 and nodes(s=None) == -1
    bad = sel.copy()
    bad[-1] = n
    assert nodes(s=bad) == -1 and b"out of range" in L.ugp_last_error() and (kept == 7).all() and (par == 7).all() and (off == 7).all()
    assert a.value == 7 and b.value == 7
    assert nodes(na=None) == -1 and nodes(nb=None) == -1 and nodes(kb=None) == -1 and nodes(kb=None, cap=0) == 0
    assert L.ugp_subtree_owner(h, 0, _ptr(sel), _ptr(own)) == -1 and L.ugp_subtree_owner(h, len(bad), _ptr(bad), _ptr(own)) == -1
    assert (own == 7).all() and L.ugp_subtree_owner(h, len(sel), _ptr(sel), None) == -1
    assert L.ugp_subtree_entries(h, None, None, None, 1, C.byref(a)) == -1 and L.ugp_subtree_entries(h, None, None, None, 0, None) == -1
    assert L.ugp_subtree_time(h, len(sel), _ptr(sel), 0, C.byref(ms), C.byref(ms)) == -1
    assert R.same(pl.subtree_nodes(sel), want, pl.subtree_owner(everyone(case)))   # the state is as it was
    pl.close()


def test_attach_order_with_select_and_mask():
    case = SC.by_name()["one_masked"]
    big = SC.by_name()["scaterpillar"]
    for case in (case, big):
        pos, nuc = SLC.queries(case.arrays)
        want_sel = SR.literal_mutations(SR.tree_from_arrays(case.arrays), pos, nuc)
        want = [oracle(case, s) for s in case.sels]
        for order in (("subtree", "select", "mask"), ("select", "mask", "subtree"), ("mask", "subtree", "select")):
            pl = Placer(SMC.topology(case.arrays))
            for what in order:
                getattr(pl, what + "_attach")(case.arrays)
            for s, w in zip(case.sels, want):
                assert R.same(pl.subtree_nodes(s), w, pl.subtree_owner(everyone(case))), order
            mask, counts = pl.select_mutations(pos, nuc)
            assert np.array_equal(mask, want_sel[0]) and np.array_equal(counts, want_sel[1]), order
            pl.subtree_attach(case.arrays)                    # a second attach replaces the first
            assert R.same(pl.subtree_nodes(case.sels[0]), want[0]), order
            pl.close()


# ---- the command-line tool -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    return CPU.SEL.Model()


def both_paths(tmp_path, name, pb, opts):
    dev, dwarn, r = CPU.outputs(tmp_path, name + "_dev", "subtree", pb, opts, extra=())
    host, hwarn, _ = CPU.outputs(tmp_path, name + "_host", "subtree", pb, opts)
    return dev, host, r


def test_cli_device_against_host_on_the_fixture(model, tmp_path):
    ran = 0
    for name, opts, _ in CPU.SEL.option_sets(model):
        dev, host, r = both_paths(tmp_path, name, CPU.PB, opts)
        assert dev == host, (name, r.stderr[-800:])
        if isinstance(dev, dict) and "Extracting subtree" in r.stderr:
            ran += 1
            assert "Selection step subtree (device): " in r.stderr, name
    assert ran >= 8
    rng = np.random.default_rng(5)   # a sample file with internal nodes among the names
    T = model.T
    inner = [n.identifier for n in T.depth_first_expansion() if not n.is_leaf()]
    some = [model.leaves[i] for i in rng.permutation(len(model.leaves))[:150]] + [inner[i] for i in rng.permutation(len(inner))[:10]]
    (tmp_path / "some.txt").write_text("".join(s + "\n" for s in some))
    dev, host, r = both_paths(tmp_path, "some", CPU.PB, ["-s", tmp_path / "some.txt"])
    assert isinstance(dev, dict) and dev == host, r.stderr[-800:]


@pytest.mark.parametrize("name", CPU.HAND_CLI)
def test_cli_device_against_host_on_hand_cases(tmp_path, name):
    case = SC.by_name()[name]
    pb, names = CPU.hand_pb(tmp_path, case)
    for k, sel in enumerate(case.sels[:3]):
        (tmp_path / ("s%d.txt" % k)).write_text("".join(names[v] + "\n" for v in sel))
        dev, host, r = both_paths(tmp_path, "%s_%d" % (name, k), pb, ["-s", tmp_path / ("s%d.txt" % k)])
        assert isinstance(dev, dict) and dev == host, (name, k, r.stderr[-800:])
        assert ("consecutive mutations at one position disagree" in r.stderr) == (name == "disagreement" and k < 2), (name, k)
