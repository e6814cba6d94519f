"""The ugp_mask calls (Placer.mask_*) against the literal restatement of tests/mask_ref.py on every hand-shaped case of
tests/mask_cases.py, exactly -- roots, masked entries, first lines and counts; the line batches of the _chunked hook, `skip`, a
named internal node, the attach order with select and summary on one handle, the error codes, and `matutils-amd mask` on the
device byte for byte against its own --host output."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import refio
from tests import mask_cases as MC
from tests import mask_ref as R
from tests import select_cases as SC
from tests import select_ref as SR
from tests import summary_cases as SMC
from tests import test_mask_cpu as CPU
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu
CASES = MC.all_cases()
reference, same = CPU.reference, CPU.same


def placer(case):
    pl = Placer(SMC.topology(case.arrays))
    pl.mask_attach(case.arrays)
    return pl


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_cases(case):
    ref = reference(case)
    pl = placer(case)
    for s, want in ref["sets"]:
        got = pl.mask_restricted(s)
        assert same(got, want) and pl._msk_n_masked == int(want[1].sum()), s[:20]
    cols = MC.line_arrays(ref["lines"])
    assert same(pl.mask_mutations(*cols), ref["mutations"])
    assert same(pl.mask_mutations(*cols, skip=ref["skip"]), ref["skipped"])
    fast = R.Fast(case.arrays)   # (held against the literal walk, line by line, by tests/test_mask_cpu.py)
    for l in range(0, len(ref["lines"]), 7):   # single lines
        one = ref["lines"][l:l + 1]
        want = R.literal_mutations(case.arrays, one) if case.arrays["n"] <= 2000 else fast.mutations(one)
        assert same(pl.mask_mutations(*MC.line_arrays(one)), want), l
    pl.close()


@pytest.mark.parametrize("name", ["polytomy", "mstar129", "two_at_one", "mcaterpillar"])
def test_line_batches(name):
    case = MC.by_name()[name]
    ref = reference(case)
    pl = placer(case)
    cols = MC.line_arrays(ref["lines"])
    m = len(ref["lines"])
    for chunk in (1, 2, m - 1, m, m + 1, 0):
        assert same(pl.mask_mutations(*cols, chunk_lines=chunk), ref["mutations"]), chunk
        assert same(pl.mask_mutations(*cols, skip=ref["skip"], chunk_lines=chunk), ref["skipped"]), chunk
    first, counts = pl.mask_mutations([], [], [], [], [])   # no line: nothing matches
    assert (first == R.NIL).all() and len(counts) == 0
    everything = np.ones(len(first), np.uint8)
    first, counts = pl.mask_mutations(*cols, skip=everything)
    assert (first == R.NIL).all() and not counts.any()
    t_r, t_m = pl.mask_time(ref["sets"][0][0], *cols, reps=2)
    assert t_r > 0 and t_m > 0
    assert pl.mask_time(None, *cols, reps=1)[0] == 0 and pl.mask_time(ref["sets"][0][0], reps=1)[1] == 0
    pl.close()


def test_named_internal_node_is_unsupported():
    case = MC.by_name()["nested_full"]
    pl = placer(case)
    _, lv, kids = MC.tables(case.arrays)
    for named in ([case.tags["mid"]], lv + [case.tags["deep"]], [0]):
        with pytest.raises(UgpError) as e:
            pl.mask_restricted(named)
        assert e.value.code == -2 and "not a leaf" in str(e.value), named
    assert same(pl.mask_restricted(lv), R.literal_restricted(case.arrays, lv))   # the state is as it was
    pl.close()


def test_attach_order_with_select_and_summary():
    case = MC.by_name()["masked_before"]
    ref = reference(case)
    cols = MC.line_arrays(ref["lines"])
    pos, nuc = SC.queries(case.arrays)
    want_sel = SR.literal_mutations(SR.tree_from_arrays(case.arrays), pos, nuc)
    answers = []
    for order in (("mask", "select", "summary"), ("select", "summary", "mask"), ("summary", "mask", "select")):
        pl = Placer(SMC.topology(case.arrays))
        for what in order:
            getattr(pl, what + "_attach")(case.arrays)
        for s, want in ref["sets"]:
            assert same(pl.mask_restricted(s), want), order
        assert same(pl.mask_mutations(*cols), ref["mutations"]), order
        assert same(pl.select_mutations(pos, nuc), want_sel), order
        answers.append(pl.summary_mutations().tobytes())
        pl.mask_attach(case.arrays)                    # a second attach replaces the first
        assert same(pl.mask_mutations(*cols, skip=ref["skip"]), ref["skipped"]), order
        pl.close()
    assert answers[0] == answers[1] == answers[2] and len(answers[0]) > 0


def test_other_arrays_are_refused_and_error_codes():
    case = MC.by_name()["polytomy"]
    ref = reference(case)
    cols = MC.line_arrays(ref["lines"])
    pl = Placer(SMC.topology(case.arrays))
    L, h = pl._L, pl._h
    n, m = int(case.arrays["n"]), len(case.arrays["mut_pos"])
    leaves = np.asarray(MC.tables(case.arrays)[1], np.uint32)
    masked, roots = np.full(m, 0xA5, np.uint8), np.full(len(leaves), 7, np.uint32)
    nr, nm, ms = C.c_uint64(7), C.c_uint64(7), C.c_double(0)
    pos, par, nuc, node = np.asarray([4], np.int32), np.asarray([15], np.uint8), np.asarray([15], np.uint8), np.asarray([0], np.uint32)
    off, first, counts = np.zeros(2, np.uint64), np.full(m, 0xA5A5A5A5, np.uint32), np.zeros(1, np.uint64)

    def restricted(k=len(leaves), lv=leaves, em=masked, rb=roots, cap=len(roots), a=nr, b=nm):
        return L.ugp_mask_restricted(h, k, _ptr(lv) if lv is not None else None, _ptr(em) if em is not None else None,
                                     _ptr(rb) if rb is not None else None, cap, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None)

    def mutations(k=1, p=pos, a=par, b=nuc, t=node, o=off, f=first, c=counts):
        q = lambda x: _ptr(x) if x is not None else None
        return L.ugp_mask_mutations(h, k, q(p), q(a), q(b), q(t), q(o), None, None, q(f), q(c))

    # before the attach
    assert restricted() == -1 and b"ugp_mask_attach" in L.ugp_last_error()
    assert mutations() == -1 and b"ugp_mask_attach" in L.ugp_last_error()
    assert L.ugp_mask_time(h, 0, None, 0, None, None, None, None, None, None, 1, C.byref(ms), C.byref(ms)) == -1
    pl.mask_attach(case.arrays)
    # tables built from other arrays are refused, the state stays
    other = dict(case.arrays)
    other["mut_pos"] = np.asarray(case.arrays["mut_pos"]) + 1
    with pytest.raises(UgpError) as e:
        pl.mask_attach(other)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    assert same(pl.mask_mutations(*cols), ref["mutations"])
    # an allele above 15 is unsupported
    wide = dict(case.arrays)
    wide["mut_nuc"] = np.asarray(case.arrays["mut_nuc"]).copy()
    wide["mut_nuc"][0] = 16
    pl2 = Placer(SMC.topology(case.arrays))
    with pytest.raises(UgpError) as e:
        pl2.mask_attach(wide)
    assert e.value.code == -2
    pl2.close()
    # no names, a node out of range (nothing is written), null pointers
    assert restricted(k=0) == -1 and restricted(lv=None) == -1
    bad = leaves.copy()
    bad[-1] = n
    assert restricted(lv=bad) == -1 and b"out of range" in L.ugp_last_error() and (masked == 0xA5).all() and (roots == 7).all() and nr.value == 7
    assert restricted(em=None) == -1 and restricted(rb=None) == -1 and restricted(a=None) == -1 and restricted(b=None) == -1
    assert restricted(rb=None, cap=0) == 0 and nr.value == len(ref_roots(case, leaves)) and (masked != 0xA5).all()
    some = np.ascontiguousarray(leaves[::2])
    want = ref_roots(case, some)
    assert len(want) > 1 and restricted(k=len(some), lv=some, cap=1) == 0 and nr.value == len(want) and roots[0] == want[0] and roots[1] == 7
    # lines: null pointers, a node out of range, an allele above 15, offsets that do not ascend
    assert mutations(p=None) == -1 and mutations(a=None) == -1 and mutations(b=None) == -1 and mutations(t=None) == -1 and mutations(o=None) == -1
    assert mutations(f=None) == -1 and mutations(c=None) == -1
    assert mutations(t=np.asarray([n], np.uint32)) == -1 and b"out of range" in L.ugp_last_error() and (first == 0xA5A5A5A5).all()
    assert mutations(a=np.asarray([16], np.uint8)) == -1 and mutations(b=np.asarray([16], np.uint8)) == -1
    assert mutations(o=np.asarray([1, 1], np.uint64)) == -1 and mutations(o=np.asarray([0, 1], np.uint64)) == -1   # an exclusion without a list
    assert (first == 0xA5A5A5A5).all()
    assert mutations() == 0 and counts[0] == (first == 0).sum() > 0
    assert L.ugp_mask_time(h, 0, None, 0, None, None, None, None, None, None, 0, C.byref(ms), C.byref(ms)) == -1
    pl.close()


def ref_roots(case, leaves):
    return R.literal_restricted(case.arrays, leaves)[0]


# ---- the command-line tool -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture():
    return CPU.Fixture()


def both_paths(tmp_path, pb, name, kw):
    """The option set on the device and with --host: the same exit code, contract lines and bytes."""
    out = {}
    for path in ("dev", "host"):
        files = {}
        if kw.get("samples") is not None:
            files["-s"] = ("s.txt", kw["samples"])
        if kw.get("mutations") is not None:
            files["-m"] = ("m.csv" if kw.get("csv") else "m.tsv", kw["mutations"])
        if kw.get("rename") is not None:
            files["-r"] = ("r.tsv", kw["rename"])
        paths = CPU.write_files(tmp_path, name, files)
        pbo = tmp_path / ("%s_%s.pb" % (name, path))
        args = ["-i", pb, "-o", pbo] + [x for k, p in paths.items() for x in (k, p)] + (["-c"] if kw.get("condense") else []) + \
            (["--host"] if path == "host" else [])
        r = CPU.run(args, ok=None)
        out[path] = (r.returncode, CPU.contract_lines(r.stderr), open(pbo, "rb").read() if os.path.exists(pbo) else None)
        if path == "dev":
            where = [l for l in r.stderr.split("\n") if l.startswith("Restricted samples on the")]
    assert out["dev"] == out["host"], name
    return out["dev"], where


@pytest.mark.parametrize("name", CPU.OPTION_SETS)
def test_cli_device_against_host(fixture, tmp_path, name):
    kw = fixture.option_sets()[name]
    (rc, log, data), where = both_paths(tmp_path, CPU.PB, name, kw)
    assert rc == 0 and data is not None and len(data) > 1000
    if "samples" in name:   # a named internal node walks on the host, with a message; leaves run on the device
        assert len(where) == 1 and ("on the host" in where[0]) == (name == "samples_internal"), where
    T = refio.load_mutation_annotated_tree(CPU.PB)   # and both against the restatement
    assert log == R.mask_main(T, kw.get("samples"), kw.get("mutations"), kw.get("csv", False), kw.get("rename"), kw.get("condense", False))


@pytest.mark.parametrize("name", ["two_at_one", "masked_before", "nested_full", "mstar65", "polytomy"])
def test_cli_device_against_host_on_hand_cases(tmp_path, name):
    case, pb, names = CPU.hand_pb(tmp_path, name)
    lines = [l for l in MC.lines(case.arrays) if l[0] > 0 and all(x < len(names) for x in l[4])]
    text = "".join("%s%d%s\t%s\t%s\n" % (refio.get_nuc(a), p, refio.get_nuc(b), names[t], ";".join(names[x] for x in ex)) for p, a, b, t, ex in lines)
    for k, s in enumerate(MC.leaf_sets(case.arrays)[:6]):
        (rc, log, data), _ = both_paths(tmp_path, pb, "%s_s%d" % (name, k), dict(samples="".join(names[v] + "\n" for v in s), mutations=text if k % 2 else None,
                                                                                   condense=k == 3))
        assert rc == 0 and data is not None
    (rc, log, data), _ = both_paths(tmp_path, pb, name + "_m", dict(mutations=text))
    assert rc == 0 and any(l.startswith("Masked a total of") for l in log)


def test_cli_errors_on_the_device_path(fixture, tmp_path):
    for name, kw in [("unknown_sample", dict(samples=fixture.leaves[0] + "\nno_such_sample\n")), ("empty_samples", dict(samples="")),
                     ("unknown_target", dict(mutations="%s\tno_such_node\n" % fixture.common[1])), ("bad_mutation", dict(mutations="11083T\n")),
                     ("empty_line", dict(mutations=fixture.common[0] + "\n\n"))]:
        (rc, log, data), _ = both_paths(tmp_path, CPU.PB, name, kw)
        assert rc == 1 and data is None and len(log) >= 1, name
