"""ugp_translate (Placer.translate) against the literal restatement of matUtils translate (tests/translate_ref.py) on every hand-shaped
case of tests/translate_cases.py, exactly: records and counts where the closed form holds, the refusal with its counts and first
offender where it does not; the launch windows of ugp_translate_chunked, the cap / n_out protocol, the error codes, a second codon
table, and `matutils-amd translate` on the device byte for byte against its own --host output."""
import ctypes as C

import numpy as np
import pytest

from tests import summary_cases as SC
from tests import test_summary_cpu as SCPU
from tests import test_translate_cpu as CPU
from tests import translate_cases as TC
from tests import translate_ref as R
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu
CASES = TC.all_cases()
REFERENCE = {}      # case name -> (records, info), computed once


def reference(case):
    if case.name not in REFERENCE:
        T, codons = case.tree(), case.codons()
        REFERENCE[case.name] = (R.records(T, codons) if case.device else None, R.info(T, codons))
    return REFERENCE[case.name]


def placer(case):
    pl = Placer(SC.topology(case.arrays))
    pl.translate_attach(case.arrays)
    pl.translate_codons(*R.slot_tables(case.codons()))
    return pl


def as_dict(info):
    return {k: int(info[k]) for k in info.dtype.names}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_cases(case):
    want, info = reference(case)
    pl = placer(case)
    if case.device:
        recs, got = pl.translate()
        assert R.device_records(recs) == want
        assert as_dict(got) == info and (recs["pad"] == 0).all()
    else:
        with pytest.raises(UgpError) as e:
            pl.translate()
        assert e.value.code == -2 and as_dict(pl._tr_info) == info
        # nothing is written, whatever room there is
        buf = np.full(8, 0xA5, np.uint8).repeat(Placer.TR_RECORD.itemsize).view(Placer.TR_RECORD)
        n_out, raw = C.c_uint64(7), np.zeros(1, Placer.TR_INFO)
        assert pl._L.ugp_translate(pl._h, _ptr(buf), 8, C.byref(n_out), _ptr(raw)) == -2
        assert n_out.value == 0 and (buf.view(np.uint8) == 0xA5).all() and as_dict(raw[0]) == info
        assert pl._L.ugp_translate(pl._h, None, 0, C.byref(n_out), None) == -2          # info may be NULL
    pl.close()


@pytest.mark.parametrize("name", TC.WINDOW_CASES)
def test_launch_windows(name):
    case = TC.by_name()[name]
    want, info = reference(case)
    m = TC.n_items(case)
    assert m > 2
    pl = placer(case)
    for w in (1, 2, m - 1, m, m + 1, 0):
        recs, got = pl.translate(chunk_items=w)
        assert R.device_records(recs) == want and as_dict(got) == info, w
    pl.close()


def test_refusal_in_a_late_window():
    case = TC.by_name()["inconsistent_par"]
    _, info = reference(case)
    pl = placer(case)
    for w in (1, 2, 0):
        with pytest.raises(UgpError) as e:
            pl.translate(chunk_items=w)
        assert e.value.code == -2 and as_dict(pl._tr_info) == info, w
    pl.close()


def test_cap_protocol():
    case = TC.by_name()["wide65"]
    pl = placer(case)
    full, info = pl.translate()
    n = len(full)
    assert n > 3
    n_out = C.c_uint64(0)
    assert pl._L.ugp_translate(pl._h, None, 0, C.byref(n_out), None) == 0 and n_out.value == n          # cap = 0: the count alone
    for cap in (n - 1, n, n + 2):
        buf = np.full(n + 2, 0xA5, np.uint8).repeat(Placer.TR_RECORD.itemsize).view(Placer.TR_RECORD)
        n_out = C.c_uint64(0)
        assert pl._L.ugp_translate(pl._h, _ptr(buf), cap, C.byref(n_out), None) == 0 and n_out.value == n
        k = min(cap, n)
        assert buf[:k].tobytes() == full[:k].tobytes() and (buf[k:].view(np.uint8) == 0xA5).all(), cap
    part, _ = pl.translate(cap=2, chunk_items=3)
    assert len(part) == 2 and pl._tr_n_out == n and part.tobytes() == full[:2].tobytes()
    assert pl._L.ugp_translate(pl._h, None, 3, C.byref(n_out), None) == -1
    pl.close()


def test_error_codes_and_a_second_table():
    case = TC.by_name()["two_frames"]
    pos, init = R.slot_tables(case.codons())
    pl = Placer(SC.topology(case.arrays))
    n_out = C.c_uint64(7)
    assert pl._L.ugp_translate(pl._h, None, 0, C.byref(n_out), None) == -1 and b"ugp_translate_attach" in pl._L.ugp_last_error()
    assert pl._L.ugp_translate_codons(pl._h, len(pos), _ptr(pos), _ptr(init)) == -1 and b"ugp_translate_attach" in pl._L.ugp_last_error()
    assert n_out.value == 7
    bad = dict(case.arrays)
    bad["mut_par"] = np.zeros_like(case.arrays["mut_par"])
    with pytest.raises(UgpError) as e:
        pl.translate_attach(bad)
    assert e.value.code == -2
    pl.translate_attach(case.arrays)
    assert pl._L.ugp_translate(pl._h, None, 0, C.byref(n_out), None) == -1 and b"ugp_translate_codons" in pl._L.ugp_last_error()
    for row, col, value in ((0, 0, 0), (3, 1, -5), (2, 2, int(pos[2, 0])), (1, 0, 1 << 28)):
        wrong = pos.copy()
        wrong[row, col] = value
        with pytest.raises(UgpError) as e:
            pl.translate_codons(wrong, init)
        assert e.value.code == -1, (row, col, value)
    assert pl._L.ugp_translate(pl._h, None, 0, C.byref(n_out), None) == -1       # a refused table is no table
    # the whole table, then gene C alone, then no codon at all, then the whole table again
    want = R.records(case.tree(), case.codons())
    pl.translate_codons(pos, init)
    assert R.device_records(pl.translate()[0]) == want
    pl.translate_codons(pos[22:], init[22:])
    recs, info = pl.translate()
    assert R.device_records(recs) == [(n, c - 22, b, a, e) for n, c, b, a, e in want if c >= 22] and int(info["n_records"]) == 1
    pl.translate_codons(pos[:0], init[:0])
    recs, info = pl.translate()
    assert len(recs) == 0 and as_dict(info)["n_nodes"] == 0
    pl.translate_codons(pos, init.tobytes())
    assert R.device_records(pl.translate()[0]) == want
    # tables built from other arrays are refused, the state stays
    other = dict(case.arrays)
    other["mut_pos"] = np.asarray(case.arrays["mut_pos"]) + 1
    with pytest.raises(UgpError) as e:
        pl.translate_attach(other)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    assert R.device_records(pl.translate()[0]) == want
    pl.close()


def test_shared_tables():
    """A handle made from the tree's own arrays attaches by itself, beside the other users of the depth-first tables."""
    from tests import summary_ref as SR
    from tests import synth
    arrays = synth.make_case(2, n_leaves=250, n_queries=1, n_sites=60, genome_len=500)[0]
    genome = np.array(list("ACGT"))[np.random.default_rng(3).integers(0, 4, 500)]
    genome[np.asarray(arrays["mut_pos"]).astype(np.int64) - 1] = np.array(list(SR.NUC))[np.asarray(arrays["mut_ref"]).astype(np.int64)]
    gtf = TC.gtf_line("a", 1, 300) + "\n" + TC.gtf_line("b", 200, 499) + "\n"
    codons = R.build_codon_map(gtf, "".join(genome))
    T = SR.Tree(arrays)
    want, winfo = R.records(T, codons), R.info(T, codons)
    assert len(want) > 100 and winfo["n_inconsistent"] == 0
    pl = Placer(arrays)
    pl.nearest_k([3], 2)
    pl.translate_codons(*R.slot_tables(codons))          # attaches on the first call
    recs, info = pl.translate()
    assert R.device_records(recs) == want and as_dict(info) == winfo
    assert pl.translate_time(2) > 0
    pl.close()


@pytest.mark.parametrize("name", ["survey"] + [c.name for c in CASES])
def test_cli_device_against_host(name, tmp_path):
    if name == "survey":
        T, codons, gtf, fa = CPU.survey_inputs(tmp_path)
        pb = CPU.SURVEY_PB
    else:
        case = TC.by_name()[name]
        pb, gtf, fa = CPU.write_inputs(case, tmp_path)
        T, codons = SCPU.load_model(pb)[0], case.codons()
    args = ["-i", pb, "-g", gtf, "-f", fa, "-t", "t.tsv"]
    dev = CPU.run(args + ["-d", tmp_path / "dev"])
    host = CPU.run(args + ["-d", tmp_path / "host", "--host"])
    assert open(tmp_path / "dev" / "t.tsv", "rb").read() == open(tmp_path / "host" / "t.tsv", "rb").read()
    # the note about the fallback: there exactly when the tree as loaded is one the device refuses
    info = R.info(T, codons)
    refused = info["n_inconsistent"] or info["n_duplicate"]
    note = [line for line in dev.stderr.split("\n") if "walking it on the host" in line]
    assert len(note) == (1 if refused else 0), dev.stderr
    if refused:
        assert "%d inconsistent" % info["n_inconsistent"] in note[0] and "%d nodes" % info["n_duplicate"] in note[0]
        if info["n_inconsistent"]:
            node = int(np.searchsorted(np.asarray(T.arrays["mut_off"]), info["first_inconsistent"], side="right")) - 1
            assert "(first: %s on %s)" % (T.mstr[info["first_inconsistent"]], T.names[node]) in note[0]
    assert "walking" not in host.stderr
    if name in ("survey", "minus_ordinary", "inconsistent_par"):
        assert refused
    if name in ("single_slots", "minus_consistent", "caterpillar", "wide65"):
        assert not refused
