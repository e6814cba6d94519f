"""ugp_summary_mutations / _roho / _clades (Placer.summary_*) against the literal restatement of matUtils summary
(tests/summary_ref.py) on every hand-shaped case of tests/summary_cases.py, exactly; the launch windows of the _chunked twins, the
cap / n_out protocol, the error codes, and `matutils-amd summarize` on the device byte for byte against its own --host output."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import summary_cases as SC
from tests import summary_ref as R
from tests import test_summary_cpu as CPU
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu


def placer(arrays):
    pl = Placer(SC.topology(arrays))
    pl.summary_attach(arrays)
    return pl


def mutation_rows(recs):
    return [(int(r["pos"]), int(r["par"]), int(r["nuc"]), int(r["count"])) for r in recs]


def check_clades(pl, T, columns):
    per, leaf_clade = pl.summary_clades(columns)
    want = R.clade_records(T, columns)
    assert leaf_clade.shape == (len(columns), len(T.leaves()))
    at = 0
    for c, (incl, excl, near) in enumerate(want):
        rows = per[at:at + len(columns[c])]
        at += len(columns[c])
        assert rows["column"].tolist() == [c] * len(rows) and rows["node"].tolist() == list(columns[c])
        assert rows["inclusive"].tolist() == incl and rows["exclusive"].tolist() == excl
        assert leaf_clade[c].tolist() == near
    assert at == len(per)


@pytest.mark.parametrize("case", SC.all_cases(), ids=repr)
def test_cases(case):
    T = R.Tree(case.arrays, case.ann)
    pl = placer(case.arrays)
    assert mutation_rows(pl.summary_mutations()) == R.mutation_records(T)
    assert R.device_roho(T, pl.summary_roho()) == R.roho_records(T)
    cols = SC.columns(case)
    check_clades(pl, T, cols)
    check_clades(pl, T, cols[::-1] + [[], list(range(case.arrays["n"]))])   # an empty column, every node listed
    pl.close()


@pytest.mark.parametrize("name", ["wide65", "caterpillar", "star600", "later_child_owns"])
def test_launch_windows(name):
    case = {c.name: c for c in SC.all_cases()}[name]
    T = R.Tree(case.arrays, case.ann)
    pl = placer(case.arrays)
    want_m, want_r = R.mutation_records(T), R.roho_records(T)
    m, nc = len(case.arrays["mut_pos"]), SC.n_candidates(case.arrays)
    assert m > 2 and (nc > 2 or name == "star600")     # (the star has no non-leaf child: its 601 entries are for the mutation table)
    for w in (1, 2, m - 1, m, m + 1, 0):
        assert mutation_rows(pl.summary_mutations(chunk_items=w)) == want_m, w
    for w in sorted({1, 2, max(nc - 1, 1), max(nc, 1), nc + 1, 0}):
        assert R.device_roho(T, pl.summary_roho(chunk_items=w)) == want_r, w
    pl.close()


def test_cap_protocol():
    case = {c.name: c for c in SC.all_cases()}["wide65"]
    T = R.Tree(case.arrays, case.ann)
    pl = placer(case.arrays)
    full_m, full_r = pl.summary_mutations(), pl.summary_roho()
    for fn, full, dtype in ((pl._L.ugp_summary_mutations, full_m, Placer.SM_MUTATION), (pl._L.ugp_summary_roho, full_r, Placer.SM_ROHO)):
        n = len(full)
        assert n > 3
        n_out = C.c_uint64(0)
        assert fn(pl._h, None, 0, C.byref(n_out)) == 0 and n_out.value == n          # cap = 0: the count alone
        for cap in (n - 1, n, n + 2):
            buf = np.full(n + 2, 0xA5, np.uint8).repeat(dtype.itemsize).view(dtype)
            n_out = C.c_uint64(0)
            assert fn(pl._h, _ptr(buf), cap, C.byref(n_out)) == 0 and n_out.value == n
            k = min(cap, n)
            assert buf[:k].tobytes() == full[:k].tobytes() and (buf[k:].view(np.uint8) == 0xA5).all(), cap
    assert len(pl.summary_roho(cap=2, chunk_items=3)) == 2 and pl._sm_n_out == len(full_r)
    pl.close()


def test_plain_handle_and_shared_tables():
    """A handle made from the tree's own arrays attaches by itself, beside the other users of the depth-first tables."""
    from tests import synth
    arrays = synth.make_case(2, n_leaves=250, n_queries=1, n_sites=60, genome_len=500)[0]
    T, F = R.Tree(arrays), R.Fast(arrays)
    pl = Placer(arrays)
    pl.nearest_k([3], 2)
    assert mutation_rows(pl.summary_mutations()) == F.mutations()
    assert R.device_roho_fast(F, pl.summary_roho()) == F.roho()[0]
    check_clades(pl, T, CPU.random_columns(arrays, 11))
    other = dict(arrays)
    other["mut_pos"] = np.asarray(arrays["mut_pos"]) + 1
    with pytest.raises(UgpError) as e:
        pl.summary_attach(other)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    assert mutation_rows(pl.summary_mutations()) == F.mutations()        # the state stayed
    pl.close()


def test_error_codes():
    case = SC.roho_cases()[0]
    pl = Placer(SC.topology(case.arrays))
    n_out = C.c_uint64(7)
    buf = np.zeros(4, Placer.SM_ROHO)
    assert pl._L.ugp_summary_roho(pl._h, _ptr(buf), 4, C.byref(n_out)) == -1 and b"ugp_summary_attach" in pl._L.ugp_last_error()
    assert pl._L.ugp_summary_mutations(pl._h, None, 0, C.byref(n_out)) == -1 and n_out.value == 7
    bad = dict(case.arrays)
    bad["mut_par"] = np.zeros_like(case.arrays["mut_par"])
    with pytest.raises(UgpError) as e:
        pl.summary_attach(bad)
    assert e.value.code == -2
    pl.summary_attach(case.arrays)
    with pytest.raises(UgpError) as e:
        pl.summary_clades([[1, 1]])
    assert e.value.code == -1
    with pytest.raises(UgpError) as e:
        pl.summary_clades([[case.arrays["n"]]])
    assert e.value.code == -1
    assert pl._L.ugp_summary_roho(pl._h, None, 3, C.byref(n_out)) == -1
    pl.close()


@pytest.mark.parametrize("name", ["survey", "annotated"] + CPU.CLI_CASES)
def test_cli_device_against_host(name, tmp_path):
    if name == "survey":
        pb = CPU.SURVEY_PB
    elif name == "annotated":
        pb = CPU.ANNOTATED_PB
    else:
        pb = CPU.write_annotated({c.name: c for c in SC.all_cases()}[name], tmp_path / "case.pb")
    args = ["-i", pb, "-A", "-R", "roho.tsv", "-C", "sample-clades.tsv"]
    CPU.run(args + ["-d", tmp_path / "dev"])
    CPU.run(args + ["-d", tmp_path / "host", "--host"])
    for f in CPU.TABLES:
        assert open(tmp_path / "dev" / f, "rb").read() == open(tmp_path / "host" / f, "rb").read(), f
    assert sorted(os.listdir(tmp_path / "dev")) == sorted(CPU.TABLES)
