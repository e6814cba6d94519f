"""The cases of tests/touched_cases.py are what their names claim -- in the ORACLE's own answers -- and the plain restatement of the
record scoring (tests/touched_ref.py) equals the oracle on every one of them.  No GPU, no device library."""
import functools

import pytest

from tests import touched_cases as TC
from tests import touched_ref as TR

INT_MAX = TC.INT_MAX


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("ties"):
        return TC.ties_case(int(name[4:]))
    return {"entry_batches": TC.entry_case, "values": TC.values_case, "running": TC.running_case}[name]()


NAMES = ["entry_batches", "ties63", "ties64", "ties65", "ties200", "values", "running"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle(name):
    c = case(name)
    recs = [c.record(r) for r in range(c.n_rec)]
    prefixes = [range(c.first_id(g + 1)) for g in range(len(c.groups))]
    for live in prefixes:
        got = TR.place(recs, c.samples, live)
        for q, s in enumerate(c.samples):
            best, nb, ties = c.oracle(s, live)
            assert got[q] == (best, ties) and nb == len(ties), (name, q)


def test_restatement_equals_the_oracle_record_by_record():
    c = case("entry_batches")
    n_elig = 0
    for r in range(c.n_rec):
        rec = c.record(r)
        for q, s in enumerate(c.samples):
            v = TR.score_record(rec, s)
            best, nb, ties = c.oracle(s, [r])
            assert (best, nb, ties) == ((v["cost"], 1, {r: v["has_unique"]}) if v["elig"] else (INT_MAX, 0, {})), (r, q)
            n_elig += v["elig"]
    assert n_elig > c.n_rec * len(c.samples) // 2


def test_entry_batches_case_is_what_it_claims():
    c = case("entry_batches")
    assert c.n_rec == 31 and len(c.samples) == 65
    for (n_path, n_own), r in c.cells.items():
        rec = c.record(r)
        assert (len(rec["path"]), len(rec["own"])) == (n_path, n_own)
    assert set(c.cells) == {(p, o) for p in TC.ENTRY_PATH for o in TC.ENTRY_OWN} | {(23, 17)}
    n_all = [len(c.record(r)["path"]) + len(c.record(r)["own"]) for r in range(c.n_rec)]
    at_min = set()
    for s in c.samples:
        at_min.update(n_all[r] for r in c.oracle(s, range(c.n_rec))[2])
    assert set(TC.ENTRY_N_ALL) <= at_min, sorted(at_min)
    # a switch k < n_path inside an unrolled group of eight, and at its edges
    assert {(len(c.record(r)["path"]) % 8) for r in range(c.n_rec)} >= {0, 1, 7}
    # positions beyond the table: the ninth path entry of P(9)'s children, the last own mutation from eight on
    n_pos = c.n_pos()
    assert n_pos == 52
    for (n_path, n_own), r in c.cells.items():
        path_far, own_far = c.beyond(r)
        assert path_far == ([TC.FAR + 10] if n_path == 9 else []) and own_far == ([TC.FAR + n_own - 1] if n_own >= 8 else []), (n_path, n_own)
    # own mutations at a position of the parent's state: prev is that state; to a third base and back to the reference base
    kinds = set()
    for r in range(c.n_rec):
        rec = c.record(r)
        state = {p: s for p, s, _ in rec["path"]}
        for p, al, prev, ref in rec["own"]:
            if p in state:
                assert prev == state[p] != ref
                kinds.add("back" if al == ref else "third")
            else:
                assert prev == ref != al
    assert kinds == {"back", "third"}
    # the samples' rows at record positions hit, miss, are ambiguous and are missing
    seen = set()
    for s in c.samples:
        rows = {int(p): (int(n), int(m)) for p, n, m in zip(s["pos"], s["nuc"], s["is_missing"])}
        for r in range(c.n_rec):
            for p, al, _, _ in c.record(r)["own"]:
                if p in rows:
                    n, m = rows[p]
                    seen.add("missing" if m else "ambiguous" if bin(n).count("1") > 1 else "hit" if n == al else "miss")
                else:
                    seen.add("no row")
    assert seen == {"missing", "ambiguous", "hit", "miss", "no row"}


@pytest.mark.parametrize("k", [63, 64, 65, 200])
def test_ties_cases_have_exactly_k_records_at_the_minimum(k):
    c = case("ties%d" % k)
    assert c.n_rec == k + 2
    got = [c.oracle(s, range(c.n_rec)) for s in c.samples]
    assert [g[1] for g in got] == [k, 1, k, k, 0, 0] == c.want_num_best
    assert got[0][2] == {r: False for r in range(k)} and got[4] == (INT_MAX, 0, {}) == got[5]
    assert got[2][2] == got[3][2] == {r: False for r in range(k)} and got[1][2] == {k: False}


def test_values_case_is_what_it_claims():
    c = case("values")
    assert c.n_rec == 13 and c.n_rec % 2 == 1 and len(c.samples) == 70
    rec = {v: c.record(v - 1) for v in range(1, 14)}       # by node of R
    ref, alt = TC.REF, TC.alt
    # an own mutation whose prev is a non-reference parent state listed among the path entries of the same record
    assert rec[2]["own"][0] == (3, alt(3, 2), alt(3), ref(3)) and (3, alt(3), ref(3)) in rec[2]["path"]
    # a back-mutation to the reference base, and a sample without a row there for which that record is the best
    assert rec[3]["own"] == [(5, ref(5), alt(5, 1), ref(5))]
    assert any(5 not in s["pos"].tolist() and 2 in c.oracle(s, range(13))[2] for s in c.samples)
    # zero-mutation leaf (never eligible, for no sample) and internal node (eligible for every sample)
    assert rec[4]["own"] == [] == rec[5]["own"] and rec[4]["leaf"] and not rec[5]["leaf"] and not rec[4]["masked"] and not rec[5]["masked"]
    for s in c.samples:
        assert c.oracle(s, [3]) == (INT_MAX, 0, {}) and c.oracle(s, [4])[1] == 1
    assert any(4 in c.oracle(s, range(13))[2] for s in c.samples)
    # masked records with and without own mutations in front of the mask
    assert rec[7]["masked"] and [e[0] for e in rec[7]["own"]] == [11] and rec[8]["masked"] and rec[8]["own"] == []
    assert all(c.oracle(s, [7]) == (INT_MAX, 0, {}) for s in c.samples)
    hit7 = [c.oracle(s, range(13))[2] for s in c.samples]
    assert any(t.get(6) is True for t in hit7)                    # has_unique of a masked record at the minimum
    # positions at or beyond the dense table
    assert c.n_pos() == 26
    assert c.beyond(8) == ([], [TC.FAR]) and c.beyond(9) == ([], [TC.FAR + 1]) and c.beyond(10) == ([TC.FAR + 1], [TC.FAR + 1])
    assert all(c.beyond(r) == ([], []) for r in range(13) if r not in (8, 9, 10))
    for r in (8, 9, 10):
        assert any(r in c.oracle(s, range(13))[2] for s in c.samples), r
    # D(bottom) from rows no record names; missing rows do not count
    named = {e[0] for r in rec.values() for e in r["path"] + r["own"]}
    assert not named & {20, 21}
    assert TR.d_bottom(c.samples[2]) == 2 and TR.d_bottom(c.samples[1]) == 0 and TR.d_bottom(c.samples[3]) == 1
    assert c.oracle(c.samples[1], range(13))[0] < INT_MAX
    # ambiguous and missing rows at record positions
    assert any(bin(int(n)).count("1") > 1 and not m and int(p) in named for s in c.samples for p, n, m in zip(s["pos"], s["nuc"], s["is_missing"]))
    assert any(m and int(p) in named for s in c.samples for p, m in zip(s["pos"], s["is_missing"]))


def test_running_case_takes_every_branch_in_every_call_within_one_wave():
    c = case("running")
    assert [len(g) for g in c.groups] == [3, 3, 3, 3] and len(c.samples) == 129
    for g in (1, 2, 3):
        seen = {TC.branch_of_call(c, s, g) for s in c.samples[:64]}
        assert seen >= {"falls", "equals", "above"}, (g, seen)
    # 30 is in the samples' rows and beyond BASE's positions: the table is sized by the batch
    assert c.n_pos() == 31


@pytest.mark.parametrize("first_sample", [0, 1, 63, 64, 65, 128, 129])
def test_running_case_groups_2_and_3_change_samples_on_both_sides_of_first_sample(first_sample):
    """touched_score(first id of group 2, first_sample) on 129 samples: the new records change the answer of samples behind
    first_sample (so a call that did nothing fails) and WOULD change samples in front of it (so a call that scored them fails)."""
    c = case("running")
    changed = [c.oracle(s, range(6)) != c.oracle(s, range(12)) for s in c.samples]
    if first_sample > 0:
        assert any(changed[:first_sample])
    if first_sample < 129:
        assert any(changed[first_sample:])
    if first_sample in (1, 128):
        assert changed[0] and changed[128]
