"""Record scoring of the add mode on the device (k_touched<1>, k_touched_reset, k_touched<2>, k_dense_scatter behind ugp_mat_update
and ugp_touched_open / _score / _rescore / _fetch) against the oracle's literal mapper2_body over the live record nodes, on the
hand-shaped cases of tests/touched_cases.py: entry batches of eight, lists longer than the device keeps, the running list across
calls within one wave, record ranges, rescoring, value edges and the error codes.  Integers, compared exactly; the complete set of
(record, has_unique) pairs wherever the true count is at most 64."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import capi
from tests import synth
from tests import touched_cases as TC
from tests.test_touched_cpu import case
from usher_amd import Placer, QueryBatch, UgpError, _lib
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu
INT_MAX = TC.INT_MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID_FILL, HU_FILL = 0xA5A5A5A5, 0x5A


def fetch_raw(pl, first, n, cap):
    """ugp_touched_fetch into arrays filled with a pattern: (rc, best, count, ids [n][cap], has_unique [n][cap])."""
    best, cnt = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), 0xFFFFFFF0, np.uint32)
    ids, hu = np.full((max(n, 1), max(cap, 1)), ID_FILL, np.uint32), np.full((max(n, 1), max(cap, 1)), HU_FILL, np.uint8)
    rc = pl._L.ugp_touched_fetch(pl._h, first, n, cap, _ptr(best), _ptr(cnt), _ptr(ids), _ptr(hu))
    return rc, best, cnt, ids, hu


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


class Session:
    """A handle on BASE with records of one case: device record id -> record of the case, and which are live."""

    def __init__(self, c):
        self.c, self.pl = c, Placer(TC.base_arrays())
        self.rec_of, self.live, self.n_rec = {}, set(), 0

    def update(self, rids=(), retired=()):
        first = self.pl.update([self.c.record(r) for r in rids], list(retired))
        assert first == self.n_rec
        for k, r in enumerate(rids):
            self.rec_of[first + k] = r
            self.live.add(first + k)
        self.live -= set(retired)
        self.n_rec += len(rids)
        return first

    def want(self, smp, live=None):
        live = self.live if live is None else live
        dev_of = {self.rec_of[d]: d for d in live}
        assert len(dev_of) == len(live)
        best, nb, ties = self.c.oracle(smp, dev_of)
        return best, nb, {dev_of[r]: h for r, h in ties.items()}

    def check(self, samples, q0=0, q1=None, overflow=False):
        """Samples [q0, q1) of the open batch against the oracle over the live records."""
        q1 = len(samples) if q1 is None else q1
        if q1 == q0:
            return
        best, cnt, ids, hu = self.pl.touched_fetch(q0, q1 - q0)
        for k in range(q1 - q0):
            wb, wn, wt = self.want(samples[q0 + k])
            assert (int(best[k]), int(cnt[k])) == (wb, wn), (self.c.name, q0 + k, int(best[k]), int(cnt[k]), wb, wn)
            m = min(wn, 64)
            got = list(zip(ids[k][:m].tolist(), hu[k][:m].astype(bool).tolist()))
            assert len({r for r, _ in got}) == m, (self.c.name, q0 + k)
            if wn <= 64:
                assert dict(got) == wt, (self.c.name, q0 + k)
            else:
                assert overflow, (self.c.name, q0 + k, wn)     # only the cases named for it
                assert all(r in wt and wt[r] == h for r, h in got), (self.c.name, q0 + k)

    def check_record_by_record(self, samples):
        """Every record alone: handed over again with everything else retired, every sample scored again from the live records."""
        for r in range(self.c.n_rec):
            self.update([r], sorted(self.live))
            assert len(self.live) == 1
            for q in range(len(samples)):
                self.pl.touched_rescore(q)
            self.check(samples)


# ---- the eight-entry batches ------------------------------------------------------------------------------------------------------

def check_entry_all_together():
    c = case("entry_batches")
    s = Session(c)
    s.update(range(c.n_rec))
    s.pl.touched_open(QueryBatch(c.samples))
    s.check(c.samples)
    return s


def test_entry_batches_all_together_and_record_by_record():
    s = check_entry_all_together()
    s.check_record_by_record(s.c.samples)
    s.pl.close()


# ---- samples: batch sizes and first_sample at the wave edges ----------------------------------------------------------------------

@pytest.mark.parametrize("Q", [1, 63, 64, 65, 129])
def test_score_from_first_sample(Q):
    """Groups 0 and 1 of the running case are live when the batch is opened; groups 2 and 3 arrive in one update and are scored
    against the samples from first_sample on: those equal the oracle over all live records, the ones in front are untouched."""
    c = case("running")
    samples = c.samples[:Q]
    batch = QueryBatch(samples)
    s = Session(c)
    s.update(c.ids(0))
    s.update(c.ids(1))
    late = []
    for fs in sorted({f for f in (0, 1, 63, 64, 65, 128, 129, Q - 1, Q) if 0 <= f <= Q}):
        s.update((), late)
        s.pl.touched_open(batch)
        s.check(samples)
        before = fetch_raw(s.pl, 0, Q, 64)
        first = s.update(c.ids(2) + c.ids(3))
        late = list(range(first, first + 6))
        s.pl.touched_score(first, fs)
        after = fetch_raw(s.pl, 0, Q, 64)
        assert before[0] == 0 == after[0]
        assert same_bytes([x[:fs] for x in before[1:]], [x[:fs] for x in after[1:]]), fs
        s.check(samples, fs)
    s.pl.close()


# ---- lists longer than the device keeps -------------------------------------------------------------------------------------------

def check_ties(k):
    c = case("ties%d" % k)
    s = Session(c)
    s.update(range(c.n_rec))
    s.pl.touched_open(QueryBatch(c.samples))
    s.check(c.samples, overflow=k in (65, 200))
    return s


@pytest.mark.parametrize("k", [63, 64, 65, 200])
def test_lists_at_the_capacity_and_fetch_widths(k):
    s = check_ties(k)
    Q = len(s.c.samples)
    rc, best, cnt, ids, hu = fetch_raw(s.pl, 0, Q, 64)
    assert rc == 0 and cnt.tolist() == s.c.want_num_best
    for cap in (0, 1, 63, 64, 65, 100):
        for first, n in ((0, Q), (2, 3)):
            rc, b2, c2, i2, h2 = fetch_raw(s.pl, first, n, cap)
            assert rc == 0 and b2.tolist() == best[first:first + n].tolist() and c2.tolist() == cnt[first:first + n].tolist(), (cap, first)
            w = min(cap, 64)
            if w:
                assert np.array_equal(i2[:, :w], ids[first:first + n, :w]) and np.array_equal(h2[:, :w], hu[first:first + n, :w]), (cap, first)
            assert (i2[:, w:] == ID_FILL).all() and (h2[:, w:] == HU_FILL).all(), (cap, first)     # as the caller initialised them
    s.pl.close()


# ---- the running list within one wave ---------------------------------------------------------------------------------------------

def test_running_list_falls_is_equalled_and_stays_within_one_wave():
    c = case("running")
    samples = c.samples[:64]
    batch = QueryBatch(samples)
    s = Session(c)
    s.update(c.ids(0))
    s.pl.touched_open(batch)
    s.check(samples)
    for g in (1, 2, 3):
        s.pl.touched_score(s.update(c.ids(g)), 0)
        s.check(samples)
    a = s.pl.touched_fetch(0, 64)
    s.pl.touched_open(batch)
    b = s.pl.touched_fetch(0, 64)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    for q in range(64):
        n = int(a[1][q])
        assert n <= 64 and sorted(zip(a[2][q][:n].tolist(), a[3][q][:n].tolist())) == sorted(zip(b[2][q][:n].tolist(), b[3][q][:n].tolist())), q
    s.pl.close()


# ---- retire and rescore -----------------------------------------------------------------------------------------------------------

def none_everywhere(pl, Q):
    rc, best, cnt, _, _ = fetch_raw(pl, 0, Q, 64)
    return rc == 0 and (best == INT_MAX).all() and (cnt == 0).all()


def test_retire_the_holders_of_a_minimum_then_rescore():
    c = case("values")
    batch = QueryBatch(c.samples)
    s = Session(c)
    s.update(range(c.n_rec))
    s.pl.touched_open(batch)
    rounds = 0
    for q in list(range(4, len(c.samples))) + [0, 1, 2, 3]:      # (the first four samples are tied at most records: one or two a time first)
        holders = sorted(s.want(c.samples[q])[2])
        if not holders:
            continue
        s.update((), holders)
        s.pl.touched_rescore(q)
        s.check(c.samples, q, q + 1)
        rounds += 1
    assert rounds >= 6 and s.live == {3, 7}           # what is left is eligible for no sample: the leaf without mutations, the mask in front
    s.update((), sorted(s.live))
    for q in range(len(c.samples)):
        s.pl.touched_rescore(q)
    assert none_everywhere(s.pl, len(c.samples))
    s.pl.touched_open(batch)
    assert none_everywhere(s.pl, len(c.samples))
    s.pl.close()


def test_a_handle_without_records_reports_none():
    c = case("values")
    pl = Placer(TC.base_arrays())
    pl.touched_open(QueryBatch(c.samples))
    assert none_everywhere(pl, len(c.samples))
    pl.touched_score(0, 0)
    pl.touched_rescore(3)
    assert none_everywhere(pl, len(c.samples))
    pl.close()


# ---- empty ranges -----------------------------------------------------------------------------------------------------------------

def test_empty_record_and_sample_ranges_change_nothing():
    c = case("values")
    Q = len(c.samples)
    s = Session(c)
    s.update(range(c.n_rec))
    s.pl.touched_open(QueryBatch(c.samples))
    before = fetch_raw(s.pl, 0, Q, 64)
    s.pl.touched_score(c.n_rec, 0)
    s.pl.touched_score(0, Q)
    s.pl.touched_score(c.n_rec, Q)
    assert s.pl.update([], []) == c.n_rec
    assert fetch_raw(s.pl, 0, 0, 64)[0] == 0 and fetch_raw(s.pl, Q, 0, 64)[0] == 0
    assert same_bytes(before[1:], fetch_raw(s.pl, 0, Q, 64)[1:])
    s.check(c.samples)
    s.pl.close()


# ---- UGP_TOUCHED_RECS -------------------------------------------------------------------------------------------------------------

def test_records_per_block_that_do_not_divide_the_range_in_fresh_processes():
    """UGP_TOUCHED_RECS is read once per process: the 31 records of the entry-batch case and the 67 of the 65-ties case (odd
    numbers both) with 1, 3 and 64 records per block, one child process per value, one child at a time."""
    for recs in (1, 3, 64):
        env = {k: v for k, v in os.environ.items() if not k.startswith("UGP_")}
        env.update({"UGP_TOUCHED_RECS": str(recs), "PYTHONPATH": ROOT})
        code = ("from tests.test_touched_gpu import check_entry_all_together, check_ties\n"
                "assert check_entry_all_together().c.n_rec == 31\nassert check_ties(65).c.n_rec == 67")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, ("UGP_TOUCHED_RECS=%d" % recs, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- values -----------------------------------------------------------------------------------------------------------------------

def test_value_edges_all_together_and_record_by_record():
    c = case("values")
    s = Session(c)
    s.update(range(c.n_rec))
    s.pl.touched_open(QueryBatch(c.samples))
    s.check(c.samples)
    s.check_record_by_record(c.samples)
    s.pl.close()


# ---- error codes ------------------------------------------------------------------------------------------------------------------

INVALID, UNSUPPORTED = -1, -2


def raw_update(pl, flat_j, flags, n_path, ent_off, pos, allele, prev, ref, retired=(), n_retired=None, null=()):
    """ugp_mat_update with the arrays as given (`null`: field names handed over as NULL); returns the status."""
    a = {"flat_j": np.asarray(flat_j, np.uint32), "flags": np.asarray(flags, np.uint8), "n_path": np.asarray(n_path, np.uint32),
         "ent_off": np.asarray(ent_off, np.uint64), "pos": np.asarray(pos, np.int32), "allele": np.asarray(allele, np.uint8),
         "prev": np.asarray(prev, np.uint8), "ref": np.asarray(ref, np.uint8)}
    t = _lib.ugp_touched(len(a["flat_j"]), *[None if k in null else _ptr(a[k]) for k in ("flat_j", "flags", "n_path", "ent_off", "pos", "allele", "prev", "ref")])
    ret = np.asarray(list(retired), np.uint32)
    first = C.c_uint32()
    return pl._L.ugp_mat_update(pl._h, C.byref(t), None if "retired" in null else _ptr(ret), len(ret) if n_retired is None else n_retired, C.byref(first))


NONE_J = 0xFFFFFFFF
A_, C_, G_ = TC.A, TC.C, TC.G
# one new node: a path entry at 4 (A -> C), an own mutation at 6 (G -> A); every call below spoils one thing of it
GOOD = dict(flat_j=[NONE_J], flags=[1], n_path=[1], ent_off=[0, 2], pos=[4, 6], allele=[C_, A_], prev=[0, G_], ref=[A_, G_])


def refused_updates(n_rec, n_nodes):
    yield "retired id == n_rec", INVALID, dict(GOOD, retired=[n_rec])
    yield "retired id far beyond", INVALID, dict(GOOD, retired=[0, 2 ** 32 - 1])
    yield "retired id, no new records", INVALID, dict(flat_j=[], flags=[], n_path=[], ent_off=[0], pos=[], allele=[], prev=[], ref=[], retired=[n_rec])
    two = dict(flat_j=[NONE_J] * 2, flags=[1, 1], n_path=[0, 0], pos=[4, 6], allele=[C_, A_], prev=[A_, G_], ref=[A_, G_])
    yield "ent_off falls", INVALID, dict(two, ent_off=[0, 2, 1])
    yield "ent_off falls below its start", INVALID, dict(two, ent_off=[1, 0, 2])
    yield "n_path larger than the record", INVALID, dict(GOOD, n_path=[3])
    yield "ambiguous path allele", UNSUPPORTED, dict(GOOD, allele=[C_ | G_, A_])
    yield "ambiguous own allele", UNSUPPORTED, dict(GOOD, allele=[C_, 15])
    yield "no allele", UNSUPPORTED, dict(GOOD, allele=[0, A_])
    yield "ambiguous ref", UNSUPPORTED, dict(GOOD, ref=[A_, G_ | A_])
    yield "ambiguous own prev", UNSUPPORTED, dict(GOOD, prev=[0, G_ | C_])
    yield "own prev missing", UNSUPPORTED, dict(GOOD, prev=[0, 0])
    yield "flat_j = 0", UNSUPPORTED, dict(GOOD, flat_j=[0])
    yield "flat_j = N", INVALID, dict(GOOD, flat_j=[n_nodes])
    yield "a good record, then flat_j = N", INVALID, dict(two, ent_off=[0, 1, 2], flat_j=[1, n_nodes])
    for k in ("flat_j", "flags", "n_path", "ent_off", "pos", "allele", "prev", "ref"):
        yield "null " + k, INVALID, dict(GOOD, null=(k,))
    yield "null retired", INVALID, dict(GOOD, null=("retired",), n_retired=1)


def test_refused_calls_return_the_documented_code_and_leave_the_handle_as_it_was():
    c = case("values")
    Q = len(c.samples)
    s = Session(c)
    pl = s.pl
    for name, call in (("score", lambda: pl._L.ugp_touched_score(pl._h, 0, 0)), ("rescore", lambda: pl._L.ugp_touched_rescore(pl._h, 0)),
                       ("fetch", lambda: fetch_raw(pl, 0, 1, 64)[0]), ("empty fetch", lambda: fetch_raw(pl, 0, 0, 64)[0])):
        assert call() == INVALID, name + " before any touched_open"
    s.update(range(c.n_rec))
    pl.touched_open(QueryBatch(c.samples))
    s.check(c.samples)
    probe = QueryBatch(TC.random_samples(np.random.default_rng(8), 20, [3, 11, 17, 19, 25]))
    n_nodes = int(TC.base_arrays()["n"])

    def state():
        res = pl.place(probe)
        return [pl.update([], []), res.tobytes()] + [x.tobytes() for x in fetch_raw(pl, 0, Q, 64)[1:]]

    before = state()
    assert before[0] == c.n_rec
    calls = [(name, code, (lambda kw=kw: raw_update(pl, **kw))) for name, code, kw in refused_updates(c.n_rec, n_nodes)]
    calls += [("first_id > n_rec", INVALID, lambda: pl._L.ugp_touched_score(pl._h, c.n_rec + 1, 0)),
              ("first_sample > Q", INVALID, lambda: pl._L.ugp_touched_score(pl._h, 0, Q + 1)),
              ("rescore(Q)", INVALID, lambda: pl._L.ugp_touched_rescore(pl._h, Q)),
              ("fetch from Q", INVALID, lambda: fetch_raw(pl, Q, 1, 64)[0]),
              ("fetch past Q", INVALID, lambda: fetch_raw(pl, 1, Q, 64)[0]),
              ("fetch into null", INVALID, lambda: pl._L.ugp_touched_fetch(pl._h, 0, 1, 64, None, None, None, None))]
    for name, code, call in calls:
        assert call() == code, name
        assert state() == before, name
    with pytest.raises(UgpError) as ei:
        pl.update([c.record(0)], [c.n_rec])
    assert ei.value.code == INVALID
    # the handle still works: the good record is taken and scored (no sample of the batch has a row at its position: never eligible)
    assert raw_update(pl, **GOOD) == 0 and pl.update([], []) == c.n_rec + 1
    pl.touched_score(c.n_rec, 0)
    s.check(c.samples)
    pl.close()


# ---- a flattened node named twice -------------------------------------------------------------------------------------------------

def test_a_flattened_node_named_twice_in_one_update_and_again_in_the_next(monkeypatch):
    """The same flat_j twice within one update (two lanes of k_or_words on one word) and once more in a second update, with the
    coarse tree of the locality pre-pass present: the node is never answered, every sample equals the oracle over the other nodes."""
    monkeypatch.setenv("UGP_COARSE_MIN_NODES", "0")
    arrays, queries = synth.make_case(31, n_leaves=150, n_queries=70, n_sites=60, n_ambig=(0, 0, 1))
    assert 200 <= int(arrays["n"]) <= 600
    T, flat_nodes = TC.tree_from_arrays(arrays)
    ot = capi.OracleTree(arrays)
    counts = np.bincount([int(j) for s in queries for j in ot.place(s)["ties"]], minlength=int(arrays["n"]))
    counts[0] = 0
    victim = int(np.argmax(counts))                     # the node most samples tie at
    assert counts[victim] >= 3
    batch = QueryBatch(queries)
    pl = Placer(arrays)
    rec = TC.record_of(flat_nodes[victim], victim)
    assert pl.update([rec, rec], []) == 0
    assert pl.update([rec], [0]) == 2
    res = pl.place(batch)
    tj, th, tc = pl.tied_nodes(batch, 512)
    allowed = np.array([j for j in range(int(arrays["n"])) if j != victim], np.int64)
    changed = 0
    for i, s in enumerate(queries):
        w = ot.place_list(s, allowed, jidx=allowed, tie_cap=1 << 12)
        assert (int(res["best_set_difference"][i]), int(res["num_best"][i]), int(tc[i])) == (w["best"], w["num_best"], w["num_best"]), i
        assert victim not in tj[i].tolist() and int(res["best_j"][i]) != victim, i
        assert tj[i].tolist() == w["ties"].tolist() and th[i].tolist() == w["ties_has_unique"].tolist(), i
        changed += victim in ot.place(s)["ties"].tolist()
    assert changed >= 3
    pl.close()
