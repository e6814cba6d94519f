"""The segmented flag scan of usher_amd/csrc/ugp_scan.hpp (k_flag_segsum / k_flag_scan, and k_gt_rank on the same body) as matUtils
summary, translate, genotypes, nearest and relatives launch it, the tiles of k_gt_compact and the 16-column store of k_gt_rows
exactly on their edges: item counts of a segment less one, a segment, one more, a segment and a pass, two segments, two and one
item; launch windows of a segment less one, a segment, one more and two; `cap` cutting the records at the seam between two
windows; chosen flags on both sides of the seam.  Every field that comes back is compared with summary_ref.Fast,
translate_ref.Fast, genotypes_ref.Fast, nearest_ref.Fast and relatives_ref.Fast, exactly;
tests/test_scan_edge_cases_cpu.py proves that the fixtures of tests/scan_edge_cases.py have the properties relied on here and that
those references follow the literal ones on these shapes of tree."""
import ctypes as C

import numpy as np
import pytest

from tests import genotypes_cases as GC
from tests import genotypes_ref as GR
from tests import nearest_ref as NR
from tests import relatives_ref as RR
from tests import scan_edge_cases as S
from tests import summary_cases as SC
from tests import summary_ref as SR
from tests import test_genotypes_gpu as TG
from tests import test_scan_edge_cases_cpu as CPU
from tests import translate_ref as TR
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu

KSEG, KBLOCK, GT_TILE = S.KSEG, S.KBLOCK, S.GT_TILE   # guarded by tests/test_dense_cases_cpu.py and the CPU module


def mutation_rows(recs):
    return list(zip(recs["pos"].tolist(), recs["par"].tolist(), recs["nuc"].tolist(), recs["count"].tolist()))


def as_dict(info):
    return {k: int(info[k]) for k in info.dtype.names}


def filled(n, dtype):
    return np.full(n, 0xA5, np.uint8).repeat(dtype.itemsize).view(dtype)


def cut_at(r1):
    """The values of `cap` around r1, the records of the first window."""
    return sorted({c for c in (r1 - 1, r1, r1 + 1) if c >= 0})


# ---- summary: the run heads over the M entries of the occurrence list --------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("M", S.EDGES)
def test_mutation_table(M, variant, masked):
    arrays = S.occurrence_tree(M, variant, masked)
    want = SR.Fast(arrays).mutations()
    nruns = len(want)
    assert nruns == S.occurrence_heads(arrays)[1] - (1 if masked else 0) > 50
    if masked:      # masked entries go to a handle of the bare topology, as in tests/test_summary_gpu.py
        pl = Placer(SC.topology(arrays))
        pl.summary_attach(arrays)
    else:
        pl = Placer(arrays)
    assert mutation_rows(pl.summary_mutations()) == want
    for w in (KSEG - 1, KSEG, KSEG + 1, KBLOCK):
        assert mutation_rows(pl.summary_mutations(chunk_items=w)) == want, w
    part = pl.summary_mutations(cap=nruns - 1)
    assert mutation_rows(part) == want[:nruns - 1] and pl._sm_n_out == nruns
    pl.close()


# ---- summary: the leaf prefix over the N nodes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", S.EDGES)
def test_leaf_prefix(N):
    arrays = S.leaf_prefix_tree(N, True)
    F = SR.Fast(arrays)
    cols = CPU.clade_columns(arrays, N)
    assert len(cols[0]) > 1000 and 4 <= len(cols[1]) <= 5
    pl = Placer(arrays)
    per, leaf_clade = pl.summary_clades(cols)
    at = 0
    for c, (incl, excl, near) in enumerate(F.clades(cols)):
        rows = per[at:at + len(cols[c])]
        at += len(cols[c])
        assert rows["column"].tolist() == [c] * len(rows) and np.array_equal(rows["node"], cols[c])
        assert np.array_equal(rows["inclusive"], incl) and np.array_equal(rows["exclusive"], excl), c
        assert np.array_equal(leaf_clade[c].astype(np.int64), near), c
    assert at == len(per)
    # the same leaf counts decide RoHo's > 5 rule; the mutation table of the same handle
    assert SR.device_roho_fast(F, pl.summary_roho()) == F.roho()[0]
    assert mutation_rows(pl.summary_mutations()) == F.mutations()
    pl.close()


# ---- nearest and relatives: the leaf prefix over the N nodes -----------------------------------------------------------------------

@pytest.mark.parametrize("N", S.LEAF_QUERY_EDGES)
def test_nearest_leaf_prefix(N):
    arrays = S.leaf_prefix_tree(N, True)
    nodes = np.repeat(S.leaf_prefix_queries(arrays, N), len(S.NEAREST_KS))
    ks = np.tile(S.NEAREST_KS, len(nodes) // len(S.NEAREST_KS))
    want = CPU.nearest_answers(NR.Fast(arrays), S.leaf_prefix_queries(arrays, N))
    pl = Placer(arrays)
    got = pl.nearest_k(nodes, ks)
    pl.close()
    for i, w in enumerate(want):
        NR.check(got, w, i, max(S.NEAREST_KS))


@pytest.mark.parametrize("N", S.LEAF_QUERY_EDGES)
def test_relatives_leaf_prefix(N):
    arrays = S.leaf_prefix_tree(N, True)
    nodes, rank = S.leaf_prefix_queries(arrays, N), CPU.name_ranks(N)
    want = CPU.relatives_answers(RR.Fast(arrays, rank), nodes)
    pl = Placer(arrays)
    pl.relatives_attach(rank)
    got = [pl.relatives_closest(nodes)] + [pl.relatives_within(nodes, k) for k in S.WITHIN_KS]
    pl.close()
    for i, w in enumerate(want):
        RR.check(got[i // len(nodes)], w, i % len(nodes))


# ---- summary: the records of every RoHo window -------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("Cn", S.EDGES)
def test_roho_windows(Cn, variant):
    arrays = S.roho_tree(Cn, variant)
    F = SR.Fast(arrays)
    want, _ = F.roho()
    flags = S.roho_flags(arrays, F, want)
    order = S.roho_order(arrays, F)
    n = len(want)
    assert len(flags) == Cn and n == flags.sum() > 1000
    pl = Placer(arrays)
    full = pl.summary_roho()
    assert SR.device_roho_fast(F, full) == want
    assert full["entry"].tolist() == order[flags == 1].tolist()       # the records come out in the candidates' order
    for w in (KSEG - 1, KSEG, KSEG + 1, 2 * KSEG):
        recs = pl.summary_roho(chunk_items=w)
        assert SR.device_roho_fast(F, recs) == want and recs.tobytes() == full.tobytes(), w
    # cap cuts the records where the first window ends
    r1 = int(flags[:KSEG].sum())
    for cap in cut_at(r1):
        buf = filled(n + 2, Placer.SM_ROHO)
        n_out = C.c_uint64(0)
        assert pl._L.ugp_summary_roho_chunked(pl._h, _ptr(buf), cap, C.byref(n_out), KSEG) == 0 and n_out.value == n, cap
        k = min(cap, n)
        assert buf[:k].tobytes() == full[:k].tobytes() and (buf[k:].view(np.uint8) == 0xA5).all(), cap
        part = pl.summary_roho(chunk_items=KSEG, cap=cap)
        assert part.tobytes() == full[:k].tobytes() and pl._sm_n_out == n, cap
    pl.close()


# ---- translate: the records of every window of work-items ---------------------------------------------------------------------------

@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("In", S.EDGES)
def test_translate_windows(In, variant):
    case, flags = S.translate_tree(In, variant)
    F = TR.Fast(case.arrays, *S.translate_slots())
    want, info = F.records, F.info
    n = len(want)
    assert n == flags.sum() > 1000 and info["n_inconsistent"] == info["n_duplicate"] == 0
    pl = Placer(case.arrays)
    pl.translate_codons(*S.translate_slots())
    full = None
    for w in (0, KSEG - 1, KSEG, KSEG + 1):
        recs, got = pl.translate(chunk_items=w)
        assert TR.device_records(recs) == want and as_dict(got) == info and (recs["pad"] == 0).all(), w
        assert pl._tr_n_out == n
        full = recs if full is None else full
        assert recs.tobytes() == full.tobytes(), w
    r1 = int(flags[:KSEG].sum())
    for cap in cut_at(r1):
        buf = filled(n + 2, Placer.TR_RECORD)
        n_out, raw = C.c_uint64(0), np.zeros(1, Placer.TR_INFO)
        assert pl._L.ugp_translate_chunked(pl._h, _ptr(buf), cap, C.byref(n_out), _ptr(raw), KSEG) == 0 and n_out.value == n, cap
        k = min(cap, n)
        assert buf[:k].tobytes() == full[:k].tobytes() and (buf[k:].view(np.uint8) == 0xA5).all() and as_dict(raw[0]) == info, cap
        part, got = pl.translate(chunk_items=KSEG, cap=cap)
        assert part.tobytes() == full[:k].tobytes() and pl._tr_n_out == n and as_dict(got) == info, cap
    pl.close()


def test_translate_refusal_from_the_second_segment():
    """The one inconsistent entry owns the last of KSEG + 1 items: the second segment of one window, the second window of two."""
    case, _ = S.translate_tree(KSEG + 1, "11", refused=True)
    info = TR.Fast(case.arrays, *S.translate_slots()).info
    assert info["n_inconsistent"] == 1 and info["first_inconsistent"] != TR.NIL
    pl = Placer(case.arrays)
    pl.translate_codons(*S.translate_slots())
    for w in (0, KSEG, 1):
        with pytest.raises(UgpError) as e:
            pl.translate(chunk_items=w)
        assert e.value.code == -2 and as_dict(pl._tr_info) == info, w
        buf = filled(8, Placer.TR_RECORD)
        n_out, raw = C.c_uint64(7), np.zeros(1, Placer.TR_INFO)
        assert pl._L.ugp_translate_chunked(pl._h, _ptr(buf), 8, C.byref(n_out), _ptr(raw), w) == -2
        assert n_out.value == 0 and (buf.view(np.uint8) == 0xA5).all() and as_dict(raw[0]) == info, w
    pl.close()


# ---- genotypes: the ranks of a selection over the N nodes ------------------------------------------------------------------------------

@pytest.mark.parametrize("N", S.EDGES)
def test_genotype_ranks(N):
    arrays = S.leaf_prefix_tree(N, True)
    F = GR.Fast(arrays)
    d2b = S.dfs_to_bfs(arrays)
    pl = Placer(arrays)
    pl.genotypes_attach(arrays)
    want = TG._check(pl, F, d2b[S.node_selection(N)])
    assert len(want.sites) > 20
    if N == 2 * KSEG:
        every = TG._check(pl, F, np.arange(N), literal=False)
        assert len(every.columns) == N and every.columns.tolist() == d2b.tolist()
    # a smaller selection after one of several segments
    lv = GC.leaves_of(arrays)
    three = TG._check(pl, F, lv[[3, len(lv) // 2, len(lv) - 1]])
    assert len(three.columns) == 3
    pl.close()


# ---- genotypes: the compaction of the sites over the P positions that have owners --------------------------------------------------------

@pytest.mark.parametrize("P", S.GT_EDGES)
def test_genotype_sites(P):
    arrays = S.genotype_positions_tree(P)
    leaves = S.position_selection(P)
    F = GR.Fast(arrays)
    pl = Placer(arrays)
    pl.genotypes_attach(arrays)
    want = TG._check(pl, F, leaves + 1)
    assert pl._gt_shape == (len(leaves), len(leaves))
    pos = pl.genotype_sites()["pos"].tolist()
    assert pos == (leaves + 1).tolist() == sorted(pos)
    lo, hi = int(np.searchsorted(leaves, GT_TILE - 1)), int(np.searchsorted(leaves, GT_TILE + 1, "right"))
    assert hi - lo == len({GT_TILE - 1, GT_TILE, GT_TILE + 1} & set(range(P)))
    for a, b in ((lo, hi), (0, 1)):
        assert np.array_equal(pl.genotype_rows(a, b), want.codes[a:b]), (a, b)
        assert GR.device_sites(pl.genotype_sites(a, b)) == GR.site_rows(want.sites[a:b]), (a, b)
    pl.close()


# ---- genotypes: column counts around the 16-cell store ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cols", [1, 15, 16, 17, 32, 33])
def test_genotype_column_counts(n_cols):
    arrays = GC.random_cases()[1][1]
    lv = GC.leaves_of(arrays)
    sel = lv[::len(lv) // n_cols][:n_cols]
    F = GR.Fast(arrays)
    want = F.run(sel, text=False)
    pl = Placer(arrays)
    pl.genotypes_attach(arrays)
    assert pl.genotype_select(sel) == (n_cols, len(want.sites)) and len(want.sites) > 0 and want.codes.any()
    assert np.array_equal(pl.genotype_columns(), want.columns)
    for cells in (0, 1, 16, n_cols, 16 * len(want.sites)):
        assert np.array_equal(pl.genotype_rows(chunk_cells=cells), want.codes), cells
    pl.close()
