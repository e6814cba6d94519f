"""The fixtures of tests/scan_edge_cases.py have the properties tests/test_scan_edges_gpu.py relies on -- shown with the references
alone (tests/summary_ref.py, translate_ref.py, genotypes_ref.py), so that a fixture that stops meeting one fails here instead of
letting the GPU test pass vacuously: exact item counts at every edge, the flags each variant claims on both sides of the seam
between the first two segments, a set flag in every segment and a last segment that does not hold the whole count (so that a lost
carry or an unwritten out[n] changes the answer), and -- with the same generators run small, the seam at 128 -- the fast references
against the literal ones on these shapes of tree.  For the leaf prefix of nearest and relatives (tests/nearest_ref.py, relatives_ref.py)
the references themselves are run with a prefix that dropped its carry: an answer to one of the queried nodes changes.  CPU only.

The carry loop of the scan kernels, `for (k = threadIdx.x; k < g; k += kBlock)`, takes a second stride only in a scan of more than
256 * KSEG = 4,194,304 items.  The largest scan anywhere in the suite is that of test_summary_at_size's tree: M = 1,005,501 entries
(N = 1,000,000 nodes, 225,574 RoHo candidates), which does not exceed it, and the launch windows default to 2^22 items, exactly that
many.  No few-second test reaches the second stride and none is added here: it remains untested at its edge."""
import os
import re

import numpy as np
import pytest

from tests import genotypes_ref as GR
from tests import nearest_ref as NR
from tests import relatives_ref as RR
from tests import scan_edge_cases as S
from tests import summary_cases as SC
from tests import summary_ref as SR
from tests import translate_cases as TC
from tests import translate_ref as TR
from usher_amd import FlatTreeView

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "usher_amd", "csrc")
KSEG, KBLOCK = S.KSEG, S.KBLOCK
SMALL = 128     # the seam of the small runs


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def segment_counts(flags, seg=KSEG):
    return [int(np.sum(flags[lo:lo + seg])) for lo in range(0, len(flags), seg)]


def model_scan(flags, seg, fault=None):
    """out[0 .. n] of the two-kernel scan (out[i] = flags set before i, out[n] = all of them) as a model in numpy, or with one of
    the off-by-ones the fixtures are placed to catch: 'no_carry' (a block starts from 0 instead of the segments before),
    'short_carry' (the carry loop stops one segment early), 'seam_item' (the first item of a segment takes the carry of the segment
    before), 'unwritten_total' (out[n] is not written when n is a whole number of segments; -1 stands for the stale word)."""
    f = np.asarray(flags, np.int64)
    n = len(f)
    starts = np.arange(0, n, seg)
    segsum = np.add.reduceat(f, starts)
    carry = np.cumsum(segsum) - segsum
    g = np.arange(n) // seg
    out = np.r_[np.cumsum(f) - f, f.sum()]
    before = np.r_[0, segsum[:-1]]                     # the segment in front of each
    if fault == "no_carry":
        out[:n] -= carry[g]
        out[n] -= carry[-1]
    elif fault == "short_carry":
        out[:n] -= before[g]
        out[n] -= before[-1]
    elif fault == "seam_item":
        out[starts[1:]] -= before[1:]
    elif fault == "unwritten_total" and n % seg == 0:
        out[n] = -1
    return out


def caught(flags, seg=KSEG):
    """The modelled faults that change what a caller sees: the places out[] gives to the flagged items, and the total."""
    f = np.asarray(flags, np.int64)
    right = model_scan(f, seg)
    seen = lambda out: (out[:-1][f == 1].tolist(), int(out[-1]))
    return {fault for fault in ("no_carry", "short_carry", "seam_item", "unwritten_total") if seen(model_scan(f, seg, fault)) != seen(right)}


def discriminates(flags, seg=KSEG):
    """Every segment holds a set flag and the last one does not hold them all, so that a scan that drops or shortens a carry gives
    other numbers (shown on the model above); a list of a whole number of segments shows an unwritten out[n].  A last segment of
    ONE item may hold no set flag -- the '00' variants at one item past the seam claim just that of it, and a masked run of several
    entries ends every masked list -- and still out[n], the count every call returns, is all carry there."""
    counts = segment_counts(flags, seg)
    if len(counts) < 2:
        return True
    alone = len(flags) % seg == 1
    shape = min(counts[:-1]) > 0 and (counts[-1] > 0 or alone) and counts[-1] != sum(counts)
    faults = caught(flags, seg)
    return shape and {"no_carry", "short_carry"} <= faults and (len(flags) % seg != 0 or "unwritten_total" in faults)


def test_constants_follow_the_sources():
    for name in ("ugp_summary.hip", "ugp_translate.hip"):
        assert re.search(r"constexpr uint64_t kDefaultItems = 1ull << (\d+);", _text(name)).group(1) == "22", name
    gt = _text("ugp_genotypes.hip")
    assert re.search(r"constexpr uint32_t kScanTile = (\d+);", gt).group(1) == "16"
    assert re.search(r"constexpr uint32_t kCellsPerThread = (\d+);", gt).group(1) == "16"
    assert "t0 += (uint64_t)kBlock * kScanTile" in gt
    assert S.GT_TILE == KBLOCK * 16
    assert S.EDGES == (KSEG - 1, KSEG, KSEG + 1, KSEG + KBLOCK - 1, KSEG + KBLOCK, 2 * KSEG, 2 * KSEG + 1)
    assert S.GT_EDGES == (S.GT_TILE - 1, S.GT_TILE, S.GT_TILE + 1, 2 * S.GT_TILE, 2 * S.GT_TILE + 1)
    assert 256 * KSEG == 4_194_304 == 1 << 22


# ---- the occurrence list --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("M", S.EDGES)
def test_occurrence_trees(M, variant, masked):
    arrays = S.occurrence_tree(M, variant, masked)
    pos = np.asarray(arrays["mut_pos"])
    assert len(pos) == M == arrays["mut_off"][-1] and arrays["n"] < 70000
    head, runs = S.occurrence_heads(arrays)
    F = SR.Fast(arrays)
    nm = int((pos < 0).sum())
    assert len(F.mutations()) == runs - (1 if masked else 0)
    if masked:
        assert nm == S.occurrence_masked(M, variant) >= 3
        assert len(np.unique(F.node[pos < 0])) == nm            # on several nodes
    else:
        assert nm == 0 and FlatTreeView(arrays) is not None     # a tree the placement tables take
    lens = np.diff(np.r_[np.flatnonzero(head), M])
    assert lens.min() == 1 and 200 <= lens.max() <= S.OCC_MAX_RUN and lens.sum() == M     # the last run ends at M
    # keys repeat across nodes; one position with two (par, nuc) pairs
    keys = np.unique(F.key[F.key != SR.MASKED_KEY])
    assert len(np.unique(keys >> 8)) < len(keys)
    if M > KSEG:
        seam = (int(head[KSEG - 1]), int(head[KSEG]))
        if masked and M - nm <= KSEG - 1:
            assert M == KSEG + 1 and seam == (0, 0)             # three masked entries cover the seam of the smallest list
        else:
            assert seam == ((1, 1) if variant == "11" else (0, 0)) and (variant == "00" or "seam_item" in caught(head))
        if masked and variant == "11" and M - nm == KSEG:
            assert np.sort(F.key)[KSEG] == SR.MASKED_KEY        # the head at the seam is the masked run's
        assert discriminates(head)


# ---- the leaf prefix and the ranks of a selection -------------------------------------------------------------------------------

def clade_columns(arrays, N, seam=KSEG):
    """[every internal node; the root, the chain and the node that straddles the seam] as breadth-first indices."""
    F = SR.Fast(arrays)
    d2b = np.argsort(F.pre)
    chain, straddle = S.leaf_prefix_marks(N, seam)
    marks = [0] + chain + ([straddle] if straddle is not None and straddle not in chain else [])
    return [np.flatnonzero(~F.leaf), d2b[marks]]


@pytest.mark.parametrize("N", S.EDGES)
def test_leaf_prefix_trees(N):
    for muts in (False, True):
        arrays = S.leaf_prefix_tree(N, muts)
        assert arrays["n"] == N == len(arrays["parent"])
        assert FlatTreeView(arrays) is not None
    F = SR.Fast(arrays)
    d2b = np.argsort(F.pre)
    end = F.pre + F.size
    chain, straddle = S.leaf_prefix_marks(N)
    for d in [0] + chain:                                        # lpre[N] is read for these
        assert not F.leaf[d2b[d]] and end[d2b[d]] == N
    assert F.par[d2b[chain[0]]] == 0 and d2b[chain[0]] == np.flatnonzero(F.par == 0)[-1]      # the root's last child
    assert F.par[d2b[chain[1]]] == d2b[chain[0]] and F.par[d2b[chain[2]]] == d2b[chain[1]]
    for d in (KSEG - 1, KSEG):
        assert d >= N or F.leaf[d2b[d]]
    if N > KSEG:
        v = d2b[straddle]
        assert not F.leaf[v] and v != 0 and F.pre[v] < KSEG < end[v]
        leaf_dfs = F.leaf[d2b].astype(np.int64)
        assert discriminates(leaf_dfs) and "seam_item" in caught(leaf_dfs)
        # the selection of the genotype test: a column in every segment, sites from mutations on both sides of the seam
        sel = S.node_selection(N)
        flags = np.zeros(N, np.int64)
        flags[sel] = 1
        assert {0, KSEG - 1, KSEG, KSEG + 1, N - 1} & set(range(N)) <= set(sel.tolist()) and discriminates(flags) and "seam_item" in caught(flags)
        assert (~F.leaf[d2b[sel]]).sum() > 5
        want = GR.Fast(arrays).run(d2b[sel], text=False)
        assert len(want.sites) > 20 and want.codes.any(axis=0)[[np.searchsorted(sel, KSEG - 1), np.searchsorted(sel, KSEG)]].all()


def nearest_answers(F, nodes):
    return [F.query(int(v), k) for v in nodes for k in S.NEAREST_KS]


def relatives_answers(F, nodes):
    return [F.closest(int(v)) for v in nodes] + [F.within(int(v), k) for k in S.WITHIN_KS for v in nodes]


def name_ranks(N):
    return np.random.default_rng(N).permutation(N).astype(np.uint32)


@pytest.mark.parametrize("N", S.LEAF_QUERY_EDGES)
def test_leaf_prefix_queries(N):
    """What test_scan_edges_gpu asks nearest and relatives: the two seam leaves and a node behind the seam are among the queries,
    and a leaf prefix without its carry gives another answer to at least one of them, from either reference."""
    arrays = S.leaf_prefix_tree(N, True)
    nodes = S.leaf_prefix_queries(arrays, N)
    F = SR.Fast(arrays)
    asked = F.pre[nodes].tolist()
    chain, _ = S.leaf_prefix_marks(N)
    assert len(set(asked)) == len(asked) and set(chain) <= set(asked) and N - 1 in asked and F.leaf[nodes].sum() == len(nodes) - 3
    assert {d for d in (KSEG - 1, KSEG) if d < N} <= set(asked)
    leaf_dfs = F.leaf[np.argsort(F.pre)].astype(np.int64)
    for fast, answers in ((NR.Fast(arrays), nearest_answers), (RR.Fast(arrays, name_ranks(N)), relatives_answers)):
        assert fast.lpre.tolist() == model_scan(leaf_dfs, KSEG).tolist()
        right = answers(fast, nodes)
        assert sum(w["count"] > 0 for w in right) > len(right) // 2
        if N > KSEG:
            assert max(asked) >= KSEG                           # a node in the second segment
            fast.lpre = model_scan(leaf_dfs, KSEG, "no_carry")
            assert answers(fast, nodes) != right


# ---- RoHo ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("Cn", S.EDGES)
def test_roho_trees(Cn, variant):
    arrays = S.roho_tree(Cn, variant)
    assert SC.n_candidates(arrays) == Cn and arrays["n"] < 70000 and FlatTreeView(arrays) is not None
    F = SR.Fast(arrays)
    recs, erased = F.roho()
    flags = S.roho_flags(arrays, F, recs)
    assert len(flags) == Cn and flags.sum() == len(recs) and len(recs) % KBLOCK != 0 and erased > 50
    order = S.roho_order(arrays, F)
    assert sorted(r[4] for r in recs) == sorted(order[flags == 1].tolist())
    want = (1, 1) if variant == "11" else (0, 0)
    assert (int(flags[-2]), int(flags[-1])) == want              # the end of the list, below an inner parent
    if Cn > KSEG:
        assert (int(flags[KSEG - 1]), int(flags[KSEG])) == want and discriminates(flags)
        assert "seam_item" in caught(flags) or variant == "00"
        assert F.node[order[KSEG - 1]] != F.node[order[KSEG]]    # two hubs meet at the seam
    # exactly 5 and exactly 6 leaves, most 6 or more; both median branches; owners that are the later of two
    hubs = np.unique(F.node[order])
    assert (F.lc[hubs] == 5).sum() > 100 and (F.lc[hubs] == 6).sum() > 100 and (F.lc[hubs] >= 6).mean() > 0.8
    assert not np.isin(F.node[order[flags == 1]], hubs[F.lc[hubs] == 5]).any()
    big = np.bincount(F.par[hubs[F.lc[hubs] > 5]], minlength=F.n)
    parents = np.unique(F.par[F.node[order[flags == 1]]])
    assert {int(big[p] - 1) % 2 for p in parents} == {0, 1}
    key_of = F.key[order]
    first = {}
    for i in np.flatnonzero(F.par[F.node[order]] == 0):
        first.setdefault(int(key_of[i]), []).append(int(i))
    shared = [v for v in first.values() if len(v) > 1]
    assert len(shared) > 50 and all(flags[v[0]] == 0 for v in shared)
    assert (F.depth[hubs] == 2).sum() == sum(3 if g == S.ROHO_GROUPS - 1 else 2 + g % 2 for g in range(S.ROHO_GROUPS))


# ---- translate ------------------------------------------------------------------------------------------------------------------

def translate_flags(arrays, records):
    """Per work-item 1 when it owns a record: the item at the lowest mutated position of its (node, codon).  From the reference's
    records and the item order (nodes depth-first, owners by position, codons by index)."""
    slot_pos = S.translate_slots()[0]
    at = {}
    for c in range(len(slot_pos)):
        for k in range(3):
            at.setdefault(int(slot_pos[c, k]), []).append(c)
    lowest = {}
    pos = np.asarray(arrays["mut_pos"])
    for node, codon, _, _, ent in records:
        lowest[(node, codon)] = min(int(pos[e]) for e in ent if e != TR.NIL)
    F = SR.Fast(arrays)
    flags = []
    for v in np.argsort(F.pre).tolist():
        own = sorted({int(pos[k]) for k in range(int(F.off[v]), int(F.off[v + 1])) if pos[k] >= 0})
        for p in own:
            flags += [1 if lowest[(v, c)] == p else 0 for c in at.get(p, ())]
    return np.asarray(flags, np.int64)


@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("In", S.EDGES)
def test_translate_trees(In, variant):
    case, claimed = S.translate_tree(In, variant)
    assert S.translate_items(case.arrays) == In == len(claimed) and FlatTreeView(case.arrays) is not None
    F = TR.Fast(case.arrays, *S.translate_slots())
    assert F.info["n_inconsistent"] == F.info["n_duplicate"] == 0 and F.info["n_records"] == len(F.records)
    flags = translate_flags(case.arrays, F.records)
    assert flags.tolist() == claimed.tolist() and flags.sum() == len(F.records)
    assert 0.5 < flags.mean() < 0.9                              # a real mixture
    if In > KSEG:
        assert (int(flags[KSEG - 1]), int(flags[KSEG])) == ((1, 1) if variant == "11" else (0, 0)) and discriminates(flags)
        assert "seam_item" in caught(flags) or variant == "00"
    if In == 2 * KSEG + 1:
        assert TC.n_items(case) == In                            # the vectorised count is translate_cases' own


def test_translate_refused_twin():
    case, flags = S.translate_tree(KSEG + 1, "11", refused=True)
    twin, _ = S.translate_tree(KSEG + 1, "11")
    assert S.translate_items(case.arrays) == KSEG + 1
    differ = np.flatnonzero(np.asarray(case.arrays["mut_par"]) != np.asarray(twin.arrays["mut_par"]))
    assert len(differ) == 1 and all(np.array_equal(case.arrays[k], twin.arrays[k]) for k in ("parent", "mut_off", "mut_pos", "mut_nuc"))
    F = TR.Fast(case.arrays, *S.translate_slots())
    assert F.info["n_inconsistent"] == 1 and F.info["n_duplicate"] == 0 and F.info["first_inconsistent"] == differ[0]
    # the offender owns the last item: the last node of the depth-first order with a coding mutation, and one item of its own
    node = int(np.searchsorted(np.asarray(case.arrays["mut_off"]), differ[0], side="right")) - 1
    pre = SR.Fast(case.arrays).pre
    with_muts = np.flatnonzero(np.diff(np.asarray(case.arrays["mut_off"])) > 0)
    assert pre[node] == pre[with_muts].max() and case.arrays["mut_pos"][differ[0]] in (1, 2, 3)


# ---- genotypes over the positions ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", S.GT_EDGES)
def test_genotype_position_trees(P):
    arrays = S.genotype_positions_tree(P)
    pos = np.asarray(arrays["mut_pos"])
    assert len(np.unique(pos[pos >= 0])) == P == arrays["n"] - 1 and FlatTreeView(arrays) is not None
    sel = S.position_selection(P)
    assert {0, 15, 16, 17, P - 1} <= set(sel.tolist()) and {S.GT_TILE - 1, S.GT_TILE, S.GT_TILE + 1} & set(range(P)) <= set(sel.tolist())
    want = GR.Fast(arrays).run(sel + 1, text=False)
    assert [s["pos"] for s in want.sites] == (sel + 1).tolist()              # a site exactly where the leaf is selected
    assert np.array_equal(want.codes, np.eye(len(sel), dtype=np.uint8))
    flags = np.zeros(P, np.int64)
    flags[sel] = 1
    assert discriminates(flags, S.GT_TILE) and (P <= S.GT_TILE or "seam_item" in caught(flags, S.GT_TILE))


# ---- the references on these shapes, small ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("variant", S.VARIANTS)
def test_references_agree_on_small_occurrence_trees(variant, masked):
    for M in (SMALL + 1, 2 * SMALL + 60, 700):
        arrays = S.occurrence_tree(M, variant, masked, seam=SMALL)
        head, _ = S.occurrence_heads(arrays)
        if not masked or M > SMALL + 3:
            assert (int(head[SMALL - 1]), int(head[SMALL])) == ((1, 1) if variant == "11" else (0, 0))
        assert SR.Fast(arrays).mutations() == SR.mutation_records(SR.Tree(arrays))


@pytest.mark.parametrize("N", [SMALL + 1, SMALL + 100, 500])
def test_references_agree_on_small_leaf_prefix_trees(N):
    arrays = S.leaf_prefix_tree(N, True, seam=SMALL)
    T, F = SR.Tree(arrays), SR.Fast(arrays)
    assert T.dfs() == np.argsort(F.pre).tolist()
    cols = clade_columns(arrays, N, SMALL)
    for lit, fast in zip(SR.clade_records(T, [c.tolist() for c in cols]), F.clades(cols)):
        for x, y in zip(lit, fast):
            assert [int(v) for v in x] == [int(v) for v in y]
    d2b = np.argsort(F.pre)
    G = GR.Fast(arrays)
    for sel in (d2b[S.node_selection(N, SMALL, 60)], np.arange(N), None):
        lit, fast = GR.literal(arrays, sel), G.run(sel)
        assert GR.site_rows(lit.sites) == GR.site_rows(fast.sites) and len(lit.sites) > 5
        assert np.array_equal(lit.codes, fast.codes) and np.array_equal(lit.columns, fast.columns)


@pytest.mark.parametrize("N", [SMALL + 1, SMALL + 100, 500])
def test_references_agree_on_small_leaf_prefix_queries(N):
    arrays = S.leaf_prefix_tree(N, True, seam=SMALL)
    nodes = S.leaf_prefix_queries(arrays, N, SMALL)
    rank = name_ranks(N)
    NT, RT = NR.Tree(arrays), RR.Tree(arrays)
    assert nearest_answers(NR.Fast(arrays), nodes) == [NR.literal(NT, int(v), k) for v in nodes for k in S.NEAREST_KS]
    assert relatives_answers(RR.Fast(arrays, rank), nodes) == ([RR.literal(RT, int(v), False, 0, rank) for v in nodes] +
                                                                [RR.literal(RT, int(v), True, k) for k in S.WITHIN_KS for v in nodes])


@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("Cn", [SMALL + 1, SMALL + 60, 400])
def test_references_agree_on_small_roho_trees(Cn, variant):
    arrays = S.roho_tree(Cn, variant, seam=SMALL)
    T, F = SR.Tree(arrays), SR.Fast(arrays)
    assert SC.n_candidates(arrays) == Cn
    rows = SR.roho_records(T)
    assert SR.fast_roho_rows(F, T) == rows and len(rows) > 40 and F.roho()[1] > 0
    flags = S.roho_flags(arrays, F)
    want = (1, 1) if variant == "11" else (0, 0)
    assert (int(flags[SMALL - 1]), int(flags[SMALL])) == want == (int(flags[-2]), int(flags[-1]))


@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("In", [SMALL + 1, SMALL + 60, 400])
def test_references_agree_on_small_translate_trees(In, variant):
    case, claimed = S.translate_tree(In, variant, seam=SMALL)
    T, codons = case.tree(), case.codons()
    F = TR.Fast(case.arrays, *S.translate_slots())
    assert TC.n_items(case) == In == S.translate_items(case.arrays)
    assert F.info == TR.info(T, codons) and F.records == TR.records(T, codons)
    assert translate_flags(case.arrays, F.records).tolist() == claimed.tolist()
    if variant == "11" and In == SMALL + 1:
        bad, _ = S.translate_tree(In, variant, seam=SMALL, refused=True)
        Fb = TR.Fast(bad.arrays, *S.translate_slots())
        assert Fb.info == TR.info(bad.tree(), bad.codons()) and Fb.info["n_inconsistent"] == 1


def test_references_agree_on_a_small_position_star():
    arrays = S.genotype_positions_tree(300)
    sel = S.position_selection(300, 40) + 1
    lit, fast = GR.literal(arrays, sel), GR.Fast(arrays).run(sel)
    assert GR.site_rows(lit.sites) == GR.site_rows(fast.sites) and np.array_equal(lit.codes, fast.codes) and len(lit.sites) == len(sel)
