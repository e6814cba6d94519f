"""Fixtures for tests/test_scan_edges_gpu.py (and tests/test_scan_edge_cases_cpu.py, which proves with the references alone that each
one has the property its GPU test relies on): trees that put the segmented flag scan of usher_amd/csrc/ugp_scan.hpp, as matUtils
summary, translate, genotypes, nearest and relatives launch it (ugp_summary.hip, ugp_translate.hip, ugp_genotypes.hip,
ugp_nearest.hip, ugp_relatives.hip), exactly on its edges -- an item count of one segment less one, one segment, one more, one
segment and one pass, two segments, two and one item -- with chosen flags on both sides of the seam between the first two segments.  Every generator takes its count and the place of the seam as parameters, so that the CPU
module runs the same shapes small against the literal references.  Everything is built here, nothing is read from disk."""
import collections
import functools
import itertools

import numpy as np

from tests import dense_cases as D
from tests import summary_ref as SR
from tests import translate_cases as TC
from tests import translate_ref as TR

KSEG, KBLOCK = D.KSEG, D.KBLOCK        # usher_amd/csrc/ugp_dense.hpp, guarded by tests/test_dense_cases_cpu.py
EDGES = (KSEG - 1, KSEG, KSEG + 1, KSEG + KBLOCK - 1, KSEG + KBLOCK, 2 * KSEG, 2 * KSEG + 1)
GT_TILE = 4096                         # kBlock * kScanTile of k_gt_compact, guarded by tests/test_scan_edge_cases_cpu.py
GT_EDGES = (GT_TILE - 1, GT_TILE, GT_TILE + 1, 2 * GT_TILE, 2 * GT_TILE + 1)
VARIANTS = ("11", "00")                # the flags of the items seam - 1 | seam

A, C, G, T = 1, 2, 4, 8


def _node(muts=(), kids=()):
    return [list(muts), list(kids)]


def _arrays(root):
    """The breadth-first arrays of a nested [mutations, children] tree; a mutation is (position, ref, par, allele).  Children keep
    their order, so the depth-first order of the arrays is the order the nodes were nested in."""
    order, parent, q = [], [], collections.deque([(root, -1)])
    while q:
        nd, p = q.popleft()
        j = len(order)
        order.append(nd)
        parent.append(p)
        q.extend((k, j) for k in nd[1])
    n = len(order)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(nd[0]) for nd in order])
    flat = np.asarray([m for nd in order for m in nd[0]], np.int64).reshape(-1, 4)
    return {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": off, "mut_pos": flat[:, 0].astype(np.int32),
            "mut_ref": flat[:, 1].astype(np.int8), "mut_par": flat[:, 2].astype(np.int8), "mut_nuc": flat[:, 3].astype(np.int8),
            "names": ["n%d" % j for j in range(n)]}


def dfs_to_bfs(arrays):
    """Per depth-first position the breadth-first index of the node there."""
    return np.argsort(SR.Fast(arrays).pre)


# ---- the occurrence list: M entries ----------------------------------------------------------------------------------------

OCC_LEAVES = 1000       # 25 hubs of 40 leaves; list entry x lies on leaf x % 1000
OCC_MAX_RUN = 300


def _run_lengths(total, fixed, rng):
    """Run lengths that sum to `total`: random ones of 1 .. OCC_MAX_RUN around the runs of `fixed` [(start, length)], which begin
    exactly at their start (cut at total)."""
    lens, at = [], 0
    for start, length in list(fixed) + [(total, 0)]:
        start = min(start, total)
        while at < start:
            lens.append(min(int(rng.integers(1, OCC_MAX_RUN + 1)), start - at))
            at += lens[-1]
        if min(length, total - at) > 0:
            lens.append(min(length, total - at))
            at += lens[-1]
    assert at == total
    return lens


def occurrence_masked(M, variant, seam=KSEG):
    """The masked entries of occurrence_tree(M, variant, True): three, or with '11' the whole list behind the seam when that is 3 ..
    OCC_MAX_RUN entries, so that the head at the seam is the masked run's."""
    return M - seam if variant == "11" and 3 <= M - seam <= OCC_MAX_RUN else 3


def occurrence_tree(M, variant, masked, seam=KSEG):
    """Exactly M mutation entries on a root over 25 hubs over 40 leaves each.  Sorted by key, the list is runs of 1 .. 300 entries
    (every 50th position carries two keys: A>C and A>G); variant '11': runs begin at seam - 1 (of one entry) and at seam, '00': one
    run covers seam - 100 .. seam + 99.  masked: the last run is the masked entries, on as many leaves, at distinct negative
    positions.  (With masked entries and M <= seam + 2 the masked run covers the seam in both variants.)"""
    rng = np.random.default_rng(M + (7 if masked else 0))
    nm = occurrence_masked(M, variant, seam) if masked else 0
    fixed = [(0, 1), (1, 250 if seam > 600 else 5)]     # the shortest run, and a long one
    fixed += [(seam - 1, 1)] if variant == "11" else [(seam - 100, 200)]
    if M - nm - 1 > seam + 100:
        fixed += [(M - nm - 1, 1)]                      # the last non-masked entry is a head: alone in its segment at 2 * seam + 1
    lens = _run_lengths(M - nm, fixed, rng)
    assert len(lens) < OCC_LEAVES and max(lens) <= OCC_MAX_RUN
    leaves = [_node() for _ in range(OCC_LEAVES)]
    x, pos = 0, 99
    for i, ln in enumerate(lens):
        second = i % 50 == 8                # the position of the run before, with another allele: the larger key
        pos += 0 if second else 1
        for _ in range(ln):
            leaves[x % OCC_LEAVES][0].append((pos, A, A, G if second else C))
            x += 1
    for j in range(nm):
        leaves[x % OCC_LEAVES][0].append((-1 - j, A, A, C))
        x += 1
    assert x == M
    return _arrays(_node((), [_node((), leaves[h:h + 40]) for h in range(0, OCC_LEAVES, 40)]))


def occurrence_heads(arrays):
    """(the run heads of the sorted list as 0 / 1, the number of runs): what k_sm_heads writes and scan_flags counts."""
    key = np.sort(SR.Fast(arrays).key)
    head = np.r_[1, (key[1:] != key[:-1]).astype(np.int64)] if len(key) else np.zeros(0, np.int64)
    return head, int(head.sum())


# ---- the leaf prefix, and the ranks of a selection: N nodes -------------------------------------------------------------------

def _leaf_muts(d, seam, muts):
    return [(200 + d % 7, A, A, G)] if muts and (abs(d - seam) <= 20 or d % 5 == 0) else []


def leaf_prefix_tree(N, muts=False, seam=KSEG):
    """Exactly N nodes, written down in depth-first order: the root, then hubs over leaves as its children (and a leaf child here and
    there), and as its last child a chain c1 - c2 - c3, each with five leaves in front of the next and c3 with leaves to the end: the
    ranges of the root and the chain end at N.  When there is room, a hub of 30 leaves begins at seam - 10; otherwise (N = seam + 1) the
    chain itself straddles the seam.  Depth-first positions seam - 1 and seam are leaves.  muts: hubs, chain nodes, the root, every
    fifth leaf and the leaves around the seam carry one mutation (the genotype tests' sites); no position twice on a root path."""
    root = _node([(400, A, A, C)] if muts else ())
    sizes = itertools.cycle((7, 3, 12, 2, 9, 5, 31, 1, 4))
    at = 1

    def hub(d, leaves):
        return _node([(100 + d % 40, A, A, C)] if muts else (), [_node(_leaf_muts(d + 1 + k, seam, muts)) for k in range(leaves)])

    def hubs(end):
        nonlocal at
        while at < end:
            s = min(next(sizes), end - at)
            root[1].append(hub(at, s - 1) if s > 1 else _node(_leaf_muts(at, seam, muts)))
            at += s

    tail = min(41, N - 1)
    assert tail >= 14
    if N - tail > seam + 21:
        hubs(seam - 10)
        root[1].append(hub(at, 30))
        at += 31
    hubs(N - tail)
    chain = None
    for k, d in ((2, N - tail + 12), (1, N - tail + 6), (0, N - tail)):
        leaves = tail - 13 if k == 2 else 5
        kids = [_node(_leaf_muts(d + 1 + i, seam, muts)) for i in range(leaves)] + ([chain] if chain else [])
        chain = _node([(300 + k, A, A, T)] if muts else (), kids)
    root[1].append(chain)
    arrays = _arrays(root)
    assert arrays["n"] == N
    return arrays


def leaf_prefix_marks(N, seam=KSEG):
    """Depth-first positions of leaf_prefix_tree(N)'s chain [c1, c2, c3] and of the internal node that straddles the seam (None when
    N <= seam)."""
    tail = min(41, N - 1)
    chain = [N - tail, N - tail + 6, N - tail + 12]
    if N - tail > seam + 21:
        return chain, seam - 10
    return chain, (chain[0] if N > seam else None)


LEAF_QUERY_EDGES = (KSEG - 1, KSEG, KSEG + 1, 2 * KSEG + 1)
NEAREST_KS = (1, 4, 30, 45, 1000)      # below, at and above the 30 leaves of the hub at the seam and the 38 of the chain
WITHIN_KS = (0, 1, 2, 5)


def leaf_prefix_queries(arrays, N, seam=KSEG):
    """Breadth-first indices of the nodes the nearest and relatives tests ask about on leaf_prefix_tree(N, True): the leaves at
    depth-first positions seam - 1 and seam (where N has them), the first and the last leaf, and the chain [c1, c2, c3]."""
    d2b = dfs_to_bfs(arrays)
    leaf = np.ones(N, bool)
    leaf[np.asarray(arrays["parent"])[1:]] = False
    leaf_dfs = np.flatnonzero(leaf[d2b])
    want = [seam - 1, seam, int(leaf_dfs[0]), int(leaf_dfs[-1])] + leaf_prefix_marks(N, seam)[0]
    return d2b[[d for d in dict.fromkeys(want) if d < N]]


def node_selection(N, seam=KSEG, extra=300):
    """Depth-first positions for a genotype selection of leaf_prefix_tree(N, True): the first, those around the seam, the last, and
    `extra` more drawn with a fixed seed (internal nodes among them)."""
    rng = np.random.default_rng(N)
    want = {0, seam - 1, seam, seam + 1, N - 1} | set(rng.choice(N, min(extra, N), replace=False).tolist())
    return np.asarray(sorted(d for d in want if 0 <= d < N), np.int64)


# ---- RoHo: C candidates --------------------------------------------------------------------------------------------------------

ROHO_GROUPS = 8


def roho_tree(Cn, variant, seam=KSEG):
    """Exactly Cn RoHo candidates (entries of non-leaf nodes other than the root); candidate i of the (parent, entry) order carries
    position 1000 + i unless said otherwise.  The root's children are hubs of 3 .. 5 entries over 5 .. 9 leaves (exactly 5: no
    record; exactly 6: a record); every 11th hub's first entry repeats the first key of the hub before (the later hub owns it), every
    13th hub's first leaf repeats the hub's last key (depth + 2: erased).  Behind them come ROHO_GROUPS entry-less nodes over two or
    three sub-hubs of one entry each -- parents with an odd and an even number of other qualifying children -- whose candidates sort
    behind the root's; the first sub-hub repeats candidate 10's key two levels below the root.  Variants: with more than seam + 1
    candidates under the root a hub ends at candidate seam - 1 and the next begins at seam; '11' both are reported, '00' the first is
    erased by a leaf and the second sits over exactly 5 leaves.  The last group ends the list the same way: '11' its last two
    sub-hubs are reported, '00' the last has 5 leaves and one of them erases the key of the one before."""
    deep = [3 if g == ROHO_GROUPS - 1 else 2 + g % 2 for g in range(ROHO_GROUPS)]
    n1 = Cn - sum(deep)
    assert n1 > 20
    at_seam = n1 > seam + 1
    bounds = [seam, n1] if at_seam else [n1]
    ne_cycle, nl_cycle = (3, 4, 5, 4), (6, 7, 5, 6, 8, 6, 9, 6)
    key = lambda p: (p, A, A, C)

    def hub(keys, leaves, leaf0=()):
        return _node([key(p) for p in keys], [_node([key(p) for p in leaf0] if k == 0 else ()) for k in range(leaves)])

    kids, ci, j, prev_first, prev_special = [], 0, 0, None, True
    while ci < n1:
        ne = min(ne_cycle[j % 4], next(b for b in bounds if b > ci) - ci)
        keys, nl, leaf0, special = [1000 + ci + k for k in range(ne)], nl_cycle[j % 8], [], False
        if at_seam and ci + ne == seam:
            nl, special, leaf0 = 8, True, ([keys[-1]] if variant == "00" else [])
        elif at_seam and ci == seam:
            nl, special = (8 if variant == "11" else 5), True
        else:
            if j % 11 == 4 and not prev_special:
                keys[0] = prev_first
            if j % 13 == 6:
                leaf0 = [keys[-1]]
        kids.append(hub(keys, nl, leaf0))
        prev_first, prev_special = keys[0], special
        ci += ne
        j += 1
    for g, q in enumerate(deep):
        subs = []
        for s in range(q):
            keys, nl, leaf0 = [1000 + ci], 6 + (g + s) % 4, []
            if g == 0 and s == 0:
                keys = [1010]
            if g == ROHO_GROUPS - 1 and variant == "00" and s == 2:
                nl, leaf0 = 5, [1000 + ci - 1]
            subs.append(hub(keys, nl, leaf0))
            ci += 1
        kids.append(_node((), subs))
    assert ci == Cn
    return _arrays(_node((), kids))


def roho_order(arrays, F=None):
    """The candidates (indices into the mutation arrays) in the order of k_sm_candkey's sort: by the parent's depth-first position,
    then depth-first entry order."""
    F = F or SR.Fast(arrays)
    inner = ~F.leaf
    inner[0] = False
    ce = np.flatnonzero(inner[F.node])
    return ce[np.lexsort((ce, F.pre[F.node[ce]], F.pre[F.par[F.node[ce]]]))]


def roho_flags(arrays, F=None, records=None):
    """Per candidate of roho_order: 1 when the reference reports it."""
    F = F or SR.Fast(arrays)
    records = F.roho()[0] if records is None else records
    return np.isin(roho_order(arrays, F), np.asarray([r[4] for r in records], np.int64)).astype(np.int64)


# ---- translate: I work-items -----------------------------------------------------------------------------------------------------

def _tmut(p, k=1):
    ref = TC.GENOME[p - 1]
    return (p, SR.NUC.index(ref, 1), SR.NUC.index(ref, 1), SR.NUC.index(TC._other(ref, k), 1))


class TranslateCase(TC.Case):
    """A translate_cases.Case around ready arrays, on the default genome and GTF."""

    def __init__(self, name, arrays, device=True):
        self.name, self.rule, self.device, self.lines, self.fasta, self.gtf = name, "", device, None, TC.FASTA, TC.GTF
        self.arrays, self.tags, self.counts = arrays, {}, {}


def _translate_units():
    """Unit -> (its nodes in depth-first order as one child of the root, its items' flags)."""
    one = lambda i: (_node([_tmut(1 + i % 3, 1 + (i // 3) % 3)]), [1])                      # star600's leaves
    six = lambda i: (_node([_tmut(6, 1 + i % 3)]), [1, 1])                                  # position 6: codons A:2 and C:1
    two = lambda i: (_node([_tmut(3, 1 + i % 3), _tmut(1, 1 + i % 2)]), [1, 0])             # two mutations in codon A:1: one record
    three = lambda i: (_node([_tmut(2), _tmut(3, 2), _tmut(1, 1 + i % 3)]), [1, 0, 0])
    # an inner node A1C over C1G (the state from the parent) and T2C (slot 0 read from the parent)
    inner = lambda i: (_node([(1, A, A, C)], [_node([(1, A, C, G)]), _node([(2, T, T, C)])]), [1, 1, 1])
    return {"one": one, "six": six, "two": two, "three": three, "inner": inner}


def translate_tree(In, variant, seam=KSEG, refused=False):
    """Exactly In work-items on translate_cases.GENOME / GTF: a star whose children are star600's leaves (1 item, 1 record), leaves at
    position 6 (2 items, 2 records), leaves with two or three mutations in codon A:1 (2 or 3 items, 1 record) and, every 50th, an
    inner node with two leaves (3 items, 3 records).  Variant '11': items seam - 1 and seam are two one-mutation leaves; '00': they
    are the second and third item of a three-mutation leaf.  refused: the last item's owner stores a wrong parent allele (its node
    must be a one-mutation leaf: variant '11' with In = seam + 1)."""
    units = _translate_units()
    cycle = ("one", "six", "two", "one", "one", "three", "six", "one")
    kids, flags, n = [], [], 0

    def put(name):
        nd, f = units[name](len(kids))
        kids.append(nd)
        flags.extend(f)

    def fill(end):
        nonlocal n
        while len(flags) < end:
            name = "inner" if n % 50 == 49 else cycle[n % 8]
            n += 1
            put(name if len(flags) + len(units[name](0)[1]) <= end else "one")

    if In > seam:
        if variant == "11":
            fill(seam - 1)
            put("one")
            put("one")
        else:
            fill(seam - 2)
            put("three")
    fill(In)
    assert len(flags) == In
    if refused:
        p, ref, par, nuc = kids[-1][0][0]
        assert len(kids[-1][0]) == 1 and not kids[-1][1]
        kids[-1][0][0] = (p, ref, next(b for b in (A, C, G, T) if b not in (par, nuc)), nuc)
    arrays = _arrays(_node((), kids))
    return TranslateCase("translate%d_%s%s" % (In, variant, "_refused" if refused else ""), arrays, not refused), np.asarray(flags, np.int64)


@functools.lru_cache(maxsize=None)
def translate_slots():
    return TR.slot_tables(TR.build_codon_map(TC.GTF, TR.build_reference(TC.FASTA)))


def translate_items(arrays):
    """ugp_translate's work-items, vectorised: per (node, coding position) once, the codons of the position."""
    slot_pos = translate_slots()[0]
    per = np.bincount(slot_pos.reshape(-1), minlength=int(max(slot_pos.max(), np.asarray(arrays["mut_pos"]).max(initial=0))) + 1)
    pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
    node = np.repeat(np.arange(arrays["n"]), np.diff(np.asarray(arrays["mut_off"]).astype(np.int64)))
    keep = pos >= 0
    pairs = np.unique(node[keep] * (len(per) + 1) + pos[keep])
    return int(per[pairs % (len(per) + 1)].sum())


# ---- genotypes: P positions with owners --------------------------------------------------------------------------------------------

def genotype_positions_tree(P):
    """A star of P leaves; leaf i alone mutates position i + 1: P positions have owners, and one is a site exactly when its leaf is
    selected."""
    return _arrays(_node((), [_node([(i + 1, A, A, C)]) for i in range(P)]))


def position_selection(P, extra=200):
    """Leaves (as 0-based leaf numbers; the node is the number + 1) at the 16-position and the tile edges, and `extra` more drawn with
    a fixed seed."""
    rng = np.random.default_rng(P)
    want = {0, 15, 16, 17, GT_TILE - 1, GT_TILE, GT_TILE + 1, P - 1} | set(rng.choice(P, min(extra, P), replace=False).tolist())
    return np.asarray(sorted(i for i in want if 0 <= i < P), np.int64)
