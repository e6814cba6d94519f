"""Hand-shaped trees for the RIPPLES search (ugp_ripples, usher_amd/csrc/ugp_ripples.hip): every case puts one edge of the
kernels k_count / k_pairs / k_merge where the events depend on it -- tile, chunk and block counts, the pair count against the
block, the LDS tile of a long sample, ambiguous and masked alleles, ties in the sort key, the budget and the pair-validity
limits at equality, every clause of the eligibility rule.  tests/test_ripples_cases_cpu.py shows that each case reaches its
edge; tests/test_ripples_edges_gpu.py runs them on the device.

A case is (name, arrays, branches, name_rank, opts, limits): breadth-first arrays with names, the branch list, the rank of
every node's name, the options of ripples_ref.literal / closed, and None or a UGP_RIPPLES_LIMITS string.  INFO[name] holds
what the CPU test asserts about it (node ids are breadth-first).

Most trees are stars: the branch nid mutates M sample positions, every other node repeats a subset ("mask") of those rows
and nothing else, so its unmatched set U is the rows outside its mask: for a pair (i, j) its donor count is the number of
rows of [i, j) outside the mask, its acceptor count the number of the others outside it.  Nodes with one mask tie in both
counts, and the name rank -- which the builder hands out -- decides."""
import numpy as np

from tests import ripples_ref as RR

# the constants of the sources (tests/test_ripples_cases_cpu.py keeps them equal)
KBLOCK, KTILEMAX, KLDSINTS = 256, 64, 12288
KCOUNT, KSLAB = 1 << 29, 1 << 28
BIG = 10 ** 7


def REF(p):
    return (1, 2, 4, 8)[p % 4]


def alt(p, k=0):
    """The k-th base that is not the reference base at p."""
    return [b for b in (1, 2, 4, 8) if b != REF(p)][k % 3]


# ---- the formulas of rip_run -----------------------------------------------------------------------------------------

def limits_for(M, P, Cc=None, T=None, nblk=None):
    """The UGP_RIPPLES_LIMITS string that forces a chunk length, a tile (>= 2) and a number of slab rows."""
    count = KCOUNT if Cc is None else 4 * (2 * M + 2) * Cc
    slab = KSLAB if nblk is None else 48 * P * nblk
    lds = KLDSINTS if T is None else (2 * M + 2) * (T + 1)
    return "%d,%d,%d" % (count, slab, lds)


def geometry(M, P, C, limits=None):
    """Cc, tile, nblk as rip_run derives them, the chunk lengths, and the tiles each block folds (summed over the chunks)."""
    count, slab, lds = KCOUNT, KSLAB, KLDSINTS
    if limits:
        a, b, c = (int(x) for x in limits.split(","))
        count, slab, lds = max(1, min(a, KCOUNT)), max(1, min(b, KSLAB)), max(1, min(c, KLDSINTS))
    nb = 2 * M + 1
    Cc = max(1, min(C, count // (4 * (nb + 1))))
    fit = lds // (nb + 1)
    tile = min(KTILEMAX, fit - 1) if fit >= 2 else 1
    tiles_all = (C + tile - 1) // tile
    nblk = max(1, min(1024, tiles_all, slab // (48 * P)))
    chunks = [min(Cc, C - c0) for c0 in range(0, C, Cc)]
    folds = [0] * nblk
    block_of = {}   # candidate index -> the block that folds it
    for ci, cc in enumerate(chunks):
        nt = (cc + tile - 1) // tile
        grid = min(nblk, nt)
        for g in range(nt):
            folds[g % grid] += 1
            for c in range(g * tile, min(cc, (g + 1) * tile)):
                block_of[ci * Cc + c] = g % grid
    return {"Cc": Cc, "tile": tile, "nblk": nblk, "chunks": chunks, "folds": folds, "block_of": block_of,
            "last_tiles": [cc - (cc - 1) // tile * tile for cc in chunks],
            "count_blocks": [(cc + KBLOCK - 1) // KBLOCK for cc in chunks]}


# ---- trees ----------------------------------------------------------------------------------------------------------------

class Builder:
    """Nodes in any order; a mutation is (pos, nuc) -- the reference base is REF(pos) -- or (pos, nuc, ref), which a masked
    one (pos < 0) needs.  finish() numbers breadth-first, fills in the parent states and hands out the names."""

    def __init__(self, root=()):
        self.par, self.muts = [-1], [list(root)]

    def add(self, parent, muts=()):
        self.par.append(parent)
        self.muts.append(list(muts))
        return len(self.par) - 1

    def leaves(self, parent, k, muts=()):
        return [self.add(parent, muts) for _ in range(k)]

    def finish(self, first=(), last=()):
        """(arrays, ids): ids[builder id] = breadth-first id.  The nodes of `first` get the name ranks 0, 1, ..; those of
        `last` the highest; the others rank against the breadth-first order, so that byte order never follows it."""
        n = len(self.par)
        kids = [[] for _ in range(n)]
        for v in range(1, n):
            kids[self.par[v]].append(v)
        order, h = [0], 0
        while h < len(order):
            order.extend(kids[order[h]]); h += 1
        ids = [0] * n
        for i, o in enumerate(order):
            ids[o] = i
        state, node_muts = [None] * n, []
        for o in order:
            g = dict(state[self.par[o]]) if o else {}
            out = []
            for m in self.muts[o]:
                p, nuc = m[0], m[1]
                ref = m[2] if len(m) > 2 else REF(p)
                out.append((p, ref, ref if p < 0 else g.get(p, ref), nuc))
            for (p, _, _, nuc) in out:
                if p >= 0:
                    g[p] = nuc
            state[o] = g
            node_muts.append(out)
        rest = [o for o in reversed(order) if o not in set(first) | set(last)]
        rank = {o: r for r, o in enumerate(list(first) + rest + list(last))}
        assert len(rank) == n
        names = ["n%04d" % rank[o] for o in order]
        arrays = RR._bfs_arrays([-1] + [ids[self.par[o]] for o in order[1:]], node_muts, names)
        assert arrays["parent"].tolist() == [-1] + [ids[self.par[o]] for o in order[1:]]
        return arrays, ids


def renamed(arrays, how):
    """The same tree with the name ranks reversed or rotated by a third."""
    rank = RR.name_ranks(arrays).astype(np.int64)
    n = len(rank)
    new = (n - 1 - rank) if how == "reversed" else (rank + n // 3) % n
    out = dict(arrays)
    out["names"] = ["n%04d" % r for r in new]
    return out


POS6 = [1000, 2000, 3000, 4000, 5000, 6000]


def share(pos, mask):
    return [(pos[q], alt(pos[q])) for q in sorted(mask)]


def o3(**kw):
    """l = 3 on six rows: the pairs (0, 3), (1, 4), (2, 5)."""
    o = dict(l=3, r=0, R=BIG, p=3, n_desc=1)
    o.update(kw)
    return o


CASES, INFO = [], {}


def case(name, arrays, branches, opts, limits=None, **info):
    CASES.append((name, arrays, [int(b) for b in branches], RR.name_ranks(arrays), opts, limits))
    info.setdefault("events", True)
    INFO[name] = info


T0, T1, T3, TC, FULL = {0, 1, 2}, {1, 2, 3}, {3, 4, 5}, {0, 4, 5}, {0, 1, 2, 3, 4, 5}


# ---- tile_and_block_counts ------------------------------------------------------------------------------------------------

def _threshold_tree(C, nd=4):
    """C candidates at num_descendants = nd: the root and C - 1 children of nd nodes, masks T0 / T3 in turn; the last two
    (one of each mask) hold the lowest ranks.  Left out at nd - 1 nodes: nid and three children whose mask is every row."""
    b = Builder()
    nid = b.add(0, share(POS6, FULL))
    b.leaves(nid, nd - 2)
    thr = []
    for t in range(C - 1):
        v = b.add(0, share(POS6, T0 if (C - 2 - t) % 2 == 0 else T3))
        b.leaves(v, nd - 1)
        thr.append(v)
    small = []
    for _ in range(3):
        v = b.add(0, share(POS6, FULL))
        b.leaves(v, nd - 2)
        small.append(v)
    arrays, ids = b.finish(first=thr[::-1][:2])
    return arrays, ids[nid], [ids[v] for v in thr], [ids[v] for v in small]


for _C in (1, 2, 63, 64, 65, 255, 256, 257):
    _arr, _nid, _thr, _small = _threshold_tree(max(_C, 2))
    _nd = 4 if _C > 1 else _arr["n"]
    case("tile_and_block_counts/C%d" % _C, _arr, [_nid], o3(n_desc=_nd), C=_C, nd=_nd, threshold=_thr if _C > 1 else [0],
         left_out=_small + [_nid] if _C > 1 else [], events=_C > 1)


# ---- partial_tile_in_every_chunk ------------------------------------------------------------------------------------------

def _chunk_tree():
    """336 nodes, all candidates: the root, nid (1), X (2), leaves 3 .. 140 of the root, ten leaves of nid (141 .. 150, the
    lowest ranks: they win every list unless their flag says "under nid"), leaves 151 .. 335 of X.  The winners sit at
    99, 100, 199 and 335."""
    b = Builder()
    nid = b.add(0, share(POS6, FULL))
    X = b.add(0)
    want = {99: T0, 100: T3, 199: T1, 335: TC}
    cyc = (T0, T3, T1, TC)
    at = {}
    for idx in range(3, 141):
        at[idx] = b.add(0, share(POS6, want.get(idx, cyc[idx % 4])))
    under = b.leaves(nid, 10)
    for idx in range(151, 336):
        at[idx] = b.add(X, share(POS6, want.get(idx, cyc[idx % 4])))
    arrays, ids = b.finish(first=under + [at[99], at[100], at[199], at[335]])
    assert all(ids[v] == idx for idx, v in at.items()) and [ids[v] for v in under] == list(range(141, 151))
    return arrays, ids[nid]


_arr, _nid = _chunk_tree()
case("partial_tile_in_every_chunk", _arr, [_nid], o3(), limits_for(6, 3, Cc=100), C=336, M=6, P=3, winners={99, 100, 199, 335},
     under=list(range(141, 151)))


# ---- grid_stride_with_wide_tiles ------------------------------------------------------------------------------------------

def _stride_tree(spread):
    """600 nodes, all candidates: the root, nid (1) and 598 leaves of the root with the masks T0 / T3 in turn.  spread: nid
    has rank 0 and heads both lists; a node that shares every row (300) and a T0 (599) follow, a T3 (24) after them: with
    tiles of 8 and three blocks the top three donors lie in blocks 0, 1 and 2.  Otherwise nid ranks last and the lowest ranks
    lie at 597 (every row), 598, 596 (T0) and 599 (T3): the tile that block 2 folds last."""
    b = Builder()
    nid = b.add(0, share(POS6, FULL))
    want = {300: FULL, 599: T0, 24: T3} if spread else {597: FULL, 598: T0, 596: T0, 599: T3}
    at = {idx: b.add(0, share(POS6, want.get(idx, (T0, T3)[idx % 2]))) for idx in range(2, 600)}
    if spread:
        arrays, ids = b.finish(first=[nid, at[300], at[599], at[24]])
    else:
        arrays, ids = b.finish(first=[at[597], at[598], at[599], at[596]], last=[nid])
    assert all(ids[v] == idx for idx, v in at.items())
    return arrays, ids[nid]


for _spread in (True, False):
    _arr, _nid = _stride_tree(_spread)
    for _cc in (None, 100):
        _tag = "%s%s" % ("three_blocks" if _spread else "last_tile", "_chunks" if _cc else "")
        case("grid_stride_with_wide_tiles/" + _tag, _arr, [_nid],
             o3(), limits_for(6, 3, Cc=_cc, T=8, nblk=3), C=600, M=6, P=3, spread=_spread, chunked=bool(_cc),
             top3=[1, 300, 599] if _spread else [597, 598, 596])


# ---- pairs_across_the_block -----------------------------------------------------------------------------------------------

def _caterpillar():
    """A chain of six nodes of six mutations each below the root, at 36 shuffled positions (M = 36 for the last, nid); every
    chain node has a leaf that repeats some rows of the nodes below it, nid has three siblings that repeat most of its rows."""
    rng = np.random.default_rng(41)
    pos = np.sort(rng.choice(np.arange(100, 29000), 36, replace=False)).tolist()
    level = rng.permutation(36) % 6
    b = Builder()
    spine, v = [], 0
    for d in range(6):
        v = b.add(v, [(p, alt(p)) for q, p in enumerate(pos) if level[q] == d])
        spine.append(v)
    own = [p for q, p in enumerate(pos) if level[q] == 5]
    for d in range(5):
        deeper = [p for q, p in enumerate(pos) if level[q] > d]
        b.add(spine[d], [(p, alt(p)) for p in deeper[d::3]])
    for k in range(3):
        b.add(spine[4], [(p, alt(p)) for x, p in enumerate(own) if x != k and x != k + 3])
    arrays, ids = b.finish()
    return arrays, ids[spine[5]], pos


def _range_for(pos, l, target):
    """A max_range at which exactly `target` pairs are valid."""
    spans = sorted({pos[j - 1] - pos[i] for i in range(len(pos)) for j in range(i + 1, len(pos))})
    for R in spans:
        if len(RR.valid_pairs(pos, l, 0, R)) == target:
            return R
    raise AssertionError("no max_range gives %d pairs" % target)


_arr, _nid, _pos = _caterpillar()
for _P in (255, 256, 257):
    case("pairs_across_the_block/P%d" % _P, _arr, [_nid], dict(l=3, r=0, R=_range_for(_pos, 3, _P), p=3, n_desc=1), M=36, P=_P)
case("pairs_across_the_block/P558", _arr, [_nid], dict(l=3, r=0, R=BIG, p=3, n_desc=1), M=36, P=558)


# ---- narrow_lds_tile, mixed_call ----------------------------------------------------------------------------------------------

def spine_tree(M, C, seed):
    """A chain s1 .. s12 below the root; nid = s12 has eight mutations, the other rows are dealt round to s1 .. s11, at the
    positions 50 q + 7.  Nine rows of s9 .. s11 are mutated three times on the way down (to the sample's base, away from it,
    and back: the telescoping term changes sign twice).  Leaves hang mostly on the lowest chain nodes and repeat, or miss,
    rows of the nodes below their parent; some mutate a position outside the sample.  Two more children of the root: m2 (two
    mutations, two leaves) and m1 (one mutation).  C nodes in all.  Returns (arrays, ids by name)."""
    rng = np.random.default_rng(seed)
    pos = [50 * q + 7 for q in range(M)]
    level = {}
    own = set(int(x) for x in rng.choice(M, 8, replace=False))
    q2 = 0
    for q in range(M):
        if q in own:
            level[q] = 12
        else:
            level[q] = 1 + q2 % 11
            q2 += 1
    per = {d: {} for d in range(1, 13)}
    for q in range(M):
        per[level[q]][pos[q]] = alt(pos[q])
    triple = [q for q in range(M) if level[q] in (9, 10, 11)][:9]
    for q in triple:
        per[level[q] - 8][pos[q]] = alt(pos[q])
        per[level[q] - 4][pos[q]] = alt(pos[q], 1)
    b = Builder()
    spine, v = [0], 0
    for d in range(1, 13):
        v = b.add(v, sorted(per[d].items()))
        spine.append(v)
    m2 = b.add(0, [(50 * 3 + 31, alt(50 * 3 + 31)), (50 * 9 + 31, alt(50 * 9 + 31))])
    b.leaves(m2, 2)
    m1 = b.add(0, [(50 * 5 + 31, alt(50 * 5 + 31))])
    hang = (11, 11, 10, 9, 11, 5, 10, 2, 11, 0, 8, 11)
    t, leaf = 0, None
    while len(b.par) < C:
        d = hang[t % len(hang)]
        deeper = [q for q in range(M) if level[q] > d]
        muts = {}
        for q in rng.choice(deeper, int(rng.integers(0, 4)), replace=False):
            muts[pos[q]] = alt(pos[q], 0 if rng.random() < 0.7 else 2)
        if rng.random() < 0.25:
            p = 50 * int(rng.integers(0, M)) + 30
            muts[p] = alt(p)
        v = b.add(spine[d], sorted(muts.items()))
        if d == 10 and len(muts) >= 2:
            leaf = v
        t += 1
    arrays, ids = b.finish()
    return arrays, {"nid": ids[spine[12]], "m2": ids[m2], "m1": ids[m1], "leaf": ids[leaf], "triple": [pos[q] for q in triple]}


_SPINES = {}
for _M in (93, 95, 96, 120):   # fit = 12288 / (2M + 2) = 65, 64, 63, 50: the tile is min(64, fit - 1)
    _arr, _ids = spine_tree(_M, 130, 60 + _M)
    _SPINES[_M] = (_arr, _ids)
    _l = _M // 2 - 2
    case("narrow_lds_tile/M%d" % _M, _arr, [_ids["nid"]], dict(l=_l, r=0, R=BIG, p=0, n_desc=1), M=_M, C=130,
         tile={93: 64, 95: 63, 96: 62, 120: 49}[_M], triple=_ids["triple"])

_arr, _ids = _SPINES[96]
_MIXED = [_ids["nid"], _ids["m2"], _ids["m1"], 0, _ids["leaf"]]
for _tag, _nd in (("nd1", 1), ("nd3", 3), ("nd1_again", 1)):
    case("mixed_call/" + _tag, _arr, _MIXED, dict(l=1, r=0, R=120, p=0, n_desc=_nd), nd=_nd)


# ---- alleles --------------------------------------------------------------------------------------------------------------

def _alleles_tree(iupac):
    """iupac = False: the same tree with the first base of every ambiguous allele.  ugp_mat_create refuses ambiguous tree
    alleles, ugp_ripples_attach takes them: the ambiguous case runs on the handle of the one-hot tree (INFO[...]["handle"]),
    with its own arrays attached."""
    amb = (lambda x, y: x | y) if iupac else (lambda x, y: x)
    b = Builder(root=[(0, alt(0))])
    a = b.add(0, [(10, amb(alt(10), REF(10)) if iupac else alt(10)), (20, amb(alt(20), alt(20, 1))), (30, alt(30)),
                  (50, alt(50))])
    bb = b.add(a, [(30, REF(30)), (40, alt(40)), (60, alt(60))])
    nid = b.add(bb, [(70, alt(70)), (80, amb(alt(80), alt(80, 1))), (90, alt(90))])
    e = {}
    e["own_is_lowbit"] = b.add(bb, [(20, alt(20))])
    e["own_third_base"] = b.add(bb, [(20, alt(20, 2)), (70, alt(70))])
    e["root_third_base"] = b.add(0, [(20, alt(20, 2))])
    e["in_row_with_ref"] = b.add(0, [(10, alt(10))])
    e["outside_row_with_ref"] = b.add(0, [(10, alt(10, 1))])
    d1 = b.add(0, [(10, amb(alt(10), alt(10, 1)))])
    e["iupac_own"] = d1
    e["iupac_above"] = b.add(d1, [(20, alt(20)), (70, alt(70))])
    e["replaces_iupac"] = b.add(d1, [(10, alt(10, 2))])
    f = b.add(0, [(5, amb(alt(5), alt(5, 1)))])
    e["between_rows"] = f
    e["at_dropped"] = b.add(f, [(30, alt(30))])
    e["at_dropped_below_bb"] = b.add(bb, [(30, alt(30, 1)), (80, alt(80))])
    # a branch without the root's row at 0: the reversion takes the position, so the root's mutation lies below its first row
    g = b.add(0, [(0, REF(0)), (33, alt(33)), (44, alt(44)), (55, alt(55)), (66, alt(66))])
    e["g_half"] = b.add(0, [(0, REF(0)), (33, alt(33)), (44, alt(44))])
    e["g_other_half"] = b.add(0, [(0, REF(0)), (55, alt(55)), (66, alt(66))])
    # a branch with an ambiguous row that excludes the reference base, among siblings: one stops loop 1 at a masked mutation
    # and then repeats the row's lowest base, one repeats it in the ordinary way
    h = b.add(0, [(20, amb(alt(20), alt(20, 1))), (25, alt(25)), (35, alt(35)), (45, alt(45))])
    e["masked_then_lowbit"] = b.add(0, [(-1, 2, 1), (20, alt(20)), (25, alt(25))])
    e["plain_lowbit"] = b.add(0, [(20, alt(20)), (25, alt(25))])
    e["second_bit"] = b.add(0, [(20, alt(20, 1)), (35, alt(35)), (45, alt(45))])
    arrays, ids = b.finish(first=[e["masked_then_lowbit"], e["own_is_lowbit"]])
    return arrays, [ids[nid], ids[g], ids[h]], {k: ids[v] for k, v in e.items()}


_one_hot = _alleles_tree(False)[0]
for _tag, _iupac in (("alleles/iupac", True), ("alleles/one_hot", False)):
    _arr, _br, _e = _alleles_tree(_iupac)
    case(_tag, _arr, _br, dict(l=2, r=0, R=BIG, p=0, n_desc=1), nodes=_e, iupac=_iupac, handle=_one_hot if _iupac else None)


# ---- masked ---------------------------------------------------------------------------------------------------------------

def _masked_tree():
    b = Builder(root=[(-7, 2, 1), (-3, 4, 4), (100, alt(100))])
    a = b.add(0, [(-9, 8, 1), (200, alt(200)), (300, alt(300))])
    # nidA overrides the root's masked position with a reversion: rows -9 and -5, none at -7
    nidA = b.add(a, [(-7, 1, 1), (-5, 2, 4), (400, alt(400)), (500, alt(500)), (600, alt(600))])
    nidB = b.add(0, [(150, alt(150)), (250, alt(250)), (350, alt(350))])
    b.leaves(nidB, 2)
    e = {}
    e["masked_first"] = b.add(a, [(-2, 2, 1), (400, alt(400))])
    e["plain"] = b.add(a, [(500, alt(500))])
    e["masked_first_inner"] = b.add(a, [(-2, 2, 1), (500, alt(500)), (600, alt(600))])
    b.leaves(e["masked_first_inner"], 1, [(400, alt(400))])
    e["masked_last"] = b.add(a, [(400, alt(400)), (-4, 2, 1), (600, alt(600))])
    e["shares_150"] = b.add(0, [(150, alt(150))])
    e["shares_250"] = b.add(0, [(250, alt(250)), (350, alt(350))])
    arrays, ids = b.finish(first=[0, e["masked_first"], e["masked_first_inner"]])
    return arrays, [ids[nidA], 0, ids[nidB]], {k: ids[v] for k, v in e.items()}


_arr, _br, _e = _masked_tree()
case("masked", _arr, _br, dict(l=1, r=0, R=BIG, p=0, n_desc=1), nodes=_e)


# ---- ties_and_nid ---------------------------------------------------------------------------------------------------------

def _ties_tree(kind):
    """A polytomy Q of 300 leaves with one mask.  'd1a2': nid is one of them and every leaf repeats all of its rows: every
    count is 0, nid heads both lists, the best donor is the best acceptor and the event is (d1, a2).  'd2a1': nid hangs beside
    Q; the leaves share rows 0, 1, 3 and x (a child of the root) all but row 2, with B = 2: for the pair (0, 3) the leaves count
    (1, 2) and x (1, 0), so (x, leaf) costs 3 and the event is (d2, a1) = (leaf, x).  The lowest ranks after nid lie on x, the
    last leaf and the leaf at candidate 64."""
    b = Builder()
    Q = b.add(0)
    if kind == "d1a2":
        lv = b.leaves(Q, 150, share(POS6, FULL))
        nid = b.add(Q, share(POS6, FULL))
        lv += b.leaves(Q, 150, share(POS6, FULL))
        first = [nid, lv[-1], lv[62], lv[0]]
    else:
        nid = b.add(0, share(POS6, FULL))
        x = b.add(0, share(POS6, {0, 1, 3, 4, 5}))
        lv = b.leaves(Q, 300, share(POS6, {0, 1, 3}))
        first = [nid, x, lv[-1], lv[60]]
    arrays, ids = b.finish(first=first)
    return arrays, ids[nid], [ids[v] for v in first]


for _kind in ("d1a2", "d2a1"):
    _arr, _nid, _first = _ties_tree(_kind)
    for _how in ("plain", "reversed", "rotated"):
        _a = _arr if _how == "plain" else renamed(_arr, _how)
        case("ties_and_nid/%s_%s" % (_kind, _how), _a, [_nid], o3(p=3 if _kind == "d1a2" else 4), kind=_kind, how=_how,
             first=_first)


# ---- budget_edges ---------------------------------------------------------------------------------------------------------

def _budget_tree():
    """nid with six rows and leaves with the masks {0, 3, 4, 5} (two rows of [0, 3) missing) and {3, 4, 5} (three missing); a
    second branch with six rows of its own and leaves that repeat one half each."""
    b = Builder()
    nid = b.add(0, share(POS6, FULL))
    for mask in ({0, 3, 4, 5}, {3, 4, 5}) * 4:
        b.add(0, share(POS6, mask))
    pos2 = [p + 10000 for p in POS6]
    nid2 = b.add(0, share(pos2, FULL))
    for mask in (T0, T3) * 2:
        b.add(0, share(pos2, mask))
    arrays, ids = b.finish()
    return arrays, [ids[nid], ids[nid2]]


_arr, _br = _budget_tree()
for _p in (4, 5, 6, 7):
    case("budget_edges/p%d" % _p, _arr, _br, o3(p=_p), p=_p, events=_p < 7)


# ---- pair_validity_edges --------------------------------------------------------------------------------------------------

VALIDITY_POS = [-4, 1000, 2100, 3300, 4600, 6000]   # spans of (0, 3), (1, 4), (2, 5): 2104, 2300, 2500


def _validity_tree():
    b = Builder()
    nid = b.add(0, [(-4, 2, 1)] + share(VALIDITY_POS, {1, 2, 3, 4, 5}))
    for mask in ({1, 2}, {3, 4, 5}, {1, 2, 3}, {4, 5}, {2, 3, 4}, {1, 5}) * 2:
        b.add(0, share(VALIDITY_POS, mask))
    short = b.add(0, [(p, alt(p)) for p in (1500, 2500, 3500, 4500)])   # M = 4 < 2 l
    b.leaves(short, 2)
    arrays, ids = b.finish()
    return arrays, [ids[nid], ids[short]]


_arr, _br = _validity_tree()
for _tag, _kw, _pairs in (("r_eq", dict(r=2300), [(1, 4), (2, 5)]), ("r_plus", dict(r=2301), [(2, 5)]),
                          ("R_eq", dict(R=2300), [(0, 3), (1, 4)]), ("R_minus", dict(R=2299), [(0, 3)]),
                          ("r_eq_masked", dict(r=2104), [(0, 3), (1, 4), (2, 5)]),
                          ("r_plus_masked", dict(r=2105), [(1, 4), (2, 5)])):
    case("pair_validity_edges/" + _tag, _arr, _br, o3(p=2, **_kw), pairs=_pairs)


# ---- eligibility_and_sibling ----------------------------------------------------------------------------------------------

def _elig_tree():
    """nid (a leaf, six rows) and, under the root:
      Ic   internal, rows 0-4, nothing else: eligible by 'none unique, all common', set difference 1
      X    internal child of Ic with one mutation below the first row: has unique, none common: not eligible; a mutation
           that loop 1 does not keep changes no count, so X ties with Ic everywhere and the rank puts it first
      Iuc  internal, rows 1-5 and a mutation above the last row: unique and common, set difference 1
      Lc   a leaf with rows 0-2
    and a second branch nid2 (rows at 11000 ..) with a leaf Lc2 that repeats its first three rows: there the root is the best
    partner.  At num_descendants = 2 the candidates are the root, Ic, X and Iuc, the smallest eligible set difference is 1 and
    Ic and Iuc tie at it; at 1 nid itself is a candidate and alone at the minimum, and the leaves win."""
    b = Builder()
    nid = b.add(0, share(POS6, FULL))
    Ic = b.add(0, share(POS6, {0, 1, 2, 3, 4}))
    X = b.add(Ic, [(500, alt(500))])
    b.leaves(X, 1, [(700, alt(700))])
    Iuc = b.add(0, share(POS6, {1, 2, 3, 4, 5}) + [(7000, alt(7000))])
    b.leaves(Iuc, 1, [(800, alt(800)), (900, alt(900))])
    Lc = b.add(0, share(POS6, T0))
    pos2 = [p + 10000 for p in POS6]
    nid2 = b.add(0, share(pos2, FULL))
    Lc2 = b.add(0, share(pos2, T0))
    arrays, ids = b.finish(first=[0, X, Ic, Lc, Iuc, Lc2])
    return arrays, [ids[nid], ids[nid2]], {"Ic": ids[Ic], "X": ids[X], "Iuc": ids[Iuc], "Lc": ids[Lc], "Lc2": ids[Lc2], "root": 0}


_arr, _br, _e = _elig_tree()
case("eligibility_and_sibling/internal", _arr, _br, o3(n_desc=2), nodes=_e)
case("eligibility_and_sibling/leaves", _arr, _br, o3(n_desc=1), nodes=_e)


def by_name(name):
    return next(c for c in CASES if c[0] == name)
