"""Hand-shaped trees and samples for ugp_vectors (tests/test_vectors_cpu.py, tests/test_vectors_gpu.py): every edge of
usher_amd/csrc/ugp_vectors.hip by name.  A case is a dict: name, arrays (BFS flat arrays), samples (row dicts), pairs (a list of
(sample, node), every pair of the case unless it says otherwise) and refused (the nodes whose pairs are refused: only `twice`).
Behind the hand cases, generators that take their sizes as parameters (wide, ragged_path, random_case, seam_pairs) and the sizes the
GPU module picks of them; tests/test_vectors_cpu.py runs them all and proves that the picks lie on the kernel's steps.

The reference base of position p is REF(p) everywhere, so that the rows pass the checks of ugp_place_batch on a handle that holds
the tree's own mutations; stored parent alleles are the true states above.  One edge of the issue cannot be reached: an entry of
part 2 has nuc != par for every row the row checks admit (nuc is a bit of the row, or its reference, and neither is the ancestral
state when the row does not hold that state), so `nuc == par gives no excess entry` only ever shows as the absence of an entry for
rows that agree with g(p), which every case has.
"""
import numpy as np

ONEHOT = (1, 2, 4, 8)
A, C, G, T = ONEHOT


def REF(p):
    return ONEHOT[p % 4]


def other(a, k=0):
    """The k-th single base that is not a."""
    return [b for b in ONEHOT if b != a][k % 3]


def arrays_of(parent, muts):
    """muts[j]: the entries of node j in stored order, (pos, nuc) or (pos, nuc, ref) -- pos < 0: masked, ref as given."""
    n = len(parent)
    state, off, rows = [None] * n, [0], []
    for j in range(n):
        st = dict(state[parent[j]]) if j else {}
        for m in muts[j]:
            p, nuc = m[0], m[1]
            ref = m[2] if len(m) > 2 else REF(p)
            rows.append((p, ref, st.get(p, ref), nuc))
            if p >= 0 and p not in [q[0] for q in muts[j][:muts[j].index(m)]]:
                st[p] = nuc
        state[j] = st
        off.append(len(rows))
    r = np.asarray(rows, np.int64).reshape(-1, 4)
    return {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": np.asarray(off, np.int64), "mut_pos": r[:, 0].astype(np.int32),
            "mut_ref": r[:, 1].astype(np.int8), "mut_par": r[:, 2].astype(np.int8), "mut_nuc": r[:, 3].astype(np.int8),
            "names": ["n%d" % j for j in range(n)]}


def sample(rows, name="s"):
    """rows: (pos, allele) or (pos, None) for a missing row, ascending positions."""
    rows = sorted(rows)
    return {"name": name, "pos": np.asarray([p for p, _ in rows], np.int32), "ref": np.asarray([REF(p) for p, _ in rows], np.int8),
            "nuc": np.asarray([15 if a is None else a for _, a in rows], np.int8),
            "is_missing": np.asarray([a is None for _, a in rows], np.int8)}


def case(name, parent, muts, samples, pairs=None, refused=()):
    arrays = arrays_of(parent, muts)
    if pairs is None:
        pairs = [(s, j) for s in range(len(samples)) for j in range(len(parent))]
    return {"name": name, "arrays": arrays, "samples": samples, "pairs": pairs, "refused": set(refused)}


def _root():
    # the root with own entries: off its reference, on its reference, masked off and on its reference, and rows that agree, disagree,
    # are missing or absent at each
    parent = [-1, 0, 0, 1, 1]
    muts = [[(10, other(REF(10))), (-1, G, A), (14, REF(14)), (-1, C, C), (18, other(REF(18), 1)), (-1, T, A)],
            [(10, REF(10)), (22, other(REF(22)))], [(14, other(REF(14)))], [], [(18, REF(18))]]
    samples = [sample([]), sample([(10, other(REF(10)))]), sample([(10, REF(10)), (14, None), (18, other(REF(18), 2))]),
               sample([(10, other(REF(10)) | REF(10)), (14, REF(14)), (18, other(REF(18), 1)), (22, 15 ^ REF(22))]),
               sample([(9, other(REF(9))), (11, None), (30, other(REF(30), 2))])]
    return case("root", parent, muts, samples)


def _loop1():
    # every outcome of loop 1 on one node, as an internal node (1) and as a leaf (5): a bit match at 20, a missing row at 24, absent
    # with nuc == ref at 28 (its parent left the reference there), absent off the reference at 32, present with another allele at
    # 36, a masked entry, and an entry behind it; node 6 stores its entries in descending position, so the merge pointer passes rows
    parent = [-1, 0, 0, 1, 1, 2, 2]
    own = [(20, other(REF(20))), (24, other(REF(24))), (28, REF(28)), (32, other(REF(32))), (36, other(REF(36))), (-1, A, C), (40, other(REF(40)))]
    top = [(28, other(REF(28))), (44, other(REF(44)))]
    muts = [top, own, [], [(20, REF(20))], [], own, [(52, other(REF(52))), (48, REF(48)), (44, REF(44)), (40, other(REF(40), 1))]]
    muts[2] = [(48, other(REF(48)))]
    samples = [sample([(20, other(REF(20))), (24, None), (36, other(REF(36), 1)), (40, other(REF(40)))]),
               sample([(20, other(REF(20), 1)), (24, other(REF(24))), (28, REF(28)), (32, other(REF(32))), (36, other(REF(36)))]),
               sample([(40, other(REF(40), 1)), (44, REF(44)), (48, REF(48)), (52, other(REF(52)))]),
               sample([(44, other(REF(44))), (48, other(REF(48))), (52, None)]),
               sample([(20, None), (24, None), (28, None), (32, None), (36, None)]), sample([])]
    return case("loop1", parent, muts, samples)


def _eligible():
    # every clause of the eligibility on leaves and internal nodes: no entries, all common, some common, none common, masked first
    parent = [-1, 0, 0, 0, 1, 1, 2, 2, 3, 3]
    e = lambda p, k=0: (p, other(REF(p), k))
    muts = [[], [e(10), e(14)], [e(18)], [(-1, A, C), e(22)], [], [e(10, 1), e(26)], [e(30), e(34), e(38)], [(-1, G, A)], [e(22)], [e(42)]]
    samples = [sample([e(10), e(14), e(18), e(22), e(30)]), sample([e(10), e(26), e(34), e(42)]), sample([e(14, 1), e(18, 1), e(38)]), sample([])]
    return case("eligible", parent, muts, samples)


def _ambiguous():
    # rows of 2, 3 and 4 bits in each imputed branch (found; no ancestral entry and the reference bit; neither), with and without
    # the reference bit, on a path with entries at 50, 54, 58 and none at 62, 66
    parent = [-1, 0, 1, 1, 2]
    e = lambda p, k=0: (p, other(REF(p), k))
    muts = [[], [e(50), e(54)], [e(58), (50, REF(50))], [], [e(54, 1)]]
    masks = lambda p: [m for m in range(1, 16) if m & (m - 1)] + [REF(p), other(REF(p))]
    samples = [sample([(p, masks(p)[(i + 3 * k) % 13]) for k, p in enumerate((50, 54, 58, 62, 66))], "amb%d" % i) for i in range(13)]
    return case("ambiguous", parent, muts, samples)


def _rewrite():
    # one position rewritten at depths 1, 3 and 5, the last one back to the reference, with and without a row there; 74 ends off it
    parent = [-1, 0, 1, 2, 3, 4, 5, 5]
    p, q = 70, 74
    muts = [[], [(p, other(REF(p)))], [(q, other(REF(q)))], [(p, other(REF(p), 1))], [], [(p, REF(p)), (q, other(REF(q), 2))], [], [(q, REF(q))]]
    samples = [sample([]), sample([(p, REF(p))]), sample([(p, other(REF(p), 1))]), sample([(p, None), (q, other(REF(q), 2))]), sample([(q, 15)])]
    return case("rewrite", parent, muts, samples)


PATH_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)


def _caterpillar(flip):
    # a chain 1,026 deep, one entry a node below the root, a leaf hanging off every picked node: the picked nodes have 0 .. 1,025
    # entries on their root path.  flip: one position changes at every level; else every level has a position of its own.
    depth = 1025
    parent, muts = [-1], [[]]
    for d in range(1, depth + 1):
        parent.append(d - 1)
        muts.append([(100, (other(REF(100)), REF(100))[d % 2 == 0])] if flip else [(100 + 4 * d, other(REF(100 + 4 * d), d))])
    picked = list(PATH_COUNTS)
    for v in picked:   # the hanging leaves, behind the chain in breadth-first order: parent[] stays ascending
        parent.append(v)
        muts.append([])
    order = sorted(range(len(parent)), key=lambda j: (0, 0) if j == 0 else (_depth(parent, j), parent[j], j))
    renum = {j: i for i, j in enumerate(order)}
    parent2 = [-1 if parent[j] < 0 else renum[parent[j]] for j in order]
    muts2 = [muts[j] for j in order]
    nodes = [renum[v] for v in picked] + [renum[depth + 1 + i] for i in range(len(picked))]
    if flip:
        samples = [sample([]), sample([(100, REF(100))]), sample([(100, other(REF(100)))]), sample([(100, None)])]
    else:
        samples = [sample([]), sample([(100 + 4 * d, other(REF(100 + 4 * d), d)) for d in range(1, depth + 1, 3)]),
                   sample([(100 + 4 * d, REF(100 + 4 * d) if d % 5 else None) for d in range(2, depth + 1, 2)])]
    return case("caterpillar_flip" if flip else "caterpillar", parent2, muts2, samples, [(s, j) for s in range(len(samples)) for j in nodes])


def _depth(parent, j):
    d = 0
    while parent[j] >= 0:
        j, d = parent[j], d + 1
    return d


def _rows():
    # samples of 0, 1, 63, 64, 65 and 257 rows and one all-missing sample, on a small tree whose entries lie among the rows
    parent = [-1, 0, 0, 1, 1, 2]
    e = lambda p, k=0: (p, other(REF(p), k))
    muts = [[e(203)], [e(207), e(331)], [e(203, 1), e(459)], [e(207, 2)], [(331, REF(331))], [e(715), e(1227)]]
    rows = lambda n: [(201 + 2 * i, (other(REF(201 + 2 * i), i), None, 15 ^ REF(201 + 2 * i), REF(201 + 2 * i) | other(REF(201 + 2 * i)))[i % 4 if i % 7 else 0])
                      for i in range(n)]
    samples = [sample(rows(n), "rows%d" % n) for n in (0, 1, 63, 64, 65, 257)] + [sample([(201 + 2 * i, None) for i in range(70)], "allN")]
    return case("rows", parent, muts, samples)


def _polytomy():
    # 129 leaves under one node, entries on every third, and the same position on many of them
    parent = [-1, 0] + [1] * 129
    muts = [[], [(300, other(REF(300)))]] + [[(304 + 4 * (i % 5), other(REF(304 + 4 * (i % 5)), i))] if i % 3 == 0 else [] for i in range(129)]
    samples = [sample([(300, other(REF(300))), (304, other(REF(304))), (312, other(REF(312), 1))]), sample([(308, None), (316, 15)])]
    return case("polytomy", parent, muts, samples)


def _twice():
    # node 2 stores position 400 twice (refused); nodes 1 and 3 store it once each on one path (not refused); node 4 stores it twice
    # with a masked entry between; nodes 5 and 6 are NOT refused below node 2: their g(400) is node 2's first entry, and node 6
    # rewrites 404 below it
    parent = [-1, 0, 0, 1, 2, 2, 5]
    a, b = other(REF(400)), other(REF(400), 1)
    muts = [[], [(400, a)], [(400, a), (404, other(REF(404))), (400, b)], [(400, b)], [(400, REF(400)), (-1, A, C), (400, a)],
            [(408, other(REF(408)))], [(404, REF(404))]]
    samples = [sample([]), sample([(400, a)]), sample([(400, b), (404, None)]), sample([(400, a | b), (404, other(REF(404))), (408, REF(408))])]
    return case("twice", parent, muts, samples, refused=(2, 4))


# ---- generators with their sizes as parameters: the CPU module runs them all, the GPU module picks the edges -----------------------

WIDE_WIDTHS = (63, 64, 65, 128, 129, 200)
WIDE_ORDERS = ("asc", "desc", "shuffled")
WIDE_KINDS = 6    # a sample's row at W's i-th position: matching, another allele, missing, ambiguous with / without ref, absent


def wide(width, order="asc", mask_at=None, as_root=False):
    """A node W with `width` own entries, at positions 2000 + 3 i in `order` of storage, as an internal node (2) and as a leaf (3)
    below A (1), which owns every fourth of W's positions; W's child (4) rewrites every fifth and its child (5) puts one of those
    back on the reference.  mask_at: one masked entry is inserted at that stored index.  as_root: the same entries on the root
    instead (its child 1 rewrites, 2 is a leaf, 3 below 1 restores), with masked entries at 1, 62 .. 65, 127, 128 and the last
    index, on and off their reference."""
    assert order in WIDE_ORDERS and width >= 8
    pos = [2000 + 3 * i for i in range(width)]
    above = {i: other(REF(pos[i]), i // 4) for i in range(0, width, 4)}

    def w_nuc(i):
        if i % 8 == 0:
            return REF(pos[i])                       # back on the reference: kept by loop 1 when the sample has no row
        if i % 8 == 4:
            return other(REF(pos[i]), i // 4 + 1)    # another allele than A's
        return other(REF(pos[i]), i)
    idx = list(range(width))
    if order == "desc":
        idx.reverse()
    elif order == "shuffled":
        idx = [int(x) for x in np.random.default_rng(width).permutation(width)]
    own = [(pos[i], w_nuc(i)) for i in idx]
    masks = sorted({m for m in (1, 62, 63, 64, 65, 127, 128, width - 1) if m < width} | ({mask_at} if mask_at is not None else set())) \
        if as_root else ([] if mask_at is None else [mask_at])
    for k, m in enumerate(masks):
        assert 0 <= m <= len(own)
        own.insert(m, (-1, (G, A)[k % 3 == 2], A))   # every third one on its reference
    child = [(pos[i], other(w_nuc(i), i)) for i in range(0, width, 5)]
    back = next((p, REF(p)) for p, a in child[1:] if a != REF(p))
    if as_root:
        parent = [-1, 0, 0, 1]
        muts = [own, child, [(pos[2], REF(pos[2])), (pos[3], other(w_nuc(3)))], [back]]
    else:
        parent = [-1, 0, 1, 1, 2, 4]
        muts = [[(1990, other(REF(1990)))], [(pos[i], a) for i, a in above.items()] + [(1993, other(REF(1993)))], own, own, child, [back]]

    def row(i, kind):
        p, ref, a = pos[i], REF(pos[i]), w_nuc(i)
        return [(p, a)], [(p, other(a, i // WIDE_KINDS))], [(p, None)], [(p, ref | other(ref, i // WIDE_KINDS))], \
            [(p, other(ref, i // WIDE_KINDS) | other(ref, i // WIDE_KINDS + 1))], []
    samples = [sample([], "empty")]
    for k in range(3):
        rows = [r for i in range(width) for r in row(i, 0)[(i + 2 * k) % WIDE_KINDS]]
        rows += [(pos[i] + 1, other(REF(pos[i] + 1), i)) for i in range(3 + k, width, 7)]   # rows between W's positions
        samples.append(sample(rows, "cycle%d" % k))
    c = case("wide_%d_%s_%s%s" % (width, order, "none" if mask_at is None else mask_at, "_root" if as_root else ""), parent, muts, samples)
    c["W"] = (0,) if as_root else (2, 3)
    return c


RAGGED_COUNTS = (0, 1, 3, 0, 7, 2)
RAGGED_WIDE = 70
RAGGED_HANG = (1, 63, 64, 65, 127, 128, 129)


def ragged_path(depth, counts=RAGGED_COUNTS, pool=None):
    """A chain of `depth` nodes below the root whose entry counts cycle through `counts`, but RAGGED_WIDE at depths 20 and depth - 10.
    Positions 3000 + 3 k cycle through a pool (about 3/5 of all entries, so most positions are owned more than once on the chain),
    every allele differs from the state above and some return to the reference.  A leaf with a few entries of its own hangs off the
    chain nodes at depths RAGGED_HANG and `depth`, in front of the chain's next node in depth-first order: the last owner of a
    position in front of a deeper target is then often such a leaf, not a node of its path.  The pairs are those leaves and their
    parents, for every sample."""
    assert depth >= 130
    cnt = [0] + [counts[d % len(counts)] for d in range(1, depth + 1)]
    cnt[20] = cnt[depth - 10] = RAGGED_WIDE
    pool = pool or max(RAGGED_WIDE + 10, 3 * sum(cnt) // 5)
    hang = sorted(set(RAGGED_HANG) | {depth})
    parent, muts, chain, leaves = [-1], [[]], [0], []
    state, c = {}, 0
    for d in range(1, depth + 2):
        up = chain[d - 1]
        if d - 1 in hang:          # the leaf first: a lower breadth-first index than the chain's node, so in front of it depth-first
            i = len(leaves)
            ents = []
            for t in range((2, 0, 5, 1)[i % 4]):
                p = 3000 + 3 * ((17 * i + 11 * t) % pool)
                ents.append((p, other(state.get(p, REF(p)), i + t + 1)))
            leaves.append(len(parent))
            parent.append(up)
            muts.append(ents)
        if d <= depth:
            ents = []
            for _ in range(cnt[d]):
                p = 3000 + 3 * (c % pool)
                cur = state.get(p, REF(p))
                ents.append((p, REF(p) if c % 9 == 4 and cur != REF(p) else other(cur, c)))
                c += 1
            for p, a in ents:
                state[p] = a
            chain.append(len(parent))
            parent.append(up)
            muts.append(ents)
    P = lambda k: 3000 + 3 * k
    samples = [sample([], "empty"),
               sample([(P(k), (other(REF(P(k)), k), REF(P(k)), 15 ^ REF(P(k)), REF(P(k)) | other(REF(P(k)), k))[(k // 3) % 4]) for k in range(0, pool, 3)], "third"),
               sample([(P(k), None) for k in range(1, pool, 2)], "allN")]
    nodes = sorted(set(leaves) | {chain[h] for h in hang})
    c = case("ragged_%d_%s" % (depth, "-".join(map(str, counts))), parent, muts, samples, [(s, j) for s in range(len(samples)) for j in nodes])
    c["chain"], c["leaves"], c["hang"] = chain, leaves, hang
    return c


def random_case(seed, max_nodes=300, max_entries=4):
    """A random tree of up to max_nodes nodes in breadth-first order with up to max_entries entries a node: masked entries, no
    position twice on a node, and samples with missing rows and ambiguous alleles at and around the tree's positions."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, max_nodes + 1))
    parent = [-1] + sorted(int(rng.integers(0, max(1, j))) for j in range(1, n))
    parent = [-1] + [min(p, j - 1) for j, p in enumerate(parent[1:], 1)]
    npos = int(rng.integers(3, 40)) if max_entries < 40 else int(rng.integers(max_entries, 2 * max_entries))   # room for the widest node
    muts = []
    for j in range(n):
        ents = []
        for p in rng.permutation(npos)[:int(rng.integers(0, max_entries + 1))]:
            p = 10 + 3 * int(p)
            ents.append((p, ONEHOT[int(rng.integers(0, 4))]))
        if rng.random() < 0.15:
            ents.insert(int(rng.integers(0, len(ents) + 1)), (-1, ONEHOT[int(rng.integers(0, 4))], ONEHOT[int(rng.integers(0, 4))]))
        muts.append(ents)
    samples = []
    for _ in range(3):
        rows = []
        for p in range(9, 10 + 3 * npos):
            u = rng.random()
            if u < 0.25:
                rows.append((p, None if rng.random() < 0.2 else int(rng.integers(1, 16))))
        samples.append(sample(rows))
    name = "random%d" % seed if (max_nodes, max_entries) == (300, 4) else "random%d_%d_%d" % (seed, max_nodes, max_entries)
    return case(name, parent, muts, samples)


# what tests/test_vectors_gpu.py runs of them; tests/test_vectors_cpu.py proves that these picks have the edges
WIDE_PICKS = ((63, "asc", None, False), (64, "desc", 63, False), (65, "shuffled", 64, False), (128, "asc", 0, False), (129, "desc", None, False),
              (129, "shuffled", 65, False), (200, "shuffled", 1, False), (200, "asc", 200, False), (64, "asc", 1, False), (129, "asc", None, True), (200, "shuffled", 64, True))
RAGGED_PICKS = ((200, RAGGED_COUNTS),)
RANDOM_PICKS = tuple((seed, 150, 80) for seed in (0, 2, 3, 4, 7, 8, 10, 13, 15, 17, 18, 20))   # the trees of at least 100 nodes
SEAM_TILE = 2048                         # kBlock * kScanTile of k_vec_scan, guarded by tests/test_vectors_cpu.py
SEAM_COUNTS = (SEAM_TILE - 1, SEAM_TILE, SEAM_TILE + 1, 2 * SEAM_TILE, 2 * SEAM_TILE + 1)


# test_window_seams repeats the pairs of `rows` (the one hand case that has all three kinds): without any entry, with entries of part
# 3 only, with both lists (two entries each at least, for the caps that cut inside the pair)
SEAM_CASE, SEAM_EMPTY, SEAM_PART3, SEAM_BOTH = "rows", (6, 0), (0, 1), (2, 3)


def seam_pairs(n, both):
    """n pairs of SEAM_CASE, all its pairs over and over in a seeded order; at 2 047, 2 048 and 2 049 (where n reaches them) SEAM_BOTH
    three times, or SEAM_EMPTY twice and SEAM_PART3."""
    distinct = next(c for c in cases() if c["name"] == SEAM_CASE)["pairs"]
    rng = np.random.default_rng(n)
    pairs = [distinct[int(k)] for k in np.concatenate([rng.permutation(len(distinct)) for _ in range(n // len(distinct) + 1)])[:n]]
    for i, pr in zip(range(SEAM_TILE - 1, SEAM_TILE + 2), (SEAM_BOTH,) * 3 if both else (SEAM_EMPTY, SEAM_EMPTY, SEAM_PART3)):
        if i < n:
            pairs[i] = pr
    return pairs


_CASES = []


def cases():
    if not _CASES:
        _CASES.extend([_root(), _loop1(), _eligible(), _ambiguous(), _rewrite(), _caterpillar(False), _caterpillar(True), _rows(), _polytomy(),
                       _twice()])
    return _CASES
