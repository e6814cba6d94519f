"""Hand-shaped trees and samples for ugp_vectors (tests/test_vectors_cpu.py, tests/test_vectors_gpu.py): every edge of
usher_amd/csrc/ugp_vectors.hip by name.  A case is a dict: name, arrays (BFS flat arrays), samples (row dicts), pairs (a list of
(sample, node), every pair of the case unless it says otherwise) and refused (the nodes whose pairs are refused: only `twice`).

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


_CASES = []


def cases():
    if not _CASES:
        _CASES.extend([_root(), _loop1(), _eligible(), _ambiguous(), _rewrite(), _caterpillar(False), _caterpillar(True), _rows(), _polytomy(),
                       _twice()])
    return _CASES
