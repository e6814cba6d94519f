"""Hand-shaped trees for the select calls (tests/select_ref.py), at the smallest sizes where the kernels can go wrong.

Trees are written as the nested N(mutations, children, tag=) of tests/summary_cases.py.  Every Case carries the queries that aim at
its rule; `queries` adds, for every case alike, each position that occurs with every allele code worth asking (the four bases, an
ambiguous code, N and 0 -- so the reference base and absent alleles are always among them), a position without an owner, and the
positions at the edges of the position table: tp - 1, tp, -1 and INT32_MAX.
"""
import numpy as np

from tests import summary_cases as SC

N, F = SC.N, SC.F
INT32_MAX = 2 ** 31 - 1
ALLELES = (1, 2, 4, 8, 5, 15, 0)


class Case:
    def __init__(self, name, root, rule, literal_ok=True):
        self.name, self.rule, self.literal_ok = name, rule, literal_ok
        self.arrays, self.tags, _ = SC.build(root)

    def __repr__(self):
        return self.name

    @property
    def topology(self):
        return SC.topology(self.arrays)


def _leaf(i):
    """Leaf i of a star: an entry at one of seven positions, alleles in rotation; every 11th leaf has none."""
    if i % 11 == 10:
        return N()
    p = 1 + i % 7
    return N(["A%d%s" % (p, "CGT"[(i // 7) % 3])])


def star(k):
    return Case("star%d" % k, N(["A3G", "C20T"], [_leaf(i) for i in range(k)]),
                "%d leaves under one root that owns position 3 itself: the tail word and the wave edges" % k)


def caterpillar(depth=150):
    """v1 - v2 - ...: v_i flips position 1 between A and C and has a side leaf; every 13th side leaf flips it back itself."""
    node = N(["G3T"])
    for i in range(depth, 0, -1):
        flip = "%s1%s" % ("AC"[(i + 1) % 2], "AC"[i % 2])
        side = N(["%s1%s" % ("AC"[i % 2], "AC"[(i + 1) % 2])]) if i % 13 == 0 else N(["G%dA" % (2 + i % 3)])
        node = N([flip], [node, side], tag="v%d" % i)
    return Case("caterpillar", N((), [node, N(["T2C"])]), "a caterpillar of depth %d: the climb over the owners above is long" % depth)


def hand_cases():
    c = [Case("one_leaf", N(["A5C"], [N(["C5G"], tag="l")]), "a single leaf: one word with one bit")]
    c += [star(k) for k in (63, 64, 65, 129, 1000)]
    c.append(caterpillar())
    c.append(Case("owner_chain", N((), [N(["A10T"], [N(), N(["T10A"], [N(), N(["A10T"], [N(), N(["T10A"], [N(), N(["G11A"])], tag="d")], tag="c")],
                                                                tag="b")], tag="a"), N(["G11C"])]),
                  "owners A>T>A>T four deep at position 10 with a leaf hanging at every level: the nearest owner decides, not any owner"))
    c.append(Case("owner_on_leaf", N((), [N(["A10T"], [N(["T10G"], tag="l"), N()]), N()]), "the leaf itself owns the position"))
    c.append(Case("owner_on_root", N(["A10T", "C30G"], [F(3), N((), [F(2)])]), "only the root owns the positions: every leaf reads it"))
    c.append(Case("two_entries", N((), [N(["A7C", "A7G"], [N(), N(["C7T", "T7C"])], tag="x"), N(["A7G"])]),
                  "two entries at one position on one node: the first counts", literal_ok=False))
    c.append(Case("masked", N(["MASKED"], [N(["MASKED", "A7C", "MASKED:-7"], [N(["MASKED"]), N()]), N(["MASKED:-7"], [F(2, ["A7G"])])]),
                  "masked entries on the queried nodes own nothing"))
    c.append(Case("predecessor_not_ancestor", N((), [N(["A1C"], [F(2, ["C1G"]), N(["T2C"], tag="L")]), F(2, ["A1T"]), N()]),
                  "the owner in front of a leaf in depth-first order is not its ancestor: the one enclosing it further up, or none"))
    c.append(Case("polytomy", N((), [N(["A4C"], [F(9, ["C4A"], tag="poly"), F(2)]), F(3, ["A4G"])]),
                  "a set inside one polytomy has the polytomy's node as its ancestor"))
    c.append(Case("no_mutations", N((), [F(3), F(2)]), "no entry anywhere: the position table is empty"))
    return c


def all_cases():
    return hand_cases()


def by_name():
    return {c.name: c for c in all_cases()}


def queries(arrays):
    """(pos, nuc) int32 / uint8 arrays."""
    pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
    there = sorted(set(int(p) for p in pos if p >= 0))
    tp = there[-1] + 1 if there else 0
    gap = next((p for p in range(tp) if p not in there), None)
    ps = there + ([gap] if gap is not None else []) + [tp - 1, tp, tp + 1, -1, -7, INT32_MAX, -INT32_MAX - 1]
    out = [(p, a) for p in ps for a in ALLELES]
    return np.asarray([p for p, _ in out], np.int32), np.asarray([a for _, a in out], np.uint8)


def leaves_of(arrays):
    par = np.asarray(arrays["parent"])
    inner = set(int(p) for p in par if p >= 0)
    return [j for j in range(int(arrays["n"])) if j not in inner]


def node_sets(arrays):
    """Subtree queries: nested, equal and disjoint nodes, a leaf node, everything, nothing."""
    n, lv = int(arrays["n"]), leaves_of(arrays)
    par = [int(p) for p in arrays["parent"]]
    inner = [j for j in range(1, n) if j not in set(lv)]
    sets = [[], [0], [lv[0]], [lv[-1]], [lv[-1], lv[-1]], [lv[0], lv[-1]], list(range(n))[::-1]]
    if inner:
        v = inner[-1]
        kids = [j for j in range(n) if par[j] == v]
        sets += [[v], [v, kids[0]], [kids[0], v, par[v]], [inner[0], inner[-1]], [lv[0], v]]
    return [np.asarray(s, np.uint32) for s in sets]


def leaf_sets(arrays):
    """MRCA queries as lists of leaves (BFS indices): one leaf, two siblings, the first and last leaf, a few drawn."""
    lv = leaves_of(arrays)
    par = [int(p) for p in arrays["parent"]]
    sets = [[lv[0]], [lv[-1]], [lv[0], lv[-1]], lv if len(lv) <= 200 else lv[::7]]   # (the literal MRCA is quadratic in the set)
    sib = [(a, b) for a, b in zip(lv, lv[1:]) if par[a] == par[b]]
    if sib:
        sets += [list(sib[0]), list(sib[-1])]
    rng = np.random.default_rng(len(lv))
    if len(lv) > 3:
        sets += [sorted(int(v) for v in rng.choice(lv, 3, replace=False)), sorted(int(v) for v in rng.choice(lv, min(len(lv) // 2, 100), replace=False))]
    out = []
    for s in sets:
        s = sorted(set(s))
        if s not in out:
            out.append(s)
    return out
