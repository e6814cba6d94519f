"""Hand-shaped trees for the mask calls (tests/mask_ref.py), at the smallest sizes where the kernels can go wrong.

The trees of tests/select_cases.py are reused; the ones added here aim at the restricted pass: stars at the edges of the bitmap's
64-bit words, entry counts around one block, a restricted root whose depth-first range straddles the first segment boundary of the
scans (kSeg = 16,384 positions), a caterpillar with every leaf named (the nodes of F nest as deep as the tree), a node with two
entries at one position, masked entries, and a tree of one node.  `leaf_sets` and `lines` make, for every case alike, the named
sets and the mask lines worth asking.
"""
import numpy as np

from tests import select_cases as SC
from tests import summary_cases as SMC

N, F = SC.N, SC.F
Case = SC.Case
KSEG = 16384


def _leaf(i):
    """Leaf i of a star: a private entry (its own position) on every third leaf, an entry shared in rotation on the others."""
    if i % 3 == 0:
        return N(["A%dC" % (100 + i)])
    if i % 11 == 10:
        return N()
    return N(["A%d%s" % (1 + i % 7, "CGT"[(i // 7) % 3])])


def star(k):
    return Case("mstar%d" % k, N(["A3G"], [N(["C20T"], [_leaf(i) for i in range(k)], tag="hub"), N(["A1C"]), N(["A100C"])]),
                "%d leaves under one inner node, two more leaves beside it: the named bits end at a word edge" % k)


def entries(m):
    """A tree with exactly m entries: a comb of pairs whose leaves share four keys."""
    kids = [N(["A%d%s" % (1 + i % 4, "CG"[i % 2])]) for i in range(m - 2)]
    c = Case("entries%d" % m, N(["T9A"], [F(2), N(["G8A"], kids, tag="hub")]), "%d entries: the last block of the entry passes" % m)
    assert len(c.arrays["mut_pos"]) == m
    return c


def straddle():
    """More than kSeg nodes; the inner node `big` sits before the segment boundary and its leaves run past it."""
    a = N(["A5C"], [N(["A%dG" % (1 + i % 50)]) for i in range(8200)], tag="front")
    b = N(["A6C"], [N(["A%d%s" % (1 + i % 60, "GT"[i % 2])]) for i in range(8200)], tag="big")
    c = Case("straddle", N((), [a, b, N(["A7T"])]), "a restricted root whose range crosses position %d: the scans' carry" % KSEG)
    return c


def caterpillar(depth=300):
    """Every inner node has one leaf child; shared and private entries alternate down the spine."""
    node = N(["G3T"])
    for i in range(depth, 0, -1):
        side = N(["A%dC" % (10 + i)]) if i % 2 else N(["A%dG" % (1 + i % 5)])
        node = N(["C%dT" % (1 + i % 5)] if i % 3 else [], [node, side], tag="v%d" % i)
    return Case("mcaterpillar", N((), [node, N(["A2G"])]), "a caterpillar of depth %d: every inner node can be a node of F" % depth)


def hand_cases():
    c = [Case("one_node", N(["A5C", "MASKED"]), "a tree of one node: the root is a leaf and its own restricted root")]
    c += [star(k) for k in (63, 64, 65, 128, 129)]
    c += [entries(m) for m in (255, 256, 257)]
    c.append(straddle())
    c.append(caterpillar())
    c.append(Case("two_at_one", N((), [N(["A7C", "A7G", "A7C"], [N(["A7C"]), N(["C7T", "T7C"], tag="y")], tag="x"), N(["A7G"], [F(2, ["A7C"])])]),
                  "two entries at one position on one node, and the same key twice", literal_ok=False))
    c.append(Case("masked_before", N(["MASKED"], [N(["MASKED", "A7C", "MASKED:-7"], [N(["MASKED", "A8G"]), N(["A7C"])], tag="x"),
                                                    N(["MASKED:-7"], [F(2, ["A7G"])])]),
                  "masked entries are there already: they have no key and are never masked again or matched"))
    c.append(Case("code_zero", N((), [N(["A7C"], [N(), N()]), F(2, ["A9G"])]), "an entry whose stored parent allele is 0 prints as N"))
    c[-1].arrays["mut_par"] = np.asarray(c[-1].arrays["mut_par"]).copy()
    c[-1].arrays["mut_par"][0] = 0
    c.append(Case("nested_full", N((), [N(["A4C"], [N(["A5C"], [F(3, ["A6C"], tag="deep"), N(["A6C"])], tag="mid"), N(["A5G"])], tag="top"), F(2, ["A4C"])]),
                  "full nodes without a leaf child above a node of F: the topmost node of F is not the topmost full node"))
    return c


def all_cases():
    return SC.all_cases() + hand_cases()


def by_name():
    return {c.name: c for c in all_cases()}


def tables(arrays):
    """(parent list, leaves, children lists) by BFS index."""
    par = [int(p) for p in arrays["parent"]]
    kids = [[] for _ in par]
    for j in range(1, len(par)):
        kids[par[j]].append(j)
    return par, [j for j in range(len(par)) if not kids[j]], kids


def below(kids, v):
    out, stack = [], [v]
    while stack:
        x = stack.pop()
        out.append(x)
        stack.extend(kids[x])
    return out


def leaf_sets(arrays):
    """Named leaves (BFS indices): one, all, all but one, every leaf of the first and last inner nodes alone, beside a stranger and
    short of one, halves, a name twice, and drawn sets.  The literal search for the roots is quadratic where no ancestor is full, so
    a tree of more than 300 leaves gets the sets with few such climbs only."""
    par, lv, kids = tables(arrays)
    big = len(lv) > 300
    sets = [[lv[0]], [lv[-1]], lv, [lv[0], lv[0], lv[-1]]]
    if not big:
        sets += [lv[:-1], lv[1:], lv[::2], lv[: len(lv) // 2]]
    inner = [j for j in range(1, len(par)) if kids[j]]
    for v in inner[:2] + inner[-2:]:
        under = [x for x in below(kids, v) if not kids[x]]
        sets += [under, under + [lv[0]]] + ([] if big else [under[:-1]])
    rng = np.random.default_rng(len(par))
    for frac in (0.1, 0.5, 0.9):
        k = min(20, len(lv)) if big else max(1, int(len(lv) * frac))
        sets.append(sorted(int(x) for x in rng.choice(lv, k, replace=False)))
    out = []
    for s in sets:
        if s and s not in out:
            out.append(s)
    return out


def lines(arrays, max_pos=None):
    """Mask lines (pos, par, nuc, node, excl): per position asked the exact key tree-wide, the three wildcard forms, an allele that
    is absent; the same below inner nodes with exclusions -- a child, a grandchild, the target itself, a node beside the target, an
    index that is no node, two nested -- then an absent position, a negative one and the first line again."""
    par, lv, kids = tables(arrays)
    n = len(par)
    pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
    mp, mn = np.asarray(arrays["mut_par"]).astype(np.int64) & 0xFF, np.asarray(arrays["mut_nuc"]).astype(np.int64) & 0xFF
    there = sorted(set(int(p) for p in pos if p >= 0))
    counts = {p: int((pos == p).sum()) for p in there}
    if max_pos is None:
        max_pos = 1 if n > 2000 else 5   # (the literal walk of a line visits every node below its target)
    ask = sorted(there, key=lambda p: -counts[p])[:max_pos] + there[-1:]
    inner = [j for j in range(1, n) if kids[j]]
    targets = inner[-1:] + inner[:1] + [0]
    out = []
    for p in ask:
        k = int(np.flatnonzero(pos == p)[0])
        a, b = int(mp[k]), int(mn[k])
        for t in targets:   # the lines with exclusions first: what they leave is there for the plain lines behind them
            sub = kids[t]
            if sub:
                grand = [g for s in sub for g in kids[s]]
                beside = (t + 1) % n if (t + 1) % n not in below(kids, t) else 0
                if grand:
                    out += [(p, a, 15, t, [grand[-1]]), (p, 15, 15, t, [grand[0], par[grand[0]]])]
                out += [(p, 15, b, t, [sub[0]]), (p, 15, 15, t, [t, n + 3]), (p, 15, 15, t, [sub[-1], beside])]
            out += [(p, a, b, t, []), (p, 15, b, t, []), (p, a, 15, t, [])]
        out += [(p, a ^ 3, b, 0, []), (p, 15, 15, 0, [])]
    tp = there[-1] + 1 if there else 0
    out += [(tp, 15, 15, 0, []), (tp + 5, 1, 2, 0, []), (-1, 15, 15, 0, []), (0, 15, 15, 0, [])]
    if there:
        out.append(out[0])
    return out


def line_arrays(ls):
    return ([l[0] for l in ls], [l[1] for l in ls], [l[2] for l in ls], [l[3] for l in ls], [l[4] for l in ls])
