"""Batches of selections for the batched induced subtree (ugp_subtree_batch.hip), built from the trees of tests/subtree_cases.py and
from a few more whose only point is how the selections' windows lie to one another.

The WINDOW of a selection is the depth-first range of its lowest common ancestor.  A Batch is a tree (arrays) and a list of
selections (BFS indices); `rule` says what the batch is for.  `windows(batch)` restates the window sizes from the arrays alone, so
that a test can say where the seams of the concatenation fall.
"""

from tests import subtree_cases as SC

N = SC.N
KBLOCK, KSEG = 256, 16384


class Batch:
    def __init__(self, name, arrays, sels, rule):
        self.name, self.arrays, self.rule = name, arrays, rule
        self.sels = [[int(v) for v in s] for s in sels]

    def __repr__(self):
        return self.name


def of_case(case, sels=None, name=None, rule=None):
    sels = case.sels if sels is None else [[case.tags[t] if isinstance(t, str) else int(t) for t in s] for s in sels]
    return Batch(name or case.name, case.arrays, sels, rule or case.rule)


def case_batches():
    """Every case of subtree_cases with all its selections as one batch."""
    return [of_case(c) for c in SC.all_cases()]


def _relations_tree():
    return SC.Case("relations",
                   N(["A3G"], [N(["A1C"], [N(["C2T"], [N(["G3A"], tag="l1"), N(["G4A"], tag="l2")], tag="y"), N(["T6C"], tag="l3")], tag="x"),
                               N(["A8G"], [N(["C9T"], tag="l4"), N((), tag="l5")], tag="z"),
                               N(["T2C"], tag="l6")], tag="root"),
                   "windows that repeat, share a top, nest and touch", [["l1"]])


def relation_batches():
    c = _relations_tree()
    b = [
        ("same_twice", [["l1", "l2"], ["l1", "l2"]], "the same selection twice: two windows over the same positions"),
        ("one_lca", [["l1", "l3"], ["l2", "l3"]], "two selections with one lowest common ancestor"),
        ("nested", [["l1", "l3"], ["l1", "l2"], ["l1", "l3"]], "a window inside another's, on either side of it"),
        ("adjacent", [["l1", "l2"], ["l3"], ["l4", "l5"], ["l6"]], "disjoint windows that touch in depth-first order"),
        ("one_leaf", [["l1"], ["l5"], ["l6"]], "one leaf each: a window of one position whose chain is the whole root path"),
        ("one_internal", [["y"], ["x"], ["z"], ["root"]], "one internal node each, the root among them"),
        ("root_lca", [["l1", "l6"], ["l2", "l4"]], "the lowest common ancestor is the tree's root: no root path"),
        ("duplicates", [["l1", "l1", "l2", "l1"], ["l3", "l3"]], "nodes named more than once in a selection"),
        ("with_descendant", [["x", "l1"], ["y", "l2", "x"], ["root", "l5"]], "an internal node together with its descendant"),
        ("mixed", [["l1"], ["l1", "l6"], ["y"], ["l4", "l5"], ["l1", "l2"], ["x", "l1"], ["l3", "l3"], ["root"]], "all of these in one batch"),
    ]
    return [of_case(c, sels, "rel_" + name, rule) for name, sels, rule in b]


def _straddle(name, above, at_lca, rule, leaf=()):
    """root - a(above) - b(at_lca) - {l(leaf), m}: with l and m selected, b is the first kept node and its chain is root, a, b."""
    c = SC.Case(name, N((), [N(above, [N(at_lca, [N(leaf, tag="l"), N(["G6T"], tag="m")], tag="b")], tag="a"), N(["T9C"], tag="out")], tag="root"), rule,
                [["l", "m"]])
    return of_case(c, [["l", "m"], ["l"], ["m", "out"], ["l", "m"]], "path_" + name, rule)


def root_path_batches():
    cat = SC.by_name()["scaterpillar"]
    return [
        of_case(cat, [["deepest", "side300"], ["deepest"], ["side299", "side300"], ["deepest", "out"]], "path_caterpillar",
                "a selection at the bottom of a caterpillar of depth 300: the root path is as long as the tree is deep"),
        _straddle("reverted", ["A5C"], ["C5A"], "an entry above the lowest common ancestor is reverted by one inside the window"),
        _straddle("changed", ["A5C"], ["C5G", "T7A"], "an entry above the lowest common ancestor is changed again inside the window"),
        _straddle("masked", ["MASKED", "A7C"], ["C7T"], "a masked entry on the root path", leaf=["MASKED"]),
        _straddle("disagree", ["A5C"], ["G5A"], "a disagreement whose two entries lie on either side of the lowest common ancestor", leaf=["G5A"]),
    ]


def _hubs(sizes):
    """A root over hubs: hub i has sizes[i] leaf children, every node one entry.  Returns a Case with tags h<i> and h<i>_<j>."""
    hubs = [N(["A%dC" % (10 + i)], [N(["C%d%s" % (20 + j % 50, "GT"[j % 2])], tag="h%d_%d" % (i, j)) for j in range(k)], tag="h%d" % i)
            for i, k in enumerate(sizes)]
    return SC.Case("hubs_" + "_".join(str(k) for k in sizes), N(["G5T"], hubs, tag="root"), "hubs of %s leaves under one root" % (sizes,), [["h0_0"]])


def whole(i, k):
    """Two leaves of hub i (k leaves): the window is the hub with all its leaves, k + 1 positions."""
    return ["h%d_0" % i, "h%d_%d" % (i, k - 1)]


def block_seam_batches():
    """Window seams one before, on and one after a multiple of kBlock, and star windows at the wave and block edges."""
    sizes = (62, 63, 64, 65, 254, 255, 256, 257)   # hubs of 63 .. 257 children beside windows of 63 .. 258 positions
    at = {k: i for i, k in enumerate(sizes)}
    c = _hubs(sizes)
    out = []
    for i, k in enumerate(sizes):
        nxt = sizes[(i + 1) % len(sizes)]
        out.append(of_case(c, [whole(i, k), ["h0_0"], whole(at[nxt], nxt)], "block_%d" % (k + 1),
                           "a window of %d positions in front of two more: a seam at %d" % (k + 1, k + 1)))
    out.append(of_case(c, [whole(at[254], 254), ["h0_1"], ["h0_2"], whole(at[255], 255), whole(at[256], 256), ["h1_0"], whole(at[254], 254)],
                       "block_255_256_257", "seams at 255, 256, 257, 513, 770, 771"))
    every = [["h%d_%d" % (i, j) for j in range(k)] for i, k in enumerate(sizes)]
    out.append(of_case(c, every, "block_every_leaf", "every leaf of every hub, hub by hub"))
    return out


def segment_seam_batch():
    """Window seams at kSeg - 1, kSeg and kSeg + 1 concatenated positions, of entries as of positions (every node has one entry)."""
    big = KSEG - 2
    c = _hubs((big, 200, 3))
    sels = [whole(0, big), ["h1_0"], ["h1_1"], whole(1, 200), whole(2, 3), ["h0_%d" % j for j in range(0, big, 97)], whole(1, 200)]
    return of_case(c, sels, "segment_seams", "windows of %d, 1, 1, 201, 4, %d, 201 positions: seams at kSeg - 1, kSeg, kSeg + 1" % (big + 1, big + 1))


def windows(batch):
    """Per selection (lca as BFS index, window positions): restated from the parent array."""
    par = [int(p) for p in batch.arrays["parent"]]
    n = len(par)
    size = [1] * n
    for j in range(n - 1, 0, -1):   # breadth-first: children after parents
        size[par[j]] += size[j]
    out = []
    for s in batch.sels:
        paths = []
        for v in s:
            p = [v]
            while p[-1]:
                p.append(par[p[-1]])
            paths.append(p[::-1])
        k = 0
        while all(len(p) > k for p in paths) and len({p[k] for p in paths}) == 1:
            k += 1
        out.append((paths[0][k - 1], size[paths[0][k - 1]]))
    return out


def all_batches():
    return case_batches() + relation_batches() + root_path_batches() + block_seam_batches()


def by_name():
    return {b.name: b for b in all_batches()}
