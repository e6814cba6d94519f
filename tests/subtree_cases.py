"""Hand-shaped trees and selections for the induced subtree (tests/subtree_ref.py), at the smallest sizes where the kernels of
ugp_subtree.hip can go wrong.

Trees are the nested N(mutations, children, tag=) of tests/summary_cases.py.  A Case carries its selections (lists of tags; a tag
may name any node) and, for the first selection, what it is for as data: `kept` (the kept nodes' tags in depth-first order),
`merged` (tag -> the merged entries as the reference prints them) and `disagree`.  tests/test_subtree_cpu.py holds the literal
restatement to exactly that (test_cases_do_what_they_say), so the device tests compare against a yardstick known to hit the rule.
The stars and the caterpillar say what they are for in `rule` and are checked there by their counts.
"""
import numpy as np

from tests import select_cases as SC

N, F = SC.N, SC.F


class Case(SC.Case):
    def __init__(self, name, root, rule, sels, kept=None, merged=None, disagree=0):
        super().__init__(name, root, rule, literal_ok=False)
        self.sels = [[self.tags[t] if isinstance(t, str) else int(t) for t in s] for s in sels]
        self.kept, self.merged, self.disagree = kept, merged or {}, disagree


def star(k):
    leaves = [N(["A%d%s" % (1 + i % 7, "CGT"[(i // 7) % 3])] if i % 11 != 10 else [], tag="s%d" % i) for i in range(k)]
    every = ["s%d" % i for i in range(k)]
    return Case("sstar%d" % k, N(["A3G", "C20T"], leaves, tag="root"),
                "%d leaves under a root with entries, the first and the last selected, then all: the flags' wave and block edges" % k,
                [[every[0], every[-1]], every, [every[0]], [every[-1]]])


def caterpillar(depth=300):
    """v1 - v2 - ... with a side leaf each; position 1 flips at every level, position 2 is set once near the top."""
    node = N(["G3T"], tag="deepest")
    for i in range(depth, 0, -1):
        flip = "%s1%s" % ("AC"[(i + 1) % 2], "AC"[i % 2])
        node = N([flip] + (["G2A"] if i == 2 else []), [node, N(["G%dA" % (4 + i % 3)], tag="side%d" % i)], tag="v%d" % i)
    return Case("scaterpillar", N((), [node, N(["T9C"], tag="out")], tag="root"),
                "a caterpillar of depth %d with its deepest leaf and one shallow leaf selected: one chain as long as the tree is deep" % depth,
                [["deepest", "side1"], ["deepest"], ["deepest", "out"], ["side%d" % depth, "deepest", "side7"]])


def hand_cases():
    c = [
        Case("one_leaf", N(["A5C"], [N(["C5A", "G7T"], [N(["T9G"], tag="l"), N(["A1C"])]), N(["A2C"])]),
             "one selected leaf: its chain is its whole root path, and the reversal on the path cancels",
             [["l"]], kept=["l"], merged={"l": ["G7T", "T9G"]}),
        Case("siblings", N(["A3G"], [N(["C4T"], tag="a"), N(["G5A"], tag="b")], tag="root"),
             "two sibling leaves under a root that carries entries: the root is kept with its own entries",
             [["a", "b"], ["b", "a"]], kept=["root", "a", "b"], merged={"root": ["A3G"], "a": ["C4T"], "b": ["G5A"]}),
        Case("inner_selected", N((), [N(["A1C"], [N(["C2T"], [N(["G3A"], tag="l1"), N(["G4A"], tag="l2")], tag="y"), N(["T6C"], tag="l3")], tag="x"), N(["A8G"])]),
             "a selected inner node with a selected descendant: it is kept with one child with members, and the node between collapses",
             [["x", "l1"], ["l1", "x", "y"], ["x"]], kept=["x", "l1"], merged={"x": ["A1C"], "l1": ["C2T", "G3A"]}),
        Case("named_twice", N((), [N(["A1C"], tag="l"), N(["A2C"], tag="m"), N(["A3C"])], tag="root"),
             "a node named twice counts once", [["l", "l", "m", "l"]], kept=["root", "l", "m"], merged={"l": ["A1C"], "m": ["A2C"]}),
        Case("all_leaves", N((), [N(["A1C"], [N(["C2T"], [N(["G3A"], tag="l1"), N((), tag="l2")], tag="b")], tag="a"), N(["T4C"], [N(["G5T"], tag="l3")], tag="c")],
                              tag="root"),
             "every leaf selected: the single-child inner nodes a and c collapse into the chains below them",
             [["l1", "l2", "l3"]], kept=["root", "b", "l1", "l2", "l3"], merged={"b": ["A1C", "C2T"], "l1": ["G3A"], "l2": [], "l3": ["T4C", "G5T"]}),
        Case("deep_lca", N(["A1C"], [N(["C2T"], [N(["G3A"], [N(["T4G"], tag="l1"), N((), tag="l2")], tag="b")]), N(["A9C"])]),
             "the selection's common ancestor is deep: the subtree's root takes the chain from the tree's root",
             [["l1", "l2"]], kept=["b", "l1", "l2"], merged={"b": ["A1C", "C2T", "G3A"], "l1": ["T4G"], "l2": []}),
        Case("changed_twice", N((), [N(["A5C"], [N(["C5G"], [N((), tag="l")])]), N()]),
             "one position changed twice on a chain: A>C, C>G gives A>G", [["l"]], kept=["l"], merged={"l": ["A5G"]}),
        Case("reverted", N((), [N(["A5C"], [N(["C5A"], [N(["G6T"], tag="l")])]), N()]),
             "one position changed and reverted: A>C, C>A gives nothing", [["l"]], kept=["l"], merged={"l": ["G6T"]}),
        Case("reverted_and_changed", N((), [N(["A5C"], [N(["C5A"], [N(["G5T"], tag="l")])]), N()]),
             "reverted and changed again: A>C, C>A, then G>T opens a new state with the third entry's own parent allele",
             [["l"]], kept=["l"], merged={"l": ["G5T"]}),
        Case("twice_on_one_node", N((), [N(["A7C", "C7G", "T8A"], [N((), tag="l")]), N()]),
             "one node with the same position twice: its entries merge in stored order", [["l"]], kept=["l"], merged={"l": ["A7G", "T8A"]}),
        Case("one_masked", N((), [N(["MASKED", "A7C"], [N(["C7T"], tag="l")]), N()]),
             "one masked entry on a chain stays, in front of the positions", [["l"]], kept=["l"], merged={"l": ["MASKED", "A7T"]}),
        Case("two_masked", N(["MASKED"], [N(["A7C"], [N(["MASKED", "C8T"], tag="l")]), N()]),
             "two masked entries on a chain cancel, as two entries A>A at position -1 do", [["l"]], kept=["l"], merged={"l": ["A7C", "C8T"]}),
        Case("parent_differs", N((), [N(["A5C"], [N(["G5T"], tag="l")]), N()]),
             "a stored parent allele that differs from the state above without a disagreement: A>C then G>T gives A>T",
             [["l"]], kept=["l"], merged={"l": ["A5T"]}),
        Case("disagreement", N((), [N(["A5C"], [N(["G5A", "T6C"], tag="l")]), N(["A5C"], [N((), tag="m")])], tag="root"),
             "a stored parent allele that makes a disagreement: A>C then G>A is skipped and counted",
             [["l"], ["l", "m"], ["m"]], kept=["l"], merged={"l": ["A5C", "T6C"]}, disagree=1),
        Case("opens_with_par_eq_nuc", N((), [N(["A5A"], [N(["G6T"], tag="l")]), N()]),
             "an entry with par == nuc opens a state: nothing is checked", [["l"]], kept=["l"], merged={"l": ["A5A", "G6T"]}),
    ]
    c += [star(k) for k in (63, 64, 65, 255, 256, 257)]
    c.append(caterpillar())
    return c


def all_cases():
    return hand_cases()


def by_name():
    return {c.name: c for c in all_cases()}


def selections(arrays, rng):
    """Selections worth asking of any tree (BFS indices): one leaf, two, a drawn third of the leaves, every leaf, and leaves with some
    inner nodes; capped so that the literal walk, which is quadratic, stays quick."""
    n = int(arrays["n"])
    lv = SC.leaves_of(arrays)
    inner = [j for j in range(n) if j not in set(lv)]
    third = sorted(int(v) for v in rng.choice(lv, max(1, min(len(lv) // 3, 60)), replace=False))
    sets = [[lv[0]], [lv[0], lv[-1]], third, lv if len(lv) <= 120 else lv[::len(lv) // 100]]
    if inner:
        some = [int(v) for v in rng.choice(inner, min(3, len(inner)), replace=False)]
        sets += [third[:10] + some, some, [0]]
    return sets


# ---- trees that put the three flag scans of a call on their seams ------------------------------------------------------------------
# (the selected positions over N nodes, the entries of nodes with members over M entries, the survivors over G sorted entries)

VARIANTS = ("11", "00")    # the flags of the items seam - 1 | seam


def seam_selection(N, variant, seam, extra=300):
    """(arrays, selection as BFS indices) on scan_edge_cases.leaf_prefix_tree(N): exactly N nodes, hubs and a chain, with the nodes at
    depth-first positions seam - 1 and seam (leaves) selected ('11') or not ('00') beside drawn ones, inner nodes among them."""
    from tests import scan_edge_cases as E
    arrays = E.leaf_prefix_tree(N, True, seam=seam)
    want = set(E.node_selection(N, seam, extra).tolist()) - {seam - 1, seam}
    if variant == "11":
        want |= {d for d in (seam - 1, seam) if d < N}
    return arrays, E.dfs_to_bfs(arrays)[np.asarray(sorted(want), np.int64)]


def entry_star(K, variant, seam):
    """(arrays, selection): a root with one entry over K - 1 leaves with one entry each: K nodes and K entries, entry i on the node at
    depth-first position i.  '11': every leaf is selected -- K kept nodes, K gathered entries, K survivors; '00': all but the leaves
    at positions seam - 1 and seam, whose entries are not gathered."""
    from tests import scan_edge_cases as E
    arrays = E._arrays(E._node([(5, E.A, E.A, E.C)], [E._node([(10 + i % 90, E.A, E.A, E.G)]) for i in range(K - 1)]))
    skip = {seam - 1, seam} if variant == "00" else set()
    return arrays, np.asarray([j for j in range(1, K) if j not in skip], np.uint32)   # a star's breadth-first order is its depth-first order


def cancel_star(G, variant, seam):
    """(arrays, selection): every leaf selected and exactly G gathered entries -- the root's one, then one per leaf, in sorted order
    as in depth-first order.  '00': the leaf whose entry would be item seam - 1 carries a cancelling pair instead (items seam - 1 and
    seam: a run head that does not survive, and its tail); '11': both items are surviving heads."""
    from tests import scan_edge_cases as E
    leaves = [E._node([(10 + i % 90, E.A, E.A, E.G)]) for i in range(G - 1 - (1 if variant == "00" and G > seam else 0))]
    if variant == "00" and G > seam:
        leaves[seam - 2] = E._node([(10, E.A, E.A, E.C), (10, E.A, E.C, E.A)])
    arrays = E._arrays(E._node([(5, E.A, E.A, E.C)], leaves))
    assert len(arrays["mut_pos"]) == G
    return arrays, np.arange(1, arrays["n"], dtype=np.uint32)


def deep_caterpillar(depth):
    """(arrays, selection): a spine of `depth` nodes with a side leaf each (position 1 flips down the spine, the side leaves carry
    position 2), its deepest leaf and the side leaf of the second spine node selected: the deepest leaf's chain is depth - 2 long."""
    from tests import scan_edge_cases as E
    node = E._node([(3, E.G, E.G, E.T)])
    for i in range(depth, 0, -1):
        flip = (1, E.A, E.A, E.C) if i % 2 else (1, E.A, E.C, E.A)
        node = E._node([flip], [node, E._node([(2, E.G, E.G, E.A)])])
    arrays = E._arrays(E._node((), [node, E._node([(9, E.T, E.T, E.C)])]))
    # breadth-first: root 0, v1 1, out 2, then per level (spine node, side leaf); the deepest leaf is the last level's first node
    n = arrays["n"]
    return arrays, np.asarray([n - 2, 6], np.uint32)


def half_star(k):
    """(arrays, selection): a star of k leaves with every second leaf selected."""
    arrays, _ = entry_star(k + 1, "11", 0)
    return arrays, np.arange(1, k + 1, 2, dtype=np.uint32)
