"""Hand-shaped trees for matUtils summary (tests/summary_ref.py), as the breadth-first arrays of tests/synth.py.

A tree is written as nested N(mutations, children, tag=, ann=) and flattened breadth-first; a mutation is the reference's string
("A100C": stored parent allele, position, allele; "MASKED" or "MASKED:-7" for a masked entry at that negative position).  F(k, ..)
is a non-leaf node with k leaf children.  Every Case says which rule it pins and names the rows that exist (or are missing) BECAUSE
of the rule: `present` rows (parent tag, mutation, child tag, child_count, offspring_with, median_without) must be among the literal
restatement's records, `absent` (parent tag, mutation) must not, `total` is the number of records.  tests/test_summary_cpu.py checks
those against the literal restatement, so the device tests compare against a yardstick that is known to exercise the rule.
"""
import collections

import numpy as np

from tests import summary_ref as R


class N:
    def __init__(self, muts=(), kids=(), tag=None, ann=None):
        self.muts, self.kids, self.tag, self.ann = list(muts), list(kids), tag, ann


def F(k, muts=(), tag=None, ann=None, leaf_muts=None):
    """A non-leaf node with k leaf children; leaf_muts = {i: [mutations of the i-th leaf]}."""
    leaf_muts = leaf_muts or {}
    return N(muts, [N(leaf_muts.get(i, ())) for i in range(k)], tag, ann)


def parse(m):
    if m.startswith("MASKED"):
        return (int(m.split(":")[1]) if ":" in m else -1, 1, 1)
    return (int(m[1:-1]), R.NUC.index(m[0], 1), R.NUC.index(m[-1], 1))


def build(root, n_ann=None):
    """(arrays, tags, ann): breadth-first arrays with names n<j>, tag -> index, per node its annotation list ([""] * n_ann when the
    node gives none; n_ann None: no annotations anywhere)."""
    order, parent, q = [], [], collections.deque([(root, -1)])
    while q:   # Tree::breadth_first_expansion
        nd, p = q.popleft()
        j = len(order)
        order.append(nd)
        parent.append(p)
        q.extend((k, j) for k in nd.kids)
    n = len(order)
    off, rows, tags, ann = [0], [], {}, []
    for j, nd in enumerate(order):
        rows += [parse(m) for m in nd.muts]
        off.append(len(rows))
        if nd.tag is not None:
            assert nd.tag not in tags
            tags[nd.tag] = j
        ann.append(list(nd.ann) if nd.ann is not None else [""] * (n_ann or 0))
    r = np.asarray(rows, np.int64).reshape(len(rows), 3)
    arrays = {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": np.asarray(off, np.int64), "mut_pos": r[:, 0].astype(np.int32),
              "mut_ref": r[:, 1].astype(np.int8), "mut_par": r[:, 1].astype(np.int8), "mut_nuc": r[:, 2].astype(np.int8),
              "names": ["n%d" % j for j in range(n)]}
    return arrays, tags, ann


class Case:
    def __init__(self, name, root, rule, present=(), absent=(), total=None, n_ann=None):
        self.name, self.rule = name, rule
        self.arrays, self.tags, self.ann = build(root, n_ann)
        self.present, self.absent, self.total = list(present), list(absent), total

    def __repr__(self):
        return self.name


M, M2, M3 = "A100C", "G200T", "C300A"


def _pair(owner, *others, extra=()):
    """root P with the non-leaf children `owner`, `others` and whatever else."""
    return N((), [owner] + list(others) + list(extra), tag="P")


def roho_cases():
    c = []
    # ---- candidates
    c.append(Case("plain", _pair(F(7, [M], "X"), F(6, tag="Z")),
                  "a key on a non-leaf child with > 5 leaves and one other such child is reported", [("P", M, "X", 2, 7, 6)], total=1))
    c.append(Case("later_child_owns", _pair(F(7, [M, M2], "X"), F(8, [M], "Y"), F(6, tag="Z")),
                  "two non-leaf children carry M: the later one (Y) owns it, X is not reported for M but is for M2; all_non of Y is "
                  "[6, 7]: even size, odd sum, (6 + 7) / 2 = 6", [("P", M, "Y", 3, 8, 6), ("P", M2, "X", 3, 7, 7)], total=2))
    c.append(Case("later_child_owns_with_small_owner", _pair(F(7, [M], "X"), F(3, [M], "Y"), F(6, tag="Z")),
                  "the later child owns M even when its own count (3) then drops the candidate: X does not get it back", absent=[("P", M)], total=0))
    c.append(Case("leaf_sibling_owns_nothing", _pair(F(7, [M], "X"), F(6, tag="Z"), extra=[N([M])]),
                  "a LEAF child of P after X carries M: leaves own nothing and erase nothing", [("P", M, "X", 2, 7, 6)], total=1))
    c.append(Case("twice_on_one_child", _pair(F(7, [M, M2, M], "X"), F(6, tag="Z")),
                  "M stored twice on X is one candidate", [("P", M, "X", 2, 7, 6), ("P", M2, "X", 2, 7, 6)], total=2))
    c.append(Case("root_entries", N([M3], [F(7, [M], "X"), F(6, tag="Z")], tag="P"),
                  "the root's own entry M3 is no candidate of anything; the root as a parent reports its children's", [("P", M, "X", 2, 7, 6)],
                  absent=[("P", M3)], total=1))
    # ---- erasure
    c.append(Case("leaf_grandchild_erases", _pair(F(7, [M, M2], "X", leaf_muts={3: [M]}), F(6, tag="Z")),
                  "a leaf GRANDchild of P (under the owner) carries M: erased; M2 stays", [("P", M2, "X", 2, 7, 6)], absent=[("P", M)], total=1))
    c.append(Case("leaf_child_does_not_erase", _pair(F(7, [M, M2], "X"), F(6, tag="Z"), extra=[N([M]), N([M2])]),
                  "leaf CHILDREN of P carry M and M2: nothing is erased", [("P", M, "X", 2, 7, 6), ("P", M2, "X", 2, 7, 6)], total=2))
    c.append(Case("erased_under_sibling", _pair(F(7, [M, M2], "X"), F(6, tag="Z", leaf_muts={0: [M]})),
                  "M recurs under the sibling Z: erased", [("P", M2, "X", 2, 7, 6)], absent=[("P", M)], total=1))
    c.append(Case("erased_at_last_node_inside", _pair(F(7, [M, M2], "X"), F(6, tag="Z", leaf_muts={5: [M]})),
                  "M recurs on the LAST node of P's depth-first range: erased", [("P", M2, "X", 2, 7, 6)], absent=[("P", M)], total=1))
    c.append(Case("first_node_outside", N((), [F(2, [], "before", leaf_muts={1: [M]}), N((), [F(7, [M, M2], "X"), F(6, tag="Z")], tag="P"),
                                                F(2, [M], "after", leaf_muts={0: [M]})]),
                  "M occurs right before P's range, on the first node after it and below that: outside (dfs(P), dend(P)), not erased",
                  [("P", M, "X", 2, 7, 6), ("P", M2, "X", 2, 7, 6)], total=2))
    c.append(Case("other_parent_allele_or_allele", _pair(F(7, [M], "X", leaf_muts={0: ["G100C"], 1: ["A100T"], 2: ["A101C"]}), F(6, tag="Z")),
                  "position 100 recurs below X with another stored parent allele, another allele, and 101: other keys", [("P", M, "X", 2, 7, 6)], total=1))
    c.append(Case("deep_recurrence", _pair(N([M], [F(6), N((), [N((), [F(2, leaf_muts={1: [M]})])])], tag="X"), F(6, tag="Z")),
                  "M recurs five levels below P on a leaf: erased", absent=[("P", M)], total=0))
    c.append(Case("recurrence_on_inner_grandchild", _pair(N([M, M2], [F(7, [M], "G")], tag="X"), F(6, tag="Z")),
                  "M recurs on a non-leaf grandchild: erased at P; X has one non-leaf child only and reports nothing itself",
                  [("P", M2, "X", 2, 7, 6)], absent=[("P", M), ("X", M)], total=1))
    # ---- masked
    c.append(Case("masked_candidate", _pair(F(7, ["MASKED"], "X"), F(6, tag="Z")), "the masked key is a candidate like any other",
                  [("P", "MASKED", "X", 2, 7, 6)], total=1))
    c.append(Case("masked_eraser", _pair(F(7, ["MASKED", M], "X"), F(6, tag="Z", leaf_muts={2: ["MASKED:-7"]})),
                  "every masked entry has the one key MASKED: position -7 under Z erases position -1 on X", [("P", M, "X", 2, 7, 6)],
                  absent=[("P", "MASKED")], total=1))
    # ---- leaf counts
    c.append(Case("counts_1_and_2", _pair(F(7, [M], "X"), F(1, [M2], "Y1"), F(2, [M3], "Y2")),
                  "the other children hold 1 and 2 leaves: child_increment has X and Y2, all_non is empty", total=0))
    c.append(Case("counts_1_and_2_beside_a_6", _pair(F(7, [M], "X"), F(1, [M2], "Y1"), F(2, [M3], "Y2"), F(6, tag="Z")),
                  "children with 1 and 2 leaves count in child_count (4) and nowhere else", [("P", M, "X", 4, 7, 6)], absent=[("P", M2), ("P", M3)], total=1))
    c.append(Case("owner_5", _pair(F(5, [M], "X"), F(6, tag="Z")), "the owner has exactly 5 leaves: dropped", absent=[("P", M)], total=0))
    c.append(Case("owner_6", _pair(F(6, [M], "X"), F(6, tag="Z")), "the owner has exactly 6 leaves: reported", [("P", M, "X", 2, 6, 6)], total=1))
    c.append(Case("other_5", _pair(F(7, [M], "X"), F(5, tag="Z")), "the only other child has exactly 5: exactly ONE qualifying child, all_non empty", total=0))
    c.append(Case("other_5_and_6", _pair(F(7, [M], "X"), F(5, tag="Z"), F(6, tag="Z2")),
                  "others with 5 and 6: exactly TWO qualifying children, all_non = [6]", [("P", M, "X", 3, 7, 6)], total=1))
    c.append(Case("counts_are_leaves_not_nodes", _pair(N([M], [F(3), F(3)], tag="X"), F(6, tag="Z")),
                  "X has 8 nodes below it but 6 leaves", [("P", M, "X", 2, 6, 6)], total=1))
    # ---- medians
    c.append(Case("all_non_2", _pair(F(7, [M], "X"), F(6), F(9)), "all_non = [6, 9]: (6 + 9) / 2 = 7 in integers", [("P", M, "X", 3, 7, 7)], total=1))
    c.append(Case("all_non_3", _pair(F(7, [M], "X"), F(20), F(6), F(9)), "all_non = [6, 9, 20]: 9", [("P", M, "X", 4, 7, 9)], total=1))
    c.append(Case("owner_below_median", _pair(F(6, [M], "X"), F(12), F(8), F(10)), "owner 6 < [8, 10, 12]", [("P", M, "X", 4, 6, 10)], total=1))
    c.append(Case("owner_at_median", N((), [F(12), F(10, [M], "X"), F(8), F(10)], tag="P"), "owner 10 among [8, 10, 12]", [("P", M, "X", 4, 10, 10)], total=1))
    c.append(Case("owner_above_median", N((), [F(12), F(8), F(10), F(20, [M], "X")], tag="P"), "owner 20 > [8, 10, 12]", [("P", M, "X", 4, 20, 10)], total=1))
    c.append(Case("owner_between_even", N((), [F(8), F(9, [M], "X"), F(12), F(13, [M2], "Y"), F(6)], tag="P"),
                  "owner inside an even all_non: X -> [6, 8, 12, 13] = 10, Y -> [6, 8, 9, 12] = 8", [("P", M, "X", 5, 9, 10), ("P", M2, "Y", 5, 13, 8)], total=2))
    c.append(Case("equal_counts", N((), [F(7, [M2], "Y"), F(7, [M], "X"), F(7)], tag="P"), "all counts equal", [("P", M, "X", 3, 7, 7), ("P", M2, "Y", 3, 7, 7)],
                  total=2))
    c.append(Case("no_record", N((), [F(3, [M]), N([M2]), N([M3])]), "one non-leaf child only: no record at all", total=0))
    c.append(Case("no_mutations", N((), [F(7), F(6)]), "a tree without a single mutation entry", total=0))
    return c


def wide_case(k):
    """P with k non-leaf children, child i with 6 + i % 5 leaves and its own mutation; every third one's mutation recurs under the next."""
    kids = []
    for i in range(k):
        lm = {0: ["A%dC" % (1000 + i - 1)]} if i % 3 == 1 else {}
        kids.append(F(6 + i % 5, ["A%dC" % (1000 + i)], "c%d" % i, leaf_muts=lm))
    counts = [6 + i % 5 for i in range(k)]
    present = []
    for i in range(k):
        if i % 3 == 0 and i + 1 < k:
            continue   # erased by the leaf under child i + 1
        rest = sorted(counts[:i] + counts[i + 1:])
        h = len(rest) // 2
        med = (rest[h - 1] + rest[h]) // 2 if len(rest) % 2 == 0 else rest[h]
        present.append(("P", "A%dC" % (1000 + i), "c%d" % i, k, counts[i], med))
    return Case("wide%d" % k, N((), kids, tag="P"), "%d non-leaf children of one parent: the per-parent work crosses a wave / block edge" % k, present,
                total=len(present))


def caterpillar(depth=42, annotate=False):
    """v0 - v1 - ... : every v_i has the next one and a fan of 6 as non-leaf children; v_i's mutation recurs under v_(i+3)'s fan
    when i % 4 == 0 (erased at v_(i-1)).  annotate: every v_i carries an annotation."""
    def mk(i):
        lm = {2: ["C%dT" % (500 + i - 3)]} if i >= 3 and (i - 3) % 4 == 0 else {}
        side = F(6, ["G%dA" % (9000 + i)], "s%d" % i, leaf_muts=lm)
        ann = ["L%d" % i, "even" if i % 2 == 0 else ""] if annotate else None
        if i == depth:
            return N(["C%dT" % (500 + i)], [side, F(7)], "v%d" % i, ann)
        return N(["C%dT" % (500 + i)], [mk(i + 1), side], "v%d" % i, ann)
    return mk(0)


def caterpillar_case():
    depth = 42
    present, absent = [], []
    for i in range(1, depth + 1):
        if (i % 4 == 0) and i + 3 <= depth:
            absent.append(("v%d" % (i - 1), "C%dT" % (500 + i)))
        else:
            w = 6 * (depth - i + 1) + 7
            present.append(("v%d" % (i - 1), "C%dT" % (500 + i), "v%d" % i, 2, w, 6))
    return Case("caterpillar", caterpillar(depth), "a caterpillar of depth 42: deep ranges nested in each other", present, absent)


def mutation_cases():
    c = []
    c.append(Case("star600", N([M], [N([M]) for _ in range(600)]), "one key with more occurrences (601) than two blocks cover"))
    c.append(Case("par_or_nuc", N((), [N(["A100C", "G100C"]), N(["A100T", "A100C"]), N(["A100C"])]), "keys that differ only in par or only in nuc"))
    c.append(Case("all_masked", N(["MASKED"], [N(["MASKED", "MASKED:-5"]), N(["MASKED"])]), "every entry is masked: an empty table"))
    c.append(Case("big_position", N(["A16777216C"], [N(["A16777217C", "T20000000G"]), N(["A3C", "A16777216C"])]), "positions >= 2^24"))
    c.append(Case("name_order", N((), [N(["A100G", "A23G"]), N(["A23G", "C9T", "T1000A"])]), "A100G sorts before A23G in the table the CLI writes"))
    return c


def clade_cases():
    c = []
    c.append(Case("same_name_twice", N((), [N((), [N((), [N(), N()], ann=["B"]), N()], ann=["B"]), N()], ann=[""]), "the same name twice on one root path",
                  n_ann=1))
    c.append(Case("annotated_leaf", N((), [N(ann=["leafclade"]), F(2, ann=["A"])], ann=[""]), "an annotated leaf: it counts nothing and the name "
                  "never appears in -c", n_ann=1))
    c.append(Case("annotated_root", N((), [F(2), N()], ann=["rootclade"]), "an annotated root", n_ann=1))
    c.append(Case("three_columns", N((), [F(2, ann=["a1", "", "c1"]), N((), [F(2, ann=["", "b2", "c2"]), N()], ann=["a2", "b1", ""])], ann=["", "", "c0"]),
                  "three columns: -c reads two, -C all", n_ann=3))
    c.append(Case("no_annotated_ancestor", N((), [F(2, ann=["A"]), N(), F(2)], ann=[""]), "leaves with no annotated ancestor: None", n_ann=1))
    c.append(Case("predecessor_not_ancestor_enclosed", N((), [N((), [F(2, ann=["inner"]), N(tag="L")], ann=["outer"]), N()], ann=[""]),
                  "the annotated node in front of leaf L is not its ancestor; the enclosing `outer` further up is", n_ann=1))
    c.append(Case("predecessor_not_ancestor_none", N((), [F(2, ann=["inner"]), N(tag="L"), F(1)], ann=[""]),
                  "the annotated node in front of leaf L is not its ancestor and nothing encloses it: None", n_ann=1))
    c.append(Case("fewer_annotations", N((), [F(2, ann=["a"]), N((), [N(), N(ann=[])], ann=["x", "y", "z"]), F(2, ann=["", "b"])], ann=["", ""]),
                  "nodes with fewer (and more) annotations than the root", n_ann=2))
    c.append(Case("none_as_a_name", N((), [N((), [F(2, ann=["None"]), N()], ann=["real"])], ann=[""]), "a clade literally named None", n_ann=1))
    c.append(Case("caterpillar_annotated", caterpillar(40, annotate=True), "every node of a depth-40 caterpillar's spine annotated", n_ann=2))
    return c


def all_cases():
    return roho_cases() + [wide_case(65), wide_case(257), caterpillar_case()] + mutation_cases() + clade_cases()


def columns(case):
    """The annotation columns of a case as ugp_summary_clades takes them."""
    k = max([len(a) for a in case.ann] + [0])
    return [[j for j in range(case.arrays["n"]) if len(case.ann[j]) > col and case.ann[j][col] != ""] for col in range(k)]


def topology(arrays):
    """The same tree without mutations: a handle for arrays the placement tables refuse (masked entries, a key twice on a node)."""
    n = arrays["n"]
    return {"n": n, "parent": arrays["parent"], "mut_off": np.zeros(n + 1, np.int64), "mut_pos": np.zeros(0, np.int32),
            "mut_ref": np.zeros(0, np.int8), "mut_par": np.zeros(0, np.int8), "mut_nuc": np.zeros(0, np.int8), "names": arrays["names"]}


def n_candidates(arrays):
    """RoHo's work-items: the entries of non-leaf nodes other than the root."""
    par = np.asarray(arrays["parent"]).astype(np.int64)
    inner = np.zeros(arrays["n"], bool)
    inner[par[1:]] = True
    inner[0] = False
    return int(np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))[inner].sum())
