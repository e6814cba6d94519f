"""Hand-shaped trees for matUtils summary --haplotype (tests/haplotypes_ref.py), as the breadth-first arrays of tests/synth.py.

Trees are written as the nested N(mutations, children, tag=) of tests/summary_cases.py.  A mutation is "A100C" (reference and stored
parent allele A, position 100, allele C), "A/C100G" (reference allele A, stored parent allele C) or "MASKED"; letters are those of
get_nuc, so R, Y and N are the ambiguous codes 5, 10 and 15.  Every Case names the rule it pins and, where the table is short, the
very text the reference writes after its header (`text`).  `device` is False for the one case the device refuses, `cli` for the
trees of one node, which no newick string names (the loader refuses them as the reference's does).  The mutations of
a node ascend by position, masked ones first, no entry has mut_nuc == par_nuc and reference and parent alleles are single bases, so
that every case survives the trip through a .pb file unchanged (mutation_annotated_tree.cpp:566-594 drops and sorts otherwise).
tests/test_haplotypes_cpu.py checks the texts against the literal restatement, so the device tests compare against a yardstick that
is known to exercise the rule.
"""
import collections

import numpy as np

from tests import summary_cases as SC
from tests import summary_ref as SR

N, F = SC.N, SC.F


def parse(m):
    """(position, ref, par, nuc)."""
    if m.startswith("MASKED"):
        return (-1, 0, 0, 0)
    ref = par = SR.NUC.index(m[0], 1)
    body = m[1:]
    if body[0] == "/":
        par = SR.NUC.index(body[1], 1)
        body = body[2:]
    return (int(body[:-1]), ref, par, SR.NUC.index(body[-1], 1))


def build(root):
    """(arrays, tags): SC.build with a reference allele of its own per entry."""
    order, parent, q = [], [], collections.deque([(root, -1)])
    while q:   # Tree::breadth_first_expansion
        nd, p = q.popleft()
        j = len(order)
        order.append(nd)
        parent.append(p)
        q.extend((k, j) for k in nd.kids)
    off, rows, tags = [0], [], {}
    for j, nd in enumerate(order):
        rows += [parse(m) for m in nd.muts]
        off.append(len(rows))
        if nd.tag is not None:
            assert nd.tag not in tags
            tags[nd.tag] = j
    r = np.asarray(rows, np.int64).reshape(len(rows), 4)
    n = len(order)
    arrays = {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": np.asarray(off, np.int64), "mut_pos": r[:, 0].astype(np.int32),
              "mut_ref": r[:, 1].astype(np.int8), "mut_par": r[:, 2].astype(np.int8), "mut_nuc": r[:, 3].astype(np.int8),
              "names": ["n%d" % j for j in range(n)]}
    return arrays, tags


class Case:
    def __init__(self, name, root, rule, text=None, device=True, cli=True):
        self.name, self.rule, self.text, self.device, self.cli = name, rule, text, device, cli
        self.arrays, self.tags = build(root)
        self.ann = [[] for _ in range(self.arrays["n"])]     # (write_annotated of tests/test_summary_cpu.py reads it)

    def __repr__(self):
        return self.name

    def tree(self):
        return SR.Tree(self.arrays)


def caterpillar(depth, every=1):
    """A spine of `depth` internal nodes, each with two leaf children in front of the next spine node; spine node i (from the top)
    sets position 10 + i when i is a multiple of `every`, and every seventh of those puts an earlier position back."""
    node = None
    for i in reversed(range(depth)):
        muts = []
        if i % every == 0:
            k = i // every
            if k % 7 == 6:
                muts.append("A/C%dA" % (10 + i - 3 * every))
            muts.append("A%dC" % (10 + i))
        node = N(muts, [N(), N()] + ([node] if node is not None else []))
    return node


def star(n_leaves, root_muts=("A100C",), every=0):
    """A root with n_leaves leaf children; every `every`-th leaf carries one of three private mutations (0: none does)."""
    own = ("G200T", "G200A", "C300T")
    return N(list(root_muts), [N([own[(i // every) % 3]] if every and i % every == 0 else []) for i in range(n_leaves)])


def cli_cases():
    return [c for c in hand_cases() if c.cli]


def hand_cases():
    c = []
    # ---- rules
    c.append(Case("revert_equals_reference", N((), [N(["A100C"], [N(["A/C100A"]), N()]), N()]),
                  "a leaf whose own entry puts the position back equals a leaf elsewhere that never left the reference",
                  "reference\t2\n100C\t1\n"))
    c.append(Case("different_histories", N((), [N(["A100G"], [N()]), N(["A100T"], [N(["A/T100G"]), N()])]),
                  "equal sets under different children of the root: A>G on one side, A>T then T>G on the other",
                  "100G\t2\n100T\t1\n"))
    c.append(Case("revert_nothing_set", N((), [N(["A/C100A"]), N(), N(["A/C100A", "G200T"])]),
                  "an entry with mut_nuc == ref_nuc at a position nothing set erases nothing",
                  "reference\t2\n200T\t1\n"))
    c.append(Case("each_by_its_own_ref", N((), [N(["A100C"], [N(), N(["C/A100C"]), N(["G/C100A"])])]),
                  "two entries at one position on a path with different stored ref_nuc: the lower one is judged by its own (C == C "
                  "erases; A != G sets A)", "reference\t1\n100A\t1\n100C\t1\n"))
    c.append(Case("ambiguous_codes", N((), [N(["A100N"]), N(["A100Y"]), N(["A100R"]), N(["A100C"]), N(["A100R"])]),
                  "ambiguous allele codes 5, 10 and 15 are alleles like any other and order by their code",
                  "100C\t1\n100R\t2\n100Y\t1\n100N\t1\n"))
    c.append(Case("masked_entries", N(["MASKED", "A50C"], [N(["MASKED", "G200T"], [N(), N(["MASKED"])]), N()]),
                  "masked entries on the root, on a path and on a leaf change nothing", "50C\t1\n50C,200T\t2\n"))
    c.append(Case("root_mutations", N(["A10C", "G20T"], [N(), N(["C30T"]), N(["A/C10A"])]),
                  "the root's own entries count for every leaf; one leaf puts one of them back",
                  "10C,20T\t1\n10C,20T,30T\t1\n20T\t1\n"))
    c.append(Case("proper_prefix", N((), [N(["A100C", "G200T"]), N(["A100C"]), N(["A100C", "T150G"]), N(["A100C"])]),
                  "a set that is a proper prefix of another comes first", "100C\t2\n100C,150G\t1\n100C,200T\t1\n"))
    c.append(Case("allele_only", N((), [N(["A100G"]), N(["A100C"]), N(["A100T"]), N(["A100C"], [N(), N(["G200T"])])]),
                  "sets that differ only in the allele at one position order by the allele code",
                  "100C\t2\n100C,200T\t1\n100G\t1\n100T\t1\n"))
    c.append(Case("override_deeper", N((), [N(["A100C", "A200G"], [N(["C100T"], [N(), N()]), N()])]),
                  "an entry overridden deeper on the path: the deepest one counts", "100C,200G\t1\n100T,200G\t2\n"))
    # ---- shapes
    c.append(Case("single_node", N(), "a tree that is only a root counts the root", "reference\t1\n", cli=False))
    c.append(Case("single_node_mutated", N(["A5C", "G9T"]), "... with the root's own entries", "5C,9T\t1\n", cli=False))
    c.append(Case("no_mutations", N((), [F(3), N()]), "no mutation anywhere: one group", "reference\t4\n"))
    c.append(Case("all_distinct", N(["A5C"], [N(["A%dC" % (100 + i)]) for i in range(70)]), "every leaf its own set"))
    c.append(Case("caterpillar600", caterpillar(600), "a caterpillar of 600: sets of up to some 500 pairs, every set on two leaves"))
    c.append(Case("star_shared", star(700), "a star whose leaves all share one set", "100C\t700\n"))
    c.append(Case("set_sizes", N((), [N(["A%dC" % (10 + i) for i in range(63)]), N(), N(["A%dC" % (10 + i) for i in range(64)]),
                                      N(["A%dG" % (10 + i) for i in range(65)]), N(["A%dT" % (10 + i) for i in range(300)])]),
                  "sets of 63, 0, 64, 65 and 300 pairs on neighbouring leaves"))
    # ---- refusal
    c.append(Case("duplicate_position", N((), [N(["A200C"], [N(["A100C", "C100G"], tag="D"), N()]), N(["A100G"])]),
                  "a node with two non-masked entries at one position: the walk takes the last, the device refuses",
                  "100G\t1\n100G,200C\t1\n200C\t1\n", device=False))
    return c


def segment_edge_tree():
    """A first child of the root whose subtree ends exactly at depth-first position 16384 (one scan segment), a last child whose
    subtree ends at n; both carry an entry that must not leak past their subtree."""
    a = N(["A100C"], [N(["G200T"] if i % 1000 == 0 else []) for i in range(16382)])
    b = N(["A100G"], [N(["G200T"] if i % 10 == 0 else []) for i in range(99)])
    return N((), [a, N(), N(["G200T"]), b])
