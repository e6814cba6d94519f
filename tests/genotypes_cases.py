"""Trees and selections for the genotype tests (tests/genotypes_ref.py), as the breadth-first arrays of tests/synth.py.  Every
case is (name, arrays, [selection, ...]); a selection is a list of breadth-first node indices, None: all leaves.  `plain` says
whether Placer takes the arrays as its own tree (one-hot alleles, one mutation per position and node); the others are attached to
a handle of the bare topology."""
import numpy as np

from tests import nearest_cases as NC
from tests import synth

A, C, G, T = 1, 2, 4, 8


def with_entries(arrays, extra, front=False):
    """arrays with the entries extra[node] = [(pos, ref, par, nuc), ...] appended to (front: put before) the node's own."""
    off = np.asarray(arrays["mut_off"]).astype(np.int64)
    cols = [np.asarray(arrays[k]).astype(np.int64) for k in ("mut_pos", "mut_ref", "mut_par", "mut_nuc")]
    rows, noff = [], [0]
    for v in range(arrays["n"]):
        own = [tuple(int(c[k]) for c in cols) for k in range(off[v], off[v + 1])]
        add = list(extra.get(v, ()))
        rows += add + own if front else own + add
        noff.append(len(rows))
    out = dict(arrays)
    out["mut_off"] = np.asarray(noff, np.int64)
    r = np.asarray(rows, np.int64).reshape(len(rows), 4)
    out["mut_pos"] = r[:, 0].astype(np.int32)
    for i, k in enumerate(("mut_ref", "mut_par", "mut_nuc"), 1):
        out[k] = r[:, i].astype(np.int8)
    return out


def hand(parent, muts):
    n = len(parent)
    base = {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": np.zeros(n + 1, np.int64), "mut_pos": np.zeros(0, np.int32),
            "mut_ref": np.zeros(0, np.int8), "mut_par": np.zeros(0, np.int8), "mut_nuc": np.zeros(0, np.int8), "names": ["n%d" % j for j in range(n)]}
    return with_entries(base, muts)


def topology(arrays):
    """The same tree without mutations."""
    return hand(arrays["parent"], {})


def leaves_of(arrays):
    par = np.asarray(arrays["parent"])
    return np.setdiff1d(np.arange(arrays["n"]), par[1:])


def under(arrays, v):
    """The nodes of v's subtree."""
    par = np.asarray(arrays["parent"]).astype(np.int64)
    inside = np.zeros(arrays["n"], bool)
    inside[v] = True
    for j in range(v + 1, arrays["n"]):   # parents precede their children
        inside[j] = inside[par[j]]
    return inside


def random_cases():
    out = []
    for seed, n_leaves in ((1, 130), (2, 700), (3, 1700)):
        arrays = synth.make_case(seed, n_leaves=n_leaves, n_queries=1, n_sites=80, genome_len=600)[0]
        rng = np.random.default_rng(100 + seed)
        third = rng.choice(arrays["n"], arrays["n"] // 3, replace=False)
        lv = leaves_of(arrays)
        dup = np.concatenate([lv[::3], lv[::6], lv[:5]])
        out.append(("random%d" % n_leaves, arrays, [None, third, [int(lv[len(lv) // 2])], [int(third[0])], dup], True))
    return out


def segment_case():
    """nearest_cases.segment_tree(): a node with m entries mutates positions 1 .. m, so w, v, c2 and most leaves inside them share
    position 1 (alleles and stored parent alleles are redrawn at random here); position 9 is mutated by v, c2, leaves of c2 and, after
    v in depth-first order, leaves of c3 only: with the leaves outside v selected its first owners have no column."""
    arrays, ids = NC.segment_tree()
    rng = np.random.default_rng(21)
    m = len(arrays["mut_pos"])
    arrays["mut_nuc"] = rng.choice([A, C, G, T], m).astype(np.int8)
    arrays["mut_par"] = rng.choice([A, C, G, T], m).astype(np.int8)
    par = np.asarray(arrays["parent"])
    in_c2 = np.flatnonzero(par == ids["c2"])
    in_c3 = np.flatnonzero(par == ids["c3"])
    extra = {ids["v"]: [(9, A, A, C)], ids["c2"]: [(9, A, C, G)]}
    for v in in_c2[::500]:
        extra[int(v)] = [(9, A, G, T)]
    for v in in_c3[10::700]:
        extra[int(v)] = [(9, A, T, C)]
    arrays = with_entries(arrays, extra)
    lv = leaves_of(arrays)
    in_v = under(arrays, ids["v"])
    return ("segments", arrays, [None, in_c2, lv[~in_v[lv]]], True), ids


def caterpillar_case():
    """Position 5000 flips A -> C -> A -> C down the chain of 150 (a 150-deep climb, back-mutations to REF); at position 5001 the root
    goes A -> C and both its children C -> A: every covered column carries REF and the position is no site."""
    arrays = synth.caterpillar_case(5, depth=150, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=300)[0]
    extra = {0: [(5001, A, A, C)], 2: [(5001, A, C, A)]}
    for k in range(1, 151):
        extra.setdefault(2 * k - 1, []).append((5000, A, A if k % 2 else C, C if k % 2 else A))
    extra[1].append((5001, A, C, A))
    arrays = with_entries(arrays, extra)
    chain = [2 * k - 1 for k in range(1, 151)]
    return ("caterpillar", arrays, [None, chain + [2, 300], list(range(arrays["n"]))], True)


def polytomy_case():
    """One position (6000) mutated by all 300 children of the root: hundreds of sibling owners."""
    arrays = synth.polytomy_case(6, fanouts=(300,), n_queries=1)[0]
    rng = np.random.default_rng(7)
    extra = {v: [(6000, A, A, int(rng.choice([A, C, G, T])))] for v in range(1, arrays["n"])}
    arrays = with_entries(arrays, extra)
    return ("polytomy", arrays, [None, list(range(0, arrays["n"], 7)), [0]], True)


#        0
#      / | \
#     1  2  3
#    /|  |  |\
#   4 5  6  7 8
#  /|       |
# 9 10      11
HAND = [-1, 0, 0, 0, 1, 1, 2, 3, 3, 4, 4, 7]


def hand_cases():
    out = []
    # two entries at one position on one node: the allele from the last, REF from the first
    out.append(("two_entries", hand(HAND, {1: [(10, A, G, C), (10, A, C, T)], 4: [(10, A, T, G)], 6: [(10, A, A, C), (20, C, C, A), (10, A, C, A)]}),
                [None, [4, 5, 1], [6]], False))
    # the outermost owner stores a parent allele that is not the reference base
    out.append(("par_not_ref", hand(HAND, {1: [(10, A, G, C)], 9: [(10, A, C, A)], 3: [(10, A, T, G)], 11: [(10, A, G, T)]}), [None, [9, 10, 11], [3, 11]], True))
    # masked entries (negative positions) at and beside a site position
    out.append(("masked", hand(HAND, {0: [(-10, A, A, C)], 1: [(-10, 0, 0, 0), (10, A, A, G)], 4: [(-1, 0, 0, 0)], 10: [(10, A, G, A), (-10, A, A, T)], 3: [(-20, C, C, T)],
                                      8: [(20, C, C, G)]}), [None, [1, 10, 8]], False))
    # ambiguous alleles: codes 2 .. 12 on eleven leaves under a polytomy, REF = 1
    par = [-1] + [0] * 12 + [1]
    muts = {v: [(33, A, A, v)] for v in range(2, 13)}
    muts[1] = [(33, A, A, 15), (40, G, G, 14)]
    muts[13] = [(33, A, 15, A)]
    out.append(("ambiguous", hand(par, muts), [None, list(range(14)), [12, 11, 13]], False))
    out.append(("no_mutation", hand(HAND, {}), [None, [3]], True))
    out.append(("all_masked", hand(HAND, {1: [(-5, A, A, C)], 7: [(-6, A, A, C)]}), [None], False))
    return out


def seven_sites():
    """Seven sites over twelve nodes, for row windows."""
    muts = {1: [(3, A, A, C), (9, G, G, T)], 2: [(5, C, C, T)], 3: [(3, A, A, G), (11, T, T, A)], 4: [(7, A, A, T), (9, G, T, G)], 7: [(13, C, C, A)],
            9: [(15, G, G, A)], 11: [(11, T, A, C), (15, G, G, C)]}
    return hand(HAND, muts)


FIVE = hand([-1, 0, 0, 1, 1], {1: [(100, A, A, C)], 3: [(100, A, C, T), (200, G, G, A)], 2: [(-7, A, A, C), (300, T, T, 5)],
                               4: [(200, G, G, G)]})
FIVE["names"] = ["root", "inner", "s2", "s3", "s4"]
# all leaves, depth-first: s3, s4, s2.  Position 100: REF A, s3 = T, s4 = C (from `inner`), s2 uncovered; 200: REF G, s3 = A, s4 = G;
# 300: REF T, s2 = R (code 5).
FIVE_VCF = ("##fileformat=VCFv4.2\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts3\ts4\ts2\n"
            "NC_045512v2\t100\tA100C,A100T\tA\tC,T\t.\t.\tAC=1,1;AN=3\tGT\t2\t1\t0\n"
            "NC_045512v2\t200\tG200A\tG\tA\t.\t.\tAC=1;AN=3\tGT\t1\t0\t0\n"
            "NC_045512v2\t300\tT300R\tT\tR\t.\t.\tAC=1;AN=3\tGT\t0\t0\t1\n")


def all_cases():
    return random_cases() + [segment_case()[0], caterpillar_case(), polytomy_case()] + hand_cases() + [("seven", seven_sites(), [None, [9, 10, 11, 6]], True)]
