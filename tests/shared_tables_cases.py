"""The eleven query families that read one handle's depth-first tables, each as (attach, ask, want), for the tests of their sharing
(tests/test_shared_tables_cpu.py, tests/test_shared_tables_gpu.py).

A handle owns one set of depth-first tables; whichever family attaches first builds them, `onode` is made by the first of translate,
select and haplotypes, and the leaf ranks by whoever needs them first.  So every family has to answer the same after every other,
and every attach has to refuse mutation arrays other than the ones the tables were built from.

Two trees, built here:
  plain  a random tree the placement tables accept; the handle is Placer(arrays);
  bare   a hand tree with masked entries and ambiguous alleles, no node with two entries at one position, alleles 1 .. 15; the handle
         is Placer(topology(arrays)) and every attach is given the arrays.
Per tree X, three sets of other arrays on the same topology with the same number of entries:
  Y_pos     every non-masked position + 1;
  Y_allele  mut_nuc of one non-masked entry (Tree.allele_entry) is another single allele, not mut_ref;
  Y_move    the last entry of a leaf (Tree.move_leaf) is the first of its next sibling, a leaf too: the flat entry arrays are the
            same, mut_off and so the per-node counts and cum differ.
A Family's questions are fixed by X (nodes, positions, codons); want(arrays) answers them from the family's reference in tests/*_ref.py
for X or a Y, ask(pl) from the device, both as plain Python data that compares with ==.  CHANGES says which Y changes which family's
answer: a silent acceptance of that Y would show in ask().
"""

import numpy as np

from oracle import capi
from tests import annotate_ref as AR
from tests import genotypes_ref as GR
from tests import haplotypes_ref as HR
from tests import mask_ref as MR
from tests import nearest_ref as NR
from tests import relatives_ref as RR
from tests import select_ref as SLR
from tests import subtree_ref as STR
from tests import summary_cases as SMC
from tests import summary_ref as SMR
from tests import synth
from tests import translate_cases as TC
from tests import translate_ref as TR
from tests import uncertainty_ref as UR
from tests import vectors_ref as VR
from usher_amd import Placer, QueryBatch

NAMES = ("uncertainty", "annotate", "nearest", "relatives", "select", "mask", "subtree", "genotypes", "summary", "translate", "haplotypes")
YS = ("Y_pos", "Y_allele", "Y_move")
ONEHOT = (1, 2, 4, 8)

# Which other arrays change which family's answer, per tree (asserted by tests/test_shared_tables_cpu.py).  A shift of every position
# leaves what depends on the entries' identity and counts alone; nearest and relatives read only the counts per node, so only Y_move
# shows there; the mutation table, the RoHo records and the clade counts of summary do not see an entry move between two leaves.
_ALL = {"Y_pos": True, "Y_allele": True, "Y_move": True}
_COUNTS = {"Y_pos": False, "Y_allele": False, "Y_move": True}
CHANGES = {
    "plain": {"uncertainty": {"Y_pos": False, "Y_allele": True, "Y_move": False}, "annotate": _ALL, "nearest": _COUNTS, "relatives": _COUNTS,
              "select": _ALL, "mask": _ALL, "subtree": _ALL, "genotypes": _ALL, "summary": {"Y_pos": True, "Y_allele": True, "Y_move": False},
              "translate": _ALL, "haplotypes": _ALL},
    "bare": {"uncertainty": {"Y_pos": False, "Y_allele": True, "Y_move": True}, "annotate": _ALL, "nearest": _COUNTS, "relatives": _COUNTS,
             "select": _ALL, "mask": _ALL, "subtree": _ALL, "genotypes": _ALL, "summary": {"Y_pos": True, "Y_allele": True, "Y_move": False},
             "translate": _ALL, "haplotypes": _ALL},
}


# ---- the trees -----------------------------------------------------------------------------------------------------------------

def bare_arrays():
    """241 nodes: the root, 5 clades of 4 sub-clades with 10 leaves each and 3 leaves of their own.  Node j carries 0 .. 3 entries at
    45 odd positions (so positions repeat over the tree), each from the true state of its parent; every 13th node begins with a masked
    entry, and some leaf entries carry the three-base ambiguity code that leaves out the parent allele."""
    spec = [[[[] for _ in range(10)] for _ in range(4)] + [[] for _ in range(3)] for _ in range(5)]
    parent, kids_of, queue, head = [-1], [spec], [], 0
    while head < len(parent):   # breadth-first numbering
        for c in kids_of[head]:
            parent.append(head)
            kids_of.append(c)
        head += 1
    n = len(parent)
    ref = lambda p: ONEHOT[p % 4]
    state, off, rows = [None] * n, [0], []
    for j in range(n):
        st = dict(state[parent[j]]) if j else {}
        if j % 13 == 5:
            rows.append((-1, 1, 1, 1))
        for t in range((0, 1, 2, 1, 3, 0, 2)[j % 7] if j else 0):
            p = 3 + 2 * ((j * 11 + t * 17) % 45)
            cur = st.get(p, ref(p))
            new = [a for a in ONEHOT if a != cur][(j + t) % 3]
            if not kids_of[j] and (3 * j + t) % 29 == 0:
                new = cur ^ 15
            rows.append((p, ref(p), cur, new))
            st[p] = new
        state[j] = st
        off.append(len(rows))
    r = np.asarray(rows, np.int64)
    return {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": np.asarray(off, np.int64), "mut_pos": r[:, 0].astype(np.int32),
            "mut_ref": r[:, 1].astype(np.int8), "mut_par": r[:, 2].astype(np.int8), "mut_nuc": r[:, 3].astype(np.int8),
            "names": ["n%d" % j for j in range(n)]}


def _kids(arrays):
    kids = [[] for _ in range(int(arrays["n"]))]
    for j in range(1, int(arrays["n"])):
        kids[int(arrays["parent"][j])].append(j)
    return kids


class Tree:
    """X, its three Ys and the nodes the questions are about."""

    def __init__(self, name, arrays, plain, allele_leaf, genome_len):
        self.name, self.X, self.plain, self.genome_len = name, arrays, plain, genome_len
        self.n = n = int(arrays["n"])
        self.kids = kids = _kids(arrays)
        par = self.par = [int(p) for p in arrays["parent"]]
        off, pos = np.asarray(arrays["mut_off"]).astype(np.int64), np.asarray(arrays["mut_pos"]).astype(np.int64)
        self.leaves = [j for j in range(n) if not kids[j]]
        # Y_move: the first leaf whose last entry is non-masked and at a position its next sibling, a leaf too, does not have
        self.move_leaf = next(a for a in range(1, n - 1) if not kids[a] and not kids[a + 1] and par[a] == par[a + 1] and off[a + 1] > off[a]
                              and pos[off[a + 1] - 1] >= 0 and pos[off[a + 1] - 1] not in pos[off[a + 1]:off[a + 2]].tolist())
        # Y_allele: the first non-masked entry of a chosen leaf
        assert not kids[allele_leaf]
        self.allele_leaf = allele_leaf
        self.allele_entry = next(k for k in range(off[allele_leaf], off[allele_leaf + 1]) if pos[k] >= 0)
        self.Y = {"Y_pos": self._y_pos(), "Y_allele": self._y_allele(), "Y_move": self._y_move()}
        for y in self.Y.values():
            assert int(y["mut_off"][-1]) == int(off[-1]) and np.array_equal(y["parent"], arrays["parent"])
        a, v = self.move_leaf, allele_leaf
        sib = next(c for c in kids[par[v]] if c != v)
        self.nodes = list(dict.fromkeys([v, a, a + 1, sib, par[v], par[a]]))           # a handful, internal ones among them
        self.some_leaves = list(dict.fromkeys([v, a, a + 1] + [c for c in (sib, self.leaves[0], self.leaves[-1]) if not kids[c]]))
        below = [[j] if not kids[j] else [] for j in range(n)]                         # the leaves below every node
        for j in range(n - 1, 0, -1):
            below[par[j]] = below[j] + below[par[j]]
        self.clade_leaves = below[next(j for j in range(1, n) if 20 <= len(below[j]) <= 80)]   # a whole clade: some keys are its own

    def _y_pos(self):
        y = dict(self.X)
        p = np.asarray(self.X["mut_pos"])
        y["mut_pos"] = np.where(p >= 0, p + 1, p).astype(np.int32)
        return y

    def _y_allele(self):
        y, k = dict(self.X), self.allele_entry
        nuc = np.asarray(self.X["mut_nuc"]).copy()
        nuc[k] = next(a for a in ONEHOT if a != int(nuc[k]) and a != int(self.X["mut_ref"][k]))
        y["mut_nuc"] = nuc
        return y

    def _y_move(self):
        y = dict(self.X)
        off = np.asarray(self.X["mut_off"]).copy()
        off[self.move_leaf + 1] -= 1
        y["mut_off"] = off
        return y

    def handle(self):
        return Placer(self.X) if self.plain else Placer(SMC.topology(self.X))

    def __repr__(self):
        return self.name


_TREES = {}


def trees():
    if not _TREES:
        plain = synth.make_case(2, n_leaves=250, n_queries=1, n_sites=60, genome_len=500)[0]
        _TREES["plain"] = Tree("plain", plain, True, PLAIN_ALLELE_LEAF, 500)
        _TREES["bare"] = Tree("bare", bare_arrays(), False, BARE_ALLELE_LEAF, 100)
    return _TREES


# leaves whose first entry decides their own placement (its position mutates elsewhere in the tree too), found by search
PLAIN_ALLELE_LEAF = 4
BARE_ALLELE_LEAF = 46


# ---- the families ----------------------------------------------------------------------------------------------------------------

def _ints(x):
    return [int(v) for v in x]


def _sub_plain(d):
    """A Placer.subtree_nodes dict, or a tests/subtree_ref.py result, as plain data."""
    return {k: _ints(d[k]) for k in ("kept", "parent", "ent_off", "pos", "first_entry", "nuc")} | \
        {k: int(d["info"][k]) for k in ("n_selected", "n_gathered", "n_disagree", "longest_chain", "first_disagree")}


class Family:
    """attach(pl, arrays) / ask(pl) / want(arrays) of one family on one Tree, and call_unattached(pl): a run call of the family with
    no arguments, for the error a handle without the family's attach gives."""

    def __init__(self, tree, name):
        self.tree, self.name = tree, name
        self.attach = getattr(self, "_attach_" + name, None) or (lambda pl, arrays: getattr(pl, name + "_attach")(arrays))
        self.ask, self.want = getattr(self, "_ask_" + name), getattr(self, "_want_" + name)
        self._wants = {}
        getattr(self, "_init_" + name, lambda: None)()

    def __repr__(self):
        return self.name

    def wanted(self, which="X"):
        """want() of X or of a Y, computed once."""
        if which not in self._wants:
            self._wants[which] = self.want(self.tree.X if which == "X" else self.tree.Y[which])
        return self._wants[which]

    def check(self, pl, why):
        """ask(pl) equals the reference's answer for X, exactly."""
        assert self.ask(pl) == self.wanted(), (self.tree.name, self.name, why)

    def call_unattached(self, pl):
        L, h = pl._L, pl._h
        return {"uncertainty": lambda: L.ugp_uncertainty(h, None, 0, 0, None, None, None, None),
                "annotate": lambda: L.ugp_clade_descendants(h, None, None, 0, None, None, 0, None),
                "nearest": lambda: L.ugp_nearest_k(h, 0, None, None, 1, None, None, None),
                "relatives": lambda: L.ugp_relatives_closest(h, 0, None, None, None, None, 0, None),
                "select": lambda: L.ugp_select_leaves(h, None, None),
                "mask": lambda: L.ugp_mask_mutations(h, 0, None, None, None, None, None, None, None, None, None),
                "subtree": lambda: L.ugp_subtree_nodes(h, 0, None, None, None, None, 0, None, None, None),
                "genotypes": lambda: L.ugp_genotype_select(h, None, 0, None, None),
                "summary": lambda: L.ugp_summary_mutations(h, None, 0, None),
                "translate": lambda: L.ugp_translate(h, None, 0, None, None),
                "haplotypes": lambda: L.ugp_haplotype_groups(h, None, 0, None, None)}[self.name]()

    # uncertainty: EPPs, neighbourhood size and the whole tie list of a handful of nodes
    def _ask_uncertainty(self, pl):
        epps, nsize, ties, cnt = pl.uncertainty(self.tree.nodes, cap=self.tree.n)
        assert _ints(cnt) == _ints(epps)
        return [(int(e), int(s), _ints(t)) for e, s, t in zip(epps, nsize, ties)]

    def _want_uncertainty(self, arrays):
        return [(int(nb), int(ns), _ints(t)) for nb, ns, t in UR.expected(arrays, self.tree.nodes)]

    # annotate: the allele counts and descendants of one clade set, and the literal search of one row set
    def _init_annotate(self):
        t = self.tree
        self.clades = [t.nodes + t.nodes[:1], t.some_leaves, [], [t.move_leaf]]
        self.pairs = [(0, t.par[t.allele_leaf]), (0, 0), (1, t.par[t.move_leaf]), (1, t.move_leaf), (2, 0)]
        self.rows = UR.literal_sample(t.X, t.allele_leaf)      # (unsorted, masked entries kept: rows the packed search refuses)

    def _ask_annotate(self, pl):
        alleles = [dict(zip(_ints(e), _ints(c))) for e, c in pl.clade_alleles(self.clades)]
        below = _ints(pl.clade_descendants(self.clades, [c for c, _ in self.pairs], [v for _, v in self.pairs]))
        best, ties, cnt = pl.annotate_search(QueryBatch([self.rows]), cap=self.tree.n)
        assert int(cnt[0]) == len(ties[0])
        return alleles, below, (int(best[0]), _ints(ties[0]))

    def _want_annotate(self, arrays):
        best, ties = AR.search(capi.OracleTree(arrays), arrays, self.rows)
        return ([AR.alleles_literal(arrays, c) for c in self.clades], [AR.descendants(arrays, self.clades[c], v) for c, v in self.pairs],
                (int(best), _ints(ties)))

    # nearest: a handful of (node, k)
    def _init_nearest(self):
        t = self.tree
        self.near = [(v, k) for v in (t.move_leaf, t.move_leaf + 1, t.allele_leaf) for k in (1, 3, 12)] + [(t.par[t.move_leaf], 2)]

    def _ask_nearest(self, pl):
        nodes, dist, info = pl.nearest_k([v for v, _ in self.near], [k for _, k in self.near], out_stride=len(self.tree.leaves))
        out = []
        for i in range(len(self.near)):
            w = int(info["count"][i])
            out.append(dict({"nodes": _ints(nodes[i, :w]), "dist": _ints(dist[i, :w])}, **{f: int(info[f][i]) for f in info.dtype.names}))
        return out

    def _want_nearest(self, arrays):
        F = NR.Fast(arrays)
        return [F.query(v, k) for v, k in self.near]

    # relatives: the closest relatives and the leaves within 3 entries of a handful of nodes, with name ranks
    def _attach_relatives(self, pl, arrays):
        pl.relatives_attach(self.rank, arrays)

    def _init_relatives(self):
        self.rank = np.random.default_rng(5).permutation(self.tree.n).astype(np.uint32)

    def _ask_relatives(self, pl):
        out = []
        for got in (pl.relatives_closest(self.tree.nodes), pl.relatives_within(self.tree.nodes, 3)):
            info, off, nodes = got
            out.append([dict({"nodes": _ints(nodes[int(off[i]):int(off[i + 1])])}, **{f: int(info[f][i]) for f in ("dist", "count", "levels", "best")})
                        for i in range(len(self.tree.nodes))])
        return out

    def _want_relatives(self, arrays):
        F = RR.Fast(arrays, self.rank)
        return [[F.closest(v) for v in self.tree.nodes], [F.within(v, 3) for v in self.tree.nodes]]

    # select: one batch of (position, allele) queries, one set of subtrees
    def _init_select(self):
        t, X = self.tree, self.tree.X
        ents = [t.allele_entry, int(X["mut_off"][t.move_leaf + 1]) - 1] + [k for k in range(0, len(X["mut_pos"]), 97) if X["mut_pos"][k] >= 0]
        self.qpos = [int(X["mut_pos"][k]) for k in ents] + [int(X["mut_pos"][t.allele_entry]), 0]
        self.qnuc = [int(X["mut_nuc"][k]) & 15 for k in ents] + [int(X["mut_par"][t.allele_entry]) & 15, 1]

    def _ask_select(self, pl):
        mask, counts = pl.select_mutations(self.qpos, self.qnuc)
        one, _ = pl.select_mutations(self.qpos[1:2], self.qnuc[1:2])          # the moved entry's key alone
        smask, scounts = pl.select_subtrees(self.tree.nodes)
        return _ints(pl.select_leaves()), _ints(mask), _ints(counts), _ints(one), _ints(smask), _ints(scounts)

    def _want_select(self, arrays):
        T = SLR.tree_from_arrays(arrays)
        names = list(arrays["names"])
        index = {s: j for j, s in enumerate(names)}
        mask, counts = SLR.literal_mutations(T, self.qpos, self.qnuc)
        one, _ = SLR.literal_mutations(T, self.qpos[1:2], self.qnuc[1:2])
        smask, scounts = SLR.literal_subtrees(T, names, self.tree.nodes)
        return [index[s] for s in SLR.leaves_by_rank(T)], _ints(mask), _ints(counts), _ints(one), _ints(smask), _ints(scounts)

    # mask: one set of named leaves, a few lines
    def _init_mask(self):
        t, X = self.tree, self.tree.X
        self.named = list(dict.fromkeys(t.some_leaves + t.clade_leaves))
        k, m = t.allele_entry, int(X["mut_off"][t.move_leaf + 1]) - 1
        key = lambda e: (int(X["mut_pos"][e]), int(X["mut_par"][e]) & 15, int(X["mut_nuc"][e]) & 15)
        self.lines = [key(k) + (0, []), (key(k)[0], 15, 15, t.par[t.allele_leaf], [t.allele_leaf]), key(m) + (t.move_leaf, []),
                      (key(m)[0], 15, key(m)[2], 0, [t.move_leaf + 1]), (key(m)[0], 15, 15, t.move_leaf + 1, [])]

    def _ask_mask(self, pl):
        roots, masked = pl.mask_restricted(self.named)
        first, counts = pl.mask_mutations(*[[l[i] for l in self.lines] for i in range(5)])
        return _ints(roots), _ints(masked), _ints(first), _ints(counts)

    def _want_mask(self, arrays):
        roots, masked = MR.literal_restricted(arrays, self.named)
        first, counts = MR.literal_mutations(arrays, self.lines)
        return _ints(roots), _ints(masked), _ints(first), _ints(counts)

    # subtree and subtree batch: one selection alone with every node's owner, two selections in one batch
    def _init_subtree(self):
        t = self.tree
        self.sels = [t.some_leaves + [t.par[t.allele_leaf]], list(dict.fromkeys(t.leaves[::9] + [t.move_leaf + 1]))]

    def _ask_subtree(self, pl):
        one = _sub_plain(pl.subtree_nodes(self.sels[0]))
        owner = _ints(pl.subtree_owner(np.arange(self.tree.n)))
        return one, owner, [_sub_plain(d) for d in pl.subtree_batch(self.sels)]

    def _want_subtree(self, arrays):
        lit = [STR.literal(arrays, s) for s in self.sels]
        return _sub_plain(lit[0]), _ints(lit[0]["owner"]), [_sub_plain(d) for d in lit]

    # genotypes: one selection of nodes
    def _ask_genotypes(self, pl):
        shape = pl.genotype_select(self.tree.nodes + self.tree.some_leaves)
        return shape, _ints(pl.genotype_columns()), GR.device_sites(pl.genotype_sites()), pl.genotype_rows().tolist()

    def _want_genotypes(self, arrays):
        r = GR.Fast(arrays).run(self.tree.nodes + self.tree.some_leaves, text=False)
        return (len(r.columns), len(r.sites)), _ints(r.columns), GR.site_rows(r.sites), r.codes.tolist()

    # summary: the mutation table, the RoHo records, one set of clade columns
    def _init_summary(self):
        t = self.tree
        inner = [j for j in range(1, t.n) if t.kids[j]]
        self.columns = [inner[::7], list(dict.fromkeys([t.par[t.move_leaf], 0]))]

    def _ask_summary(self, pl):
        muts = [(int(r["pos"]), int(r["par"]), int(r["nuc"]), int(r["count"])) for r in pl.summary_mutations()]
        roho = sorted((int(r["parent"]), int(r["child"]), int(r["entry"]), int(r["child_count"]), int(r["offspring_with"]), int(r["median_without"]))
                      for r in pl.summary_roho())
        per, leaf_clade = pl.summary_clades(self.columns)
        return muts, roho, [(int(r["column"]), int(r["node"]), int(r["inclusive"]), int(r["exclusive"])) for r in per], leaf_clade.tolist()

    def _want_summary(self, arrays):
        F = SMR.Fast(arrays)
        roho = sorted((p, c, e, cc, w, med) for _, _, p, c, e, cc, w, med in F.roho()[0])
        clades = SMR.clade_records(SMR.Tree(arrays), self.columns)
        per = [(c, v, clades[c][0][i], clades[c][1][i]) for c, col in enumerate(self.columns) for i, v in enumerate(col)]
        return F.mutations(), roho, per, [clades[c][2] for c in range(len(self.columns))]

    # translate: one codon table of two overlapping genes over X's reference bases
    def _attach_translate(self, pl, arrays):
        pl.translate_attach(arrays)
        pl.translate_codons(*TR.slot_tables(self.codons))

    def _init_translate(self):
        X, g = self.tree.X, self.tree.genome_len
        genome = np.array(list("ACGT"))[np.random.default_rng(3).integers(0, 4, g)]
        live = np.asarray(X["mut_pos"]) >= 0
        genome[np.asarray(X["mut_pos"]).astype(np.int64)[live] - 1] = np.array(list(SMR.NUC))[np.asarray(X["mut_ref"]).astype(np.int64)[live]]
        a, b = 3 * (g * 3 // 5 // 3), 1 + 3 * (g * 2 // 5 // 3)
        gtf = TC.gtf_line("a", 1, a) + "\n" + TC.gtf_line("b", b, b + 3 * ((g - b) // 3) - 1) + "\n"
        self.codons = TR.build_codon_map(gtf, "".join(genome))

    def _ask_translate(self, pl):
        recs, info = pl.translate()
        return TR.device_records(recs), {k: int(info[k]) for k in info.dtype.names}

    def _want_translate(self, arrays):
        T = SMR.Tree(arrays)
        return TR.records(T, self.codons), TR.info(T, self.codons)

    # haplotypes: the groups of all leaves, the sets of a handful
    def _ask_haplotypes(self, pl):
        groups, _ = pl.haplotype_groups()
        off, pos, nuc = pl.haplotype_sets(self.tree.some_leaves)
        sets = [list(zip(_ints(pos[int(a):int(b)]), _ints(nuc[int(a):int(b)]))) for a, b in zip(off[:-1], off[1:])]
        return [(int(g["leaf"]), int(g["count"]), int(g["size"])) for g in groups], sets

    def _want_haplotypes(self, arrays):
        F = HR.Fast(arrays)
        return F.group_records(), F.leaf_sets(self.tree.some_leaves)


_FAMILIES = {}


def families(tree):
    """The eleven families of a tree, in the order of NAMES; their wants are computed once and shared."""
    if tree.name not in _FAMILIES:
        _FAMILIES[tree.name] = [Family(tree, name) for name in NAMES]
    return _FAMILIES[tree.name]


# ---- vectors, which asks about (sample, node) pairs and so brings samples of its own --------------------------------------------------

def vectors_questions(t):
    if t.name == "plain":
        arrays, queries = synth.make_case(2, n_leaves=250, n_queries=4, n_sites=60, genome_len=500)
        assert np.array_equal(arrays["mut_pos"], t.X["mut_pos"]) and np.array_equal(arrays["mut_off"], t.X["mut_off"])
    else:
        ref = lambda p: ONEHOT[p % 4]
        rows = lambda k: [(p, (None, 15 ^ ref(p), [a for a in ONEHOT if a != ref(p)][k % 3], ref(p) | 8)[(p // 2 + k) % 4]) for p in range(3 + 2 * k, 93, 6)]
        queries = [{"name": "b%d" % k, "pos": np.asarray([p for p, _ in rows(k)], np.int32), "ref": np.asarray([ref(p) for p, _ in rows(k)], np.int8),
                    "nuc": np.asarray([15 if a is None else a for _, a in rows(k)], np.int8),
                    "is_missing": np.asarray([a is None for _, a in rows(k)], np.int8)} for k in range(3)]
    pairs = [(s, j) for s in range(len(queries)) for j in t.nodes + [0]]
    ot = capi.OracleTree(t.X)
    return queries, pairs, [VR.oracle_answer_split(ot, queries[s], j) for s, j in pairs]


_VECTORS = {}


def vectors_asked(t):
    """(queries, pairs, the oracle's answers) of a tree, computed once."""
    if t.name not in _VECTORS:
        _VECTORS[t.name] = vectors_questions(t)
    return _VECTORS[t.name]


def vectors_answer(t, pl, why):
    queries, pairs, wanted = vectors_asked(t)
    ans = VR.device_answers(*pl.vectors(QueryBatch(queries), [j for _, j in pairs], [s for s, _ in pairs]))
    for a, w, pr in zip(ans, wanted, pairs):
        assert not a["refused"] and VR.agrees(a, w) and VR.agrees_split(a, w), (t.name, pr, why)


class Vectors:
    """Vectors with the face of a Family, as far as attach and check go."""
    name = "vectors"

    def __init__(self, tree):
        self.tree = tree

    def attach(self, pl, arrays):
        pl.vectors_attach(arrays)

    def check(self, pl, why):
        vectors_answer(self.tree, pl, why)


def family(t, name):
    """The Family of that name, or Vectors: something with attach(pl, arrays) and check(pl, why)."""
    return Vectors(t) if name == "vectors" else next(f for f in families(t) if f.name == name)


def flat(x):
    """Every number and string inside nested lists, tuples and dicts."""
    if isinstance(x, dict):
        for v in x.values():
            yield from flat(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from flat(v)
    else:
        yield x
