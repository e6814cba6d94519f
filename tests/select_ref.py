"""matUtils extract's sample selectors restated for the tests (the reference cannot be built here).

LITERAL functions follow matUtils/select.cpp and extract.cpp statement by statement on the host tree of oracle/refio.py:
get_clade_samples (select.cpp:38-65), get_mutation_samples (:67-111), Tree::get_leaves_ids, get_mrca_samples (:570-575, through
tests/usher_model.py's get_subtree), get_sample_match (:506-520), and `chain`: the selection steps of extract_main in their order
(extract.cpp:264-472) with `matutils-amd select`'s three stated conventions -- depth-first order where the reference iterates an
unordered_set, leaves only for -e with nothing selected, std::regex_match for -H.  They return sample names.

Fast gives the device calls' answers -- bool masks by LEAF RANK (the r-th leaf of the depth-first expansion), counts, the MRCA --
with numpy from the breadth-first arrays, for trees too big for the literal functions; tests/test_select_cpu.py holds it against
the literal ones on every small tree.
"""
import re

import numpy as np

from oracle import refio
from tests import relatives_ref as RR
from tests import usher_model as UM


def tree_from_arrays(arrays, ann=None):
    """The host tree of breadth-first arrays: names arrays["names"] or n<j>, annotations ann[j] (a list per node)."""
    n = int(arrays["n"])
    names = list(arrays.get("names") or ["n%d" % j for j in range(n)])
    T = refio.Tree()
    nodes = []
    off = np.asarray(arrays["mut_off"]).astype(np.int64)
    for j in range(n):
        p = int(arrays["parent"][j])
        nd = T.create_node(names[j], nodes[p] if p >= 0 else None)
        for k in range(off[j], off[j + 1]):
            nd.mutations.append(refio.Mutation(int(arrays["mut_pos"][k]), int(arrays["mut_ref"][k]), int(arrays["mut_par"][k]),
                                               int(arrays["mut_nuc"][k]) & 0xFF))
        nodes.append(nd)
    if ann is not None:
        for j in range(n):
            nodes[j].clade_annotations = list(ann[j])
    return T


# ---- literal ------------------------------------------------------------------------------------------------------------------

def get_leaves_ids(T, nid=None):
    """Tree::get_leaves_ids: the leaves of the breadth-first expansion from the node; an unknown node has none."""
    if nid is None:
        return [n.identifier for n in UM.get_leaves(T)]
    node = T.get_node(nid)
    if node is None:
        return []
    return [n.identifier for n in UM.get_leaves(T, node)]


def get_clade_samples(T, clade_name):
    for s in T.depth_first_expansion():
        canns = s.clade_annotations
        if len(canns) > 0:
            if len(canns) > 1 or canns[0] != "":
                for c in canns:
                    if c == clade_name:
                        return get_leaves_ids(T, s.identifier)
    return []


def clade_root(T, clade_name):
    """The node get_clade_samples stops at, or None."""
    for s in T.depth_first_expansion():
        canns = s.clade_annotations
        if len(canns) > 0 and (len(canns) > 1 or canns[0] != "") and clade_name in canns:
            return s
    return None


def mutation_from_string(s):
    """(position, mut_nuc) as mutation_from_string (mutation_annotated_tree.cpp:358-380) reads it, or None."""
    m = re.match(r"(.)\s*([+-]?\d+)(.)", s, re.S)   # sscanf("%c%d%c")
    if not m or not ("A" <= m.group(1) <= "Z") or not ("A" <= m.group(3) <= "Z"):
        return None
    ref, alt = refio.get_nuc_id(m.group(1)), refio.get_nuc_id(m.group(3))
    pos = int(m.group(2))
    if refio.Mutation(pos, ref, ref, alt).get_string() != s:
        return None
    return pos, alt


def deciding_allele(node, position):
    """The walk of get_mutation_samples for one leaf: the mut_nuc of the entry that sets `assigned` -- the first entry at the
    position on the leaf, else on the nearest ancestor that has one -- or None when the walk reaches the root unassigned."""
    for m in node.mutations:
        if position == m.position:
            return m.mut_nuc
    for anc in UM._rsearch(node, False):
        for m in anc.mutations:
            if position == m.position:
                return m.mut_nuc
    return None


def mutation_samples(T, position, mut_nuc):
    """get_mutation_samples from its loop over the leaves on: a leaf is good when the entry that assigns it has the allele.
    mutation_from_string hands it no position below 0 ("A-1C" does not survive its round trip), so masked entries, which sit at
    negative positions, are never asked for: such a query selects nobody."""
    if position < 0:
        return []
    return [node.identifier for node in UM.get_leaves(T) if deciding_allele(node, position) == mut_nuc]


def mutation_samples_any_owner(T, position, mut_nuc):
    """NOT the reference: a leaf counts when ANY node on its root path carries the allele.  The tests use it to show that a query
    tells the two readings apart."""
    good = []
    for node in UM.get_leaves(T):
        if any(m.position == position and m.mut_nuc == mut_nuc for a in UM._rsearch(node, True) for m in a.mutations):
            good.append(node.identifier)
    return good


def get_mutation_samples(T, mutation_id):
    pm = mutation_from_string(mutation_id)
    assert pm is not None, mutation_id
    return mutation_samples(T, *pm)


def get_mrca(T, samples):
    return UM.get_subtree(T, samples).root.identifier


def get_mrca_samples(T, samples):
    return get_leaves_ids(T, get_mrca(T, samples))


def get_sample_match(T, samples, pattern):
    if len(samples) == 0:
        samples = get_leaves_ids(T)
    pat = re.compile(pattern)
    return [s for s in samples if pat.fullmatch(s)]


def sample_intersect(sset, nsamples):
    return [s for s in nsamples if s in sset]


def dfs_order(T, sset):
    return [n.identifier for n in T.depth_first_expansion() if n.identifier in sset]


def split_commas(s):
    """std::getline(stream, item, ','): no item after a trailing comma."""
    parts = s.split(",")
    if parts and parts[-1] == "":
        parts.pop()
    return parts


class NoSamples(Exception):
    """The chain ended in one of the reference's `ERROR: No samples fulfill selected criteria` exits."""


NONE_LEFT = "ERROR: No samples fulfill selected criteria. Change arguments and try again\n"
NONE_LEFT_PRUNE = "ERROR: No samples fulfill selected criteria (tree is left empty). Change arguments and try again\n"


def chain(T, samples=None, internal=None, clade=None, mutation=None, match=None, max_parsimony=-1, from_mrca=False, prune=False,
          max_epps=0, epps=None):
    """The selection steps of extract_main that `select` adds, in its order, and -a between them: (names, warnings).  `samples`:
    the names of -s.  epps: name -> equally parsimonious placements, for -e.  Raises NoSamples(message) where the reference exits."""
    samples = list(samples or [])
    warnings = []
    if internal is not None:
        ic = get_leaves_ids(T, internal)
        samples = ic if len(samples) == 0 else sample_intersect(set(ic), samples)
    if clade is not None:
        in_clade = set()
        for cname in split_commas(clade):
            cs = get_clade_samples(T, cname)
            if len(cs) == 0:
                warnings.append("WARNING: Clade %s is not detected in the input tree!\n" % cname)
            in_clade.update(cs)
        samples = dfs_order(T, in_clade) if len(samples) == 0 else sample_intersect(in_clade, samples)
        if len(samples) == 0:
            raise NoSamples(NONE_LEFT)
    if mutation is not None:
        with_mut = set()
        for mname in split_commas(mutation):
            ms = get_mutation_samples(T, mname)
            if len(ms) == 0:
                warnings.append("WARNING: No samples with mutation %s found in tree!\n" % mname)
            with_mut.update(ms)
        samples = dfs_order(T, with_mut) if len(samples) == 0 else sample_intersect(with_mut, samples)
        if len(samples) == 0:
            raise NoSamples(NONE_LEFT)
    if match is not None:
        samples = get_sample_match(T, samples, match)
        if len(samples) == 0:
            raise NoSamples(NONE_LEFT)
    if max_parsimony >= 0:
        check = samples if samples else get_leaves_ids(T)
        samples = [s for s in check if len(T.get_node(s).mutations) <= max_parsimony]
        if len(samples) == 0:
            raise NoSamples(NONE_LEFT)
    if max_epps > 0:
        check = set(samples) if samples else set(get_leaves_ids(T))   # nothing selected: the leaves only
        samples = [n.identifier for n in T.depth_first_expansion() if n.identifier in check and epps[n.identifier] <= max_epps]
        if len(samples) == 0:
            raise NoSamples(NONE_LEFT)
    if from_mrca:
        samples = get_mrca_samples(T, samples)
    if prune:
        sset = set(samples)
        samples = [s for s in get_leaves_ids(T) if s not in sset]
        if len(samples) == 0:
            raise NoSamples(NONE_LEFT_PRUNE)
    return samples, warnings


# ---- the closed form ------------------------------------------------------------------------------------------------------------

class Fast:
    """Masks by leaf rank from the breadth-first arrays: the owner of a position on a node is its first non-masked entry there; the
    owners of a position paint their depth-first ranges in depth-first order, so that a leaf reads its nearest one."""

    def __init__(self, arrays):
        F = RR.Fast(arrays)
        self.n, self.par, self.pre, self.size = F.n, F.par, F.pre, F.size
        self.lbfs, self.lpre = F.lbfs, F.lpre                   # leaves in depth-first order (BFS indices); leaves before a position
        self.n_leaves = len(self.lbfs)
        off = np.asarray(arrays["mut_off"]).astype(np.int64)
        pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
        nuc = np.asarray(arrays["mut_nuc"]).astype(np.uint8)
        node = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(off))
        idx = np.flatnonzero(pos >= 0)
        _, first = np.unique(node[idx] << 32 | pos[idx], return_index=True)   # the first stored entry of every (node, position)
        own = idx[first]
        order = np.lexsort((self.pre[node[own]], pos[own]))
        own = own[order]
        self.opos, self.onuc, self.onode = pos[own], nuc[own], node[own]
        self.tp = int(pos.max()) + 1 if len(pos) and pos.max() >= 0 else 0
        self._paint = {}

    def owners(self, p):
        lo, hi = np.searchsorted(self.opos, [p, p + 1])
        return int(lo), int(hi)

    def alleles(self, p):
        """Per leaf rank the allele of the nearest owner of p on its root path, 0 where there is none."""
        if p not in self._paint:
            paint = np.zeros(self.n, np.uint16)
            lo, hi = self.owners(p)
            for k in range(lo, hi):
                v = self.onode[k]
                paint[self.pre[v]:self.pre[v] + self.size[v]] = 256 + int(self.onuc[k])
            self._paint = {p: paint[self.pre[self.lbfs]]}
        return self._paint[p]

    def mutations(self, pos, nuc):
        mask = np.zeros(self.n_leaves, bool)
        counts = np.zeros(len(pos), np.uint64)
        for q, (p, a) in enumerate(zip(pos, nuc)):
            p = int(p)
            if 0 <= p < self.tp:
                one = self.alleles(p) == 256 + (int(a) & 0xFF)
                counts[q] = one.sum()
                mask |= one
        return mask, counts

    def ranks(self, v):
        a = int(self.pre[v])
        return int(self.lpre[a]), int(self.lpre[a + int(self.size[v])])

    def subtrees(self, nodes):
        mask = np.zeros(self.n_leaves, bool)
        counts = np.zeros(len(nodes), np.uint64)
        for i, v in enumerate(nodes):
            lo, hi = self.ranks(int(v))
            counts[i] = hi - lo
            mask[lo:hi] = True
        return mask, counts

    def mrca(self, mask):
        r = np.flatnonzero(mask)
        v, last = int(self.lbfs[r[0]]), int(self.pre[self.lbfs[r[-1]]])
        while self.pre[v] + self.size[v] <= last:
            v = self.par[v]
        lo, hi = self.ranks(v)
        return v, hi - lo


# ---- the literal answers in the shape of the device calls ------------------------------------------------------------------------

def leaves_by_rank(T):
    """The leaves in depth-first order: leaf rank r is the r-th of them."""
    return [n.identifier for n in T.depth_first_expansion() if n.is_leaf()]


def mask_of(T, good):
    rank = {s: r for r, s in enumerate(leaves_by_rank(T))}
    mask = np.zeros(len(rank), bool)
    for s in good:
        mask[rank[s]] = True
    return mask


def literal_mutations(T, pos, nuc):
    """(mask, counts) of Placer.select_mutations from get_mutation_samples, query by query."""
    mask = np.zeros(len(leaves_by_rank(T)), bool)
    counts = np.zeros(len(pos), np.uint64)
    for q, (p, a) in enumerate(zip(np.asarray(pos).tolist(), np.asarray(nuc).tolist())):
        good = mutation_samples(T, p, a)
        counts[q] = len(good)
        mask |= mask_of(T, good)
    return mask, counts


def literal_subtrees(T, names, nodes):
    mask = np.zeros(len(leaves_by_rank(T)), bool)
    counts = np.zeros(len(nodes), np.uint64)
    for i, v in enumerate(nodes):
        ids = get_leaves_ids(T, names[int(v)])
        counts[i] = len(ids)
        mask |= mask_of(T, ids)
    return mask, counts
