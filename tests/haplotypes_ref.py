"""matUtils summary --haplotype restated for the tests (the reference cannot be built here).

LITERAL functions follow count_haplotypes and write_haplotype_table (matUtils/summary.cpp:182-264) statement by statement on the
breadth-first arrays of tests/synth.py: a dict copied from the parent into every node, one kept per internal node for the whole
walk, the leaves counted in a dict keyed by whole sets; the std::map<std::map<int,int8_t>,size_t> order is the order of the sorted
tuples of (position, allele) pairs.  `group_records` / `leaf_sets` / `duplicates` give the same answers in the shape of the C ABI
(include/usher_amd.h), for the device calls.

class Fast gives the ABI-shaped answers with numpy for trees too big for the literal walk (no per-node dicts); the CPU tests hold
it against the literal functions on every small tree.  It is exact: leaves are grouped by a hash of their sets and every leaf is
then compared, pair by pair, with the first leaf of its group.
"""
import numpy as np

from tests import summary_ref as SR

NONE = 0xFFFFFFFF
HEADER = "mutation_set\tsample_count\n"


def entry(arrays, k):
    """(position, ref_nuc, mut_nuc) of entry k as the loader leaves it (mutation_annotated_tree.cpp:566-594): a masked entry has
    ref = par = mut = 0."""
    p = int(arrays["mut_pos"][k])
    if p < 0:
        return p, 0, 0
    return p, _int8(arrays["mut_ref"][k]), _int8(arrays["mut_nuc"][k])


def _int8(v):
    v = int(v) & 0xff
    return v - 256 if v > 127 else v


# ---- literal ---------------------------------------------------------------------------------------------------------------

def node_sets(T):
    """The walk of count_haplotypes: (hapcount, per-leaf set).  hapcount maps the sorted tuple of (position, allele) pairs to its
    number of leaves; the second dict maps every leaf to its tuple."""
    hapcount, hapmap, of_leaf = {}, {}, {}
    a = T.arrays
    for s in T.dfs():
        mset = {}
        if s != 0:
            mset = dict(hapmap[T.par[s]])          # mset = hapmap[s->parent->identifier]: a copy
        for k in T.muts(s):
            pos, ref, nuc = entry(a, k)
            if nuc == ref:
                if pos in mset:
                    del mset[pos]
            else:
                mset[pos] = nuc
        if T.is_leaf(s):
            key = tuple(sorted(mset.items()))
            if key not in hapcount:
                hapcount[key] = 0
            hapcount[key] += 1
            of_leaf[s] = key
        else:
            hapmap[s] = mset
    return hapcount, of_leaf


def set_string(key):
    """One mutation_set cell.  (The reference calls pop_back() on the empty string before it writes "reference".)"""
    return ",".join("%d%s" % (p, SR.nuc(c)) for p, c in key) if key else "reference"


def render(T):
    """The text write_haplotype_table writes."""
    hapcount, _ = node_sets(T)
    return HEADER + "".join("%s\t%d\n" % (set_string(key), cnt) for key, cnt in sorted(hapcount.items()))


def group_records(T):
    """[(leaf, count, size)] per distinct set: its first leaf in depth-first order (BFS index), ascending by that leaf's
    depth-first position."""
    hapcount, of_leaf = node_sets(T)
    first = {}
    for s in T.dfs():
        if T.is_leaf(s):
            first.setdefault(of_leaf[s], s)
    return [(s, hapcount[key], len(key)) for key, s in first.items()]


def leaf_sets(T, leaves):
    """Per given leaf its sorted [(position, allele code as an unsigned byte)]."""
    _, of_leaf = node_sets(T)
    return [[(p, c & 0xff) for p, c in of_leaf[int(l)]] for l in leaves]


def duplicates(T):
    """(nodes with two non-masked entries at one position, the first of them in depth-first order or NONE)."""
    n, first = 0, NONE
    for s in T.dfs():
        ps = [int(T.arrays["mut_pos"][k]) for k in T.muts(s) if T.arrays["mut_pos"][k] >= 0]
        if len(ps) != len(set(ps)):
            n += 1
            if first == NONE:
                first = s
    return n, first


# ---- fast ------------------------------------------------------------------------------------------------------------------

def _mix(x):
    """A 64-bit mix of its own (not the library's), wrapping."""
    x = (x ^ (x >> np.uint64(33))) * np.uint64(0xff51afd7ed558ccd)
    x = (x ^ (x >> np.uint64(29))) * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(32))


class Fast:
    """The sets of all leaves as one CSR by leaf rank (the r-th leaf in depth-first order), from the closed form: an entry at
    position p on node v is in force for the leaves below v that are below no deeper entry at p.  Every non-masked entry adds its
    pair to the leaves below its node and takes it away from the leaves below each entry at p directly under it."""

    def __init__(self, arrays):
        S = self.S = SR.Fast(arrays)
        n = S.n
        pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
        ref = np.asarray(arrays["mut_ref"]).astype(np.int64) & 0xff
        nuc = np.asarray(arrays["mut_nuc"]).astype(np.int64) & 0xff
        node = S.node
        k = (node[pos >= 0] << 32) | pos[pos >= 0]
        u, c = np.unique(k, return_counts=True)
        dup_nodes = np.unique(u[c > 1] >> 32)
        self.n_duplicate = len(dup_nodes)
        self.first_duplicate = int(dup_nodes[np.argmin(S.pre[dup_nodes])]) if len(dup_nodes) else NONE
        # leaves by depth-first position; the leaf ranks below every node
        self.leaf_bfs = np.flatnonzero(S.leaf)[np.argsort(S.pre[S.leaf])]
        is_leaf_at = np.zeros(n + 1, np.int64)
        is_leaf_at[S.pre[S.leaf]] = 1
        lbefore = np.r_[0, np.cumsum(is_leaf_at)]            # leaves in front of depth-first position i
        self.rank_of = np.full(n, -1, np.int64)
        self.rank_of[self.leaf_bfs] = np.arange(len(self.leaf_bfs))
        L = self.n_leaves = len(self.leaf_bfs)
        if self.n_duplicate:
            return
        live = np.flatnonzero(pos >= 0)
        # the entries of a position in depth-first order of their node; the entry above each: the nearest one in front of it
        # (same position) whose node's range holds its node, by pointer jumping
        order = live[np.lexsort((S.pre[node[live]], pos[live]))]
        p, a, b = pos[order], S.pre[node[order]], S.pre[node[order]] + S.size[node[order]]
        m = len(order)
        up = np.arange(m) - 1
        up[np.r_[True, p[1:] != p[:-1]][:m]] = -1
        while True:
            bad = np.flatnonzero((up >= 0) & (b[np.maximum(up, 0)] <= a))
            if not len(bad):
                break
            up[bad] = up[up[bad]]
        la, lb = lbefore[a], lbefore[b]
        off_ref = nuc[order] != ref[order]
        key = (p << 8) | nuc[order]
        # +1 for its own pair over its range; -1 for the pair of the entry above over its range
        plus = np.flatnonzero(off_ref)
        minus = np.flatnonzero((up >= 0) & off_ref[np.maximum(up, 0)])
        lo = np.r_[la[plus], la[minus]]
        hi = np.r_[lb[plus], lb[minus]]
        kk = np.r_[key[plus], key[up[minus]]]
        w = np.r_[np.ones(len(plus), np.int64), -np.ones(len(minus), np.int64)]
        ln = hi - lo
        tot = int(ln.sum())
        start = np.cumsum(ln) - ln
        leaf = np.repeat(lo - start, ln) + np.arange(tot)
        # the lowest bit says "take away", so that one plain sort brings the +1 and -1 of a (leaf, pair) together
        full = np.sort((((leaf << 40) | np.repeat(kk, ln)) << 1) | np.repeat((w < 0).astype(np.int64), ln))
        sign, full = 1 - 2 * (full & 1), full >> 1
        head = np.flatnonzero(np.r_[True, full[1:] != full[:-1]]) if tot else np.zeros(0, np.int64)
        s = np.add.reduceat(sign, head) if tot else np.zeros(0, np.int64)
        assert ((s == 0) | (s == 1)).all()
        keep = full[head[s == 1]]
        self.set_leaf = keep >> 40
        self.set_pos = (keep >> 8) & 0xffffffff
        self.set_nuc = keep & 0xff
        self.off = np.r_[0, np.cumsum(np.bincount(self.set_leaf, minlength=L))]
        # groups: a hash per leaf, then every leaf against the first of its hash, pair by pair
        pair = (keep & ((1 << 40) - 1)).astype(np.uint64)
        h1, h2 = _mix(pair + np.uint64(0x51ed270b27b4f3cf)), _mix(pair * np.uint64(0xd1342543de82ef95) + np.uint64(0x2545f4914f6cdd1d))
        a1, a2 = np.zeros(L, np.uint64), np.zeros(L, np.uint64)
        full_leaves = np.flatnonzero(np.diff(self.off) > 0)     # (reduceat does not take empty slices)
        if len(keep):
            a1[full_leaves] = np.add.reduceat(h1, self.off[full_leaves])
            a2[full_leaves] = np.add.reduceat(h2, self.off[full_leaves])
        o = np.lexsort((np.arange(L), a2, a1))
        new = np.r_[True, (a1[o][1:] != a1[o][:-1]) | (a2[o][1:] != a2[o][:-1])]
        gid = np.cumsum(new) - 1
        first, cnt = o[new], np.bincount(gid)                # the first of a run has the smallest rank
        ginv = np.empty(L, np.int64)
        ginv[o] = gid
        rep = first[ginv]                                    # np.unique: the first occurrence, so the smallest rank
        size = np.diff(self.off)
        assert (size == size[rep]).all()
        at = np.arange(len(keep)) - self.off[self.set_leaf] + self.off[rep[self.set_leaf]]
        assert ((keep & ((1 << 40) - 1)) == (keep[at] & ((1 << 40) - 1))).all(), "a hash collision in the test's own closed form"
        g = np.argsort(first)
        self.group_rank, self.group_count, self.group_size = first[g], cnt[g], size[first[g]]
        self.group_of_rank = np.argsort(g)[ginv]

    def group_records(self):
        return list(zip(self.leaf_bfs[self.group_rank].tolist(), self.group_count.tolist(), self.group_size.tolist()))

    def leaf_sets(self, leaves):
        out = []
        for l in leaves:
            r = int(self.rank_of[int(l)])
            assert r >= 0
            sl = slice(int(self.off[r]), int(self.off[r + 1]))
            out.append(list(zip(self.set_pos[sl].tolist(), self.set_nuc[sl].tolist())))
        return out

    def sets_csr(self, leaves):
        """(off, pos, nuc) as ugp_haplotype_sets returns them."""
        r = self.rank_of[np.asarray(leaves, np.int64)]
        ln = self.off[r + 1] - self.off[r]
        off = np.r_[0, np.cumsum(ln)].astype(np.uint64)
        tot = int(ln.sum())
        idx = np.repeat(self.off[r] - (np.cumsum(ln) - ln), ln) + np.arange(tot)
        return off, self.set_pos[idx].astype(np.int32), self.set_nuc[idx].astype(np.uint8)
