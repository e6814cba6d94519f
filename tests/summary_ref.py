"""matUtils summary restated for the tests (the reference cannot be built here).

LITERAL functions follow matUtils/summary.cpp statement by statement on the breadth-first arrays of tests/synth.py plus node names
and annotations: write_mutation_table (:139-174), write_roho_table without dates (:343-506, with its nested subtree expansions and
string-keyed maps), write_clade_table (:88-137), write_sample_clades_table (:297-341), write_sample_table (:70-86),
write_aberrant_table (:266-295), print_mut_stats (:224-242) and the basic counts (:746-end).  They return the text the reference
writes.  `*_records` give the same answers in the shape of the C ABI (include/usher_amd.h), for the device calls.

FAST functions (class Fast) give the ABI-shaped answers with numpy for trees too big for the literal ones; the CPU tests hold them
against the literal ones on every small tree.
"""
import math

import numpy as np

NUC = "NACMGRSVTWYHKDBN"   # get_nuc (mutation_annotated_tree.cpp:88-140): 0 and anything else read 'N'
NONE = 0xFFFFFFFF


def nuc(c):
    c = int(c)
    return NUC[c] if 1 <= c <= 15 else "N"


def mut_string(arrays, k):
    """Mutation::get_string (mutation_annotated_tree.hpp:79-85)."""
    p = int(arrays["mut_pos"][k])
    if p < 0:
        return "MASKED"
    return nuc(arrays["mut_par"][k]) + str(p) + nuc(arrays["mut_nuc"][k])


def names_of(arrays):
    return list(arrays.get("names") or ["n%d" % j for j in range(arrays["n"])])


class Tree:
    """The host tree as the reference holds it: children in stored order, the depth-first expansion, names."""

    def __init__(self, arrays, ann=None):
        self.arrays = arrays
        self.n = n = int(arrays["n"])
        self.par = [int(p) for p in arrays["parent"]]
        self.kids = [[] for _ in range(n)]
        for j in range(1, n):
            self.kids[self.par[j]].append(j)
        self.names = names_of(arrays)
        self.off = [int(o) for o in arrays["mut_off"]]
        self.ann = ann if ann is not None else [[] for _ in range(n)]
        self.mstr = [mut_string(arrays, k) for k in range(self.off[n])]

    def is_leaf(self, v):
        return not self.kids[v]

    def dfs(self, v=0):
        """Tree::depth_first_expansion (mutation_annotated_tree.cpp:1253-1273)."""
        out, stack = [], [v]
        while stack:
            x = stack.pop()
            out.append(x)
            stack.extend(reversed(self.kids[x]))
        return out

    def leaves(self):
        """Tree::get_leaves: the leaves of the breadth-first expansion."""
        return [j for j in range(self.n) if not self.kids[j]]

    def rsearch(self, v, include_self):
        out = [v] if include_self else []
        while v != 0:
            v = self.par[v]
            out.append(v)
        return out

    def muts(self, v):
        return range(self.off[v], self.off[v + 1])


# ---- literal: text ---------------------------------------------------------------------------------------------------------

def f32(x):
    return float(np.float32(x))


def fmt_float(x):
    """A float through an ostream at default precision (%g with 6 digits)."""
    x = f32(x)
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return "%g" % x


def literal_mutations(T):
    counts = {}
    for s in T.dfs():
        for k in T.muts(s):
            m = T.mstr[k]
            if m != "MASKED":
                counts[m] = counts.get(m, 0) + 1
    return counts


def render_mutations(T):
    c = literal_mutations(T)
    return "ID\toccurrence\n" + "".join("%s\t%d\n" % (m, c[m]) for m in sorted(c, key=lambda s: s.encode()))


def literal_roho(T):
    """write_roho_table, get_dates = false: rows (mutation, parent, child_count, child, sum_wit, med_non as the integer held) in the
    order written."""
    rows = []
    name = T.names
    for n in T.dfs():
        candidate = {}          # mutation string -> child identifier
        child_increment = {}    # child identifier -> leaves below it
        ccheck = []
        for c in T.kids[n]:
            if not T.is_leaf(c):
                ccheck.append(name[c])
                for k in T.muts(c):
                    candidate[T.mstr[k]] = name[c]
        if not candidate:
            continue
        for c in T.kids[n]:
            ccount = 0
            if T.is_leaf(c):
                continue
            for dn in T.dfs(c):
                if name[dn] == name[c]:
                    continue
                if T.is_leaf(dn):
                    ccount += 1
                for k in T.muts(dn):
                    candidate.pop(T.mstr[k], None)
            if ccount > 1:
                child_increment[name[c]] = ccount
        if not candidate or len(child_increment) <= 1:
            continue
        for ms in sorted(candidate, key=lambda s: s.encode()):
            owner = candidate[ms]
            all_non, sum_wit = [], 0
            for cs in sorted(child_increment, key=lambda s: s.encode()):
                if cs != owner:
                    if child_increment[cs] > 5:
                        all_non.append(child_increment[cs])
                elif child_increment[cs] > 5:
                    sum_wit += child_increment[cs]
            if not all_non or sum_wit == 0:
                continue
            all_non.sort()
            h = len(all_non) // 2
            med = (all_non[h - 1] + all_non[h]) // 2 if len(all_non) % 2 == 0 else all_non[h]
            rows.append((ms, name[n], len(ccheck), owner, sum_wit, med))
    return rows


ROHO_HEADER = "mutation\tparent_node\tchild_count\toccurrence_node\toffspring_with\tmedian_offspring_without\tsingle_roho\n"


def single_roho(sum_wit, med):
    """std::log10(sum_wit / med_non) with med_non a float: the division and the logarithm are float's."""
    q = np.float32(sum_wit) / np.float32(med)
    return float(np.log10(q, dtype=np.float32))


def render_roho(T):
    out = [ROHO_HEADER]
    for ms, parent, cc, child, w, med in literal_roho(T):
        out.append("%s\t%s\t%d\t%s\t%d\t%s\t%s\t\n" % (ms, parent, cc, child, w, fmt_float(med), fmt_float(single_roho(w, med))))
    return "".join(out)


def render_clades(T):
    incl, excl = {}, {}
    for s in T.leaves():
        first = [True, True]
        for a in T.rsearch(s, False):
            canns = T.ann[a]
            for i in range(min(2, len(canns))):
                if canns[i] != "":
                    incl.setdefault(canns[i], 0)
                    excl.setdefault(canns[i], 0)
                    incl[canns[i]] += 1
                    if first[i]:
                        excl[canns[i]] += 1
                        first[i] = False
    return "clade\tinclusive_count\texclusive_count\n" + "".join("%s\t%d\t%d\n" % (c, incl[c], excl[c])
                                                                  for c in sorted(incl, key=lambda s: s.encode()))


def num_annotations(T):
    """Tree::get_num_annotations: the root's."""
    return len(T.ann[0])


def render_sample_clades(T):
    na = num_annotations(T)
    out = ["sample" + "".join("\tannotation_%d" % i for i in range(1, na + 1)) + "\n"]
    for n in T.leaves():
        found = ["None"] * na
        for a in T.rsearch(n, False):
            canns = T.ann[a]
            for i in range(min(na, len(canns))):
                if canns[i] != "" and found[i] == "None":
                    found[i] = canns[i]
            if all(f != "None" for f in found):
                break
        out.append(T.names[n] + "".join("\t" + f for f in found) + "\n")
    return "".join(out)


def render_samples(T):
    out = ["sample\tparsimony\tparent_id\n"]
    for s in T.dfs():
        if T.is_leaf(s):
            out.append("%s\t%d\t%s\n" % (T.names[s], T.off[s + 1] - T.off[s], T.names[T.par[s]] if s else ""))
    return "".join(out)


def render_aberrant(T):
    out = ["NodeID\tIssue\n"]
    na = num_annotations(T)
    seen = set()
    for n in T.dfs():
        if T.names[n] in seen:
            out.append("%s\tduplicate-node-id\n" % T.names[n])
        seen.add(T.names[n])
        if T.off[n + 1] == T.off[n] and not T.is_leaf(n) and n != 0:
            out.append("%s\tinternal-no-mutations\n" % T.names[n])
        if na != len(T.ann[n]):
            out.append("%s\tclade-annotations (%d not %d)\n" % (T.names[n], len(T.ann[n]), na))
    return "".join(out)


def render_mut_stats(T):
    """print_mut_stats: one_hot_to_two_bit = 31 - clz, the highest set bit."""
    freq = [0] * 16
    a = T.arrays
    for n in T.dfs():
        for k in T.muts(n):
            if int(a["mut_par"][k]) <= 0 or int(a["mut_nuc"][k]) <= 0:
                continue   # (a masked entry's alleles are 0: the reference takes clz(0) and indexes out of bounds; not counted here)
            fr = int(a["mut_par"][k]).bit_length() - 1
            to = int(a["mut_nuc"][k]).bit_length() - 1
            freq[4 * fr + to] += 1
    return "".join("%s->%s\t%d\n" % ("ACGT"[f], "ACGT"[t], freq[4 * f + t]) for f in range(4) for t in range(4))


def render_basic(T, condensed_nodes, condensed_leaves):
    """The basic counts (summary.cpp:746-775): level 1 is the root's."""
    level = {0: 1}
    nodes = samples = slevel = mlevel = 0
    for s in T.dfs():
        if s:
            level[s] = level[T.par[s]] + 1
        nodes += 1
        if T.is_leaf(s):
            slevel += level[s]
            mlevel = max(mlevel, level[s])
            samples += 1
    return ("Total Nodes in Tree: %d\nTotal Samples in Tree: %d\nTotal Condensed Nodes in Tree: %d\nTotal Samples in Condensed Nodes: %d\n"
            "Total Tree Parsimony: %d\nNumber of Clade Annotations: %d\nMax Tree Depth: %d\nMean Tree Depth: %f\n"
            % (nodes, samples, condensed_nodes, condensed_leaves, T.off[T.n], num_annotations(T), mlevel, f32(np.float32(slevel) / np.float32(samples))))


# ---- literal: the shape of the C ABI ---------------------------------------------------------------------------------------

def parse_mut(s):
    if s == "MASKED":
        return None
    return int(s[1:-1]), NUC.index(s[0], 1), NUC.index(s[-1], 1)


def mutation_records(T):
    """[(pos, par, nuc, count)] ascending."""
    c = literal_mutations(T)
    return sorted((parse_mut(m) + (k,)) for m, k in c.items())


def roho_records(T):
    """[(parent, mutation string, child, child_count, offspring_with, median_without)] as literal_roho orders them (names are
    unique in the test trees)."""
    idx = {s: j for j, s in enumerate(T.names)}
    assert len(idx) == T.n
    return [(idx[p], ms, idx[c], cc, w, med) for ms, p, cc, c, w, med in literal_roho(T)]


def device_roho(T, recs):
    """The device's records in the literal order: parents stay as they come (depth-first), a parent's rows sort by mutation string.
    Also checks that `entry` lies on `child`."""
    pre = {v: i for i, v in enumerate(T.dfs())}
    rows = []
    for r in recs:
        e, c = int(r["entry"]), int(r["child"])
        assert T.off[c] <= e < T.off[c + 1], (e, c)
        rows.append((int(r["parent"]), T.mstr[e], c, int(r["child_count"]), int(r["offspring_with"]), int(r["median_without"])))
    order = [pre[r[0]] for r in rows]
    assert order == sorted(order), "records do not ascend by the parent's depth-first position"
    return sorted(rows, key=lambda r: (pre[r[0]], r[1].encode()))


def columns_of(T, ncols=None):
    """Per annotation column the nodes with a non-empty annotation there, in breadth-first order."""
    k = max([len(a) for a in T.ann] + [0]) if ncols is None else ncols
    return [[j for j in range(T.n) if len(T.ann[j]) > c and T.ann[j][c] != ""] for c in range(k)]


def clade_records(T, columns):
    """Per column: (incl per listed node, excl per listed node, per leaf of get_leaves the nearest listed strict ancestor or NONE),
    by walking every leaf's root path."""
    out = []
    leaves = T.leaves()
    for col in columns:
        listed = {v: i for i, v in enumerate(col)}
        incl, excl, near = [0] * len(col), [0] * len(col), []
        for s in leaves:
            first = True
            hit = NONE
            for a in T.rsearch(s, False):
                if a in listed:
                    incl[listed[a]] += 1
                    if first:
                        excl[listed[a]] += 1
                        hit = a
                        first = False
            near.append(hit)
        out.append((incl, excl, near))
    return out


# ---- fast ------------------------------------------------------------------------------------------------------------------

MASKED_KEY = 1 << 40


class Fast:
    def __init__(self, arrays):
        par = np.asarray(arrays["parent"]).astype(np.int64)
        n = self.n = len(par)
        assert n == 1 or (np.diff(par[1:]) >= 0).all(), "breadth-first arrays: parents ascend"
        self.par = par
        # the levels are contiguous ranges of the breadth-first order
        levels, lo, hi = [], 0, 1
        while lo < hi:
            levels.append((lo, hi))
            lo, hi = hi, 1 + int(np.searchsorted(par[1:], hi, "left"))
        depth = np.zeros(n, np.int64)
        for d, (a, b) in enumerate(levels):
            depth[a:b] = d
        leaf = np.ones(n, bool)
        leaf[par[1:]] = False
        size = np.ones(n, np.int64)
        below = leaf.astype(np.int64)          # leaves in the subtree, the node included
        for a, b in reversed(levels[1:]):
            np.add.at(size, par[a:b], size[a:b])
            np.add.at(below, par[a:b], below[a:b])
        pre = np.zeros(n, np.int64)
        for a, b in levels[1:]:
            cs = np.cumsum(size[a:b]) - size[a:b]
            first = np.r_[True, par[a + 1:b] != par[a:b - 1]]
            start = np.maximum.accumulate(np.where(first, np.arange(b - a), 0))
            pre[a:b] = pre[par[a:b]] + 1 + cs - cs[start]
        self.levels, self.depth, self.leaf, self.size, self.pre = levels, depth, leaf, size, pre
        self.lc = below - leaf                  # leaves strictly below
        off = np.asarray(arrays["mut_off"]).astype(np.int64)
        self.off = off
        self.node = np.repeat(np.arange(n), np.diff(off))
        pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
        self.key = np.where(pos < 0, MASKED_KEY, (pos << 8) | ((np.asarray(arrays["mut_par"]).astype(np.int64) & 15) << 4)
                            | (np.asarray(arrays["mut_nuc"]).astype(np.int64) & 15))

    def mutations(self):
        k, c = np.unique(self.key[self.key != MASKED_KEY], return_counts=True)
        return [(int(x >> 8), int((x >> 4) & 15), int(x & 15), int(y)) for x, y in zip(k, c)]

    def roho(self):
        """(records, erased): records as sorted tuples (pre[parent], key, parent, child, entry, child_count, offspring_with,
        median_without); erased = candidates (one per child and key) that an occurrence at depth >= depth(n) + 2 removed."""
        par, pre, leaf, lc, node, key = self.par, self.pre, self.leaf, self.lc, self.node, self.key
        n = self.n
        inner = ~leaf
        inner[0] = False                                       # non-leaf children
        ccount = np.bincount(par[inner], minlength=n)
        uk, kid = np.unique(key, return_inverse=True)
        # candidates: the first entry of each (child, key)
        ce = np.flatnonzero(inner[node])
        if not len(ce):
            return [], 0
        _, firsts = np.unique((node[ce] << 25) | kid[ce], return_index=True)
        assert n < (1 << 38) and len(uk) < (1 << 25)
        ce = ce[firsts]
        c, k, p = node[ce], kid[ce], par[node[ce]]
        # the later non-leaf child with the key owns it
        grp = (p << 25) | k
        o = np.lexsort((pre[c], grp))
        last = np.r_[grp[o][1:] != grp[o][:-1], True]
        own = np.zeros(len(ce), bool)
        own[o[last]] = True
        # erased: occurrences of the key inside (pre[p], pre[p] + size[p]) that are not on children of p
        occ = np.sort((kid << 32) | pre[node])
        onp = np.sort((kid[node != 0] << 32) | par[node[node != 0]])
        inside = np.searchsorted(occ, (k << 32) | (pre[p] + self.size[p])) - np.searchsorted(occ, (k << 32) | (pre[p] + 1))
        on_kids = np.searchsorted(onp, (k << 32) | p, "right") - np.searchsorted(onp, (k << 32) | p, "left")
        erased = inside > on_kids
        # the sorted counts > 5 per parent
        big = np.flatnonzero(inner & (lc > 5))
        bo = big[np.lexsort((pre[big], lc[big], par[big]))]
        bpar, blc = par[bo], lc[bo]
        rank = np.zeros(n, np.int64)
        rank[bo] = np.arange(len(bo))
        bstart = np.searchsorted(bpar, np.arange(n), "left")
        nb = np.bincount(bpar, minlength=n)
        keep = own & ~erased & (lc[c] > 5) & (nb[p] >= 2)
        ce, c, k, p = ce[keep], c[keep], k[keep], p[keep]
        others = nb[p] - 1
        mine = rank[c] - bstart[p]
        h = others // 2
        hi_v = blc[bstart[p] + h + (h >= mine)]
        lo_i = np.maximum(h - 1, 0)
        lo_v = blc[bstart[p] + lo_i + (lo_i >= mine)]
        med = np.where(others % 2 == 0, (lo_v + hi_v) // 2, hi_v)
        recs = sorted(zip(pre[p].tolist(), uk[k].tolist(), p.tolist(), c.tolist(), ce.tolist(), ccount[p].tolist(), lc[c].tolist(), med.tolist()))
        return recs, int((own & erased).sum())

    def clades(self, columns):
        """Per column (incl, excl, nearest per leaf in breadth-first order) as numpy arrays."""
        out = []
        leaves = np.flatnonzero(self.leaf)
        for col in columns:
            col = np.asarray(col, np.int64)
            listed = np.zeros(self.n, bool)
            listed[col] = True
            near = np.full(self.n, NONE, np.int64)
            for a, b in self.levels[1:]:
                q = self.par[a:b]
                near[a:b] = np.where(listed[q], q, near[q])
            nl = near[leaves]
            excl = np.bincount(nl[nl != NONE], minlength=self.n)[col]
            out.append((self.lc[col], excl, nl))
        return out


def fast_key_string(key):
    return "MASKED" if key == MASKED_KEY else nuc((key >> 4) & 15) + str(key >> 8) + nuc(key & 15)


def device_roho_fast(F, recs):
    """The device's records as Fast.roho's tuples (sorted the same way)."""
    rows = []
    for r in recs:
        e, p = int(r["entry"]), int(r["parent"])
        rows.append((int(F.pre[p]), int(F.key[e]), p, int(r["child"]), e, int(r["child_count"]), int(r["offspring_with"]),
                     int(r["median_without"])))
    return sorted(rows)


def fast_roho_rows(F, T):
    """Fast.roho in the literal shape (roho_records)."""
    recs, _ = F.roho()
    rows = [(p, fast_key_string(k), c, cc, w, med) for _, k, p, c, e, cc, w, med in recs]
    pre = F.pre
    return sorted(rows, key=lambda r: (int(pre[r[0]]), r[1].encode()))
