"""matUtils mask restated for the tests (the reference cannot be built here).

LITERAL functions follow matUtils/mask.cpp statement by statement on the host tree of oracle/refio.py: restrictSamples (:802-905:
the restricted roots with `visited`, the counting map keyed by get_string(), the in-place masking), restrictMutationsLocally with
mask_mutation_on_branch and match_mutations (:703-800), renameSamples (:679-701) and mask_main's order of steps (:68-159), with
`matutils-amd mask`'s stated conventions: "Masking mutation" lines in depth-first order, messages instead of the reference's assert
and null pointer for an empty samples file, an empty line and a mutation that does not parse.

Fast gives the device calls' answers from the closed forms with numpy, for trees too big for the literal functions;
tests/test_mask_cpu.py holds it against the literal ones on every small tree.
"""
import re
import sys

import numpy as np

from oracle import refio
from tests import relatives_ref as RR
from tests import select_ref as SR
from tests import usher_model as UM

NIL = 0xFFFFFFFF


def tree_from_arrays(arrays):
    """SR.tree_from_arrays with every entry tagged by its index in the mutation CSR (Mutation.eid)."""
    T = SR.tree_from_arrays(arrays)
    off = np.asarray(arrays["mut_off"]).astype(np.int64)
    for j, nd in enumerate(T.breadth_first_expansion()):
        for k, m in enumerate(nd.mutations):
            m.eid = int(off[j]) + k
    return T


def names_of(arrays):
    return list(arrays.get("names") or ["n%d" % j for j in range(int(arrays["n"]))])


# ---- literal ------------------------------------------------------------------------------------------------------------------

def get_leaves_ids(T, nid):
    return [n.identifier for n in UM.get_leaves(T, T.get_node(nid))]


def restricted_roots(T, samples):
    """:820-852.  The roots in the order they were found."""
    restricted = set(samples)
    roots, visited = [], {s: False for s in restricted}
    for cn in T.breadth_first_expansion():
        s = cn.identifier
        if s not in restricted:
            continue
        if visited[s]:
            continue
        curr = T.get_node(s)
        for n in UM._rsearch(cn, False):
            found_unrestricted = False
            for l in get_leaves_ids(T, n.identifier):
                if l not in restricted:
                    found_unrestricted = True
                    break
            if not found_unrestricted:
                for l in get_leaves_ids(T, n.identifier):
                    visited[l] = True
                curr = n
                break
        if curr not in roots:
            roots.append(curr)
    return roots


def restrict_samples(T, samples, log=None):
    """:819-904 on T in place.  Returns (roots, masked): the root nodes in depth-first order and the masked entries as (node,
    index in the node's list) in depth-first order."""
    assert len(samples) > 0
    pre = {id(n): i for i, n in enumerate(T.depth_first_expansion())}
    roots = sorted(restricted_roots(T, samples), key=lambda n: pre[id(n)])
    if log is not None:
        log.append("Restricted roots size: %d" % len(roots))
    counts = {}
    for n in T.depth_first_expansion():
        for mut in n.mutations:
            if mut.is_masked():
                continue
            s = mut.get_string()
            if s not in counts:
                counts[s] = 1
            else:
                counts[s] += 1
    for r in roots:
        for n in T.depth_first_expansion(r):
            for mut in n.mutations:
                if mut.is_masked():
                    continue
                counts[mut.get_string()] -= 1
    masked = []
    for r in roots:
        for n in T.depth_first_expansion(r):
            for k, mut in enumerate(n.mutations):
                if mut.is_masked():
                    continue
                s = mut.get_string()
                if counts[s] == 0:
                    if log is not None:
                        log.append("Masking mutation %s at node %s" % (s, n.identifier))
                    mut.position = -1
                    mut.ref_nuc = mut.par_nuc = mut.mut_nuc = 0
                    masked.append((n, k))
    return roots, masked


def match_mutations(target, query):
    if target.position != query.position:
        return False
    if target.ref_nuc != 0b1111:
        if target.par_nuc != query.par_nuc:
            return False
    if target.mut_nuc != 0b1111:
        if target.mut_nuc != query.mut_nuc:
            return False
    return True


def mask_mutation_on_branch(node, mutobj, exclude_nodes, removed=None, log=None):
    instances_masked = 0
    muts_to_remove = [mut for mut in node.mutations if match_mutations(mutobj, mut)]
    instances_masked += len(muts_to_remove)
    for mut in muts_to_remove:   # std::find by operator== (position, is_missing, chrom, par_nuc, mut_nuc), then erase
        it = next(i for i, m in enumerate(node.mutations) if (m.position, m.is_missing, m.chrom, m.par_nuc, m.mut_nuc) ==
                  (mut.position, mut.is_missing, mut.chrom, mut.par_nuc, mut.mut_nuc))
        if removed is not None:
            removed.append(node.mutations[it])
        del node.mutations[it]
    for child in node.children:
        if child.identifier not in exclude_nodes:
            instances_masked += mask_mutation_on_branch(child, mutobj, exclude_nodes, removed, log)
        elif log is not None:
            log.append("Excluding %s for position %d" % (child.identifier, mutobj.position))
    return instances_masked


FROM_STRING = "mutation_from_string: expected /[A-Z][0-9]+[A-Z/, got '%s'"
FROM_STRING_TAIL = "mutation_from_string: unexpected characters at the end of '%s'"


def mutation_from_string(s):
    """The Mutation (ref_nuc = par_nuc = the first letter) as mutation_annotated_tree.cpp:358-380 reads it, or the message."""
    m = re.match(r"(.)\s*([+-]?\d+)(.)", s, re.S)   # sscanf("%c%d%c")
    if not m or not ("A" <= m.group(1) <= "Z") or not ("A" <= m.group(3) <= "Z"):
        return FROM_STRING % s
    ref, alt = refio.get_nuc_id(m.group(1)), refio.get_nuc_id(m.group(3))
    mut = refio.Mutation(int(m.group(2)), ref, ref, alt)
    if mut.get_string() != s:
        return FROM_STRING_TAIL % s
    return mut


class Exit(Exception):
    """exit(1) with the message that precedes it."""


def split(s, delim):
    return refio._string_split(s, delim)


def restrict_mutations(T, text, csv=False, log=None):
    """:752-799 on T in place, for the file's text.  Returns the per-line instances_masked."""
    sys.setrecursionlimit(100000)
    delim = "," if csv else "\t"
    rootid = T.root.identifier
    per_line = []
    for line in text.split("\n")[:-1] if text.endswith("\n") else text.split("\n"):
        if line.endswith("\r"):
            line = line[:-1]
        words = split(line, delim)
        if not words:
            raise Exit("ERROR: Empty line in the mutations file")
        exclude = set()
        target_mutation, target_node = words[0], rootid
        if len(words) > 1:
            target_node = words[1]
            if len(words) > 2:
                exclude = set(split(words[2], ";"))
        mutobj = mutation_from_string(target_mutation)
        if isinstance(mutobj, str):
            raise Exit(mutobj)
        rn = T.get_node(target_node)
        if rn is None:
            raise Exit("ERROR: Internal node %s requested for masking does not exist in the tree. Exiting" % target_node)
        per_line.append(mask_mutation_on_branch(rn, mutobj, exclude, None, log))
    if log is not None:
        log.append("Masked a total of %d mutations. Collapsing tree..." % sum(per_line))
    UM.collapse_tree(T)
    return per_line


def rename_samples(T, text, log=None):
    for line in text.split("\n")[:-1] if text.endswith("\n") else text.split("\n"):
        words = split(line, "\t")
        if len(words) != 2:
            raise Exit("ERROR: Incorrect format for the renaming file")
        n = T.get_node(words[0])
        if n is None:
            if log is not None:
                log.append("WARNING: Node %s not found in the MAT." % words[0])
            continue
        if words[1] in T.all_nodes:
            raise Exit("ERROR: rename_node: node with id '%s' already exists." % words[1])
        del T.all_nodes[words[0]]
        n.identifier = words[1]
        T.all_nodes[words[1]] = n


def mask_main(T, samples=None, mutations=None, csv=False, rename=None, condense=False):
    """mask_main's steps on T in place; the file arguments are their texts.  Returns the log lines that are part of the contract."""
    log = []
    if T.condensed_nodes:
        UM.uncondense_leaves(T)
    if samples is not None:
        names = samples.split("\n")[:-1] if samples.endswith("\n") else samples.split("\n")
        if samples == "":
            names = []
        for s in names:
            if T.get_node(s) is None:
                raise Exit("ERROR: Sample missing in input MAT!")
        if not names:
            raise Exit("ERROR: the restricted samples file")
        restrict_samples(T, names, log)
    if mutations is not None:
        restrict_mutations(T, mutations, csv, log)
    if rename is not None:
        rename_samples(T, rename, log)
    if condense:
        UM.collapse_tree(T)
        UM.condense_leaves(T)
    return log


# ---- the literal answers in the shape of the device calls ------------------------------------------------------------------------

def literal_restricted(arrays, leaves):
    """(roots, entry_masked) of Placer.mask_restricted for named nodes given by BFS index (any node)."""
    T, names = tree_from_arrays(arrays), names_of(arrays)
    index = {s: j for j, s in enumerate(names)}
    eid = {(id(n), k): m.eid for n in T.breadth_first_expansion() for k, m in enumerate(n.mutations)}
    roots, masked = restrict_samples(T, [names[int(v)] for v in leaves])
    out = np.zeros(len(arrays["mut_pos"]), bool)
    for n, k in masked:
        out[eid[(id(n), k)]] = True
    return np.asarray([index[r.identifier] for r in roots], np.uint32), out


def literal_mutations(arrays, lines, skip=None):
    """(first_line, counts) of Placer.mask_mutations: lines are (pos, par, nuc, node, excl) with BFS indices; an excluded index
    out of range stands for a name that is not in the tree.  skip: entries that -s masked before."""
    sys.setrecursionlimit(100000)
    T, names = tree_from_arrays(arrays), names_of(arrays)
    if skip is not None:
        for n in T.breadth_first_expansion():
            for m in n.mutations:
                if skip[m.eid]:
                    m.position, m.ref_nuc, m.par_nuc, m.mut_nuc = -1, 0, 0, 0
    first = np.full(len(arrays["mut_pos"]), NIL, np.uint32)
    counts = np.zeros(len(lines), np.uint64)
    for l, (pos, par, nuc, node, excl) in enumerate(lines):
        if int(pos) < 0:   # no line of a file parses to a negative position (mutation_from_string): the calls match nothing
            continue
        target = refio.Mutation(int(pos), int(par), int(par), int(nuc))
        exclude = set(names[int(x)] if int(x) < len(names) else "no such node %d" % int(x) for x in excl)
        removed = []
        counts[l] = mask_mutation_on_branch(T.get_node(names[int(node)]), target, exclude, removed)
        assert counts[l] == len(removed)
        for m in removed:
            first[m.eid] = l
    return first, counts


# ---- the closed forms ---------------------------------------------------------------------------------------------------------

class Fast:
    def __init__(self, arrays):
        F = RR.Fast(arrays)
        self.n, self.par, self.pre, self.size = F.n, np.asarray(F.par).astype(np.int64), np.asarray(F.pre).astype(np.int64), np.asarray(F.size).astype(np.int64)
        self.lpre = np.asarray(F.lpre).astype(np.int64)
        self.n_leaves = len(F.lbfs)
        off = np.asarray(arrays["mut_off"]).astype(np.int64)
        self.pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
        self.mpar = np.asarray(arrays["mut_par"]).astype(np.int64) & 0xFF
        self.mnuc = np.asarray(arrays["mut_nuc"]).astype(np.int64) & 0xFF
        self.node = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(off))
        self.leaf = self.size == 1
        self.hasleaf = np.zeros(self.n, bool)
        kids = np.flatnonzero(self.leaf & (self.par >= 0))
        self.hasleaf[self.par[kids]] = True
        # get_string() prints the codes 0 and 15 alike
        self.key = self.pos * 256 + np.where(self.mpar == 0, 15, self.mpar) * 16 + np.where(self.mnuc == 0, 15, self.mnuc)

    def _in_ranges(self, nodes):
        """Per node (BFS index) the number of the given nodes on its root path, itself included."""
        d = np.zeros(self.n + 1, np.int64)
        np.add.at(d, self.pre[nodes], 1)
        np.add.at(d, self.pre[nodes] + self.size[nodes], -1)
        return np.cumsum(d)[self.pre]

    def restricted(self, leaves):
        """(roots in depth-first order, entry_masked) for named LEAVES."""
        leaves = np.unique(np.asarray(leaves, np.int64))
        assert len(leaves) and self.leaf[leaves].all()
        named = np.zeros(self.n_leaves, np.int64)
        named[self.lpre[self.pre[leaves]]] = 1
        cs = np.concatenate([[0], np.cumsum(named)])
        lo, hi = self.lpre[self.pre], self.lpre[self.pre + self.size]
        full = cs[hi] - cs[lo] == hi - lo
        F = np.flatnonzero(~self.leaf & full & self.hasleaf)
        top = F[self._in_ranges(F)[F] == 1]                       # no proper ancestor in F
        parent_full = np.where(self.par >= 0, full[np.maximum(self.par, 0)], False)
        own = np.flatnonzero(self.leaf & full & ~parent_full)     # named leaves whose parent is not full
        roots = np.concatenate([top, own])
        roots = roots[np.argsort(self.pre[roots])]
        cover = self._in_ranges(roots) > 0
        live = self.pos >= 0
        below = cover[self.node]
        outside = np.unique(self.key[live & ~below])
        masked = live & below & ~np.isin(self.key, outside)
        return roots.astype(np.uint32), masked

    def mutations(self, lines, skip=None):
        first = np.full(len(self.pos), NIL, np.uint32)
        counts = np.zeros(len(lines), np.uint64)
        alive = self.pos >= 0
        if skip is not None:
            alive &= ~np.asarray(skip, bool)
        epre = self.pre[self.node]
        for l, (pos, par, nuc, node, excl) in enumerate(lines):
            e = np.flatnonzero((self.pos == int(pos)) & alive)
            e = e[first[e] == NIL]
            if int(par) != 15:
                e = e[self.mpar[e] == int(par)]
            if int(nuc) != 15:
                e = e[self.mnuc[e] == int(nuc)]
            t = int(node)
            tlo, thi = self.pre[t], self.pre[t] + self.size[t]
            e = e[(epre[e] >= tlo) & (epre[e] < thi)]
            for x in excl:
                x = int(x)
                if x < self.n and tlo < self.pre[x] < thi:        # a strict descendant of the target
                    e = e[(epre[e] < self.pre[x]) | (epre[e] >= self.pre[x] + self.size[x])]
            first[e] = l
            counts[l] = len(e)
        return first, counts
