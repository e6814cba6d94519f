"""get_subtree (mutation_annotated_tree.cpp:1577-1685, restated in usher_amd/csrc/host/mat.cpp) over breadth-first arrays, twice.

`literal` is the function statement by statement: the ancestor set of every selected node, the first common ancestor of every
pair, the depth-first stack that finds each kept node's subtree parent, and Node::add_mutation (:720-752) entry by entry along the
collapsed path -- with mat.cpp's reading of a disagreement (add_mutation returns false, get_subtree goes on; oracle/refio raises
there, so the function is restated here).  It is quadratic in the selection.

`closed_form` is what ugp_subtree.hip computes, by other means than the kernels use: a node is kept when it is selected or at least
two of its children have a selected node at or below them (counted child by child), a node's owner is the nearest kept node
downwards, and the merged entries come from one pass over the owned nodes in depth-first order through the state machine.

Both return the dict Placer.subtree_nodes returns: kept (BFS indices, depth-first order), parent (index into kept, NIL for the root),
ent_off, pos / first_entry / nuc of the merged entries, and info (n_selected, n_gathered, n_disagree, longest_chain, first_disagree),
plus owner: per BFS index the kept index of the chain that holds the node, or NIL.
"""
import numpy as np

NIL = 0xFFFFFFFF


class Tables:
    def __init__(self, arrays):
        self.n = n = int(arrays["n"])
        self.par = [int(p) for p in arrays["parent"]]
        self.kids = [[] for _ in range(n)]
        for j in range(1, n):
            self.kids[self.par[j]].append(j)
        self.off = [int(x) for x in arrays["mut_off"]]
        self.pos = [int(x) for x in arrays["mut_pos"]]
        self.mpar = [int(x) & 0xFF for x in arrays["mut_par"]]
        self.mnuc = [int(x) & 0xFF for x in arrays["mut_nuc"]]
        self.dfs, stack = [], [0]
        while stack:   # Tree::depth_first_expansion
            v = stack.pop()
            self.dfs.append(v)
            stack.extend(reversed(self.kids[v]))

    def rsearch(self, v):
        """v .. root."""
        out = []
        while v >= 0:
            out.append(v)
            v = self.par[v] if v else -1
        return out


def add_mutation(muts, e, pos, par, nuc):
    """Node::add_mutation on a list of [position, opening entry, par, nuc] sorted by position; False: the entries disagree."""
    it = 0
    while it < len(muts) and muts[it][0] < pos:   # std::lower_bound
        it += 1
    if it < len(muts) and muts[it][0] == pos:
        cur = muts[it]
        if cur[2] != nuc:
            cur[3] = nuc
        else:
            if cur[3] != par:
                return False
            muts[:] = [m for m in muts if m[0] != pos]
    else:
        muts.insert(it, [pos, e, par, nuc])
    return True


def _result(T, sel, kept, parent, merged, owner, gathered, disagree, longest, first_bad):
    off = np.zeros(len(kept) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in merged], dtype=np.uint64)
    flat = [m for ms in merged for m in ms]
    own = np.full(T.n, NIL, np.uint32)
    for v, k in owner.items():
        own[v] = k
    return {"kept": np.asarray(kept, np.uint32), "parent": np.asarray(parent, np.uint32), "ent_off": off,
            "pos": np.asarray([m[0] for m in flat], np.int32), "first_entry": np.asarray([m[1] for m in flat], np.uint32),
            "nuc": np.asarray([m[3] for m in flat], np.uint8), "owner": own,
            "info": {"n_selected": len(set(sel)), "n_gathered": gathered, "n_disagree": disagree, "longest_chain": longest,
                     "first_disagree": first_bad}}


def literal(arrays, sel):
    T = Tables(arrays)
    sel = [int(v) for v in sel]
    keep = set(sel)
    anc = [set(T.rsearch(v)) for v in sel]
    for i in range(len(sel)):
        for j in range(i + 1, len(sel)):
            for a in T.rsearch(sel[i]):
                if a in anc[j]:
                    keep.add(a)
                    break
    kept, parent, merged, owner, last = [], [], [], {}, []
    gathered = disagree = longest = 0
    first_bad = NIL
    for v in T.dfs:
        if v not in keep:
            continue
        while last and last[-1] not in T.rsearch(v):   # is_ancestor
            last.pop()
        sp = last[-1] if last else None
        path = T.rsearch(v)[::-1]
        if sp is not None:
            path = path[path.index(sp) + 1:]
        muts = []
        for c in path:
            assert c not in owner
            owner[c] = len(kept)
            for e in range(T.off[c], T.off[c + 1]):
                gathered += 1
                if not add_mutation(muts, e, T.pos[e], T.mpar[e], T.mnuc[e]):
                    disagree += 1
                    if first_bad == NIL:
                        first_bad = v
        longest = max(longest, len(path))
        parent.append(kept.index(sp) if sp is not None else NIL)
        kept.append(v)
        merged.append(muts)
        last.append(v)
    return _result(T, sel, kept, parent, merged, owner, gathered, disagree, longest, first_bad)


def closed_form(arrays, sel):
    T = Tables(arrays)
    n = T.n
    insel = np.zeros(n, bool)
    insel[np.asarray(sel, np.int64)] = True
    cnt = insel.astype(np.int64)
    with_members = np.zeros(n, np.int64)   # children with a member at or below them
    for v in reversed(T.dfs):             # children before parents
        if v:
            cnt[T.par[v]] += cnt[v]
            with_members[T.par[v]] += cnt[v] > 0
    is_kept = insel | (with_members >= 2)
    kept = [v for v in T.dfs if is_kept[v]]
    index = {v: k for k, v in enumerate(kept)}
    own = {}
    for v in reversed(T.dfs):              # the nearest kept node downwards
        if cnt[v] == 0:
            continue
        own[v] = index[v] if is_kept[v] else own[next(c for c in T.kids[v] if cnt[c] > 0)]
    parent, depth = [], {0: 0}
    for v in T.dfs[1:]:
        depth[v] = depth[T.par[v]] + 1
    longest = 0
    for v in kept:                          # the chain's top is a child of the subtree parent
        top = v
        while top and own.get(T.par[top]) == own[v]:
            top = T.par[top]
        parent.append(own[T.par[top]] if top else NIL)
        longest = max(longest, depth[v] - depth[top] + 1)
    state, bad = {}, {}
    gathered = 0
    for v in T.dfs:                         # top-down within every chain
        if v not in own:
            continue
        k = own[v]
        for e in range(T.off[v], T.off[v + 1]):
            gathered += 1
            key, par, nuc = (k, T.pos[e]), T.mpar[e], T.mnuc[e]
            s = state.get(key)
            if s is None:
                state[key] = [T.pos[e], e, par, nuc]
            elif s[2] != nuc:
                s[3] = nuc
            elif s[3] == par:
                del state[key]
            else:
                bad[k] = bad.get(k, 0) + 1
    merged = [[] for _ in kept]
    for (k, _), s in sorted(state.items()):
        merged[k].append(s)
    return _result(T, sel, kept, parent, merged, own, gathered, sum(bad.values()), longest, kept[min(bad)] if bad else NIL)


def same(got, want, owner=None):
    """A Placer.subtree_nodes answer (and, when given, the subtree_owner answer for every node) against a result of this file."""
    for k in ("kept", "parent", "ent_off", "pos", "first_entry", "nuc"):
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)):
            return False
    for k, v in want["info"].items():
        if int(got["info"][k]) != int(v):
            return False
    return owner is None or np.array_equal(np.asarray(owner, np.uint32), want["owner"])


def strings(arrays, res):
    """Per kept node (BFS index) its merged entries as the reference prints them, from the opening entry's stored parent allele."""
    nuc = "NACMGRSVTWYHKDBN"
    out = {}
    for k, v in enumerate(res["kept"].tolist()):
        lo, hi = int(res["ent_off"][k]), int(res["ent_off"][k + 1])
        out[v] = ["MASKED" if res["pos"][e] < 0 else "%s%d%s" % (nuc[int(arrays["mut_par"][res["first_entry"][e]]) & 15], res["pos"][e], nuc[int(res["nuc"][e]) & 15])
                  for e in range(lo, hi)]
    return out
