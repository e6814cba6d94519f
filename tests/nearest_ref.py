"""get_nearby (matUtils select.cpp:206-276) restated over the breadth-first arrays of tests/synth.py, two ways.

`literal(...)` walks as the reference does: climb rsearch(node, true), count leaves, and for every leaf under `anc` that is not a
strict descendant of `last_anc` (is_ancestor starts at the parent) walk back up summing mutations.size().  Two tie orders:
  - canonical (sorter=None): leaves in depth-first order, a stable sort by distance -- what ugp_nearest_k returns;
  - the reference's (sorter = tests/stdorder.py's StdOrder): leaves in Tree::get_leaves' queue order, std::sort.
`Fast` is the canonical answer with numpy over cum / dend, for trees too large for per-leaf walks.

A result is a dict: nodes, dist (distance to anc, also for the leaves of last_anc), count, anc, last_anc, cut_dist, n_at_cut
(anc = NONE and count = 0: no ancestor has more than k leaves; cut_dist = n_at_cut = 0: no candidate is taken)."""
import numpy as np

NONE = 0xFFFFFFFF


class Tree:
    def __init__(self, arrays):
        self.par = np.asarray(arrays["parent"]).astype(np.int64)
        self.n = len(self.par)
        self.nmut = np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))
        self.kids = [[] for _ in range(self.n)]
        for j in range(1, self.n):
            self.kids[self.par[j]].append(j)
        self.nleaves = np.array([0 if self.kids[j] else 1 for j in range(self.n)], np.int64)
        for j in range(self.n - 1, 0, -1):
            self.nleaves[self.par[j]] += self.nleaves[j]

    def rsearch(self, v):
        out = [v]
        while self.par[v] >= 0:
            v = int(self.par[v])
            out.append(v)
        return out

    def leaves_dfs(self, v):
        out, st = [], [v]
        while st:
            u = st.pop()
            if not self.kids[u]:
                out.append(u)
            st.extend(reversed(self.kids[u]))
        return out

    def leaves_queue(self, v):   # Tree::get_leaves: a queue
        out, q, h = [], [v], 0
        while h < len(q):
            u = q[h]; h += 1
            if not self.kids[u]:
                out.append(u)
            q.extend(self.kids[u])
        return out

    def is_ancestor(self, a, v):   # starts at the parent
        while self.par[v] >= 0:
            v = int(self.par[v])
            if v == a:
                return True
        return False


def literal(T, node, k, sorter=None):
    assert k > 0
    last = node
    for anc in T.rsearch(node):
        if T.nleaves[anc] <= k:
            last = anc
            continue
        leaves = T.leaves_dfs if sorter is None else T.leaves_queue
        keep = list(leaves(last))
        cand = []
        for l in leaves(anc):
            if T.is_ancestor(last, l):
                continue
            d, a = 0, l
            while a != anc:
                d += int(T.nmut[a]); a = int(T.par[a])
            cand.append((l, d))
        cand = sorted(cand, key=lambda x: x[1]) if sorter is None else sorter.sort(cand, key=lambda x: x[1])
        dist = []
        for l in keep:
            d, a = 0, l
            while a != anc:
                d += int(T.nmut[a]); a = int(T.par[a])
            dist.append(d)
        taken = []
        for (l, d) in cand:
            if len(keep) + len(taken) == k:
                break
            taken.append((l, d))
        cut = taken[-1][1] if taken else 0
        return {"nodes": keep + [l for l, _ in taken], "dist": dist + [d for _, d in taken], "count": len(keep) + len(taken), "anc": anc,
                "last_anc": last, "cut_dist": cut, "n_at_cut": sum(1 for _, d in cand if d == cut) if taken else 0}
    return {"nodes": [], "dist": [], "count": 0, "anc": NONE, "last_anc": last, "cut_dist": 0, "n_at_cut": 0}


class Fast:
    """The canonical answer from depth-first tables built with numpy."""

    def __init__(self, arrays):
        par = np.asarray(arrays["parent"]).astype(np.int64)
        n = self.n = len(par)
        nmut = np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))
        size = np.ones(n, np.int64)
        for j in range(n - 1, 0, -1):
            size[par[j]] += size[j]
        # preorder position: a node sits after its parent and the subtrees of its earlier siblings (children by index)
        pre = np.zeros(n, np.int64)
        nxt = np.ones(n, np.int64)   # offset of the next child below each node
        for j in range(1, n):        # parents come first, siblings in increasing index
            p = par[j]
            pre[j] = pre[p] + nxt[p]
            nxt[p] += size[j]
        self.pre = pre
        self.dfs = np.empty(n, np.int64); self.dfs[pre] = np.arange(n)
        self.dpar = np.where(par[self.dfs] >= 0, pre[np.maximum(par[self.dfs], 0)], -1)
        self.dend = np.arange(n) + size[self.dfs]
        cum = np.zeros(n, np.int64)
        for j in range(n):
            cum[j] = nmut[j] + (cum[par[j]] if par[j] >= 0 else 0)
        self.cum = cum[self.dfs]
        self.leaf = size[self.dfs] == 1
        self.lpre = np.concatenate([[0], np.cumsum(self.leaf)])

    def _nl(self, v):
        return int(self.lpre[self.dend[v]] - self.lpre[v])

    def query(self, node, k):
        last = a = int(self.pre[node])
        while a >= 0 and self._nl(a) <= k:
            last = a
            a = int(self.dpar[a])
        if a < 0:
            return {"nodes": [], "dist": [], "count": 0, "anc": NONE, "last_anc": int(self.dfs[last]), "cut_dist": 0, "n_at_cut": 0}
        keep = last + np.flatnonzero(self.leaf[last:self.dend[last]])
        idx = a + np.flatnonzero(self.leaf[a:self.dend[a]])
        idx = idx[(idx <= last) | (idx >= self.dend[last])]
        key = self.cum[idx] - self.cum[a]
        need = 0 if a == last else k - len(keep)
        cut = n_at = 0
        taken = np.zeros(0, np.int64)
        if need:
            cnt = np.cumsum(np.bincount(key))
            cut = int(np.searchsorted(cnt, need))
            below = int(cnt[cut - 1]) if cut else 0
            n_at = int(cnt[cut]) - below
            sel = np.concatenate([np.flatnonzero(key < cut), np.flatnonzero(key == cut)[:need - below]])
            sel = sel[np.argsort(key[sel] * self.n + idx[sel], kind="stable")]
            taken = idx[sel]
        pos = np.concatenate([keep, taken])
        return {"nodes": self.dfs[pos].tolist(), "dist": (self.cum[pos] - self.cum[a]).tolist(), "count": len(pos), "anc": int(self.dfs[a]),
                "last_anc": int(self.dfs[last]), "cut_dist": cut, "n_at_cut": n_at}


def check(got, want, i, stride=None):
    """Row i of Placer.nearest_k's outputs against a result dict, every field."""
    nodes, dist, info = got
    for f in ("count", "anc", "last_anc", "cut_dist", "n_at_cut"):
        assert int(info[f][i]) == want[f], (i, f, int(info[f][i]), want[f])
    w = want["count"] if stride is None else min(want["count"], stride)
    assert nodes[i, :w].tolist() == want["nodes"][:w], (i, "nodes")
    assert dist[i, :w].tolist() == want["dist"][:w], (i, "dist")
    assert (nodes[i, w:] == NONE).all() and (dist[i, w:] == NONE).all(), (i, "slots past the result were written")
