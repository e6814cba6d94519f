"""get_closest_samples (matUtils select.cpp:577-714) restated over the breadth-first arrays of tests/synth.py, two ways.

`literal(T, node, fixed_k, k)` runs the reference's loop statement by statement: the sibling-leaf minimum, max_path (SIZE_MAX
when no sibling is a leaf), the redundant target_parent skip, closest_samples_dfs with its pruning, leaves past max_path pushed
in closest mode, the replace / append of the running minimum and the two stop rules.
`Fast` is the closed form with numpy over pre / dend / cum: the ring of level j is two ranges of leaf ranks, a ring leaf l is
cum[t] + cum[l] - 2 cum[p_j] away, and the level bound is L_j = cum[p_0] - cum[p_j] + nm[p_j].

A result is a dict: nodes (BFS indices, in the reference's order), dist, count, levels (levels processed) and best (the listed
node with the smallest name rank; NONE without ranks, without relatives, and in within mode)."""
import numpy as np

NONE = 0xFFFFFFFF
SIZE_MAX = (1 << 64) - 1


class Tree:
    def __init__(self, arrays):
        self.par = [int(p) for p in np.asarray(arrays["parent"])]
        self.n = len(self.par)
        self.nmut = [int(x) for x in np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))]
        self.kids = [[] for _ in range(self.n)]
        for j in range(1, self.n):
            self.kids[self.par[j]].append(j)

    def is_leaf(self, v):
        return not self.kids[v]


def _dfs(T, node, path_length, max_path_length, leaves, fixed_k):   # closest_samples_dfs, :577-594
    if path_length > max_path_length:
        return
    for child in T.kids[node]:
        if T.is_leaf(child):
            if fixed_k and path_length + T.nmut[child] <= max_path_length:
                leaves.append((child, path_length + T.nmut[child]))
            elif not fixed_k:
                leaves.append((child, path_length + T.nmut[child]))
        else:
            _dfs(T, child, path_length + T.nmut[child], max_path_length, leaves, fixed_k)


def literal(T, node, fixed_k, k=0, name_rank=None):
    target = node
    target_parent = T.par[target]
    curr_target = node
    parent = T.par[target]
    names, second = [], 0
    min_dist = SIZE_MAX
    dist_to_orig_parent = 0
    levels = 0
    go_up = True
    while go_up and parent >= 0:
        levels += 1
        parent_branch_length = T.nmut[parent] + dist_to_orig_parent
        cad, cad_fixed = [], []
        min_of_sibling_leaves = SIZE_MAX
        for child in T.kids[parent]:
            if T.is_leaf(child):
                if child == curr_target:
                    continue
                if T.nmut[child] < min_of_sibling_leaves:
                    min_of_sibling_leaves = T.nmut[child]
        for child in T.kids[parent]:
            if child == curr_target:
                continue
            if child == target_parent:
                continue
            dist_so_far = dist_to_orig_parent + T.nmut[target] + T.nmut[child]
            if not T.is_leaf(child):
                if fixed_k:
                    _dfs(T, child, dist_so_far, k, cad_fixed, True)
                else:
                    max_path = SIZE_MAX if min_of_sibling_leaves == SIZE_MAX else min_of_sibling_leaves + dist_so_far
                    _dfs(T, child, dist_so_far, max_path, cad, False)
            else:
                if fixed_k and dist_so_far <= k:
                    cad_fixed.append((child, dist_so_far))
                elif not fixed_k:
                    cad.append((child, dist_so_far))
        if fixed_k:
            if parent_branch_length > k:
                go_up = False
            for child, _ in cad_fixed:
                names.append(child)
                second = 0
        else:
            for child, length in cad:
                if length < parent_branch_length:
                    go_up = False
                if length < min_dist:
                    min_dist = length
                    names = [child]
                    second = min_dist
                elif length == min_dist:
                    names.append(child)
        curr_target = parent
        parent = T.par[curr_target]
        dist_to_orig_parent = parent_branch_length
    best = NONE
    if names and not fixed_k and name_rank is not None:
        best = min(names, key=lambda v: int(name_rank[v]))
    return {"nodes": names, "dist": int(second), "count": len(names), "levels": levels, "best": best}


class Fast:
    """The closed form from depth-first tables built with numpy.  rings=True records, per query, the leaf-rank ranges of every
    level in self.seen (the tests aim them at the edges of the device's range-minimum structure)."""

    def __init__(self, arrays, name_rank=None, rings=False):
        par = [int(p) for p in np.asarray(arrays["parent"])]
        n = self.n = len(par)
        nmut = np.diff(np.asarray(arrays["mut_off"]).astype(np.int64))
        size = [1] * n
        for j in range(n - 1, 0, -1):
            size[par[j]] += size[j]
        pre, nxt = [0] * n, [1] * n   # a node sits after its parent and the subtrees of its earlier siblings (children by index)
        for j in range(1, n):
            p = par[j]
            pre[j] = pre[p] + nxt[p]
            nxt[p] += size[j]
        cum = nmut.tolist()
        for j in range(1, n):
            cum[j] += cum[par[j]]
        self.par = par
        self.pre = np.asarray(pre, np.int64)
        self.size = np.asarray(size, np.int64)
        self.cumb = np.asarray(cum, np.int64)          # by BFS index
        self.nm = nmut
        self.dfs = np.empty(n, np.int64); self.dfs[self.pre] = np.arange(n)
        self.cum = self.cumb[self.dfs]                 # by depth-first position
        self.dend = np.arange(n) + self.size[self.dfs]
        leaf = self.size[self.dfs] == 1
        self.lpre = np.concatenate([[0], np.cumsum(leaf)])
        self.lbfs = self.dfs[leaf]                     # the leaves in depth-first order
        self.lcum = self.cum[leaf]
        self.rank = None if name_rank is None else np.asarray(name_rank)
        self.rings = rings
        self.seen = []

    def levels(self, t):
        """(leaf ranks of the ring, their distances, L_j) per level, from level 0 up."""
        tc, c, p = int(self.cumb[t]), t, self.par[t]
        cp0 = int(self.cumb[p]) if p >= 0 else 0
        while p >= 0:
            cp = int(self.cumb[p])
            a1, b1 = int(self.lpre[self.pre[p]]), int(self.lpre[self.pre[c]])
            a2, b2 = int(self.lpre[self.pre[c] + self.size[c]]), int(self.lpre[self.pre[p] + self.size[p]])
            if self.rings:
                self.seen.append((a1, b1, a2, b2))
            idx = np.concatenate([np.arange(a1, b1), np.arange(a2, b2)])
            yield idx, tc + self.lcum[idx] - 2 * cp, cp0 - cp + int(self.nm[p])
            c, p = p, self.par[p]

    def closest(self, t):
        best, parts, levels = None, [], 0
        for idx, d, L in self.levels(t):
            levels += 1
            if not len(idx):
                continue
            m = int(d.min())
            if best is None or m < best:
                best, parts = m, []
            if m == best:
                parts.append(idx[d == m])
            if m < L:
                break
        nodes = self.lbfs[np.concatenate(parts)].tolist() if parts else []
        b = NONE
        if nodes and self.rank is not None:
            b = min(nodes, key=lambda v: int(self.rank[v]))
        return {"nodes": nodes, "dist": best if nodes else 0, "count": len(nodes), "levels": levels, "best": b}

    def within(self, t, k):
        parts, levels = [], 0
        for idx, d, L in self.levels(t):
            levels += 1
            parts.append(idx[d <= k])
            if L > k:
                break
        nodes = self.lbfs[np.concatenate(parts)].tolist() if parts else []
        return {"nodes": nodes, "dist": 0, "count": len(nodes), "levels": levels, "best": NONE}


def check(got, want, i):
    """Sample i of Placer.relatives_closest / relatives_within's outputs against a result dict, every field."""
    info, off, nodes = got
    for f in ("dist", "count", "levels", "best"):
        assert int(info[f][i]) == want[f], (i, f, int(info[f][i]), want[f])
    if off is not None:
        assert int(off[i + 1]) - int(off[i]) == want["count"], (i, "off")
        assert nodes[int(off[i]):int(off[i + 1])].tolist() == want["nodes"], (i, "nodes")
