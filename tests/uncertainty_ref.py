"""Restatements of matUtils uncertainty (uncertainty.cpp:41-339) for the tests of ugp_uncertainty / matutils-amd: the literal
sample findEPPs builds, the search through the oracle's literal mapper2_body (orc_place_sample_list), the literal
get_neighborhood_size, its closed form, and the -e / -o files."""
import numpy as np

from oracle import capi


def dfs_order(arrays):
    """The reference's depth-first expansion (preorder, children in stored = increasing index order): dfs[k] = BFS index."""
    par = np.asarray(arrays["parent"])
    n = len(par)
    kids = [[] for _ in range(n)]
    for j in range(1, n):
        kids[int(par[j])].append(j)
    out, st = [], [0]
    while st:
        v = st.pop()
        out.append(v)
        st.extend(reversed(kids[v]))
    return np.asarray(out, np.int64)


def literal_sample(arrays, j):
    """Q(S) of uncertainty.cpp:143-166: S's own mutations, then each ancestor's; a non-masked entry only if its position was
    not taken lower down; masked entries always; NOT sorted."""
    pos, ref, nuc, seen = [], [], [], set()
    a = int(j)
    while a >= 0:
        for i in range(int(arrays["mut_off"][a]), int(arrays["mut_off"][a + 1])):
            p = int(arrays["mut_pos"][i])
            if p < 0 or p not in seen:
                pos.append(p); ref.append(int(arrays["mut_ref"][i])); nuc.append(int(arrays["mut_nuc"][i]))
                if p >= 0:
                    seen.add(p)
        a = int(arrays["parent"][a])
    return {"pos": np.asarray(pos, np.int32), "ref": np.asarray(ref, np.int8), "nuc": np.asarray(nuc, np.int8),
            "is_missing": np.zeros(len(pos), np.int8)}


def sorted_sample(s):
    o = np.argsort(s["pos"], kind="stable")
    return {k: np.asarray(v)[o] for k, v in s.items()}


def search(ot, arrays, dfs, j, sample):
    """findEPPs' search (:167-235) as a serial run: (num_best, tie DFS positions ascending), or (0, []) for an empty sample."""
    if len(sample["pos"]) == 0:
        return 0, []
    n = len(dfs)
    keep = dfs != j
    root_muts = int(arrays["mut_off"][1] - arrays["mut_off"][0])
    w = ot.place_list(sample, dfs[keep], jidx=np.arange(n)[keep], init_best=len(sample["pos"]) + root_muts + 1, tie_cap=n + 1)
    return w["num_best"], w["ties"].tolist()


def _root_path(arrays, v):
    path = [v]
    while int(arrays["parent"][v]) >= 0:
        v = int(arrays["parent"][v])
        path.append(v)
    return path


def neighborhood_literal(arrays, tie_bfs):
    """get_neighborhood_size (:41-130) line by line: root paths (node first), the common nodes of all paths, for each common node
    the distances of get_all_distances, the widest pair, the smallest over the common nodes, capped by the parsimony score."""
    off = arrays["mut_off"]
    nmut = lambda v: int(off[v + 1] - off[v])
    paths = [_root_path(arrays, int(v)) for v in tie_bfs]
    common = set(paths[0])
    for p in paths[1:]:
        common &= set(p)
    best = int(off[-1])                                      # Tree::get_parsimony_score (:100)
    for c in common:
        dist = []
        for p in paths:
            td = 0
            for v in p:
                if v == c:
                    break
                td += nmut(v)
                dist.append(td)
        widest = 0
        for a in range(len(dist)):
            for b in range(len(dist)):
                if a != b and dist[a] + dist[b] > widest:
                    widest = dist[a] + dist[b]
        best = min(best, widest)
    return best


def neighborhood_closed(arrays, tie_bfs):
    """The closed form (the device's): c = lowest common ancestor; each tie v != c gives cum[v] - cum[a] for its ancestors a up
    to c; widest = sum of the two largest values (0 with fewer than two); capped by the parsimony score."""
    off = arrays["mut_off"]
    paths = [_root_path(arrays, int(v)) for v in tie_bfs]
    common = set(paths[0])
    for p in paths[1:]:
        common &= set(p)
    c = next(v for v in paths[0] if v in common)
    vals = []
    for p in paths:
        td = 0
        for v in p:
            if v == c:
                break
            td += int(off[v + 1] - off[v])
            vals.append(td)
    vals.sort(reverse=True)
    widest = vals[0] + vals[1] if len(vals) >= 2 else 0
    return min(widest, int(off[-1]))


def expected(arrays, nodes, ot=None, dfs=None):
    """(epps, nsize, ties as DFS positions) per node, from the oracle and the literal neighborhood."""
    ot = ot or capi.OracleTree(arrays)
    dfs = dfs_order(arrays) if dfs is None else dfs
    out = []
    for j in nodes:
        nb, ties = search(ot, arrays, dfs, int(j), literal_sample(arrays, int(j)))
        ns = neighborhood_literal(arrays, [int(dfs[t]) for t in ties]) if nb > 1 else 0
        out.append((nb, ns, ties))
    return out


def render(names, parent, dfs, samples_bfs, results):
    """The -e and -o files of findEPPs_wrapper (:279-339) for samples given by BFS index."""
    e = ["sample\tequally_parsimonious_placements\tneighborhood_size\n"]
    o = ["placement\tsample\n"]
    for j, (nb, ns, ties) in zip(samples_bfs, results):
        e.append("%s\t%d\t%d\n" % (names[j], nb, ns))
        o.append("%s\t%s\n" % (names[j], names[j]))
        if nb > 1:
            o.extend("%s\t%s\n" % (names[int(dfs[t])], names[j]) for t in ties)
        elif nb == 1:
            o.append("%s\t%s\n" % (names[int(parent[j])], names[j]))
    return "".join(e), "".join(o)
