"""Fixtures for tests/test_dense_edges_gpu.py (and tests/test_dense_cases_cpu.py, which proves with the oracle alone that each
one has the property its GPU test relies on): trees whose depth-first order fills more than one segment of the dense searches,
tie sets that cross segments, root mutations with the root as a sample.  Everything is built here, nothing is read from disk;
expected values come from tests/uncertainty_ref.py and tests/annotate_ref.py (the oracle's literal mapper2_body)."""
import functools

import numpy as np

from oracle import capi
from tests import annotate_ref as A
from tests import synth
from tests import uncertainty_ref as U

# kSeg / kBlock / the batch limit of usher_amd/csrc/ugp_dense.hpp and ugp_uncertainty.hip.  test_constants_follow_the_sources
# reads the sources and fails when they change there, so that the edges below follow them.
KSEG = 16384
KBLOCK = 256
BATCH = 4096

SIZE_EDGES = (KSEG - 1, KSEG, KSEG + 1, KSEG + KBLOCK - 1, KSEG + KBLOCK, 2 * KSEG, 2 * KSEG + 1)


def comb(K, G=7, root=(), chain=0, sub=0):
    """A root (or, with chain = c, a hub c levels below it on a chain whose nodes carry one and two mutations in turn) with K leaf
    children; child c carries one mutation at site 100 + c % G.  `root`: the root's mutations as (position, ref, allele), masked
    ones (position < 0) included.  With sub = J the hub's middle child is no leaf but a second hub without a mutation of its own
    over J more such leaves, which therefore lie two levels below the first hub.  N = 1 + chain + K + sub."""
    hub = chain
    first = hub + 1
    parent = [-1] + list(range(chain)) + [hub] * K
    mid = first + K // 2
    parent += [mid] * sub
    n = len(parent)
    muts = [[] for _ in range(n)]
    muts[0] = [(p, r, r, a) for p, r, a in root]
    above = {p: a for p, r, a in root if p >= 0}   # the state a leaf's mutation starts from
    site = 200
    for c in range(1, chain + 1):
        for _ in range(1 + (c + 1) % 2):
            muts[c].append((site, 4, 4, 8))
            site += 1
    for c in range(K):
        if not (sub and first + c == mid):
            muts[first + c] = [(100 + c % G, 1, above.get(100 + c % G, 1), 2)]
    for c in range(sub):
        muts[first + K + c] = [(100 + c % G, 1, above.get(100 + c % G, 1), 2)]
    mut_off = np.zeros(n + 1, np.int64)
    mut_off[1:] = np.cumsum([len(m) for m in muts])
    flat = [m for ms in muts for m in ms]
    col = lambda k, dt: np.asarray([m[k] for m in flat], dt)
    return {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": mut_off, "mut_pos": col(0, np.int32),
            "mut_ref": col(1, np.int8), "mut_par": col(2, np.int8), "mut_nuc": col(3, np.int8),
            "names": ["n%d" % j for j in range(n)]}


COMB_K = 40000
COMB_ROOT = ((150, 2, 4), (-7, 1, 8), (103, 1, 4))   # a plain one, a masked one, and one at a site the children mutate


@functools.lru_cache(maxsize=None)
def big_comb(variant="plain"):
    """The K = 40,000 combs: 'plain', 'root' (root mutations, one of them masked), 'chain' (two levels below the root, with a
    second hub below the first)."""
    if variant == "plain":
        return comb(COMB_K)
    if variant == "root":
        return comb(COMB_K, root=COMB_ROOT)
    assert variant == "chain"
    return comb(COMB_K - 3000, chain=2, sub=3000)


@functools.lru_cache(maxsize=None)
def bushy():
    """33,139 nodes in three levels of polytomies: 3 segments, tie sets of a few dozen nodes that cross segments."""
    return synth.polytomy_case(5, fanouts=(60, 70, 30), n_queries=1, genome_len=3000, n_sites=200)[0]


def bushy_nodes(count=9000):
    """Every internal node of the bushy tree (the root among them), then leaves drawn at random: `count` nodes, shuffled."""
    arrays = bushy()
    par = np.asarray(arrays["parent"])
    internal = np.unique(par[1:])
    leaves = np.setdiff1d(np.arange(arrays["n"]), internal)
    rng = np.random.default_rng(9)
    assert internal[0] == 0 and len(internal) < count
    nodes = np.concatenate([internal, rng.choice(leaves, count - len(internal), replace=False)])
    return rng.permutation(nodes)


# ---- root mutations -------------------------------------------------------------------------------------------------------

# (seed, n_leaves, root_muts, n_sites) of synth.make_case(..., p_masked=0.1), pinned by a search with the oracle alone
# (find_root_cases below, seeds 900-1499 with one root mutation and 2000-4999 with two and three; about one tree in 300 reaches
# either branch, always with the root as the sample); test_dense_cases_cpu.py asserts that each still reaches the branch it is
# listed under.
#   'kept'    the root's search finds nothing at or below the initial bound: best_j_vec stays {0}
#   'joined'  the best candidates tie with the initial bound and join the initial {0}
#   'below'   larger trees where every search beats the bound: root mutations in the scores of every node
ROOT_CASES = {
    "kept": ((909, 60, 1, 40), (1113, 150, 1, 40), (2652, 60, 3, 120), (3981, 60, 2, 40)),
    "joined": ((930, 150, 1, 6), (1089, 60, 1, 40), (2650, 60, 3, 120), (3325, 60, 2, 40)),
    "below": ((951, 400, 2, 40), (952, 250, 3, 120)),
}


def root_case(spec):
    seed, n_leaves, root_muts, n_sites = spec
    return synth.make_case(seed, n_leaves=n_leaves, n_queries=1, n_sites=n_sites, p_masked=0.1, root_muts=root_muts)[0]


def root_branch(arrays, j, ot=None, dfs=None):
    """Which branch of the reference's bookkeeping sample j ends in, from the oracle alone: 'empty' (no rows, no search),
    'kept', 'joined' or 'below' (some candidate beats the initial bound)."""
    ot = ot or capi.OracleTree(arrays)
    dfs = U.dfs_order(arrays) if dfs is None else dfs
    s = U.literal_sample(arrays, int(j))
    if len(s["pos"]) == 0:
        return "empty"
    n = len(dfs)
    keep = dfs != j
    init = len(s["pos"]) + int(arrays["mut_off"][1]) + 1
    # the same search with no initial bound: its best score against the bound
    w = ot.place_list(s, dfs[keep], jidx=np.arange(n)[keep], init_best=10 ** 9, tie_cap=n + 1)
    if w["num_best"] == 0 or w["best"] > init:
        return "kept"
    return "joined" if w["best"] == init else "below"


def find_root_cases(seeds, n_leaves=(60, 150), root_muts=(1, 2, 3), n_sites=(6, 40, 120)):
    """The search that produced ROOT_CASES: {branch: [(spec, sample), ...]} with the root and its children as samples."""
    found = {"kept": [], "joined": []}
    for seed in seeds:
        for spec in ((seed, nl, rm, ns) for nl in n_leaves for rm in root_muts for ns in n_sites):
            arrays = root_case(spec)
            ot, dfs = capi.OracleTree(arrays), U.dfs_order(arrays)
            for j in [0] + np.flatnonzero(np.asarray(arrays["parent"]) == 0).tolist():
                b = root_branch(arrays, j, ot, dfs)
                if b in found:
                    found[b].append((spec, j))
    return found


# ---- rows for annotate_search ----------------------------------------------------------------------------------------------

def awkward_rows(arrays, rng, k):
    """Rows at tree positions with a repeated position (G and N, two N rows) and masked rows, sorted by position."""
    pos = np.asarray(arrays["mut_pos"])
    sites = np.unique(pos[pos > 0])
    take = rng.choice(sites, size=min(len(sites), 12), replace=False)
    rows = []
    for p in take:
        i = int(np.flatnonzero(pos == p)[0])
        r, m = int(arrays["mut_ref"][i]), int(arrays["mut_nuc"][i])
        rows.append((int(p), r, m if rng.random() < 0.7 else 15))
    dup = take[k % len(take)]
    i = int(np.flatnonzero(pos == dup)[0])
    r = int(arrays["mut_ref"][i])
    rows.append((int(dup), r, 15))
    if k % 2:
        rows.append((int(dup), r, 15))
        rows.append((int(dup), r, [1, 2, 4, 8][k % 4]))
    rows.append((-int(rng.integers(1, 50)), 8, 15))
    if k % 3 == 0:
        rows.append((-int(rng.integers(1, 50)), 2, 1))
    rows.sort(key=lambda t: t[0])
    return rows_of(rows)


def rows_of(rows):
    """(position, ref, allele) triples, in the given order, as the arrays a QueryBatch takes."""
    return {"pos": np.asarray([t[0] for t in rows], np.int32), "ref": np.asarray([t[1] for t in rows], np.int8),
            "nuc": np.asarray([t[2] for t in rows], np.int8), "is_missing": np.zeros(len(rows), np.int8)}


def comb_rows(site=105, ref=1, nuc=2):
    """One- and two-row queries (for a comb: one row that ties every child mutated at `site`): the row alone; with a second row
    at the same position; with a masked row in front."""
    return [rows_of([(site, ref, nuc)]), rows_of([(site, ref, nuc), (site, ref, 15)]), rows_of([(-3, 8, 15), (site, ref, nuc)])]


def big_comb_rows(variant):
    """The query that ties every leaf of big_comb(variant) mutated at site 105: that row, and the chain's mutations above the hub."""
    chain = [(200, 4, 8), (201, 4, 8), (202, 4, 8)] if variant == "chain" else []
    return rows_of([(105, 1, 2)] + chain)


def root_rows(arrays, rng, k):
    """awkward_rows, and a row at the position of each non-masked root mutation: its allele, N, or another base in turn."""
    rows = awkward_rows(arrays, rng, k)
    t = list(zip(rows["pos"].tolist(), rows["ref"].tolist(), rows["nuc"].tolist()))
    for i in range(int(arrays["mut_off"][1])):
        p, r, m = int(arrays["mut_pos"][i]), int(arrays["mut_ref"][i]), int(arrays["mut_nuc"][i])
        if p >= 0:
            t.append((p, r, [m, 15, next(b for b in (1, 2, 4, 8) if b not in (r, m))][(k + i) % 3]))
    t.sort(key=lambda x: x[0])
    return rows_of(t)


# ---- expected values -------------------------------------------------------------------------------------------------------

def neighborhood_top2(arrays, tie_bfs):
    """U.neighborhood_literal with its quadratic pair loop (:104-113: the largest dist[a] + dist[b] over a != b) replaced by the
    sum of the two largest distances, which is the same number; everything else is the literal walk over every common node.
    For tie sets of thousands of nodes, where the pair loop takes minutes; test_dense_cases_cpu.py compares the two."""
    off = arrays["mut_off"]
    paths = [U._root_path(arrays, int(v)) for v in tie_bfs]
    common = set(paths[0])
    for p in paths[1:]:
        common &= set(p)
    best = int(off[-1])
    for c in common:
        t1 = t2 = -1
        for p in paths:
            td = 0
            for v in p:
                if v == c:
                    break
                td += int(off[v + 1] - off[v])
                if td > t1:
                    t1, t2 = td, t1
                elif td > t2:
                    t2 = td
        best = min(best, t1 + t2 if t2 >= 0 else 0)
    return best


def expected(arrays, nodes, ot=None, dfs=None):
    """U.expected, with the pair loop of the neighborhood only for tie sets of up to 64 nodes."""
    ot = ot or capi.OracleTree(arrays)
    dfs = U.dfs_order(arrays) if dfs is None else dfs
    out = []
    for j in nodes:
        nb, ties = search_ties(ot, arrays, dfs, int(j))
        bfs = [int(dfs[t]) for t in ties]
        ns = 0 if nb <= 1 else U.neighborhood_literal(arrays, bfs) if nb <= 64 else neighborhood_top2(arrays, bfs)
        out.append((nb, ns, ties))
    return out


def search_ties(ot, arrays, dfs, j):
    return U.search(ot, arrays, dfs, j, U.literal_sample(arrays, j))


def segments(ties):
    return sorted({t // KSEG for t in ties})


def cap_edges(ties):
    """(c0, c1, caps): the ties inside segments 0 and 1, and the values of `cap` that cut a list at its start, around the end
    of each of those segments' ties, and at its end."""
    c0 = sum(1 for t in ties if t < KSEG)
    c1 = sum(1 for t in ties if KSEG <= t < 2 * KSEG)
    return c0, c1, [1, 2, c0 - 1, c0, c0 + 1, c0 + c1 - 1, c0 + c1, c0 + c1 + 1, len(ties) - 1, len(ties)]


def lca_and_depths(arrays, dfs, ties):
    """(the lowest common ancestor of the tied nodes as a BFS index, its depth, the largest depth of a tied node)."""
    paths = [U._root_path(arrays, int(dfs[t])) for t in ties]
    common = set(paths[0])
    for p in paths[1:]:
        common &= set(p)
    c = next(v for v in paths[0] if v in common)
    return c, len(U._root_path(arrays, c)) - 1, max(len(p) for p in paths) - 1


@functools.lru_cache(maxsize=None)
def bushy_expected(count=9000):
    arrays = bushy()
    return expected(arrays, bushy_nodes(count))


def annotate_expected(arrays, samples, ot=None, dfs=None):
    ot = ot or capi.OracleTree(arrays)
    dfs = U.dfs_order(arrays) if dfs is None else dfs
    return [A.search(ot, arrays, s, dfs) for s in samples]
