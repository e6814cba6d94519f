"""The locality pre-pass from the samples' own rows (usher_amd/csrc/ugp_coarse.hpp) on the CPU: a small C++ driver builds the static
tables from a tree's arrays and runs the header's host restatement of k_coarse_sparse, sample by sample.  For every sample its
(cost, node) must be the cost oracle/closed_form.py calls `best` and a node whose own eligible cost is that: scores[node] == best
(an ineligible node scores one more than its cost, so equality also says "eligible").

The driver's depth-first order is children in index order and its sites are the tree's positions in ascending order; the library
takes both from the flattener.  The plan rule (ugp_plan.hpp, CallPlan::coarse_sparse) is pinned by hand-computed cases at each edge.
The same driver is built once more with -fsanitize=address,undefined as a stand-alone program."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle.closed_form import ClosedFormTree
from tests import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "ugp_plan.hpp"
static long long rd(FILE *f) { long long v = 0; if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(3); } return v; }
static int plan_main(int argc, char **argv) {
    std::map<std::string, long long> A;
    for (int i = 2; i < argc; i++) { const char *e = strchr(argv[i], '='); if (!e) return 2; A[std::string(argv[i], e - argv[i])] = atoll(e + 1); }
    auto get = [&](const char *k, long long d) { auto it = A.find(k); return it == A.end() ? d : it->second; };
    ugp::PlanTree t;
    t.n_nodes = 10000000; t.n_sites = 500; t.n_chunks = 100; t.max_chunk8_words = 1000; t.max_path_muts = 100; t.lds_slots = 4;
    t.coarse = get("coarse", 1); t.b3_events = true;
    t.coarse_nodes = get("coarse_nodes", 4097); t.coarse_max_per_pos = (uint32_t)get("per_pos", 4);
    t.coarse_excluded = get("excluded", 0); t.coarse_masked = get("masked", 0);
    ugp::PlanCall c;
    c.Q = get("Q", 16384); c.max_rows = get("max_rows", 50);
    c.ex.given = get("ex_given", 0); c.ex.packed = get("ex_packed", 0); c.ex.mask = get("ex_mask", 0); c.ex.skip = get("ex_skip", 0);
    c.ex.skip_chunk = get("ex_skip_chunk", 0); c.ex.scores = get("ex_scores", 0);
    ugp::Knobs K;
    K.no_fork = true; K.bound3 = 1; K.coarse_phase2 = get("K_coarse_phase2", 0); K.no_sort = get("K_no_sort", 0);
    const ugp::CallPlan cp = ugp::plan_call(t, K, c);
    printf("sorted=%d\ncoarse_sparse=%d\ncoarse_cap=%u\n", (int)cp.sorted, (int)cp.coarse_sparse, cp.coarse_cap);
    const ugp::PlanTree t0;   // the new fields default to "off"
    ugp::PlanTree t1 = t; t1.coarse_nodes = t0.coarse_nodes; t1.coarse_max_per_pos = t0.coarse_max_per_pos;
    printf("default_sparse=%d\n", (int)ugp::plan_call(t1, K, c).coarse_sparse);
    return 0;
}
int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return plan_main(argc, argv);
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    const uint64_t n = (uint64_t)rd(f);
    std::vector<uint32_t> parent(n);
    for (auto &v : parent) v = (uint32_t)rd(f);
    std::vector<uint64_t> mut_off(n + 1);
    for (auto &v : mut_off) v = (uint64_t)rd(f);
    const uint64_t nm = mut_off[n];
    std::vector<int32_t> mpos(nm); std::vector<uint8_t> mref(nm), mnuc(nm);
    for (auto &v : mpos) v = (int32_t)rd(f);
    for (auto &v : mref) v = (uint8_t)rd(f);
    for (auto &v : mnuc) v = (uint8_t)rd(f);
    // depth-first order, children in index order; sites = the positions in ascending order
    std::vector<std::vector<uint32_t>> ch(n);
    for (uint64_t j = 1; j < n; j++) ch[parent[j]].push_back((uint32_t)j);
    std::vector<uint32_t> dfs2bfs, st{0};
    while (!st.empty()) {
        const uint32_t j = st.back(); st.pop_back();
        dfs2bfs.push_back(j);
        for (size_t k = ch[j].size(); k > 0; k--) st.push_back(ch[j][k - 1]);
    }
    int32_t max_pos = 0;
    for (int32_t p : mpos) if (p > max_pos) max_pos = p;
    std::vector<int32_t> pos2site((size_t)max_pos + 1, -1);
    for (int32_t p : mpos) if (p >= 0) pos2site[p] = 0;
    uint64_t n_sites = 0;
    for (auto &v : pos2site) if (v == 0) v = (int32_t)n_sites++;
    ugp::CoarseTables t;
    ugp::build_coarse_tables(n, parent.data(), mut_off.data(), mpos.data(), mref.data(), mnuc.data(), dfs2bfs.data(), pos2site.data(), (uint64_t)max_pos, n_sites, t);
    printf("usable=%d consistent=%d max_per_pos=%u\n", (int)t.usable(), (int)ugp::coarse_tables_consistent(t, n, n_sites), t.max_per_pos);
    if (!t.usable()) return 0;
    const uint64_t Q = (uint64_t)rd(f);
    for (uint64_t q = 0; q < Q; q++) {
        const uint64_t r = (uint64_t)rd(f);
        std::vector<int32_t> pos(r); std::vector<uint8_t> ref(r), nuc(r), mis(r);
        for (uint64_t i = 0; i < r; i++) { pos[i] = (int32_t)rd(f); ref[i] = (uint8_t)rd(f); nuc[i] = (uint8_t)rd(f); mis[i] = (uint8_t)rd(f); }
        const uint32_t best = ugp::coarse_sparse_host(t, pos2site.data(), (uint64_t)max_pos, r, pos.data(), ref.data(), nuc.data(), mis.data());
        printf("%u %u\n", best >> 16, dfs2bfs[best & 0xFFFFu]);
    }
    fclose(f);
    return 0;
}
"""


@functools.lru_cache(None)
def _exe(sanitize=False):
    d = tempfile.mkdtemp(prefix="ugp_coarse_")
    src, exe = os.path.join(d, "coarse_driver.cpp"), os.path.join(d, "coarse_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "usher_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                   check=True)
    return exe


def _run(arrays, samples, sanitize=False):
    """(cost, node) per sample from the driver, and its first line as a dict."""
    n = int(arrays["n"])
    words = [n] + [int(v) & 0xFFFFFFFF for v in arrays["parent"]] + [int(v) for v in arrays["mut_off"]]
    for k in ("mut_pos", "mut_ref", "mut_nuc"):
        words += [int(v) for v in arrays[k]]
    words.append(len(samples))
    for s in samples:
        words.append(len(s["pos"]))
        for p, r, a, m in zip(s["pos"], s["ref"], s["nuc"], s["is_missing"]):
            words += [int(p), int(r), int(a), int(m)]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write(" ".join(map(str, words)))
        path = f.name
    try:
        r = subprocess.run([_exe(sanitize), path], capture_output=True, text=True)
    finally:
        os.unlink(path)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    head = {k: int(v) for k, v in (w.split("=") for w in lines[0].split())}
    return np.array([[int(x) for x in l.split()] for l in lines[1:]], dtype=np.int64).reshape(-1, 2), head


def _check(arrays, samples, sanitize=False):
    got, head = _run(arrays, samples, sanitize)
    assert head["usable"] == 1 and head["consistent"] == 1, head
    assert len(got) == len(samples)
    cf = ClosedFormTree(arrays)
    for i, s in enumerate(samples):
        w = cf.place(s, compute_scores=True)
        assert got[i, 0] == w["best"], (i, got[i], w["best"], w["best_j"])
        assert w["scores"][got[i, 1]] == w["best"], (i, got[i], w["best"], w["best_j"])
    return head


def _sample(rows):
    rows = sorted(rows)
    return {"pos": np.array([r[0] for r in rows], dtype=np.int32), "ref": np.array([r[1] for r in rows], dtype=np.uint8),
            "nuc": np.array([r[2] for r in rows], dtype=np.uint8), "is_missing": np.array([r[3] for r in rows], dtype=np.uint8)}


def _tree(nodes):
    """nodes: (parent, [(pos, ref, nuc), ...]) in breadth-first order; pos < 0 = a masked mutation."""
    off, pos, ref, nuc = [0], [], [], []
    for _, muts in nodes:
        for p, r, a in muts:
            pos.append(p); ref.append(r); nuc.append(a)
        off.append(len(pos))
    return {"n": len(nodes), "parent": np.array([p for p, _ in nodes], dtype=np.int32), "mut_off": np.array(off, dtype=np.uint64),
            "mut_pos": np.array(pos, dtype=np.int32), "mut_ref": np.array(ref, dtype=np.uint8), "mut_nuc": np.array(nuc, dtype=np.uint8)}


A, C, G, T = 1, 2, 4, 8
# root mutations (10, 20); position 10 mutated forth and back on the path 0 - 1 - 4 - 9; node 2 with three mutations; masked mutations
# in front of (node 3) and behind (node 5) ordinary ones; node 6 an internal node without mutations, node 7 a leaf without
HAND = [
    (-1, [(10, A, C), (20, A, G)]),                 # 0
    (0, [(10, A, A)]),                              # 1: back to the reference
    (0, [(30, C, T), (40, G, A), (50, T, C)]),      # 2
    (0, [(-1, A, A), (70, A, T)]),                  # 3: masked first
    (1, [(10, A, T), (60, C, G)]),                  # 4: forth again
    (1, [(80, G, C), (-1, A, A), (90, T, A)]),      # 5: masked in the middle
    (2, []),                                        # 6: internal, no mutations
    (2, []),                                        # 7: leaf, no mutations
    (2, [(40, G, C)]),                              # 8
    (4, [(10, A, G), (20, A, A)]),                  # 9
    (6, [(30, C, C), (95, A, C)]),                  # 10
    (6, [(50, T, G)]),                              # 11
]
HAND_REF = {10: A, 20: A, 30: C, 40: G, 50: T, 60: C, 70: A, 80: G, 90: T, 95: A, 5: G, 15: T, 99: C}


def _hand_samples():
    rng = np.random.default_rng(7)
    out = [_sample([]),                                             # no rows
           _sample([(5, G, A, 0), (15, T, C, 0), (99, C, C, 0)]),   # rows only where the tree has no position
           _sample([(30, C, T, 0), (50, T, C, 0)]),                 # two of node 2's three positions
           _sample([(30, C, T, 0), (40, G, A, 0), (50, T, C, 0)]),
           _sample([(10, A, 15, 1)]),                               # N at the position mutated forth and back
           _sample([(10, A, A | C, 0)]),                            # IUPAC sets holding both alleles
           _sample([(10, A, C | T, 0), (20, A, A | G, 0)]),
           _sample([(10, A, C, 0), (20, A, G, 0)]),                 # the root's own mutations
           _sample([(70, A, T, 0)]), _sample([(80, G, C, 0), (90, T, A, 0)]), _sample([(90, T, A, 0)]),
           _sample([(10, A, G, 0), (60, C, G, 0)]), _sample([(30, C, T, 0), (95, A, C, 0)]), _sample([(50, T, G, 0)])]
    positions = sorted(HAND_REF)
    for _ in range(400):
        rows = []
        for p in positions:
            if rng.random() < 0.35:
                miss = int(rng.random() < 0.15)
                rows.append((p, HAND_REF[p], 15 if miss else int(rng.integers(1, 16)), miss))
        out.append(_sample(rows))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_trees(seed):
    arrays, queries = synth.make_case(seed, n_leaves=300, n_queries=120, n_sites=200, n_ambig=(0, 0, 2, 5, 30))
    _check(arrays, queries)


def test_hand_made_tree():
    head = _check(_tree(HAND), _hand_samples())
    assert head["max_per_pos"] == 4   # position 10: nodes 0, 1, 4, 9


def test_single_node_and_chain():
    _check(_tree([(-1, [])]), [_sample([]), _sample([(5, G, A, 0)])])
    _check(_tree([(-1, [(10, A, C)])]), [_sample([]), _sample([(10, A, C, 0)]), _sample([(10, A, 15, 1)])])
    chain = [(-1, [])] + [(i, [(10 + i, A, C)]) for i in range(6)]
    _check(_tree(chain), [_sample([]), _sample([(10, A, C, 0)]), _sample([(10 + i, A, C, 0) for i in range(6)]), _sample([(12, A, G, 0), (15, A, C, 0)])])


def test_sanitized_driver():
    """The same driver under AddressSanitizer and UBSan, as a stand-alone program."""
    arrays, queries = synth.make_case(1, n_leaves=300, n_queries=120, n_sites=200, n_ambig=(0, 0, 2, 5, 30))
    _check(arrays, queries, sanitize=True)
    _check(_tree(HAND), _hand_samples(), sanitize=True)


def _plan(**kw):
    r = subprocess.run([_exe(), "plan"] + ["%s=%d" % (k, int(v)) for k, v in kw.items()], capture_output=True, text=True, check=True)
    return {k: int(v) for k, v in (line.split("=") for line in r.stdout.split())}


def test_plan_rule():
    # defaults: a sorted plain call of 16,384 samples of at most 50 rows, 4,097 coarse nodes, at most 4 events per position:
    # 200 events <= 512; the records' room is the power of two from 32 on that holds 2 * 200 = 400
    p = _plan()
    assert p["sorted"] == 1 and p["coarse_sparse"] == 1 and p["coarse_cap"] == 512
    assert p["default_sparse"] == 0                       # a PlanTree that says nothing about tables: the walked pass
    assert _plan(max_rows=1, per_pos=1)["coarse_cap"] == 32
    assert _plan(max_rows=0)["coarse_cap"] == 32
    # 65,536 nodes fit 16 bits of position, 65,537 do not
    assert _plan(coarse_nodes=65536)["coarse_sparse"] == 1 and _plan(coarse_nodes=65537)["coarse_sparse"] == 0
    # capacity: 128 rows x 4 = 512 events (1,024 records); 129 x 4 = 516
    p = _plan(max_rows=128)
    assert p["coarse_sparse"] == 1 and p["coarse_cap"] == 1024
    p = _plan(max_rows=129)
    assert p["sorted"] == 1 and p["coarse_sparse"] == 0 and p["coarse_cap"] == 0
    assert _plan(max_rows=512, per_pos=1)["coarse_sparse"] == 1 and _plan(max_rows=513, per_pos=1)["coarse_sparse"] == 0
    # UGP_COARSE_PHASE2 keeps the walked pass; so do excluded nodes and a mask on the streams
    assert _plan(K_coarse_phase2=1)["coarse_sparse"] == 0
    assert _plan(excluded=1)["coarse_sparse"] == 0
    assert _plan(masked=1)["coarse_sparse"] == 0
    # a call that is not sorted has no pre-pass at all
    for kw in (dict(Q=512), dict(K_no_sort=1), dict(coarse=0)):
        p = _plan(**kw)
        assert p["sorted"] == 0 and p["coarse_sparse"] == 0, kw
    assert _plan(Q=513)["coarse_sparse"] == 1
    # an extended search that only leaves one node out per sample takes it; one with a node mask does not reach the packed path
    assert _plan(ex_given=1, ex_packed=1, ex_skip=1, ex_skip_chunk=1)["coarse_sparse"] == 1
    assert _plan(ex_given=1, ex_packed=1)["coarse_sparse"] == 1
    assert _plan(ex_given=1, ex_packed=1, ex_mask=1)["coarse_sparse"] == 0
    assert _plan(ex_given=1, ex_packed=1, ex_scores=1)["coarse_sparse"] == 0
