"""The cases of tests/ripples_cases.py: the closed form the device runs equals the literal search on every one of them, and
each case has the property tests/test_ripples_edges_gpu.py relies on -- shown with the restatement alone, so that a case that
stops reaching its edge fails here instead of letting the GPU test pass vacuously.  CPU only."""
import os
import re

import numpy as np
import pytest

from oracle import capi
from tests import ripples_cases as RC
from tests import ripples_ref as RR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "usher_amd", "csrc")
NAMES = [c[0] for c in RC.CASES]
_ORACLES, _LITERAL = {}, {}


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _literal(c):
    name, arrays, br, _, opts, _ = c
    if name not in _LITERAL:
        if id(arrays) not in _ORACLES:
            _ORACLES[id(arrays)] = capi.OracleTree(arrays)
        _LITERAL[name] = RR.literal(arrays, br, _ORACLES[id(arrays)], **opts)
    return _LITERAL[name]


def _details(c):
    """Per branch: (detail of closed_branch, its events)."""
    _, arrays, br, rank, opts, _ = c
    out = []
    for bi, nid in enumerate(br):
        d = {}
        ev = RR.closed_branch(arrays, nid, bi, rank=rank, detail=d, **opts)
        out.append((d, ev))
    return out


def _counts(d, k, i, j):
    pre = d["S"][k]
    nin = pre[2 * j] - pre[2 * i + 1]
    return nin, pre[-1] - nin


def _buckets(d, k):
    pre = d["S"][k]
    return [pre[x + 1] - pre[x] for x in range(len(pre) - 1)]


def _winners(ev):
    return {e["donor"] for e in ev} | {e["acceptor"] for e in ev}


def _geo(c, d):
    return RC.geometry(len(d["rows"]), len(d["pairs"]), len(d["cand"]), c[5])


def test_constants_follow_the_sources():
    dense, rip = _text("ugp_dense.hpp"), _text("ugp_ripples.hip")
    assert re.search(r"constexpr uint32_t kBlock = (\d+);", dense).group(1) == str(RC.KBLOCK)
    assert re.search(r"constexpr uint32_t kTileMax = (\d+);", rip).group(1) == str(RC.KTILEMAX)
    assert re.search(r"constexpr uint64_t kLdsInts = (\d+);", rip).group(1) == str(RC.KLDSINTS)
    assert 1 << int(re.search(r"constexpr uint64_t kCountBudget = 1ull << (\d+);", rip).group(1)) == RC.KCOUNT
    assert 1 << int(re.search(r"constexpr uint64_t kSlabBudget = 1ull << (\d+);", rip).group(1)) == RC.KSLAB
    # the formulas geometry() restates
    assert "lim.count / (4ull * (nb + 1))" in rip and "lim.lds / (nb + 1)" in rip and "std::min(kTileMax, fit - 1)" in rip
    assert "std::min<uint64_t>({1024, tiles_all, lim.slab / (48ull * P)})" in rip
    assert [RC.geometry(M, 240, 130)["tile"] for M in (93, 94, 95, 96, 120)] == [64, 63, 63, 62, 49]


def test_case_list():
    assert len(set(NAMES)) == len(NAMES)
    families = {n.split("/")[0] for n in NAMES}
    assert families == {"tile_and_block_counts", "partial_tile_in_every_chunk", "grid_stride_with_wide_tiles",
                        "pairs_across_the_block", "narrow_lds_tile", "alleles", "masked", "ties_and_nid", "budget_edges",
                        "pair_validity_edges", "eligibility_and_sibling", "mixed_call"}
    for name, arrays, br, rank, opts, limits in RC.CASES:
        assert arrays["n"] < 2000, name
        order = np.argsort(rank)
        assert order.tolist() != list(range(arrays["n"])), name          # byte order of the names is not the BFS order
        assert np.array_equal(rank, RR.name_ranks(arrays)), name


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_equals_literal(name):
    c = RC.by_name(name)
    want = _literal(c)
    assert RR.closed(c[1], c[2], **c[4]) == want
    assert bool(want) == RC.INFO[name]["events"]


@pytest.mark.parametrize("name", NAMES)
def test_cases_reach_their_edges(name):
    c = RC.by_name(name)
    info = RC.INFO[name]
    _, arrays, br, rank, opts, limits = c
    det = _details(c)
    d, ev = det[0]
    sz = RR.subtree_sizes(arrays)
    globals()["_edge_" + name.split("/")[0]](c, info, det, d, ev, sz)


def _edge_tile_and_block_counts(c, info, det, d, ev, sz):
    C, nd = info["C"], info["nd"]
    assert d["cand"] == info["threshold"] if C == 1 else d["cand"] == [0] + info["threshold"]
    assert len(d["cand"]) == C and len(d["pairs"]) == 3 and d["B"] == 3
    assert all(sz[k] == nd for k in info["threshold"]) and all(sz[k] == nd - 1 for k in info["left_out"])
    assert info["left_out"] or C == 1
    g = _geo(c, d)
    assert g["tile"] == 64 and g["chunks"] == [C] and g["nblk"] == (C + 63) // 64 and g["count_blocks"] == [(C + 255) // 256]
    assert g["last_tiles"] == [(C - 1) % 64 + 1]
    if C == 1:
        assert ev == [] and d["cand"] == [0]
    else:   # the last candidate wins, and from three candidates on the one before it as well
        idx = {d["cand"].index(k) for k in _winners(ev)}
        assert C - 1 in idx and (C < 3 or C - 2 in idx)
        # a left-out child with every row would have won
        assert all(_counts(d, k, 0, 3)[0] <= 3 for k in d["cand"])


def _edge_partial_tile_in_every_chunk(c, info, det, d, ev, sz):
    g = _geo(c, d)
    assert len(d["cand"]) == 336 == c[1]["n"] and d["cand"] == list(range(336))
    assert g["Cc"] == 100 and g["tile"] == 64 and g["chunks"] == [100, 100, 100, 36] and g["last_tiles"] == [36, 36, 36, 36]
    assert _winners(ev) == info["winners"] and len(ev) == 3
    # the leaves of nid have the lowest ranks and no unmatched row: only their flag keeps them out, and they lie in chunk 1
    assert d["under"] == info["under"] and sorted(int(c[3][k]) for k in d["under"]) == list(range(10))
    assert all(100 <= k < 200 and d["S"][k][-1] == 0 for k in d["under"])


def _top3_donors(c, d, i, j):
    under = set(d["under"])
    keep = [k for k in d["cand"] if k not in under]
    keys = sorted((_counts(d, k, i, j)[0], int(c[3][k]), k) for k in keep if _counts(d, k, i, j)[0] <= d["B"])
    return [k for _, _, k in keys[:3]]


def _edge_grid_stride_with_wide_tiles(c, info, det, d, ev, sz):
    g = _geo(c, d)
    assert len(d["cand"]) == 600 and g["tile"] == 8 and g["nblk"] == 3 and ev
    if info["chunked"]:
        assert g["Cc"] == 100 and g["chunks"] == [100] * 6 and g["last_tiles"] == [4] * 6 and g["folds"] == [30, 24, 24]
    else:
        assert g["chunks"] == [600] and g["folds"] == [25, 25, 25] and g["folds"][2] >= 20
    top = _top3_donors(c, d, 0, 3)
    assert top == info["top3"]
    plain = RC.geometry(6, 3, 600, RC.limits_for(6, 3, T=8, nblk=3))
    if info["spread"]:
        assert [plain["block_of"][k] for k in top] == [0, 1, 2] and c[2][0] == top[0]        # nid heads the list
        e = next(e for e in ev if (e["i"], e["j"]) == (0, 3))
        assert e["donor"] == 300 and e["acceptor"] == 24                                     # d1 = a1: the second acceptor
    else:
        assert all(k // 8 == 74 and plain["block_of"][k] == 2 for k in top)                 # tile 74: the last of block 2
        assert max(t for t in range(75) if t % 3 == 2) == 74


def _edge_pairs_across_the_block(c, info, det, d, ev, sz):
    P = info["P"]
    assert len(d["rows"]) == 36 == info["M"] and len(d["pairs"]) == P
    idx = [d["pairs"].index((e["i"], e["j"])) for e in ev]
    # the first and the last pair have events: the last thread of the first trip of the pair loop at P == 256, the first of
    # the second at 257
    assert min(idx) == 0 and max(idx) == P - 1 and (P < RC.KBLOCK or RC.KBLOCK - 1 in idx)
    if P > 2 * RC.KBLOCK:
        assert any(2 * RC.KBLOCK <= x for x in idx)
    assert len({(e["donor"], e["acceptor"]) for e in ev}) >= 3


def _edge_narrow_lds_tile(c, info, det, d, ev, sz):
    M = info["M"]
    g = _geo(c, d)
    assert len(d["rows"]) == M and len(d["cand"]) == 130 and g["tile"] == info["tile"] and 200 <= len(d["pairs"]) <= 400
    assert RC.KLDSINTS // (2 * M + 2) == {93: 65, 95: 64, 96: 63, 120: 50}[M]
    assert 130 % g["tile"] != 0 and g["nblk"] == 3
    idx = {d["cand"].index(k) for k in _winners(ev)}
    assert ev and max(idx) >= g["tile"] and len(idx) >= 3        # winners beyond the first tile
    # three mutations at one position on nid's root path
    arrays, nid = c[1], c[2][0]
    seen, v = {}, nid
    while v >= 0:
        for (p, _, _) in RR._muts(arrays, v):
            seen[p] = seen.get(p, 0) + 1
        v = int(arrays["parent"][v])
    assert len(info["triple"]) == 9 and all(seen[p] == 3 for p in info["triple"])


def _edge_mixed_call(c, info, det, d, ev, sz):
    Ms = [len(x[0]["rows"]) for x in det]
    Ps = [len(x[0]["pairs"]) for x in det]
    assert Ms[0] == 96 and Ms[1:4] == [2, 1, 0] and Ms[4] > 80
    assert Ps[0] > 256 and Ps[1:4] == [1, 0, 0] and Ps[4] > 200
    assert det[0][1] and det[4][1] and not det[2][1] and not det[3][1]
    C = len(d["cand"])
    assert C == (130 if info["nd"] == 1 else int((sz >= 3).sum())) and (info["nd"] == 1 or 10 < C < 30)
    assert sz[c[2][4]] == 1 and c[2][3] == 0


def _edge_alleles(c, info, det, d, ev, sz):
    arrays, nodes = c[1], info["nodes"]
    rows = {p: (r, m) for p, r, m in d["rows"]}
    assert sorted(rows) == [0, 10, 20, 40, 50, 60, 70, 80, 90] and max(arrays["mut_pos"]) == 90
    if info["iupac"]:
        assert rows[10][1] & rows[10][0] and bin(rows[10][1]).count("1") == 2                 # ambiguous, with the reference base
        assert not rows[20][1] & rows[20][0] and bin(rows[20][1]).count("1") == 2             # ambiguous, without it
        assert sum(bin(int(m)).count("1") > 1 for m in arrays["mut_nuc"]) == 6                # on the path, own and ancestral
        # the handle's tree: the same nodes, names, positions and reference bases, one base of each allele
        h = info["handle"]
        assert all(np.array_equal(h[k], arrays[k]) for k in ("parent", "mut_off", "mut_pos", "mut_ref"))
        assert h["names"] == arrays["names"] and all(bin(int(m)).count("1") == 1 for m in h["mut_nuc"])
        assert all(int(a) & int(m) for a, m in zip(arrays["mut_nuc"], h["mut_nuc"]))
        # the ambiguous alleles change the events: a device run that kept the handle's one-hot arrays would not pass
        assert _literal(c) != _literal(RC.by_name("alleles/one_hot"))
    else:
        assert all(bin(int(m)).count("1") == 1 for m in arrays["mut_nuc"])
    assert 30 not in rows and any(p == 30 for p, _, _ in RR._muts(arrays, nodes["at_dropped"]))
    assert ev
    # the second branch: no row at 0, candidates mutate below its first row, between two rows and above the last
    d2, ev2 = det[1]
    pos2 = [p for p, _, _ in d2["rows"]]
    assert pos2 == [33, 44, 55, 66] and ev2
    allp = set(int(p) for p in arrays["mut_pos"])
    assert 0 in allp and {40, 50, 60} & allp and 90 in allp
    assert d2["S"][0][1] == 1 and d2["S"][0][-1] == 5          # the root: its mutation at 0 in bucket 0, and the four rows
    k = nodes["own_is_lowbit"]                                 # above it: 0, 10, 20 below the first row; 40, 50, 60 between rows
    assert _buckets(d2, k)[0] == 3 and [_buckets(d2, k)[x] for x in (2, 4, 6)] == [1, 1, 1]
    # the third branch, rows 0 .. 45: the same candidate counts 50 and 60 in bucket 2M, above the last row, and 40 between rows
    assert [p for p, _, _ in det[2][0]["rows"]] == [0, 20, 25, 35, 45]
    assert _buckets(det[2][0], k)[2 * 5] == 2 and _buckets(det[2][0], k)[8] == 1
    # the third: the candidate that stops at a masked mutation and then repeats the row's lowest base wins, its entry hidden
    d3, ev3 = det[2]
    k = nodes["masked_then_lowbit"]
    assert k in _winners(ev3) and d3["has_unique"][k] and not d3["elig"][k]
    assert d3["S"][k][-1] == 2 and d3["score"][k] == 4 + 1     # U hides rows 20 and 25; the set difference counts them
    assert nodes["own_is_lowbit"] in _winners(ev)


def _edge_masked(c, info, det, d, ev, sz):
    arrays, nodes = c[1], info["nodes"]
    root = RR._muts(arrays, 0)
    assert any(p < 0 and r != m for p, r, m in root) and any(p < 0 and r == m for p, r, m in root)
    posA = [p for p, _, _ in d["rows"]]
    assert posA[:2] == [-9, -5] and -7 not in posA and ev
    assert d["S"][0][3] - d["S"][0][2] == 1                    # the root's masked mutation: strictly between the two masked rows
    dR, evR = det[1]
    assert c[2][1] == 0 and len(dR["pairs"]) == 1 and evR == [] and len(dR["under"]) == len(dR["cand"]) - 1
    dB, evB = det[2]
    assert [p for p, _, _ in dB["rows"]][0] == -7 and 0 in _winners(evB)
    assert dB["S"][0][2] - dB["S"][0][1] == 2                  # at the row: the row itself and the root's own mutation
    k = nodes["masked_first"]
    assert k in _winners(ev) and d["has_unique"][k] and d["nm"][k] == 1 and d["common"][k] == 0
    assert d["nm"][nodes["masked_last"]] == 2 and d["common"][nodes["masked_last"]] == 1


def _edge_ties_and_nid(c, info, det, d, ev, sz):
    arrays, nid, rank = c[1], c[2][0], c[3]
    first = info["first"]
    assert len(d["cand"]) == arrays["n"] > 300 and len(ev) >= 1
    leaves = [k for k in d["cand"] if sz[k] == 1 and k != nid and d["S"][k] == d["S"][first[2]]]
    assert len(leaves) == 300
    e = next(e for e in ev if (e["i"], e["j"]) == (0, 3))
    if info["how"] == "plain":
        assert int(rank[nid]) == 0 and [int(rank[k]) for k in first] == [0, 1, 2, 3]
        assert _top3_donors(c, d, 0, 3) == first[:3]          # nid heads the list; the third slot is the second survivor
        if info["kind"] == "d1a2":
            assert (e["donor"], e["acceptor"]) == (first[1], first[2]) and first[1] == arrays["n"] - 1
            assert d["cand"].index(first[2]) == 64
        else:
            x, leaf = first[1], first[2]
            assert _counts(d, x, 0, 3) == (1, 0) and _counts(d, leaf, 0, 3) == (1, 2) and d["B"] == 2
            assert (e["donor"], e["acceptor"]) == (leaf, x) and leaf == arrays["n"] - 1
    else:
        assert int(rank[nid]) != 0 and e["donor"] != e["acceptor"]


def _edge_budget_edges(c, info, det, d, ev, sz):
    p = info["p"]
    assert d["B"] == 6 - p
    base = _details(RC.by_name("budget_edges/p4"))[0]
    d4, ev4 = base
    ins = {_counts(d4, k, 0, 3)[0] for k in d4["cand"] if k != c[2][0]}
    assert d4["B"] == 2 and 2 in ins and 3 in ins and 0 not in ins and 1 not in ins
    e = next(e for e in ev4 if (e["i"], e["j"]) == (0, 3))
    assert e["donor_count"] == 2 and e["acceptor_count"] == 0           # in == B, and d + a == B
    if p == 5:
        assert ev == [] and det[1][1] and d["B"] == 1          # in == B + 1 now: the pair fails; the second branch goes on
    if p == 6:
        assert ev == [] and det[1][1] and all(e["donor_count"] == 0 and e["acceptor_count"] == 0 for e in det[1][1])
    if p == 7:
        assert ev == [] and det[1][1] == []


def _edge_pair_validity_edges(c, info, det, d, ev, sz):
    assert d["pairs"] == info["pairs"] and d["rows"][0][0] == -4 and len(d["rows"]) == 6
    assert [(e["i"], e["j"]) for e in ev] == info["pairs"]
    pos = [p for p, _, _ in d["rows"]]
    assert [pos[j - 1] - pos[i] for i, j in ((0, 3), (1, 4), (2, 5))] == [2104, 2300, 2500]
    assert all(j - i == 3 == len(pos) - (j - i) for i, j in d["pairs"])
    d2, ev2 = det[1]
    assert len(d2["rows"]) == 4 and d2["pairs"] == [] and ev2 == []


def _edge_eligibility_and_sibling(c, info, det, d, ev, sz):
    seen = set()
    for name in ("eligibility_and_sibling/internal", "eligibility_and_sibling/leaves"):
        cc = RC.by_name(name)
        for dd, evs in _details(cc):
            for e in evs:
                for side in ("donor", "acceptor"):
                    k, sib = e[side], e[side + "_sibling"]
                    leaf, hu, el = sz[k] == 1, dd["has_unique"][k], dd["elig"][k]
                    nm, common = dd["nm"][k], dd["common"][k]
                    tie = el and dd["score"][k] == dd["best"]
                    if k == 0:
                        seen.add("root")
                    elif not el:
                        seen.add("ineligible")
                        assert e[side + "_score"] == dd["score"][k]
                    elif leaf:
                        assert common > 0
                        seen.add("leaf with common")
                    elif hu:
                        assert common > 0 and nm != common
                        seen.add("internal, unique and common")
                    else:
                        assert nm == common
                        seen.add("internal, all common")
                    if sib:
                        seen.add("sibling: leaf" if leaf else "sibling: tie with unique")
                        assert leaf or (tie and hu)
                    elif tie and k != 0:
                        assert not hu and not leaf
                        seen.add("tie without unique")
    assert seen == {"root", "ineligible", "leaf with common", "internal, unique and common", "internal, all common",
                    "sibling: leaf", "sibling: tie with unique", "tie without unique"}
    nodes = info["nodes"]
    if c[0].endswith("internal"):
        assert d["cand"] == sorted([0, nodes["Ic"], nodes["X"], nodes["Iuc"]]) and d["best"] == 1
        assert d["score"][nodes["Ic"]] == 1 == d["score"][nodes["Iuc"]] and d["score"][nodes["X"]] == 1 + 1
