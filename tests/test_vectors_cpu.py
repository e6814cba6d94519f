"""ugp_vectors' closed form (tests/vectors_ref.py) against the literal mapper2_body of the oracle (OracleTree.node_vecs_split: the
lists, and n_branch, eligible and the score each on its own): every (sample, node) of every case of tests/vectors_cases.py, every
size of its generators, 200 seeded random trees, the winners of OracleTree.place, and the header's declarations against the ctypes
table.  Then, from the closed form alone, that the cases tests/test_vectors_gpu.py picks lie on the edges of the kernel's wave
bookkeeping, and that a kernel which lost one piece of it would answer one of them differently."""
import os
import re
from bisect import bisect_right

import numpy as np
import pytest

from oracle import capi
from tests import vectors_cases as VC
from tests import vectors_ref as VR
from tests.dense_cases import KBLOCK
from usher_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
random_case = VC.random_case


def every_pair_agrees(case):
    """The closed form against the split oracle on every pair of the case; the refused pairs."""
    ot, T = capi.OracleTree(case["arrays"]), VR.Tables(case["arrays"])
    n = int(case["arrays"]["n"])
    refused = 0
    for s, smp in enumerate(case["samples"]):
        for j in range(n):
            mine = VR.vectors(T, smp, j)
            assert mine["refused"] == (1 if j in case["refused"] else 0), (case["name"], s, j)
            if mine["refused"]:
                refused += 1
                assert mine["excess"] == [] and mine["imputed"] == []
                continue
            orc = VR.oracle_answer_split(ot, smp, j)
            assert VR.agrees_split(mine, orc), (case["name"], s, j, mine, orc)
    assert all(0 <= s < len(case["samples"]) and 0 <= j < n for s, j in case["pairs"])
    return refused


@pytest.mark.parametrize("case", VC.cases(), ids=lambda c: c["name"])
def test_closed_form_is_the_oracle_on_every_pair(case):
    assert (every_pair_agrees(case) > 0) == (case["name"] == "twice")


def wide_masks(width):
    return [m for m in (None, 0, 1, 63, 64, 65, width) if m is None or m <= width]


@pytest.mark.parametrize("width", VC.WIDE_WIDTHS)
def test_closed_form_is_the_oracle_on_wide_nodes(width):
    for order in VC.WIDE_ORDERS:
        for mask_at in wide_masks(width):
            for as_root in (False, True):
                assert every_pair_agrees(VC.wide(width, order, mask_at, as_root)) == 0
    assert all(pk[2] in wide_masks(pk[0]) and pk[0] in VC.WIDE_WIDTHS for pk in VC.WIDE_PICKS)   # the picks are among them


@pytest.mark.parametrize("depth,counts", VC.RAGGED_PICKS + ((130, VC.RAGGED_COUNTS), (131, (2, 0, 5)), (137, (1,))))
def test_closed_form_is_the_oracle_on_ragged_paths(depth, counts):
    assert every_pair_agrees(VC.ragged_path(depth, counts)) == 0


def test_closed_form_is_the_oracle_on_random_trees():
    pairs = 0
    for seed in range(200):
        c = random_case(seed)
        ot, T = capi.OracleTree(c["arrays"]), VR.Tables(c["arrays"])
        n = int(c["arrays"]["n"])
        rng = np.random.default_rng(1000 + seed)
        for s, smp in enumerate(c["samples"]):
            for j in (range(n) if s == 0 else rng.integers(0, n, 30)):
                mine = VR.vectors(T, smp, int(j))
                assert not mine["refused"]
                assert VR.agrees_split(mine, VR.oracle_answer_split(ot, smp, int(j))), (seed, s, int(j))
                pairs += 1
    assert pairs > 30000


def test_closed_form_is_the_oracle_on_the_random_trees_of_the_device():
    """Every pair of the trees tests/test_vectors_gpu.py sends to the device, and the counts that test relies on."""
    pairs = part3 = branch = 0
    for pick in VC.RANDOM_PICKS:
        c = random_case(*pick)
        assert every_pair_agrees(c) == 0 and 100 <= c["arrays"]["n"] <= pick[1]
        T = VR.Tables(c["arrays"])
        assert max(T.moff[v + 1] - T.moff[v] for v in range(T.n)) > 64                # a second step of 64 own entries
        for s, j in c["pairs"]:
            tr = {}
            mine = VR.vectors(T, c["samples"][s], j, tr)
            pairs, part3, branch = pairs + 1, part3 + (len(tr["part3"]) > 0), branch + (mine["n_branch"] > 0)
    assert 4000 <= pairs <= 5500 and part3 >= 2000 and branch >= 500, (pairs, part3, branch)


def test_the_split_fields_are_held_apart():
    """agrees_split refuses what agrees lets through: n_branch off by one, and (eligible, set_difference) = (0, k) for (1, k + 1)."""
    c = VC.cases()[1]
    ot, T = capi.OracleTree(c["arrays"]), VR.Tables(c["arrays"])
    swapped = moved = 0
    for s, j in c["pairs"]:
        mine, orc = VR.vectors(T, c["samples"][s], j), VR.oracle_answer_split(ot, c["samples"][s], j)
        assert VR.agrees(mine, VR.oracle_answer(ot, c["samples"][s], j)) and VR.agrees_split(mine, orc)
        if mine["eligible"] and mine["set_difference"] > 0:
            wrong = dict(mine, eligible=0, set_difference=mine["set_difference"] - 1)
            assert VR.agrees(wrong, orc) and not VR.agrees_split(wrong, orc)
            swapped += 1
        wrong = dict(mine, n_branch=mine["n_branch"] + 1)
        assert VR.agrees(wrong, orc) and not VR.agrees_split(wrong, orc)
        moved += 1
    assert swapped and moved


def traced(case, fault=False):
    """Per pair of the case (sample, node, answer, trace, the faults of VR.FAULTS that change the answer)."""
    T = VR.Tables(case["arrays"])
    out = []
    for s, j in case["pairs"]:
        tr = {}
        mine = VR.vectors(T, case["samples"][s], j, tr)
        assert not mine["refused"]
        out.append((s, j, mine, tr, [f for f in VR.FAULTS if fault and VR.vectors(T, case["samples"][s], j, None, f) != mine]))
    return out


def test_the_cases_name_their_edges():
    by = {c["name"]: c for c in VC.cases()}
    T = {k: VR.Tables(c["arrays"]) for k, c in by.items()}
    for name in ("caterpillar", "caterpillar_flip"):
        nodes = sorted({j for _, j in by[name]["pairs"]})
        cum = lambda j: sum(1 for _ in _path_entries(T[name], j))
        assert sorted({cum(j) for j in nodes}) == sorted(VC.PATH_COUNTS)
    assert sorted(len(s["pos"]) for s in by["rows"]["samples"]) == [0, 1, 63, 64, 65, 70, 257]
    assert all(by["rows"]["samples"][-1]["is_missing"])
    assert sum(T["polytomy"].leaf) == 129
    # loop 1 passes a row on the node with descending entries, and both imputed lists and part 3 are exercised
    got = [VR.vectors(T[c["name"]], c["samples"][s], j) for c in VC.cases() for s, j in c["pairs"]]
    assert any(g["imputed"] for g in got) and any(len(g["excess"]) > g["n_branch"] + 1 for g in got)
    assert {(g["has_unique"], g["eligible"]) for g in got} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    bits = {bin(a & 15).count("1") for c in VC.cases() for s in c["samples"] for a, m in zip(s["nuc"], s["is_missing"]) if not m}
    assert bits == {1, 2, 3, 4}


def test_the_wide_picks_lie_on_the_steps_of_64():
    """Part 1 and the root's own loop of part 3, from the closed form's trace alone."""
    stops, nms, faults = set(), set(), set()
    carried = asked = root_steps = 0
    for pick in VC.WIDE_PICKS:
        c = VC.wide(*pick)
        Tc = VR.Tables(c["arrays"])
        assert Tc.n == len(c["arrays"]["parent"]) and not c["refused"]
        kinds = set()
        for smp in c["samples"][1:]:   # the three cycling samples see every kind of row at W's positions
            at = {int(p): (int(a) & 15, bool(m)) for p, a, m in zip(smp["pos"], smp["nuc"], smp["is_missing"])}
            for i in range(pick[0]):
                p = 2000 + 3 * i
                kinds.add("absent" if p not in at else "missing" if at[p][1] else
                          ("single", "ambiguous")[at[p][0] & (at[p][0] - 1) != 0] + ("", "+ref")[at[p][0] & VC.REF(p) != 0])
        assert kinds == {"absent", "missing", "single", "single+ref", "ambiguous", "ambiguous+ref"}, kinds
        assert len(c["samples"][0]["pos"]) == 0
        if pick[3]:
            assert sum(1 for e in range(Tc.moff[1]) if Tc.mnuc[e] != Tc.mref[e]) > 64
        for s, j, mine, tr, f in traced(c, True):
            faults |= set(f)
            if j in c["W"] and j != 0:
                stops.add(tr["stop"])
                nms.add(tr["nm"])
                # the passed entry and the first entry that left the pointer behind its row in different steps, and no entry of the
                # passed one's own step hides the row: only the carried pointer does
                carried += any(ok and a // 64 != b // 64 for a, b, ok in tr["passed"])
                asked += (not tr["allvis"]) and any(i >= 64 and here for i, here in tr["own_asks"])
            if j == 0 and pick[3]:
                root_steps += len({i // 64 for _, i, masked in tr["part3"] if masked}) >= 2
    assert {0, 63, 64, 65} <= stops, stops
    assert {63, 64, 65} <= nms and {127, 128, 129} & nms and max(nms) > 192, nms
    assert carried and asked and root_steps, (carried, asked, root_steps)
    assert faults == set(VR.FAULTS), faults          # each of the three, undone, changes an answer among these pairs


def test_the_ragged_picks_lie_on_the_steps_of_part_3():
    for depth, counts in VC.RAGGED_PICKS:
        c = VC.ragged_path(depth, counts)
        Tc = VR.Tables(c["arrays"])
        assert depth >= 130 and len(c["chain"]) == depth + 1 and not c["refused"]
        per_node = [Tc.moff[Tc.bfs2dfs[j] + 1] - Tc.moff[Tc.bfs2dfs[j]] for j in c["chain"]]
        assert per_node[20] == per_node[depth - 10] == VC.RAGGED_WIDE and {0, 1, 3, 7, 2} <= set(per_node)
        owners = [len(v) for v in Tc.pent.values()]
        assert sum(1 for k in owners if k > 1) > len(owners) // 2                       # most positions have several owners
        assert any(Tc.mnuc[e] == Tc.mref[e] for e in range(len(Tc.mpos)))               # some entries return to the reference
        assert [len(list(_path(Tc, j))) for j in c["leaves"]] == [h + 2 for h in c["hang"]]
        assert {1, 63, 64, 65, 127, 128, 129, depth} == set(c["hang"])
        assert sorted({j for _, j in c["pairs"]}) == sorted(set(c["leaves"]) | {c["chain"][h] for h in c["hang"]})
        assert [len(s["pos"]) for s in c["samples"]][0] == 0 and all(c["samples"][2]["is_missing"]) and len(c["samples"][2]["pos"]) > 64
        spread, late, counts3, side = 0, 0, set(), 0
        for s, j, mine, tr, _ in traced(c):
            path = [Tc.moff[v + 1] - Tc.moff[v] for v in _path(Tc, j)]
            # the lanes of one step of 64 path nodes run 0 and 70 trips side by side
            spread = max([spread] + [max(path[k:k + 64]) - min(path[k:k + 64]) for k in range(0, len(path), 64)])
            late = max([late] + [i for _, i, _ in tr["part3"]])
            counts3.add(len(tr["part3"]))
            # the last owner in front of j in depth-first order is a hanging leaf off the path: the search has to climb
            side += any(_last_owner_is_off_the_path(Tc, p, Tc.bfs2dfs[j]) for p in Tc.pent)
        assert spread >= 60 and late >= 8 and side, (spread, late, side)
        assert any(0 < k < 64 for k in counts3) and any(64 < k < 256 for k in counts3) and any(k > 256 for k in counts3), sorted(counts3)


def _last_owner_is_off_the_path(T, p, j):
    x = bisect_right(T.onode[p], j)
    return x > 0 and T.dend[T.mnode[T.pent[p][x - 1]]] <= j


def _path(T, j_bfs):
    v = T.bfs2dfs[j_bfs]
    while v != VR.NIL:
        yield v
        v = T.dpar[v]


def _path_entries(T, j_bfs):
    for v in _path(T, j_bfs):
        yield from range(T.moff[v], T.moff[v + 1])


def test_the_scan_tile_and_the_seam_pairs():
    """k_vec_scan's tile is what the window sizes of test_window_seams rest on, the pairs on its seam are what that test says, and a
    prefix sum that dropped the carry between its tiles gives other offsets for every one of its windows."""
    hip = open(os.path.join(ROOT, "usher_amd", "csrc", "ugp_vectors.hip")).read()
    dense = open(os.path.join(ROOT, "usher_amd", "csrc", "ugp_dense.hpp")).read()
    assert re.search(r"constexpr uint32_t kScanTile = (\d+);", hip).group(1) == "8"
    assert re.search(r"constexpr uint32_t kDefaultPairs = 1u << (\d+);", hip).group(1) == "18"
    assert int(re.search(r"constexpr uint32_t kBlock = (\d+);", dense).group(1)) == KBLOCK == 256
    assert "t0 += (uint64_t)kBlock * kScanTile" in hip
    assert VC.SEAM_TILE == KBLOCK * 8 == 2048 and max(VC.SEAM_COUNTS) < 1 << 18      # one window holds every count
    assert VC.SEAM_COUNTS == (VC.SEAM_TILE - 1, VC.SEAM_TILE, VC.SEAM_TILE + 1, 2 * VC.SEAM_TILE, 2 * VC.SEAM_TILE + 1)
    case = next(c for c in VC.cases() if c["name"] == VC.SEAM_CASE)
    Tc = VR.Tables(case["arrays"])
    assert len(set(case["pairs"])) <= 60
    ans = {}
    for s, j in case["pairs"]:
        tr = {}
        mine = VR.vectors(Tc, case["samples"][s], j, tr)
        ans[(s, j)] = (len(mine["excess"]), len(mine["imputed"]), len(tr["part3"]))
    assert ans[VC.SEAM_EMPTY] == (0, 0, 0) and ans[VC.SEAM_PART3][2] > 0 and ans[VC.SEAM_PART3][1] == 0
    assert ans[VC.SEAM_BOTH][0] >= 2 and ans[VC.SEAM_BOTH][1] >= 2 and ans[VC.SEAM_BOTH][2] > 0

    def offsets(counts, carry):
        off, run = [], 0
        for i, k in enumerate(counts):
            if i % VC.SEAM_TILE == 0 and not carry:
                run = 0
            off.append(run)
            run += k
        return off + [run]
    for n in VC.SEAM_COUNTS:
        for both in (False, True):
            pairs = VC.seam_pairs(n, both)
            assert len(pairs) == n and set(pairs) <= set(case["pairs"])
            want = (VC.SEAM_BOTH,) * 3 if both else (VC.SEAM_EMPTY, VC.SEAM_EMPTY, VC.SEAM_PART3)
            assert tuple(pairs[VC.SEAM_TILE - 1:VC.SEAM_TILE + 2]) == want[:max(0, n - VC.SEAM_TILE + 1)]
            for which in (0, 1):
                counts = [ans[pr][which] for pr in pairs]
                assert sum(counts[:VC.SEAM_TILE - 1]) > 0
                assert (offsets(counts, False) != offsets(counts, True)) == (n > VC.SEAM_TILE)


def test_winners_are_eligible_and_score_the_best():
    for c in VC.cases()[:5] + [random_case(s) for s in range(20)]:
        ot, T = capi.OracleTree(c["arrays"]), VR.Tables(c["arrays"])
        for smp in c["samples"]:
            w = ot.place(smp)
            for j in [w["best_j"]] + [int(t) for t in w["ties"]]:
                mine = VR.vectors(T, smp, j)
                if mine["refused"]:
                    continue
                assert mine["eligible"] == 1 and mine["set_difference"] == w["best"], (c["name"], j)


def test_header_declares_what_the_binding_lists():
    text = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    declared = set(re.findall(r"^int (ugp_vectors\w*)\(", text, re.M))
    assert declared == {k for k in _lib.SYMBOLS if k.startswith("ugp_vectors")} == {"ugp_vectors_attach", "ugp_vectors", "ugp_vectors_chunked",
                                                                                     "ugp_vectors_time"}
    for name in declared:   # and the argument counts agree
        args = re.search(r"^int " + name + r"\((.*?)\);", text, re.M | re.S).group(1)
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S)
        assert len(args.split(",")) == len(_lib.SYMBOLS[name][1]), name
