"""Child counts of ugp_fitch.hip at exact ties and at the edges of its counter widths (tests/fitch_cases.py says how the inputs
are made and why the random inputs of tests/test_fitch.py cannot see a miscounted child).

CPU: the vectorised set formulation equals the oracle on every case; the inputs have the properties the GPU tests rely on (the
expected set at every target and site, eight sites of every kind, every kind in every word that holds an edge site); and every
counting fault of the list -- a child dropped, counted twice or read as the reference row at the first, the last and the
word / chunk edge positions; counters that wrap mod 8, 32, 256 and 2^(K-1) -- changes the mutation list of every case, at every
target it applies to.  GPU: fitch_sankoff equals the oracle on every case in every call mode."""
import os
import re

import numpy as np
import pytest

from tests import fitch_cases as C

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "usher_amd", "csrc")
MODEL_MAX_CHILDREN = 4097   # (the oracle comparison of the model; the sensitivity test runs on every case)


def test_constants_follow_the_source():
    with open(os.path.join(CSRC, "ugp_fitch.hip")) as f:
        src = f.read()
    m = re.search(r"constexpr uint32_t FS_WIDE = (\d+), FS_CHUNK = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (C.FS_WIDE, C.FS_CHUNK)
    assert re.search(r"constexpr int FS_FN = 8;", src) and re.search(r"constexpr int FS_NB = 8;", src)
    for c in (7, 8, 31, 32, C.FS_WIDE, C.FS_WIDE + 1, 5 * C.FS_CHUNK, 5 * C.FS_CHUNK + 1):
        assert c in C.SINGLE_DEGREES
    assert len(C.MIXED_A) % 8 == 1 and len(C.MIXED_B) % 8 == 7 and len(C.BACKWARD) % 8 == 1


def test_tree_from_degrees():
    parent = C.tree_from_degrees([[3], [2, 0, 1], [0, 2, 0]])
    assert parent.tolist() == [-1, 0, 0, 0, 1, 1, 3, 5, 5]
    assert (np.diff(parent[1:]) >= 0).all()
    nch, first, lvl = C.topology(parent)
    assert nch.tolist() == [3, 2, 0, 1, 0, 2, 0, 0, 0] and lvl == [0, 1, 4, 7, 9]
    assert [int(first[j]) for j in (0, 1, 3, 5)] == [1, 4, 6, 7]
    with pytest.raises(ValueError):
        C.tree_from_degrees([[2], [1]])
    k = C.case("mixed-8k+1")
    nch, _, lvl = C.topology(k.parent)
    assert tuple(nch[lvl[1]:lvl[2]]) == C.MIXED_A and len(lvl) == 5
    assert (nch[lvl[2]:lvl[3]] > 0).sum() >= 8   # the entries the last group of level 1 reads past its end are non-zero ones


@pytest.mark.parametrize("name", [n for n in C.CASE_NAMES if max(C.CASES[n][0]) <= MODEL_MAX_CHILDREN])
def test_set_formulation_equals_oracle(name):
    k = C.case(name)
    assert C.set_model(k.parent, k.ref, k.off, k.nodes, k.nucs) == C.oracle_list(name)


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_sites_are_what_they_claim(name):
    """At every target: every site gives the set its kind is built for (a realised tie where it says so), every kind has at least
    eight sites, and every kind lies in every word that holds a listed edge site or the end of the sites; the listed edge sites
    between them hold every kind.  Leaves without a row exist beside leaves with one in every tile (from 8 children on)."""
    k = C.case(name)
    S = C.Sensitivity(k)
    assert k.targets
    sites = np.arange(k.n_sites)
    edge_sites = [s for s in C.EDGE_SITES if s < k.n_sites] + [k.n_sites - 1]
    edge_words = sorted({s // 8 for s in edge_sites})
    assert k.n_sites % 8 == 0 or k.n_sites % 8 >= len(C.KINDS)   # (the partial last word has room for every kind)
    X, Y, R = k.bases[:, 0].astype(np.int16), k.bases[:, 1].astype(np.int16), k.ref.astype(np.int16)
    want = {"XY": X | Y, "XR": X | R, "X": X}
    for t_ in k.targets:
        kinds = np.asarray([C.kind_at(s, t_["index"]) for s in sites])
        F = S.target_sets(t_)
        for kind in C.KINDS:
            at = sites[kinds == kind]
            assert len(at) >= 8, (name, t_["c"], kind)
            assert np.array_equal(F[at], want[C.TIE_OF[kind]][at]), (name, t_["c"], kind)
            for w in edge_words:
                assert ((at // 8) == w).any(), (name, t_["c"], kind, w)
        if len(edge_sites) >= 2 * len(C.KINDS) - 1:
            assert {kinds[s] for s in edge_sites} == set(C.KINDS), (name, t_["c"])
        for y, ghost in enumerate(t_["ghosts"]):
            assert ghost.any() == (t_["c"] >= 8) and not ghost[list(t_["internal"])].any()
            lo, hi = int(k.off[y * 512]), int(k.off[min((y + 1) * 512, k.n_sites)])
            with_cell = np.zeros(len(k.parent), bool)
            with_cell[k.nodes[lo:hi]] = True
            kids = with_cell[t_["first"]:t_["first"] + t_["c"]]
            assert np.array_equal(~kids, ghost), (name, t_["c"], y)   # exactly the ghosts have no cell in the tile
    assert set(k.root_mode.tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_every_counting_fault_changes_the_mutation_list(name):
    k = C.case(name)
    S = C.Sensitivity(k)
    missed, n = [], 0
    for t_ in k.targets:
        faults = C.faults_for(t_["c"], t_["internal"])
        kinds = {f[1] for f in faults}
        assert {"drop", "twice", "wrap"} <= kinds and ("asref" in kinds or t_["c"] == 2)
        labels = {f[0] for f in faults}
        c = t_["c"]
        edges = {0, c - 1} | {(c - 1 - r) // m * m + r for m, r in ((8, 0), (8, 7), (64, 0), (64, 63)) if c - 1 >= r}
        for what in ("drop", "twice"):
            assert {f[2] for f in faults if f[1] == what} == edges
        assert {f[2] for f in faults if f[1] == "asref"} == edges - set(t_["internal"])
        for m in (8, 32, 256):
            assert ("wrap mod %d" % m in labels) == (t_["c"] >= m)
        assert "wrap mod %d" % (1 << (t_["c"].bit_length() - 1)) in labels
        for label, kind, arg in faults:
            n += 1
            if not S.changes(t_, kind, arg):
                missed.append((t_["c"], label))
    assert not missed, (name, missed)
    assert n >= 6 * len(k.targets)


@pytest.mark.parametrize("name", ["single-2", "single-9", "single-33", "single-257", "backward"])
def test_quick_sensitivity_equals_the_full_model(name):
    """Sensitivity.changes() (the counters of the target alone, states down to the root's children) against the whole model run with
    the same fault: the same verdict for every fault, and -- so that the comparison is not vacuous -- a fault-free run is the oracle."""
    k = C.case(name)
    S = C.Sensitivity(k)
    base = C.set_model(k.parent, k.ref, k.off, k.nodes, k.nucs)
    assert base == C.oracle_list(name)
    for t_ in k.targets[:3]:
        for label, kind, arg in C.faults_for(t_["c"], t_["internal"]):
            full = C.set_model(k.parent, k.ref, k.off, k.nodes, k.nucs, fault=(t_["node"], kind, arg))
            assert (full != base) == S.changes(t_, kind, arg), (name, t_["c"], label)


def _modes(k):
    n = len(k.parent)
    modes = [("one pass", {}), ("1 word per pass", {"UGP_FITCH_BYTES": str((n + 1) * 4)}),
             ("65 words per pass", {"UGP_FITCH_BYTES": str((n + 1) * 4 * 65)}), ("exact listing", {"UGP_FITCH_EMIT_CAP": "3"})]
    if k.n_sites > 512:
        modes.append(("2 pieces", {"UGP_FITCH_PIECES": "2"}))
    return modes


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_gpu_fitch_counts_equal_oracle(name, monkeypatch):
    from usher_amd.fitch import fitch_sankoff
    k = C.case(name)
    want = C.oracle_list(name)
    for label, env in _modes(k):
        for var in ("UGP_FITCH_BYTES", "UGP_FITCH_EMIT_CAP", "UGP_FITCH_PIECES"):
            monkeypatch.delenv(var, raising=False)
        for var, val in env.items():
            monkeypatch.setenv(var, val)
        site, node, mpar, mnuc = fitch_sankoff(k.parent, k.ref, k.off, k.nodes, k.nucs)
        got = list(zip(site.tolist(), node.tolist(), mpar.tolist(), mnuc.tolist()))
        assert got == want, (name, label)
