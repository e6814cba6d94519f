"""The cases of tests/shared_tables_cases.py without a GPU: the references alone show that a silently accepted attach with other
mutation arrays would be visible in every family's answer.  A condition of tests/test_shared_tables_gpu.py, not a measurement: that
module asks each family after every other and compares with want(X), which proves nothing for a Y whose answer equals X's."""
import numpy as np
import pytest

from tests import shared_tables_cases as S

TREES = ("plain", "bare")


def test_the_trees_are_what_the_matrix_needs():
    plain, bare = S.trees()["plain"], S.trees()["bare"]
    assert 200 <= plain.n <= 600 and 200 <= bare.n <= 600
    X = bare.X
    pos, off = np.asarray(X["mut_pos"]), np.asarray(X["mut_off"])
    assert (pos < 0).sum() >= 10                                                  # masked entries
    for k in ("mut_ref", "mut_par", "mut_nuc"):                                   # alleles 1 .. 15 everywhere, ambiguous ones among them
        assert 1 <= int(np.asarray(X[k]).min()) and int(np.asarray(X[k]).max()) <= 15
    assert any(bin(int(a)).count("1") > 1 for a in X["mut_nuc"])
    for j in range(bare.n):                                                       # no node with two entries at one position
        own = pos[off[j]:off[j + 1]]
        assert len(set(own[own >= 0].tolist())) == (own >= 0).sum()
    assert (np.asarray(plain.X["mut_pos"]) >= 0).all()                            # the placement tables take it
    for t in (plain, bare):
        m = len(t.X["mut_pos"])
        assert t.move_leaf not in (t.allele_leaf, t.allele_leaf - 1)
        for name, y in t.Y.items():                                               # the same topology and entry count, other contents
            assert len(y["mut_pos"]) == len(y["mut_nuc"]) == m and int(y["mut_off"][-1]) == m, name
            assert any(not np.array_equal(np.asarray(y[k]), np.asarray(t.X[k])) for k in ("mut_off", "mut_pos", "mut_nuc")), name
        yp, ya, ym = t.Y["Y_pos"], t.Y["Y_allele"], t.Y["Y_move"]
        live = np.asarray(t.X["mut_pos"]) >= 0
        assert np.array_equal(np.asarray(yp["mut_pos"])[live], np.asarray(t.X["mut_pos"])[live] + 1)
        assert np.array_equal(np.asarray(yp["mut_pos"])[~live], np.asarray(t.X["mut_pos"])[~live])
        k = t.allele_entry
        diff = np.flatnonzero(np.asarray(ya["mut_nuc"]) != np.asarray(t.X["mut_nuc"]))
        assert diff.tolist() == [k] and int(ya["mut_nuc"][k]) in S.ONEHOT and int(ya["mut_nuc"][k]) != int(t.X["mut_ref"][k])
        # the moved entry: the flat arrays are the same, one offset differs; no position twice on the sibling
        a = t.move_leaf
        assert np.flatnonzero(np.asarray(ym["mut_off"]) != np.asarray(t.X["mut_off"])).tolist() == [a + 1]
        assert all(np.array_equal(np.asarray(ym[k]), np.asarray(t.X[k])) for k in ("mut_pos", "mut_ref", "mut_par", "mut_nuc"))
        own = np.asarray(ym["mut_pos"])[int(ym["mut_off"][a + 1]):int(ym["mut_off"][a + 2])]
        assert len(set(own.tolist())) == len(own) and not t.kids[a] and not t.kids[a + 1] and t.par[a] == t.par[a + 1]


@pytest.mark.parametrize("tree", TREES)
def test_every_family_has_an_answer_worth_comparing(tree):
    t = S.trees()[tree]
    fams = S.families(t)
    assert [f.name for f in fams] == list(S.NAMES) and len(fams) == 11
    for f in fams:
        x = f.wanted("X")
        items = list(S.flat(x))
        assert len(items) >= 15 and len(set(items)) >= 5, (f.name, len(items))     # lists are not empty, the numbers not all equal
    by = {f.name: f.wanted("X") for f in fams}
    assert any(e > 1 for e, _, _ in by["uncertainty"]) and any(len(t_) > 1 for _, _, t_ in by["uncertainty"])
    assert any(a for a in by["annotate"][0]) and any(by["annotate"][1]) and len(by["annotate"][2][1]) >= 1
    assert len({w["count"] for w in by["nearest"]}) > 2 and any(w["n_at_cut"] for w in by["nearest"])
    assert any(w["count"] for w in by["relatives"][0]) and len({w["count"] for w in by["relatives"][1]}) > 1
    assert 0 < sum(by["select"][1]) < len(by["select"][1]) and len(set(by["select"][2])) > 2 and sum(by["select"][3]) >= 1
    assert any(by["mask"][1]) and not all(by["mask"][1]) and any(by["mask"][3])
    assert len(by["subtree"][0]["kept"]) > len(f_sels(fams)[0]) - 1 and by["subtree"][0]["pos"] and len(by["subtree"][2]) == 2
    assert by["genotypes"][0][0] >= 6 and by["genotypes"][0][1] >= 3 and any(any(r) for r in by["genotypes"][3])
    assert len(by["summary"][0]) > 20 and len(by["summary"][1]) >= 1 and any(r[2] for r in by["summary"][2])
    assert len(by["translate"][0]) > 50 and by["translate"][1]["n_inconsistent"] == 0 and by["translate"][1]["n_duplicate"] == 0
    assert len(by["haplotypes"][0]) > 20 and any(c > 1 for _, c, _ in by["haplotypes"][0]) and any(by["haplotypes"][1])


def f_sels(fams):
    return next(f for f in fams if f.name == "subtree").sels


@pytest.mark.parametrize("tree", TREES)
def test_other_arrays_change_the_answers(tree, capsys):
    """The table of which Y changes which family's answer, computed from the references and held against CHANGES."""
    t = S.trees()[tree]
    table = {f.name: {y: f.wanted(y) != f.wanted("X") for y in S.YS} for f in S.families(t)}
    with capsys.disabled():
        print("\n%-12s %s   (%s: does want(Y) differ from want(X)?)" % ("family", "  ".join("%-8s" % y for y in S.YS), tree))
        for name in S.NAMES:
            print("%-12s %s" % (name, "  ".join("%-8s" % ("yes" if table[name][y] else "-") for y in S.YS)))
    assert table == S.CHANGES[tree]
    for name in S.NAMES:
        if name in ("nearest", "relatives"):       # they read the counts per node alone
            assert table[name] == {"Y_pos": False, "Y_allele": False, "Y_move": True}, name
        else:
            assert table[name]["Y_allele"] or table[name]["Y_pos"], name
