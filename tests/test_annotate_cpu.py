"""The annotate restatements (tests/annotate_ref.py) on hand-built trees, and the closed form of the clade allele counts
 against the literal exemplar walk of parse_clade_names on random trees.  No GPU."""
import numpy as np
import pytest

from tests import annotate_ref as A
from tests import stdorder
from tests import synth

A_, C_, G_, T_ = 1, 2, 4, 8


def hand_tree(nodes):
    """nodes[j] = (parent, [(pos, ref, nuc), ...]) in BFS order, root first with parent -1."""
    off = np.zeros(len(nodes) + 1, np.int64)
    pos, ref, nuc = [], [], []
    for j, (_, muts) in enumerate(nodes):
        for p, r, m in muts:
            pos.append(p); ref.append(r); nuc.append(m)
        off[j + 1] = len(pos)
    return {"n": len(nodes), "parent": np.asarray([p for p, _ in nodes], np.int64), "mut_off": off,
            "mut_pos": np.asarray(pos, np.int32), "mut_ref": np.asarray(ref, np.int8), "mut_par": np.asarray(ref, np.int8),
            "mut_nuc": np.asarray(nuc, np.int8), "names": ["n%d" % j for j in range(len(nodes))]}


# 0 root
# 1 <- 0: 10 A>G, 20 C>T                  2 <- 0: 30 G>A
# 3 <- 1: 10 G>T (newer at 10), 10 G>C (same node, same position: skipped), -5 masked
# 4 <- 1: 20 T>C (reversion to the reference base: blocks 20 C>T, counts nothing)
# 5 <- 3: leaf               6 <- 3: 40 A>C
HAND = hand_tree([
    (-1, []),
    (0, [(10, A_, G_), (20, C_, T_)]),
    (0, [(30, G_, A_)]),
    (1, [(10, A_, T_), (10, A_, C_), (-5, T_, 15)]),
    (1, [(20, C_, C_)]),
    (3, []),
    (3, [(40, A_, C_)]),
])


def test_walk_takes_the_newest_entry_per_position():
    # exemplar 5: node 3's 10 A>T wins over node 1's 10 A>G; node 3's second entry at 10 is skipped; masked always taken
    assert A.walk_entries(HAND, 5) == [3, 5, 1]
    assert A.walk_entries(HAND, 4) == [6, 0]          # 20 reverted at node 4 blocks node 1's 20 C>T
    assert A.alleles_literal(HAND, [4]) == {0: 1}     # the reversion itself counts nothing


def test_repeated_exemplars_count_twice():
    got = A.alleles_literal(HAND, [5, 5, 6, 4])
    assert got == {3: 3, 5: 3, 1: 3, 7: 1, 0: 1}
    assert A.alleles_closed(HAND, [5, 5, 6, 4]) == got


def test_descendants_exclude_the_node_itself():
    assert A.descendants(HAND, [5, 6, 3, 3], 3) == 2
    assert A.descendants(HAND, [5, 6, 3, 3], 1) == 4
    assert A.descendants(HAND, [5, 6, 3, 3], 5) == 0


def test_rows_keep_repeated_and_masked_positions(tmp_path):
    so = stdorder.StdOrder(tmp_path)
    # 5 of 8 exemplars carry 10 A>T, 3 carry 10 A>G: one T row at 0.625 < 0.8 -> N, one G row at 0.375 -> N
    clade = [5] * 5 + [4] * 3
    rows = A.clade_rows(HAND, clade, so)
    assert [(int(p), int(r), int(m)) for p, r, m in zip(rows["pos"], rows["ref"], rows["nuc"])] == \
        [(-5, T_, 15), (10, A_, 15), (10, A_, 15), (20, C_, 15)]
    assert A.awkward(rows)
    clean = A.clade_rows(HAND, [2, 2], so)
    assert [(int(p), int(m)) for p, m in zip(clean["pos"], clean["nuc"])] == [(30, A_)]
    assert not A.awkward(clean)


@pytest.mark.parametrize("seed,p_masked", [(11, 0.0), (12, 0.05), (13, 0.0)])
def test_closed_form_equals_the_walk(seed, p_masked):
    arrays, _ = synth.make_case(seed, n_leaves=150, n_queries=1, n_sites=25, genome_len=200, p_masked=p_masked,
                                mut_counts=(0, 1, 1, 2, 3, 4))
    rng = np.random.default_rng(seed)
    n = arrays["n"]
    for _ in range(20):
        clade = rng.integers(0, n, size=int(rng.integers(1, 30))).tolist()
        clade += clade[:3]   # repeats
        assert A.alleles_closed(arrays, clade) == A.alleles_literal(arrays, clade)


def test_caterpillar_closed_form():
    arrays, _ = synth.caterpillar_case(3, depth=60, muts_per_node=2, n_queries=1, genome_len=300, n_sites=20)
    rng = np.random.default_rng(3)
    for _ in range(10):
        clade = rng.integers(0, arrays["n"], size=12).tolist()
        assert A.alleles_closed(arrays, clade) == A.alleles_literal(arrays, clade)
