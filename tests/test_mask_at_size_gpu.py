"""The mask calls on a SARS-CoV-2-shaped tree of a million nodes against the closed forms of tests/mask_ref.py (held against the
literal restatement on every small tree by tests/test_mask_cpu.py), and on a star of more leaves than one scan segment of bitmap
words holds.  The tests check their own inputs first, so that they cannot pass on easy questions."""
import numpy as np
import pytest

from tests import mask_ref as R
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def topology(arrays):
    """The same tree without mutations, for the handle: the mask tables take the mutations as they are stored."""
    n = int(arrays["n"])
    return {"n": n, "parent": arrays["parent"], "mut_off": np.zeros(n + 1, np.int64), "mut_pos": np.zeros(0, np.int32),
            "mut_ref": np.zeros(0, np.int8), "mut_par": np.zeros(0, np.int8), "mut_nuc": np.zeros(0, np.int8)}


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_million_nodes():
    st = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2")
    arrays = st.arrays
    n = int(arrays["n"])
    F = R.Fast(arrays)
    rng = np.random.default_rng(29)
    leaves = np.flatnonzero(F.leaf)
    # every leaf of a clade of more than 100 leaves, and 1,000 drawn leaves
    nl = F.lpre[F.pre + F.size] - F.lpre[F.pre]
    clade = int(np.flatnonzero((nl > 100) & (nl < 5000) & F.hasleaf)[0])
    lo, hi = F.pre[clade], F.pre[clade] + F.size[clade]
    under = leaves[(F.pre[leaves] >= lo) & (F.pre[leaves] < hi)]
    named = np.concatenate([under, rng.choice(leaves, 1000, replace=False), under[:3]]).astype(np.uint32)
    roots, masked = F.restricted(named)
    live = int((F.pos >= 0).sum())
    assert clade in roots.tolist() and len(under) > 100                       # an inner root with more than 100 leaves
    assert F.leaf[roots].sum() > 500                                           # leaves that are their own root
    assert 0 < masked.sum() < live and masked[np.isin(F.node, under)].any() and not masked[np.isin(F.node, under)].all()
    # the lines
    per_pos = np.bincount(F.pos[F.pos >= 0])
    most = int(per_pos.argmax())
    absent = int(np.flatnonzero(per_pos[1:] == 0)[0]) + 1
    k = int(np.flatnonzero(F.pos == most)[0])
    a, b = int(F.mpar[k]), int(F.mnuc[k])
    big = int(np.flatnonzero((nl > 20000) & (nl < 200000))[0])                 # a branch with an entry of `most` well inside it
    inside = F.node[(F.pos == most) & (F.pre[F.node] > F.pre[big]) & (F.pre[F.node] < F.pre[big] + F.size[big])]
    assert len(inside) > 3
    x = int(F.par[int(inside[len(inside) // 2])]) if F.par[int(inside[len(inside) // 2])] != big else int(inside[len(inside) // 2])
    lines = [(most, 15, 15, big, [x, big, 0, n + 7]),       # a branch line whose exclusion holds entries it would match
             (most, a, b, 0, []),                            # the position with the most entries, tree-wide
             (most, 15, b, 0, []), (most, a, 15, 0, []),    # wildcards
             (absent, 15, 15, 0, []), (int(len(per_pos)) + 3, 1, 2, 0, []), (-1, 15, 15, 0, []),
             (most, a, b, 0, []),                            # a line again: nothing is left for it
             (most, 15, 15, 0, []),
             (int(F.pos[np.flatnonzero(masked)[0]]), 15, 15, 0, [])]   # an entry that -s masks: there without skip, gone with it
    for p in rng.choice(F.pos[F.pos >= 0], 40):
        t = int(rng.integers(0, n))
        lines.append((int(p), 15, int(rng.choice([1, 2, 4, 8, 15])), t if F.size[t] > 1 else 0, [int(v) for v in rng.integers(0, n, 2)]))
    first, counts = F.mutations(lines)
    assert per_pos[most] > 100 and counts[1] > 50 and counts[7] == 0 and counts[4] == counts[5] == counts[6] == 0
    assert counts[0] > 0 and F.mutations([lines[0][:4] + ([],)])[1][0] > counts[0]   # the exclusion takes entries away
    assert counts[8] > 0 and (first == R.NIL).sum() > 0 and counts.sum() == (first != R.NIL).sum()
    skipped = F.mutations(lines, masked)
    assert not same(skipped, (first, counts))
    pl = Placer(topology(arrays))
    pl.mask_attach(arrays)
    assert same(pl.mask_restricted(named), (roots, masked)) and pl._msk_n_masked == int(masked.sum())
    assert same(pl.mask_mutations(*_columns(lines)), (first, counts))
    assert same(pl.mask_mutations(*_columns(lines), skip=masked), skipped)
    assert same(pl.mask_mutations(*_columns(lines), chunk_lines=7), (first, counts))
    t_r, t_m = pl.mask_time(named, *_columns(lines), reps=2)
    assert t_r > 0 and t_m > 0
    pl.close()


def _columns(lines):
    return [l[0] for l in lines], [l[1] for l in lines], [l[2] for l in lines], [l[3] for l in lines], [l[4] for l in lines]


def test_more_leaves_than_one_segment_of_words():
    """A star of 1,100,000 leaves: the bitmap has more than kSeg = 16,384 words, so the named counts in front of a word cross a
    segment of the word scan; the named ranks end a few bits on either side of word 16,384."""
    n_leaves, edge = 1_100_000, 16384 * 64
    n = n_leaves + 3
    parent = np.zeros(n, np.int64)
    parent[0] = -1
    parent[3:] = 1                                   # node 1 holds the star, node 2 is a lone leaf
    # an entry on every 1,000th leaf, alternating between a key that also sits on the lone leaf and a private one
    owners = np.arange(3, n, 1000)
    nodes = np.concatenate([[2], owners])
    pos = np.concatenate([[5], np.where(np.arange(len(owners)) % 2 == 0, 5, 6)]).astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    off[nodes + 1] = 1
    off = np.cumsum(off)
    m = len(nodes)
    arrays = {"n": n, "parent": parent, "mut_off": off, "mut_pos": pos, "mut_ref": np.full(m, 1, np.int8), "mut_par": np.full(m, 1, np.int8),
              "mut_nuc": np.full(m, 2, np.int8)}
    F = R.Fast(arrays)
    assert F.n_leaves == n_leaves + 1 and (F.n_leaves + 64) // 64 > 16384
    pl = Placer(topology(arrays))
    pl.mask_attach(arrays)
    star = np.arange(3, n)
    for named in (star, star[: edge - 1], star[: edge + 1], star[edge - 70:], np.concatenate([star[:5], star[edge - 1: edge + 2]])):
        want = F.restricted(named)
        assert same(pl.mask_restricted(named.astype(np.uint32)), want)
    roots, masked = F.restricted(star)
    assert roots.tolist() == [1] and masked.sum() == (pos[1:] == 6).sum() > 100
    assert len(F.restricted(star[: edge + 1])[0]) == edge + 1
    pl.close()
