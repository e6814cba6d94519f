"""ugp_clade_alleles / ugp_clade_descendants / ugp_annotate_search (Placer.clade_alleles / clade_descendants / annotate_search)
against the restatements of tests/annotate_ref.py: the literal exemplar walk of parse_clade_names, is_ancestor counting, and the
oracle's literal mapper2_body over the depth-first expansion with best = 1e9 -- rows with repeated and masked positions included."""
import numpy as np
import pytest

from oracle import capi
from tests import annotate_ref as A
from tests.dense_cases import awkward_rows as _awkward_rows
from tests import stdorder
from tests import synth
from tests import uncertainty_ref as U
from usher_amd import Placer, QueryBatch, UgpError

pytestmark = pytest.mark.gpu


def _trees():
    yield synth.make_case(41, n_leaves=500, n_queries=1, n_sites=60, genome_len=400, p_masked=0.03)[0]
    yield synth.polytomy_case(42, fanouts=(8, 10, 6), n_queries=1, genome_len=3000, n_sites=200)[0]
    yield synth.caterpillar_case(43, depth=150, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=300)[0]


def _clades(arrays, rng, n_clades=25):
    n = arrays["n"]
    out = []
    for k in range(n_clades):
        if k % 3 == 0:   # exemplars below one chosen root, some from elsewhere
            root = int(rng.integers(0, n))
            below = [v for v in range(n) if root in U._root_path(arrays, v)]
            c = rng.choice(below, size=min(len(below), 20)).tolist() + rng.integers(0, n, size=2).tolist()
        else:
            c = rng.integers(0, n, size=int(rng.integers(1, 40))).tolist()
        c += c[:2]   # repeated exemplars count twice
        out.append(c)
    out.append([])   # an empty clade
    return out


@pytest.mark.parametrize("which", [0, 1, 2])
def test_alleles_and_descendants(which):
    arrays = list(_trees())[which]
    rng = np.random.default_rng(100 + which)
    clades = _clades(arrays, rng)
    pl = Placer(arrays)
    got = pl.clade_alleles(clades)
    assert len(got) == len(clades)
    for c, (ent, cnt) in zip(clades, got):
        assert dict(zip(ent.tolist(), cnt.tolist())) == A.alleles_literal(arrays, c)
    pc = rng.integers(0, len(clades), size=400)
    pn = rng.integers(0, arrays["n"], size=400)
    d = pl.clade_descendants(clades, pc, pn)
    assert d.tolist() == [A.descendants(arrays, clades[c], v) for c, v in zip(pc, pn)]
    pl.close()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_literal_search_on_awkward_rows(which, tmp_path):
    arrays = list(_trees())[which]
    rng = np.random.default_rng(200 + which)
    ot = capi.OracleTree(arrays)
    dfs = U.dfs_order(arrays)
    samples = [_awkward_rows(arrays, rng, k) for k in range(8)]
    # and the rows parse_clade_names builds, awkward or not
    so = stdorder.StdOrder(tmp_path)
    for c in _clades(arrays, rng, 6)[:6]:
        samples.append(A.clade_rows(arrays, c, so))
    assert sum(A.awkward(s) for s in samples) >= 8
    pl = Placer(arrays)
    assert pl.node_order("dfs").tolist() == dfs.tolist()
    best, ties, cnt = pl.annotate_search(QueryBatch(samples), cap=arrays["n"])
    for i, s in enumerate(samples):
        wb, wt = A.search(ot, arrays, s, dfs)
        assert (int(best[i]), ties[i].tolist(), int(cnt[i])) == (wb, wt, len(wt)), i
    # a small cap keeps the first ties and the true count
    b2, t2, c2 = pl.annotate_search(QueryBatch(samples[:3]), cap=2)
    assert [t.tolist() for t in t2] == [t.tolist()[:2] for t in ties[:3]] and c2.tolist() == cnt[:3].tolist()
    pl.close()


def test_literal_search_agrees_with_the_packed_search():
    """For rows the packed search takes, the literal path gives its scores and tie lists (depth-first order)."""
    arrays, queries = synth.make_case(44, n_leaves=400, n_queries=30, n_sites=60, genome_len=400)
    qs = [q for q in queries if not A.awkward(q) and not np.asarray(q["is_missing"]).any()]
    assert len(qs) >= 10
    pl = Placer(arrays)
    best, ties, cnt = pl.annotate_search(QueryBatch(qs), cap=arrays["n"])
    tj, _, tc = pl.tied_nodes_ex(QueryBatch(qs), cap=arrays["n"], order="dfs")
    res = pl.place_ex(QueryBatch(qs), order="dfs")
    for i in range(len(qs)):
        assert int(best[i]) == int(res[i]["best_set_difference"])
        assert ties[i].tolist() == sorted(tj[i].tolist()) and int(cnt[i]) == int(tc[i])
    pl.close()


def _repeat_a_position(arrays):
    """The arrays with one more entry on a branch: a second non-masked mutation at the position of the branch's first one,
    after its last (so no two entries at one position are adjacent)."""
    off = np.asarray(arrays["mut_off"], np.int64)
    pos = np.asarray(arrays["mut_pos"])
    j = next(v for v in range(1, arrays["n"]) if off[v + 1] - off[v] >= 2 and (pos[off[v]:off[v + 1]] >= 0).all())
    k, at = int(off[j]), int(off[j + 1])
    out = dict(arrays)
    for key in arrays:
        if key.startswith("mut_") and key != "mut_off":
            out[key] = np.insert(np.asarray(arrays[key]), at, np.asarray(arrays[key])[k])
    nuc, ref = int(arrays["mut_nuc"][k]), int(arrays["mut_ref"][k])
    out["mut_nuc"][at] = next(b for b in (1, 2, 4, 8) if b not in (nuc, ref))
    if "mut_par" in out:
        out["mut_par"][at] = nuc
    out["mut_off"] = (off + (np.arange(len(off)) > j)).astype(np.asarray(arrays["mut_off"]).dtype)
    return out


@pytest.mark.parametrize("annotate_first", [False, True])
def test_attach_with_two_mutations_at_one_position_on_one_branch(annotate_first):
    """Uncertainty and annotate share the handle's depth-first tables.  On a tree with two non-masked mutations at one position
    on one branch, both literal searches refuse it, and the clade walk still works, whichever attached first."""
    arrays = _repeat_a_position(synth.make_case(45, n_leaves=300, n_queries=1, n_sites=60, genome_len=400)[0])
    rng = np.random.default_rng(45)
    clades = _clades(arrays, rng, 6)
    rows = _awkward_rows(arrays, rng, 0)
    pl = Placer(arrays)

    def refused(call):
        with pytest.raises(UgpError) as e:
            call()
        assert e.value.code == -2   # UGP_ERR_UNSUPPORTED

    def alleles():
        for c, (ent, cnt) in zip(clades, pl.clade_alleles(clades)):
            assert dict(zip(ent.tolist(), cnt.tolist())) == A.alleles_literal(arrays, c)

    if annotate_first:
        alleles()
    refused(lambda: pl.uncertainty(np.array([1, 2])))
    alleles()
    refused(lambda: pl.annotate_search(QueryBatch([rows])))
    pl.close()
