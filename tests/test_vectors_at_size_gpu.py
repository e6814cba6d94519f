"""ugp_vectors on a SARS-CoV-2-shaped tree of a million nodes: 4,096 samples with missing rows and ambiguity codes, each at the node
Placer.place picks for it, exact against the literal mapper2_body of the oracle (orc_node_vecs); none is refused.  The test checks
its own inputs first, so that it cannot pass on empty lists."""
import numpy as np
import pytest

from oracle import capi
from tests import vectors_ref as VR
from usher_amd import Placer, QueryBatch
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def without_first_plain_row(q):
    """Every second sample loses its first row that is one base other than the reference: where that base came from the tree, the
    placement below it pays a back-mutation (part 3), which the generator's own samples hardly ever do."""
    keep = np.ones(len(q["pos"]), bool)
    plain = (q["is_missing"] == 0) & (q["nuc"] != q["ref"]) & ((q["nuc"] & (q["nuc"] - 1)) == 0)
    for i in range(0, len(q["ent_off"]) - 1, 2):
        b, e = int(q["ent_off"][i]), int(q["ent_off"][i + 1])
        hit = np.flatnonzero(plain[b:e])
        if len(hit):
            keep[b + hit[0]] = False
    off = np.concatenate([[0], np.cumsum(keep)])[q["ent_off"].astype(np.int64)].astype(np.uint64)
    return dict({k: q[k][keep] for k in ("pos", "ref", "nuc", "is_missing")}, ent_off=off, source=q["source"])


def test_a_million_nodes():
    st = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2")
    arrays = st.arrays
    q = st.queries(4096, seed=5, max_subst=4, n_lo=0, n_hi=6, iupac_hi=4)
    q = without_first_plain_row(q)
    batch = QueryBatch.from_csr(q["ent_off"], q["pos"], q["ref"], q["nuc"], q["is_missing"])
    pl = Placer(arrays)
    res = pl.place(batch)
    pl.vectors_attach()
    info, ex_off, ex, im_off, im = pl.vectors(batch, res["best_j"])
    ans = VR.device_answers(info, ex_off, ex, im_off, im)
    pl.close()
    assert not info["refused"].any() and info["eligible"].all()
    assert (info["set_difference"] == res["best_set_difference"]).all() and (info["has_unique"] == (res["best_has_unique"] != 0)).all()
    # the inputs are hard enough: entries of all three parts, imputed entries, winners deep in the tree
    assert int(info["n_branch"].sum()) > 100 and int(info["n_imputed"].sum()) > 100
    assert int((info["n_excess"] - info["n_branch"]).sum()) > 100 and len(set(res["best_j"].tolist())) > 1000
    ot = capi.OracleTree(arrays)
    back = 0
    for i, a in enumerate(ans):
        w = VR.oracle_answer(ot, gsynth.csr_sample(q, i), int(res["best_j"][i]))
        assert VR.agrees(a, w), (i, int(res["best_j"][i]), a, w)
        rows = set(int(p) for p in gsynth.csr_sample(q, i)["pos"])
        back += sum(1 for e in a["excess"][a["n_branch"]:] if e[0] not in rows)
    assert back > 0   # back-mutations (part 3) among them
