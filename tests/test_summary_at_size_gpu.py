"""matUtils summary on a 1M-node synthetic MAT of the sars2 shape (a few huge polytomies) against the numpy restatement of
tests/summary_ref.py, exactly, for all three calls.  The tree yields 63,369 RoHo records and 2,815 erased candidates."""
import numpy as np
import pytest

from tests import summary_ref as R
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_summary_at_size():
    arrays = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2").arrays
    F = R.Fast(arrays)
    want, erased = F.roho()
    assert len(want) > 0 and erased > 0, (len(want), erased)
    assert (len(want), erased) == (63369, 2815)
    pl = Placer(arrays)
    m = pl.summary_mutations()
    assert list(zip(m["pos"].tolist(), m["par"].tolist(), m["nuc"].tolist(), m["count"].tolist())) == F.mutations()
    recs = pl.summary_roho()
    assert len(recs) == len(want)
    pre = F.pre[recs["parent"].astype(np.int64)]
    assert (np.diff(pre) >= 0).all()
    assert R.device_roho_fast(F, recs) == want
    assert R.device_roho_fast(F, pl.summary_roho(chunk_items=100_003)) == want
    rng = np.random.default_rng(5)
    cols = [np.sort(rng.choice(np.flatnonzero(~F.leaf), 1500, replace=False)), np.sort(rng.choice(arrays["n"], 800, replace=False))]
    per, leaf_clade = pl.summary_clades(cols)
    at = 0
    for c, (incl, excl, near) in enumerate(F.clades(cols)):
        rows = per[at:at + len(cols[c])]
        at += len(cols[c])
        assert np.array_equal(rows["inclusive"], incl) and np.array_equal(rows["exclusive"], excl)
        assert np.array_equal(leaf_clade[c].astype(np.int64), near) and (near != R.NONE).sum() > 1000
    pl.close()
