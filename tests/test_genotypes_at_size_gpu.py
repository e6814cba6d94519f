"""Genotypes on a 1M-node synthetic MAT of the sars2 shape (a few huge polytomies): the site table of all leaves and the rows of
2,000 selected leaves against the numpy closed form of tests/genotypes_ref.py."""
import numpy as np
import pytest

from tests import genotypes_ref as R
from usher_amd import Placer
from usher_amd import synth as gsynth

pytestmark = pytest.mark.gpu


def test_genotypes_at_size():
    arrays = gsynth.SynthTree(1_000_000, n_sites=25000, seed=3, shape="sars2").arrays
    F = R.Fast(arrays)
    pl = Placer(arrays)
    want = F.run(None, rows=False, text=False)
    n_cols, n_sites = pl.genotype_select()
    assert (n_cols, n_sites) == (len(want.columns), len(want.sites)) and n_sites > 10_000
    assert R.device_sites(pl.genotype_sites()) == R.site_rows(want.sites)
    assert np.array_equal(pl.genotype_columns(), want.columns)
    leaves = F.dfs[np.flatnonzero(F.leaf[F.dfs])]
    sel = np.random.default_rng(23).choice(leaves, 2000, replace=False)
    want = F.run(sel, text=False)
    assert pl.genotype_select(sel) == (2000, len(want.sites))
    assert R.device_sites(pl.genotype_sites()) == R.site_rows(want.sites)
    assert np.array_equal(pl.genotype_rows(), want.codes)
    assert np.array_equal(pl.genotype_rows(100, 900, chunk_cells=64_000), want.codes[100:900])
    pl.close()
