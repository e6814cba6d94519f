"""ugp_genotype_select / _columns / _sites / _rows (Placer.genotype_*) against tests/genotypes_ref.py: every field of every site and
every code exact against the closed form, every 97th site against the literal walk too, on the cases of tests/genotypes_cases.py;
row windows, a second select on one handle, the survey tree against the reference's own VCF, and the error codes."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import refio
from tests import genotypes_cases as GC
from tests import genotypes_ref as R
from tests import usher_model as UM
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_ = 1


def _placer(arrays, plain=True):
    """plain: the arrays are the handle's tree.  Otherwise (ambiguous alleles, two mutations of a node at one position: trees the
    placement tables refuse) the handle takes the bare topology and the genotype tables the mutations."""
    pl = Placer(arrays if plain else GC.topology(arrays))
    pl.genotypes_attach(arrays)
    return pl


def _check(pl, F, sel, literal=True, **kw):
    want = F.run(sel, text=False)
    n_cols, n_sites = pl.genotype_select(sel)
    assert (n_cols, n_sites) == (len(want.columns), len(want.sites))
    assert np.array_equal(pl.genotype_columns(), want.columns)
    assert R.device_sites(pl.genotype_sites()) == R.site_rows(want.sites)
    codes = pl.genotype_rows(**kw)
    assert codes.shape == want.codes.shape and np.array_equal(codes, want.codes)
    if literal and n_sites:
        lit = R.literal(F.arrays, sel)
        pick = list(range(0, n_sites, 97))
        assert [R.site_rows(lit.sites)[s] for s in pick] == [R.device_sites(pl.genotype_sites())[s] for s in pick]
        assert np.array_equal(lit.codes[pick], codes[pick])
    return want


@pytest.mark.parametrize("case", GC.all_cases(), ids=lambda c: c[0])
def test_cases(case):
    name, arrays, selections, plain = case
    F = R.Fast(arrays)
    pl = _placer(arrays, plain)
    for sel in selections:   # one handle: every select replaces the one before
        _check(pl, F, sel)
    pl.close()


def test_row_windows_and_chunks():
    arrays = GC.seven_sites()
    F = R.Fast(arrays)
    pl = _placer(arrays)
    want = _check(pl, F, None)
    assert len(want.sites) == 7
    for lo in range(8):
        for hi in range(lo, 8):
            assert np.array_equal(pl.genotype_rows(lo, hi), want.codes[lo:hi]), (lo, hi)
    pl.close()
    arrays = GC.random_cases()[1][1]
    F = R.Fast(arrays)
    pl = _placer(arrays)
    for sel in (None, np.arange(0, arrays["n"], 3)):
        want = F.run(sel, text=False)
        n_cols, n_sites = pl.genotype_select(sel)
        assert n_cols > 40 and n_cols % 16 != 0 and n_sites > 20
        for cells in (1, n_cols - 1, n_cols + 1, 0, 17, 3 * n_cols + 5):
            assert np.array_equal(pl.genotype_rows(chunk_cells=cells), want.codes), cells
            assert np.array_equal(pl.genotype_rows(3, n_sites - 2, chunk_cells=cells), want.codes[3:n_sites - 2]), cells
    pl.close()


def test_reselect_replaces_the_selection():
    arrays = GC.random_cases()[0][1]
    F = R.Fast(arrays)
    pl = _placer(arrays)
    lv = GC.leaves_of(arrays)
    a = _check(pl, F, lv[:40])
    b = _check(pl, F, np.arange(arrays["n"]))
    c = _check(pl, F, lv[:40])
    assert len(b.sites) > len(a.sites) and R.site_rows(a.sites) == R.site_rows(c.sites)
    pl.close()


def test_attach_takes_the_arrays_of_the_handles_tables():
    """The depth-first tables are the handle's, built by its first dense attach: a genotypes attach with other mutation arrays --
    more entries, fewer, or as many with other contents -- is refused and leaves the handle as it was."""
    arrays = GC.seven_sites()
    more = GC.with_entries(arrays, {5: [(21, A_, A_, 2)], 8: [(3, A_, A_, 8)]})
    fewer = GC.hand(GC.HAND, {1: [(3, 1, 1, 2)]})
    same_count = dict(arrays)
    same_count["mut_pos"] = np.where(arrays["mut_pos"] == 15, 16, arrays["mut_pos"]).astype(np.int32)
    other_allele = dict(arrays)
    other_allele["mut_nuc"] = np.where(arrays["mut_nuc"] == 8, 4, arrays["mut_nuc"]).astype(np.int8)
    F = R.Fast(arrays)
    # after nearest_k built the tables from the placer's own arrays
    pl = Placer(arrays)
    pl.nearest_k([9], 2)
    for other in (more, fewer, same_count, other_allele, GC.topology(arrays)):
        with pytest.raises(UgpError) as e:
            pl.genotypes_attach(other)
        assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    with pytest.raises(UgpError):
        pl.genotype_rows()          # no state was made
    pl.genotypes_attach(arrays)     # the same arrays, given again
    _check(pl, F, None)
    # a second genotypes attach: other arrays refused, the first state still answers; the same arrays replace it
    for other in (more, fewer, same_count):
        with pytest.raises(UgpError) as e:
            pl.genotypes_attach(other)
        assert e.value.code == -1
    assert np.array_equal(pl.genotype_rows(), F.run(None, text=False).codes)
    pl.genotypes_attach()
    _check(pl, F, [9, 10, 11, 6])
    pl.close()
    # a handle of the bare topology takes whichever arrays come first, and only those
    pl = Placer(GC.topology(arrays))
    pl.genotypes_attach(more)
    _check(pl, R.Fast(more), None)
    with pytest.raises(UgpError):
        pl.genotypes_attach(arrays)
    _check(pl, R.Fast(more), [1, 5, 8])
    pl.close()


def test_survey_tree_against_the_reference_vcf():
    T = refio.load_mutation_annotated_tree(os.path.join(ROOT, "tests", "golden", "survey_ref", "global", "global_assignments.pb"))
    UM.uncondense_leaves(T)
    arrays = refio.tree_to_bfs_arrays(T)
    pl = _placer(arrays)
    pl.genotype_select()
    got = R.Result(R.sites_from_device(pl.genotype_sites()), pl.genotype_rows(), None, pl.genotype_columns())
    pl.close()
    cells, bad = R.compare_with_vcf(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "global_samples.vcf.gz"), got, arrays["names"])
    assert cells > 100_000 and bad == 0, (cells, bad)


def test_error_codes_leave_the_output_untouched():
    arrays = GC.seven_sites()
    pl = Placer(arrays)
    L, h = pl._L, pl._h
    codes = np.full(7 * 12, 0xA5, np.uint8)
    tab = np.full(7, 0x5A, np.uint8).repeat(Placer.GT_SITE.itemsize).view(Placer.GT_SITE)
    cols = np.full(12, 0xABCDEF01, np.uint32)
    nc, ns = C.c_uint32(77), C.c_uint64(77)
    # before the attach, then before a select: the text names the missing call
    assert L.ugp_genotype_select(h, None, 0, C.byref(nc), C.byref(ns)) == -1 and b"ugp_genotypes_attach" in L.ugp_last_error()
    assert L.ugp_genotype_rows(h, 0, 0, _ptr(codes)) == -1 and b"ugp_genotypes_attach" in L.ugp_last_error()
    pl.genotypes_attach()
    assert L.ugp_genotype_rows(h, 0, 0, _ptr(codes)) == -1 and b"ugp_genotype_select" in L.ugp_last_error()
    assert L.ugp_genotype_sites(h, 0, 0, _ptr(tab)) == -1 and b"ugp_genotype_select" in L.ugp_last_error()
    assert L.ugp_genotype_columns(h, _ptr(cols)) == -1 and b"ugp_genotype_select" in L.ugp_last_error()
    with pytest.raises(UgpError):
        pl.genotype_rows()
    bad = np.array([3, 12, 5], np.uint32)
    assert L.ugp_genotype_select(h, _ptr(bad), 3, C.byref(nc), C.byref(ns)) == -1 and (nc.value, ns.value) == (77, 77)
    n = len(R.fast(arrays, [9, 10, 11]).sites)
    assert pl.genotype_select([9, 10, 11]) == (3, n) and 0 < n < 7
    assert L.ugp_genotype_select(h, _ptr(bad), 3, C.byref(nc), C.byref(ns)) == -1
    for lo, hi in ((3, 2), (0, n + 1), (n + 1, n + 1)):
        assert L.ugp_genotype_rows(h, lo, hi, _ptr(codes)) == -1 and L.ugp_genotype_sites(h, lo, hi, _ptr(tab)) == -1, (lo, hi)
    assert (codes == 0xA5).all() and (tab.view(np.uint8) == 0x5A).all() and (cols == 0xABCDEF01).all()
    pl.close()
    # a tree without mut_par values in 1 .. 15 is refused
    arrays = dict(GC.seven_sites())
    arrays["mut_par"] = np.zeros_like(arrays["mut_par"])
    pl = Placer(arrays)
    with pytest.raises(UgpError) as e:
        pl.genotype_select()
    assert e.value.code == -2
    pl.close()
