"""The two restatements of make_vcf in tests/genotypes_ref.py against each other on every case of tests/genotypes_cases.py, a
five-node tree against a VCF written out by hand, and the survey tree against the VCF the reference wrote for it."""
import gzip
import os

import numpy as np
import pytest

from tests import genotypes_cases as GC
from tests import genotypes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB = os.path.join(ROOT, "tests", "golden", "survey_ref", "global", "global_assignments.pb")
VCF = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "global_samples.vcf.gz")


@pytest.mark.parametrize("case", GC.all_cases(), ids=lambda c: c[0])
def test_literal_equals_fast(case):
    name, arrays, selections, _ = case
    F = R.Fast(arrays)
    for sel in selections:
        want = R.literal(arrays, sel)
        got = F.run(sel)
        assert got.sites == want.sites, name
        assert np.array_equal(got.codes, want.codes), name
        assert got.text == want.text, name
        assert np.array_equal(got.columns, want.columns), name
        assert F.run(sel, rows=False, genotypes=False).text == R.literal(arrays, sel, genotypes=False).text


def test_cases_reach_their_edges():
    by = {c[0]: c for c in GC.all_cases()}
    r = R.fast(by["ambiguous"][1], list(range(14)))
    assert [len(s["alt"]) for s in r.sites] == [12, 1] and r.sites[0]["alt"] == list(range(2, 13)) + [15] and r.codes.max() == 12
    assert len(R.fast(by["ambiguous"][1]).sites[0]["alt"]) == 11
    assert R.fast(by["no_mutation"][1]).sites == [] and R.fast(by["all_masked"][1]).sites == []
    r = R.fast(by["caterpillar"][1])
    assert 5001 not in [s["pos"] for s in r.sites]
    s = [s for s in r.sites if s["pos"] == 5000][0]
    assert s["ref"] == 1 and s["alt"] == [2] and s["covered"] == 150 and s["ac"] == [75]
    (_, arrays, sels, _), ids = GC.segment_case()
    inside = R.fast(arrays, sels[1]).sites
    outside = R.fast(arrays, sels[2]).sites
    assert [s["ref"] for s in inside if s["pos"] == 9] == [1] and [s["ref"] for s in outside if s["pos"] == 9] == [8]
    r = R.fast(by["two_entries"][1])
    assert R.site_rows(r.sites)[0] == (10, 4, (1, 8), (1, 1), 4)   # REF G from the first entry; n1 = T, n9 / n10 = G, n6 = A
    assert len(R.fast(GC.seven_sites()).sites) == 7


def test_five_nodes_by_hand():
    assert R.literal(GC.FIVE).text == GC.FIVE_VCF
    assert R.fast(GC.FIVE).text == GC.FIVE_VCF
    assert R.literal(GC.FIVE, genotypes=False).text == "".join(l.split("\tGT")[0].split("\tFORMAT")[0] + "\n" for l in GC.FIVE_VCF.splitlines())


def test_survey_tree_against_the_reference_vcf():
    """The restatement on the survey tree, all leaves, against the VCF the reference wrote for the same samples: no cell with one
    unambiguous base disagrees (178,506 cells)."""
    from oracle import refio
    from tests import usher_model as UM
    T = refio.load_mutation_annotated_tree(PB)
    UM.uncondense_leaves(T)
    arrays = refio.tree_to_bfs_arrays(T)
    cells, bad = R.compare_with_vcf(VCF, R.fast(arrays), arrays["names"])
    assert cells > 100_000 and bad == 0, (cells, bad)
