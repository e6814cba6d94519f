"""ugp_translate on a synthetic tree of about 2^17 nodes (tests/synth.py: stored parent alleles are the true states, so the closed
form holds) against the fast restatement of tests/translate_ref.py, exactly.  The genes: three on the + strand, one of them in two
CDS lines, one in another frame over the first."""
import numpy as np
import pytest

from tests import summary_ref as SR
from tests import synth
from tests import translate_cases as TC
from tests import translate_ref as R
from usher_amd import Placer

pytestmark = pytest.mark.gpu


def test_translate_at_size():
    arrays = synth.make_case(17, n_leaves=85000, n_queries=1, n_sites=3000, genome_len=6000)[0]
    assert 120_000 < arrays["n"] < 140_000
    pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
    genome = np.array(list("ACGT"))[np.random.default_rng(1).integers(0, 4, 6000)]
    genome[pos - 1] = np.array(list(SR.NUC))[np.asarray(arrays["mut_ref"]).astype(np.int64)]
    gtf = "\n".join([TC.gtf_line("a", 1, 2400), TC.gtf_line("b", 2500, 3000), TC.gtf_line("b", 3100, 3999), TC.gtf_line("c", 2302, 2700),
                     TC.gtf_line("e", 5002, 6000)]) + "\n"
    slot_pos, slot_init = R.slot_tables(R.build_codon_map(gtf, "".join(genome)))
    F = R.Fast(arrays, slot_pos, slot_init)
    assert F.info["n_inconsistent"] == 0 and F.info["n_duplicate"] == 0 and F.info["n_records"] > 100_000
    assert sum(1 for r in F.records if sum(e != R.NIL for e in r[4]) > 1) > 10          # several mutations of a node in one codon
    pl = Placer(arrays)
    pl.translate_codons(slot_pos, slot_init)
    for w in (0, 50_021):
        recs, info = pl.translate(chunk_items=w)
        assert {k: int(info[k]) for k in info.dtype.names} == F.info, w
        assert recs["node"].tolist() == [r[0] for r in F.records] and recs["codon"].tolist() == [r[1] for r in F.records], w
        assert recs["before"].tobytes().decode() == "".join(r[2] for r in F.records), w
        assert recs["after"].tobytes().decode() == "".join(r[3] for r in F.records), w
        assert recs["ent"].tolist() == [list(r[4]) for r in F.records], w
    pl.close()
