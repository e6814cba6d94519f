"""The checks an attach makes of its own, behind the ones every attach shares (ugp_query.hpp: query_attach): mut_par missing for
genotypes, summary, translate and vectors; an allele of 16 for mask, subtree and vectors; a name_rank that repeats a value for
relatives.  Each is refused with its code after a good attach of the same family, which then still answers its reference exactly, as
does a second family attached earlier on the handle; and refused as the first attach of a handle, which then takes the good one.
The trees, questions and references are those of tests/shared_tables_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import shared_tables_cases as S
from usher_amd import UgpError, _lib
from usher_amd.placement import _TreeArrays, _ptr

pytestmark = pytest.mark.gpu

TREES = ("plain", "bare")
INVALID, UNSUPPORTED = -1, -2


def without_mut_par(f, pl):
    """The family's attach with the arrays of X and no mut_par; the return code."""
    t = _TreeArrays(f.tree.X)
    desc = _lib.ugp_tree_desc(t.n, _ptr(t.parent), _ptr(t.mut_off), _ptr(t.mut_pos), _ptr(t.mut_ref), None, _ptr(t.mut_nuc))
    rc = getattr(pl._L, "ugp_%s_attach" % f.name)(pl._h, C.byref(desc))
    return rc, (pl._L.ugp_last_error() or b"").decode()


def with_allele_16(f, pl):
    """The family's attach with X whose stored parent allele of one entry is 16: the shared checks do not read mut_par."""
    y = dict(f.tree.X)
    par = np.asarray(f.tree.X["mut_par"]).copy()
    par[f.tree.allele_entry] = 16
    y["mut_par"] = par
    with pytest.raises(UgpError) as e:
        f.attach(pl, y)
    return e.value.code, str(e.value)


def with_a_rank_twice(f, pl):
    rank = f.rank.copy()
    rank[1] = rank[0]
    with pytest.raises(UgpError) as e:
        pl.relatives_attach(rank, f.tree.X)
    return e.value.code, str(e.value)


CHECKS = [("genotypes", without_mut_par, INVALID, "mut_par"), ("summary", without_mut_par, INVALID, "mut_par"),
          ("translate", without_mut_par, INVALID, "mut_par"), ("vectors", without_mut_par, INVALID, "mut_par"),
          ("mask", with_allele_16, UNSUPPORTED, "an allele above 15"), ("subtree", with_allele_16, UNSUPPORTED, "an allele above 15"),
          ("vectors", with_allele_16, UNSUPPORTED, "not a 4-bit code"), ("relatives", with_a_rank_twice, INVALID, "not a permutation")]
ids = lambda c: "%s-%s" % (c[0], c[1].__name__) if isinstance(c, tuple) else c


def refused(f, pl, check, why):
    _, bad_attach, code, text = check
    got, msg = bad_attach(f, pl)
    assert got == code and text in msg, (f.name, why, got, msg)


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("check", CHECKS, ids=ids)
def test_refused_after_a_good_attach(check, tree):
    t = S.trees()[tree]
    A = S.family(t, check[0])
    B = S.family(t, "select" if check[0] != "select" else "uncertainty")
    pl = t.handle()
    B.attach(pl, t.X)
    A.attach(pl, t.X)
    A.check(pl, "before the refusal")
    refused(A, pl, check, "second attach")
    A.check(pl, "after its refused attach")
    B.check(pl, ("attached earlier, after the refused attach of", A.name))
    pl.close()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("check", CHECKS, ids=ids)
def test_refused_as_the_first_attach_of_a_handle(check, tree):
    t = S.trees()[tree]
    A = S.family(t, check[0])
    pl = t.handle()
    refused(A, pl, check, "first attach of the handle")
    A.attach(pl, t.X)
    A.check(pl, "after its refused first attach")
    pl.close()
