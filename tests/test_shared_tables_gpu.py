"""Every device query after every other on one handle (the families of tests/shared_tables_cases.py): the depth-first tables, the
owners' nodes and the leaf ranks are built by whichever attach comes first and read by all the others, so each family must answer
its reference exactly in every order, and every attach must refuse mutation arrays other than the ones the tables came from and
leave the handle as it was.  tests/test_shared_tables_cpu.py shows that an accepted attach would change the answers."""
import pytest

from tests import shared_tables_cases as S
from usher_amd import UgpError

pytestmark = pytest.mark.gpu

TREES = ("plain", "bare")
TREE_AND_FAMILY = [(t, a) for t in TREES for a in range(len(S.NAMES))]
ids = lambda p: "%s-%s" % (p[0], S.NAMES[p[1]])


def answers(f, pl, why):
    got = f.ask(pl)
    assert got == f.wanted(), (f.tree.name, f.name, why)


def unattached(f, pl, why):
    """A run call of a family the handle never attached: -1, and the text names the attach that is missing."""
    assert f.call_unattached(pl) == -1 and ("ugp_%s_attach" % f.name).encode() in pl._L.ugp_last_error(), (f.name, why)


def refused(f, pl, y, why):
    with pytest.raises(UgpError) as e:
        f.attach(pl, f.tree.Y[y])
    assert e.value.code == -1 and "other mutation arrays" in str(e.value) and "ugp_%s_attach" % f.name in str(e.value), (f.name, y, why)


@pytest.mark.parametrize("case", TREE_AND_FAMILY, ids=ids)
def test_same_arrays_every_ordered_pair(case):
    t = S.trees()[case[0]]
    fams = S.families(t)
    A = fams[case[1]]
    for B in fams:
        if B is A:
            continue
        pl = t.handle()
        A.attach(pl, t.X)
        answers(A, pl, ("alone, before", B.name))
        B.attach(pl, t.X)
        answers(B, pl, ("after", A.name))
        answers(A, pl, ("again, after", B.name))
        pl.close()


@pytest.mark.parametrize("case", TREE_AND_FAMILY, ids=ids)
def test_rotations(case):
    """All eleven on one handle, beginning with each in turn; after every attach, every family attached so far.  The owners' nodes are
    made by select in the rotations that begin at uncertainty .. select, by translate in mask .. translate, by haplotypes in the last."""
    t = S.trees()[case[0]]
    fams = S.families(t)
    order = fams[case[1]:] + fams[:case[1]]
    pl = t.handle()
    for i, f in enumerate(order):
        f.attach(pl, t.X)
        for g in order[:i + 1]:
            answers(g, pl, ("rotation", [h.name for h in order[:i + 1]]))
    pl.close()


@pytest.mark.parametrize("case", TREE_AND_FAMILY, ids=ids)
def test_other_arrays_every_ordered_pair(case):
    t = S.trees()[case[0]]
    fams = S.families(t)
    A = fams[case[1]]
    for B in fams:
        if B is A:
            continue
        pl = t.handle()
        A.attach(pl, t.X)
        unattached(B, pl, "never attached")
        for y in S.YS:                       # B's first attach, with other arrays than the tables'
            refused(B, pl, y, ("first attach after", A.name))
            unattached(B, pl, ("after its refused attach", y))
        answers(A, pl, ("after the refused attaches of", B.name))
        B.attach(pl, t.X)
        for y in S.YS:                       # and a second attach of B, which would replace its state
            refused(B, pl, y, ("second attach after", A.name))
        answers(B, pl, ("after its refused second attaches",))
        answers(A, pl, ("at the end, beside", B.name))
        pl.close()


@pytest.mark.parametrize("tree", TREES)
def test_a_second_attach_with_the_same_arrays_replaces_the_first(tree):
    t = S.trees()[tree]
    for A in S.families(t):
        pl = t.handle()
        A.attach(pl, t.X)
        answers(A, pl, "first attach")
        A.attach(pl, dict(t.X))
        answers(A, pl, "second attach")
        for y in S.YS:
            refused(A, pl, y, "alone on the handle")
        answers(A, pl, "after the refusals")
        pl.close()
