"""The ten Placer.*_time bench hooks, which all run their stages through one timer (ugp_query.hpp: timed, EventPair): every one
returns finite times >= 0 for reps = 1 and 3, refuses reps = 0 with -1, names the missing attach on a handle that never attached its
family, and leaves the family answering its reference exactly.  The trees, questions and references are those of
tests/shared_tables_cases.py."""
import ctypes as C
import math

import pytest

from tests import shared_tables_cases as S
from usher_amd import QueryBatch, UgpError

pytestmark = pytest.mark.gpu

TREES = ("plain", "bare")


class Hook:
    """One timing wrapper: the family whose attach it needs, time(pl, f, reps) through the wrapper, and bare(pl, *doubles): the C call
    with reps = 1 and no arrays, for a handle whose Python wrapper would attach by itself."""

    def __init__(self, name, family, time, bare, n_out, prepare=None):
        self.name, self.family, self.time, self.bare, self.n_out, self.prepare = name, family, time, bare, n_out, prepare


def _vec(t):
    queries, pairs, _ = S.vectors_asked(t)
    return QueryBatch(queries), [j for _, j in pairs], [s for s, _ in pairs]


def _vectors_bare(pl, a, b):
    q = QueryBatch([])
    return pl._L.ugp_vectors_time(pl._h, C.byref(q.desc), 0, None, None, 1, a, b)


HOOKS = [
    Hook("genotype_rows", "genotypes", lambda pl, f, r: pl.genotype_rows_time(reps=r),
         lambda pl, a: pl._L.ugp_genotype_rows_time(pl._h, 0, 0, 1, a), 1,
         prepare=lambda pl, f: pl.genotype_select(f.tree.nodes + f.tree.some_leaves)),
    Hook("summary", "summary", lambda pl, f, r: pl.summary_time(reps=r), lambda pl, a, b: pl._L.ugp_summary_time(pl._h, 1, a, b), 2),
    Hook("translate", "translate", lambda pl, f, r: pl.translate_time(reps=r), lambda pl, a: pl._L.ugp_translate_time(pl._h, 1, a), 1),
    Hook("relatives_closest", "relatives", lambda pl, f, r: pl.relatives_time(f.tree.nodes, reps=r),
         lambda pl, a, b: pl._L.ugp_relatives_time(pl._h, 0, None, 0, 0, 1, a, b), 2),
    Hook("relatives_within", "relatives", lambda pl, f, r: pl.relatives_time(f.tree.nodes, within=True, threshold=3, reps=r),
         lambda pl, a, b: pl._L.ugp_relatives_time(pl._h, 0, None, 1, 3, 1, a, b), 2),
    Hook("select", "select", lambda pl, f, r: pl.select_time(f.qpos, f.qnuc, reps=r),
         lambda pl, a: pl._L.ugp_select_time(pl._h, 0, None, None, 1, a), 1),
    Hook("mask", "mask", lambda pl, f, r: pl.mask_time(f.named, *[[l[i] for l in f.lines] for i in range(5)], reps=r),
         lambda pl, a, b: pl._L.ugp_mask_time(pl._h, 0, None, 0, None, None, None, None, None, None, 1, a, b), 2),
    Hook("vectors", "vectors", lambda pl, f, r: pl.vectors_time(*_vec(f.tree), reps=r), _vectors_bare, 2),
    Hook("subtree", "subtree", lambda pl, f, r: pl.subtree_time(f.sels[0], reps=r),
         lambda pl, a, b: pl._L.ugp_subtree_time(pl._h, 0, None, 1, a, b), 2),
    Hook("subtree_batch", "subtree", lambda pl, f, r: pl.subtree_batch_time(f.sels, reps=r),
         lambda pl, a, b: pl._L.ugp_subtree_batch_time(pl._h, 0, None, None, 1, a, b), 2),
    Hook("haplotype", "haplotypes", lambda pl, f, r: pl.haplotype_time(reps=r),
         lambda pl, a, b, c: pl._L.ugp_haplotype_time(pl._h, 1, a, b, c), 3),
]


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("hook", HOOKS, ids=lambda h: h.name)
def test_times_are_finite_and_the_family_still_answers(hook, tree):
    t = S.trees()[tree]
    f = S.family(t, hook.family)
    pl = t.handle()
    f.attach(pl, t.X)
    if hook.prepare:
        hook.prepare(pl, f)
    for reps in (1, 3):
        ms = hook.time(pl, f, reps)
        ms = (ms,) if isinstance(ms, float) else tuple(ms)
        assert len(ms) == hook.n_out and all(math.isfinite(x) and x >= 0 for x in ms), (hook.name, reps, ms)
    with pytest.raises(UgpError) as e:
        hook.time(pl, f, 0)
    assert e.value.code == -1, (hook.name, str(e.value))
    f.check(pl, ("after", hook.name + "_time"))
    pl.close()


@pytest.mark.parametrize("tree", TREES)
def test_a_handle_that_never_attached_the_family_is_refused(tree):
    t = S.trees()[tree]
    pl = t.handle()
    for hook in HOOKS:
        out = [C.c_double(0) for _ in range(hook.n_out)]
        rc = hook.bare(pl, *[C.byref(x) for x in out])
        assert rc == -1 and ("ugp_%s_attach" % hook.family).encode() in pl._L.ugp_last_error(), (hook.name, rc, pl._L.ugp_last_error())
    pl.close()
