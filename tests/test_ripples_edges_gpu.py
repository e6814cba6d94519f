"""ugp_ripples / Placer.ripples on the hand-shaped cases of tests/ripples_cases.py, event by event against the literal search:
tile, chunk and block counts, the pair count against the block, narrow LDS tiles, ambiguous and masked alleles, ties in the
sort key, the budget and pair-validity limits at equality, the eligibility clauses.  A case that carries UGP_RIPPLES_LIMITS
runs with them and again without; tests/test_ripples_cases_cpu.py shows that every case reaches the edge it is named for.

ugp_mat_create refuses a tree with an ambiguous allele, ugp_ripples_attach takes one: alleles/iupac runs on the handle of
alleles/one_hot (the same tree with one base per allele) with its own arrays attached, so term() and lowbit4() see multi-bit
states on the device."""
import numpy as np
import pytest

from oracle import capi
from tests import ripples_cases as RC
from tests import ripples_ref as RR
from usher_amd import Placer

pytestmark = pytest.mark.gpu

_ORACLES, _LITERAL = {}, {}


def _literal(c):
    name, arrays, br, _, opts, _ = c
    if name not in _LITERAL:
        if id(arrays) not in _ORACLES:
            _ORACLES[id(arrays)] = capi.OracleTree(arrays)
        _LITERAL[name] = RR.literal(arrays, br, _ORACLES[id(arrays)], **opts)
    return _LITERAL[name]


def _device(pl, c):
    _, _, br, rank, o, _ = c
    ev = pl.ripples(np.asarray(br), rank, branch_len=o["l"], min_range=o["r"], max_range=o["R"], parsimony_improvement=o["p"],
                    num_descendants=o["n_desc"])
    return [{k: (bool(e[k]) if k.endswith("sibling") else int(e[k])) for k in RR.KEYS} for e in ev]


@pytest.mark.parametrize("name", [c[0] for c in RC.CASES])
def test_case_equals_literal(name, monkeypatch):
    c = RC.by_name(name)
    want = _literal(c)
    assert bool(want) == RC.INFO[name]["events"]
    handle = RC.INFO[name].get("handle")
    pl = Placer(c[1] if handle is None else handle)
    if handle is not None:
        pl.ripples_attach(c[3], c[1])
    if c[5] is not None:
        monkeypatch.setenv("UGP_RIPPLES_LIMITS", c[5])
        assert _device(pl, c) == want
        monkeypatch.delenv("UGP_RIPPLES_LIMITS")
    assert _device(pl, c) == want
    pl.close()


def test_mixed_call_on_one_handle(monkeypatch):
    """Long, two-row, pairless, root and leaf branches in one call; then another num_descendants and back, with and without
    chunks of 50 candidates and two slab rows: the per-branch workspace carries nothing over."""
    cases = [c for c in RC.CASES if c[0].startswith("mixed_call/")]
    assert [c[4]["n_desc"] for c in cases] == [1, 3, 1] and all(c[1] is cases[0][1] for c in cases)
    pl = Placer(cases[0][1])
    for limits in (None, RC.limits_for(96, 282, Cc=50, nblk=2)):
        if limits:
            monkeypatch.setenv("UGP_RIPPLES_LIMITS", limits)
        for c in cases:
            assert _device(pl, c) == _literal(c), (c[0], limits)
    monkeypatch.delenv("UGP_RIPPLES_LIMITS")
    pl.close()
