"""The ugp_select calls (Placer.select_*) against the literal restatement of tests/select_ref.py on every hand-shaped case of
tests/select_cases.py, exactly -- masks, counts and the zero tail bits; the query batches of the _chunked hooks, the attach order
with translate and uncertainty on one handle, the error codes, and `matutils-amd select` on the device byte for byte against its
own --host output."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import select_cases as SC
from tests import select_ref as R
from tests import summary_cases as SMC
from tests import test_select_cpu as CPU
from tests import translate_cases as TC
from tests import translate_ref as TR
from tests import usher_model as UM
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu
CASES = SC.all_cases()
REFERENCE = {}   # case name -> the literal answers, computed once


def reference(case):
    if case.name not in REFERENCE:
        T = R.tree_from_arrays(case.arrays)
        names = CPU.T_names(case.arrays)
        pos, nuc = SC.queries(case.arrays)
        index = {s: j for j, s in enumerate(names)}
        REFERENCE[case.name] = {
            "leaves": [index[s] for s in R.leaves_by_rank(T)], "pos": pos, "nuc": nuc, "mutations": R.literal_mutations(T, pos, nuc),
            "subtrees": [(nodes, R.literal_subtrees(T, names, nodes)) for nodes in SC.node_sets(case.arrays)],
            "mrca": [(R.mask_of(T, [names[v] for v in ls]), index[R.get_mrca(T, [names[v] for v in ls])],
                      len(R.get_mrca_samples(T, [names[v] for v in ls]))) for ls in SC.leaf_sets(case.arrays)]}
    return REFERENCE[case.name]


def placer(case):
    pl = Placer(SMC.topology(case.arrays))
    pl.select_attach(case.arrays)
    return pl


def tail_is_zero(pl):
    n = pl._sel_leaves
    bits = np.unpackbits(pl._sel_raw.view(np.uint8), bitorder="little")
    return len(bits) == (n + 63) // 64 * 64 and not bits[n:].any()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_cases(case):
    ref = reference(case)
    pl = placer(case)
    assert pl.select_leaves().tolist() == ref["leaves"]
    assert same(pl.select_mutations(ref["pos"], ref["nuc"]), ref["mutations"]) and tail_is_zero(pl)
    for q in range(0, len(ref["pos"]), 5):   # single queries: the word of one query alone
        one = pl.select_mutations(ref["pos"][q:q + 1], ref["nuc"][q:q + 1])
        assert int(one[1][0]) == int(ref["mutations"][1][q]) == int(one[0].sum()) and tail_is_zero(pl), q
    for nodes, want in ref["subtrees"]:
        assert same(pl.select_subtrees(nodes), want) and tail_is_zero(pl), nodes
        for chunk in (1, 2):
            assert same(pl.select_subtrees(nodes, chunk_ranges=chunk), want), (nodes, chunk)
    for mask, node, below in ref["mrca"]:
        assert pl.select_mrca(mask) == (node, below)
    pl.close()


@pytest.mark.parametrize("name", ["owner_chain", "star129", "caterpillar"])
def test_query_batches(name):
    case = SC.by_name()[name]
    ref = reference(case)
    pos, nuc = ref["pos"], ref["nuc"]
    pl = placer(case)
    # no query, one, two at one position with two alleles
    mask, counts = pl.select_mutations(pos[:0], nuc[:0])
    assert not mask.any() and len(counts) == 0 and tail_is_zero(pl)
    T = R.tree_from_arrays(case.arrays)
    p = int(np.asarray(case.arrays["mut_pos"]).max())
    for qp, qn in (([p], [8]), ([p, p], [1, 8]), ([p, p], [8, 8])):
        assert same(pl.select_mutations(qp, qn), R.literal_mutations(T, qp, qn)), (qp, qn)
    # one past the staging batch, through the hook
    m = len(pos)
    for chunk in (1, 2, 3, m - 1, m, m + 1, 0):
        assert same(pl.select_mutations(pos, nuc, chunk_queries=chunk), ref["mutations"]) and tail_is_zero(pl), chunk
    assert same(pl.select_mutations(pos[:4], nuc[:4], chunk_queries=3), R.literal_mutations(T, pos[:4], nuc[:4]))
    assert pl.select_time(pos, nuc, 2) > 0
    pl.close()


def test_attach_order_with_translate():
    """translate and select search the same owners' nodes: whoever attaches first makes them, the other one reads them."""
    case = TC.by_name()["two_frames"]
    codons = case.codons()
    want_tr = TR.records(case.tree(), codons)
    T = R.tree_from_arrays(case.arrays)
    pos, nuc = SC.queries(case.arrays)
    want = R.literal_mutations(T, pos, nuc)
    for first in ("translate", "select"):
        pl = Placer(SMC.topology(case.arrays))
        if first == "select":
            pl.select_attach(case.arrays)
        pl.translate_attach(case.arrays)
        pl.translate_codons(*TR.slot_tables(codons))
        if first == "translate":
            assert TR.device_records(pl.translate()[0]) == want_tr
            pl.select_attach(case.arrays)
        assert same(pl.select_mutations(pos, nuc), want), first
        assert TR.device_records(pl.translate()[0]) == want_tr, first
        pl.select_attach(case.arrays)                  # a second attach replaces the first
        assert same(pl.select_mutations(pos, nuc), want), first
        pl.close()


def test_attach_order_with_uncertainty():
    from tests import synth
    arrays = synth.make_case(7, n_leaves=120, n_queries=1, n_sites=60, genome_len=500)[0]
    T = R.tree_from_arrays(arrays)
    pos, nuc = SC.queries(arrays)
    want = R.literal_mutations(T, pos, nuc)
    assert ((want[1] > 0) & (want[1] < len(want[0]))).any()
    nodes = np.arange(1, 40, dtype=np.uint32)
    answers = []
    for first in ("uncertainty", "select"):
        pl = Placer(arrays)
        if first == "select":
            assert same(pl.select_mutations(pos, nuc), want)     # attaches on the first call
        answers.append([a.tolist() for a in pl.uncertainty(nodes)[:2]])
        assert same(pl.select_mutations(pos, nuc), want), first
        pl.close()
    assert answers[0] == answers[1]


def test_other_arrays_are_refused_and_error_codes():
    case = SC.by_name()["owner_chain"]
    ref = reference(case)
    pl = Placer(SMC.topology(case.arrays))
    L, h = pl._L, pl._h
    words, counts = np.zeros(1, np.uint64), np.zeros(4, np.uint64)
    pos, nuc = np.asarray([10], np.int32), np.asarray([8], np.uint8)
    node, below = C.c_uint32(7), C.c_uint64(7)
    # before the attach
    assert L.ugp_select_mutations(h, 1, _ptr(pos), _ptr(nuc), _ptr(words), _ptr(counts)) == -1 and b"ugp_select_attach" in L.ugp_last_error()
    assert L.ugp_select_leaves(h, None, C.byref(below)) == -1 and L.ugp_select_subtrees(h, 0, None, _ptr(words), None) == -1
    assert L.ugp_select_mrca(h, _ptr(words), C.byref(node), C.byref(below)) == -1 and L.ugp_select_time(h, 1, _ptr(pos), _ptr(nuc), 1, C.byref(C.c_double())) == -1
    pl.select_attach(case.arrays)
    # tables built from other arrays are refused, the state stays
    other = dict(case.arrays)
    other["mut_pos"] = np.asarray(case.arrays["mut_pos"]) + 1
    with pytest.raises(UgpError) as e:
        pl.select_attach(other)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    assert same(pl.select_mutations(ref["pos"], ref["nuc"]), ref["mutations"])
    # null pointers
    assert L.ugp_select_mutations(h, 1, _ptr(pos), _ptr(nuc), None, _ptr(counts)) == -1
    assert L.ugp_select_mutations(h, 1, None, _ptr(nuc), _ptr(words), _ptr(counts)) == -1
    assert L.ugp_select_mutations(h, 1, _ptr(pos), None, _ptr(words), _ptr(counts)) == -1
    assert L.ugp_select_mutations(h, 1, _ptr(pos), _ptr(nuc), _ptr(words), None) == -1
    assert L.ugp_select_subtrees(h, 1, None, _ptr(words), _ptr(counts)) == -1 and L.ugp_select_subtrees(h, 0, None, None, None) == -1
    assert L.ugp_select_mrca(h, None, C.byref(node), C.byref(below)) == -1 and L.ugp_select_mrca(h, _ptr(words), None, C.byref(below)) == -1
    assert L.ugp_select_leaves(h, None, None) == -1
    assert L.ugp_select_time(h, 1, _ptr(pos), _ptr(nuc), 0, C.byref(C.c_double())) == -1
    # a node out of range: nothing is written
    words[0] = 0xA5
    bad = np.asarray([1, case.arrays["n"]], np.uint32)
    assert L.ugp_select_subtrees(h, 2, _ptr(bad), _ptr(words), _ptr(counts)) == -1 and b"out of range" in L.ugp_last_error() and words[0] == 0xA5
    # an empty bitmap has no ancestor; bits past the last leaf do not count
    with pytest.raises(UgpError) as e:
        pl.select_mrca(np.zeros(pl._sel_leaves, bool))
    assert e.value.code == -1 and node.value == 7
    words[0] = np.uint64(1) << np.uint64(pl._sel_leaves)
    assert L.ugp_select_mrca(h, _ptr(words), C.byref(node), C.byref(below)) == -1
    words[0] |= np.uint64(1)
    assert L.ugp_select_mrca(h, _ptr(words), C.byref(node), C.byref(below)) == 0 and node.value == ref["leaves"][0] and below.value == 1
    pl.close()


# ---- the command-line tool -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    return CPU.Model()


def both_paths(tmp_path, name, opts, files=("u.txt", "t.nh")):
    out, log = {}, {}
    for path in ("dev", "host"):
        d = tmp_path / (name + "_" + path)
        args = ["-i", CPU.PB, "-d", d, "-u", "u.txt", "-t", "t.nh"] + list(opts) + (["--host"] if path == "host" else [])
        r = CPU.run(args, ok=None)
        log[path] = r.stderr[-600:]
        out[path] = (r.returncode, CPU.warnings_of(r.stderr), [line for line in r.stderr.split("\n") if line.startswith("ERROR")],
                     {f: open(d / f, "rb").read() if os.path.exists(d / f) else None for f in files})
    assert out["dev"] == out["host"], (name, log)
    return out["dev"]


OPTION_SETS = ("clade", "two_clades", "leaf_clade", "unknown_beside_known", "mutation_T", "mutation_G", "two_mutations", "internal",
               "internal_unknown", "match", "mrca", "prune", "chained")
AFTER_A_FILE = ("clade", "mutation_T", "internal", "prune")   # these also behind -s: the file's order, the intersection


@pytest.mark.parametrize("name", OPTION_SETS)
def test_cli_device_against_host(model, tmp_path, name):
    sets = {n: (opts, kw) for n, opts, kw in CPU.option_sets(model)}
    assert tuple(sets) == OPTION_SETS
    opts, kw = sets[name]
    rc, warns, errors, files = both_paths(tmp_path, name, opts)
    want, wwarns = R.chain(model.T, **kw)   # and both against the restatement
    assert rc == 0 and warns == wwarns and files["u.txt"].decode() == "".join(s + "\n" for s in (want or model.leaves)), name
    if name in AFTER_A_FILE:
        rng = np.random.default_rng(8)
        some = [model.leaves[i] for i in rng.permutation(len(model.leaves))[:200]]
        (tmp_path / "s.txt").write_text("".join(s + "\n" for s in some))
        rc, _, _, files = both_paths(tmp_path, "s_" + name, list(opts) + ["-s", tmp_path / "s.txt"])
        want = R.chain(model.T, samples=some, **kw)[0]
        assert rc == 0 and files["u.txt"].decode() == "".join(s + "\n" for s in want), name


def test_cli_nothing_left(tmp_path):
    rc, _, errors, files = both_paths(tmp_path, "none", ["-c", "no_such_clade"])
    assert rc == 1 and errors == [R.NONE_LEFT.strip()] and files["u.txt"] is None


def test_cli_epps_and_vcf(model, tmp_path):
    # the largest clade that is not the whole tree: -e 1 keeps some of it
    by_size = sorted(model.clades.items(), key=lambda kv: -len(UM.get_leaves(model.T, kv[1])))
    c1 = next(c for c, n in by_size if len(UM.get_leaves(model.T, n)) < len(model.leaves))
    rc, _, _, files = both_paths(tmp_path, "epps", ["-c", c1, "-e", "1"])
    inside = R.chain(model.T, clade=c1)[0]
    got = files["u.txt"].decode().split("\n")[:-1]
    assert rc == 0 and 0 < len(got) < len(inside) and set(got) < set(inside)
    assert got == [s for s in R.dfs_order(model.T, set(inside)) if s in set(got)]          # depth-first order
    # a small clade that -e 1 empties: the reference's exit, on both paths
    small = CPU.option_sets(model)[0][1][1]
    rc, _, errors, files = both_paths(tmp_path, "epps_none", ["-c", small, "-e", "1"])
    assert rc == 1 and errors == [R.NONE_LEFT.strip()] and files["u.txt"] is None
    rc, _, _, files = both_paths(tmp_path, "epps_two", ["-c", small, "-e", "2"])
    assert rc == 0 and 0 < files["u.txt"].count(b"\n") < len(R.chain(model.T, clade=small)[0])
    rc, _, _, files = both_paths(tmp_path, "vcf", ["-m", "G11083T", "-v", "o.vcf"], files=("u.txt", "t.nh", "o.vcf"))
    assert rc == 0 and files["o.vcf"].count(b"\n") > 10
    # -e with nothing selected: the leaves only, in depth-first order
    rc, _, _, files = both_paths(tmp_path, "epps_all", ["-e", "1"])
    got = files["u.txt"].decode().split("\n")[:-1]
    assert rc == 0 and 0 < len(got) < len(model.leaves) and set(got) < set(model.leaves)
    assert got == [s for s in R.leaves_by_rank(model.T) if s in set(got)]
