"""ugp_relatives_closest / ugp_relatives_within (Placer.relatives_*) against the closed form of tests/relatives_ref.py, every field,
with every node as target: random, polytomy, caterpillar, star and hand-shaped trees, leaf counts at the edges of the range-minimum
blocks, name ranks, chunked batches, short output buffers, repeated samples and the error codes."""
import ctypes as C

import numpy as np
import pytest

from tests import relatives_cases as RC
from tests import relatives_ref as R
from tests import synth
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu

B = Placer.REL_BLOCK


def _run(arrays, seed=0, literal_every=97):
    """Both calls for every node against the closed form (thresholds 0, 1, 2, 5 and one above the largest cum), with random name
    ranks; every literal_every-th target also against the literal walk; then the same calls without lists.  Returns the Fast."""
    n = arrays["n"]
    rank = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    F = R.Fast(arrays, rank, rings=True)
    T = R.Tree(arrays)
    nodes = np.arange(n, dtype=np.uint32)
    pl = Placer(arrays)
    pl.relatives_attach(rank)
    got = pl.relatives_closest(nodes)
    assert pl._rel_n_out == len(got[2]) == int(got[1][-1])
    for v in range(n):
        want = F.closest(v)
        if v % literal_every == 0:
            assert want == R.literal(T, v, False, 0, rank), v
        R.check(got, want, v)
    bare = pl.relatives_closest(nodes, lists=False)
    assert bare[1] is None and bare[2] is None and (bare[0] == got[0]).all() and pl._rel_n_out == len(got[2])
    for k in (0, 1, 2, 5, int(F.cumb.max()) + 1):
        got = pl.relatives_within(nodes, k)
        for v in range(n):
            want = F.within(v, k)
            if v % literal_every == 0:
                assert want == R.literal(T, v, True, k), (v, k)
            R.check(got, want, v)
        bare = pl.relatives_within(nodes, k, lists=False)
        assert (bare[0] == got[0]).all() and pl._rel_n_out == len(got[2])
    pl.close()
    return F


@pytest.mark.parametrize("seed,n_leaves", [(1, 130), (2, 700), (3, 1700)])
def test_random_trees(seed, n_leaves):
    arrays = synth.make_case(seed, n_leaves=n_leaves, n_queries=1, n_sites=80, genome_len=600, p_masked=0.2,
                             mut_counts=(0, 0, 0, 1, 1, 2, 3))[0]
    assert 200 <= arrays["n"] <= 3000 and (np.asarray(arrays["mut_pos"]) < 0).sum() > 20
    assert (np.diff(arrays["mut_off"]) == 0).sum() > 20   # zero-length branches
    _run(arrays, seed)


def test_polytomy_tree():
    arrays = synth.polytomy_case(4, fanouts=(12, 15, 9), n_queries=1, genome_len=3000, n_sites=200)[0]
    assert 200 <= arrays["n"] <= 3000
    _run(arrays, 4)


def test_caterpillar_and_root_polytomy():
    arrays = synth.caterpillar_case(5, depth=150, muts_per_node=2, n_queries=1, genome_len=4000, n_sites=300)[0]
    _run(arrays, 5)
    arrays = synth.polytomy_case(6, fanouts=(300,), n_queries=1)[0]
    F = _run(arrays, 6)
    assert max(F.closest(v)["count"] for v in range(1, arrays["n"])) > 50   # the leaves without entries of their own tie


@pytest.mark.parametrize("name", list(RC.hand_cases()))
def test_hand_cases(name):
    arrays = RC.hand_cases()[name]
    F = _run(arrays, 7, literal_every=1)
    if name == "caterpillar":
        assert max(F.closest(v)["levels"] for v in range(arrays["n"])) > 100
    if name == "append":
        assert F.closest(RC.append_across_levels()[1])["nodes"] == RC.append_across_levels()[2]
    if name == "replace":
        assert F.closest(RC.replace_at_deeper_level()[1])["nodes"] == RC.replace_at_deeper_level()[2]


def test_range_minimum_edges():
    """Leaf counts B - 1, B, B + 1 and B * B + 1, and among the ring ranges the five shapes the range-minimum query tells apart."""
    seen = []
    for n_leaves in (B - 1, B, B + 1, B * B + 1):
        arrays = RC.rmq_tree(n_leaves)
        F = _run(arrays, n_leaves, literal_every=31)
        assert len(F.lbfs) == n_leaves
        seen += [(a, b, len(F.lbfs)) for a1, b1, a2, b2 in F.seen for a, b in ((a1, b1), (a2, b2))]
    full = [(a, b, nl) for a, b, nl in seen if a < b]
    assert any(a // B == (b - 1) // B and a % B and b % B and b != nl for a, b, nl in full)          # inside one block: read one by one
    assert any(a % B == 0 and b % B == 0 and b - a >= B for a, b, nl in full)                        # both ends on block edges
    levels = {((b - 1) // B - a // B - 1).bit_length() - 1 for a, b, nl in full if (b - 1) // B - a // B > 1}
    assert len(levels) >= 2 and max(levels) >= 2                                                     # several sparse-table levels
    assert any(a1 == b1 and a2 < b2 for a1, b1, a2, b2 in F.seen) and any(a1 < b1 and a2 == b2 for a1, b1, a2, b2 in F.seen)


def _pack(F, fn, nodes):
    info = np.zeros(len(nodes), Placer.REL_INFO)
    lists = []
    for i, v in enumerate(nodes):
        w = fn(int(v))
        info[i] = (w["dist"], w["count"], w["levels"], w["best"])
        lists += w["nodes"]
    return info, np.array(lists, np.uint32)


def test_chunks_windows_and_repeated_samples():
    for arrays in (synth.polytomy_case(8, fanouts=(12, 15, 9), n_queries=1, genome_len=3000, n_sites=200)[0], RC.star()):
        F = R.Fast(arrays)
        rng = np.random.default_rng(9)
        nodes = np.concatenate([rng.integers(0, arrays["n"], 400), [5, 5, 7, 5]]).astype(np.uint32)   # a sample given twice
        pl = Placer(arrays)
        for fn, call in ((F.closest, lambda **kw: pl.relatives_closest(nodes, **kw)),
                         (lambda v: F.within(v, 2), lambda **kw: pl.relatives_within(nodes, 2, **kw))):
            info, lists = _pack(F, fn, nodes)
            if arrays["n"] == 301:
                assert info["count"].max() > 16      # the star: a list longer than the window of a one-sample chunk
            for chunk in (0, 1, 7):
                got = call(chunk_samples=chunk)
                assert (got[0] == info).all() and (np.diff(got[1].astype(np.int64)) == info["count"]).all()
                assert (got[2] == lists).all(), chunk
        pl.close()


def test_short_output_buffer_keeps_the_rest_untouched():
    arrays = synth.polytomy_case(10, fanouts=(12, 15, 9), n_queries=1, genome_len=3000, n_sites=200)[0]
    F = R.Fast(arrays)
    nodes = np.arange(arrays["n"], dtype=np.uint32)
    pl = Placer(arrays)
    pl.relatives_attach()
    L = pl._L
    for fn, call in ((F.closest, lambda *a: L.ugp_relatives_closest_chunked(pl._h, len(nodes), _ptr(nodes), *a)),
                     (lambda v: F.within(v, 2), lambda *a: L.ugp_relatives_within_chunked(pl._h, len(nodes), _ptr(nodes), 2, *a))):
        info, lists = _pack(F, fn, nodes)
        for cap in (0, 1, len(lists) // 2, len(lists) - 1, len(lists), len(lists) + 9):
            for chunk in (0, 50):
                out = np.full(len(lists) + 20, 0xABCDEF01, np.uint32)
                off = np.zeros(len(nodes) + 1, np.uint64)
                got = np.zeros(len(nodes), Placer.REL_INFO)
                n_out = C.c_uint64(0)
                assert call(_ptr(got), _ptr(off), _ptr(out), cap, C.byref(n_out), chunk) == 0
                w = min(cap, len(lists))
                assert n_out.value == len(lists) and (out[:w] == lists[:w]).all() and (out[w:] == 0xABCDEF01).all()
                assert (got == info).all() and (off == np.concatenate([[0], np.cumsum(info["count"])])).all()
    assert len(pl.relatives_closest(nodes, cap=10)[2]) == 10 and pl._rel_n_out > 10
    pl.close()


def test_front_end_writes_the_same_bytes_as_its_host_walk(tmp_path):
    import subprocess
    from tests import test_relatives_cpu as CPU
    out = {}
    for mode, extra in (("device", []), ("host", ["--host"])):
        d = tmp_path / mode
        CPU.run(["-i", CPU.PB, "-V", "c.tsv", "--within-distance", "w.tsv", "--distance-threshold", "3", "-d", d] + extra)
        CPU.run(["-i", CPU.PB, "-V", "q.tsv", "-q", "--within-distance", "w0.tsv", "-d", d] + extra)
        out[mode] = [open(d / f, "rb").read() for f in ("c.tsv", "w.tsv", "q.tsv", "w0.tsv")]
        # a subset in another order: the first column of the within file names every sample once
        ids = [line.split(b"\t")[0].decode() for line in out[mode][1].split(b"\n") if line]
        pick = [ids[i] for i in np.random.default_rng(12).permutation(len(ids))[:50]]
        with open(d / "s.txt", "w") as f:
            f.write("".join(s + "\n" for s in pick))
        CPU.run(["-i", CPU.PB, "-s", d / "s.txt", "-V", "sc.tsv", "-q", "--within-distance", "sw.tsv", "--distance-threshold", "2", "-d", d] + extra)
        out[mode] += [open(d / f, "rb").read() for f in ("sc.tsv", "sw.tsv")]
    assert out["device"] == out["host"]
    assert all(len(b) > 1000 for b in out["host"][:4]) and out["host"][0] != out["host"][2]
    r = subprocess.run([CPU.BIN, "relatives", "-i", CPU.PB, "-V", "x.tsv", "-d", str(tmp_path), "--device", "0"], capture_output=True, text=True)
    assert r.returncode == 0 and "Relatives of" in r.stderr


def test_shared_tables_take_one_set_of_mutation_arrays():
    """The depth-first tables are the handle's, built by its first dense attach: beside nearest_k the relatives calls read the same
    tables, and an attach with other mutation arrays is refused and leaves the state as it was."""
    arrays = synth.make_case(12, n_leaves=250, n_queries=1, n_sites=60, genome_len=500)[0]
    F = R.Fast(arrays)
    nodes = np.arange(arrays["n"], dtype=np.uint32)
    pl = Placer(arrays)
    pl.nearest_k([3], 2)
    got = pl.relatives_closest(nodes)
    for v in range(arrays["n"]):
        R.check(got, F.closest(v), v)
    other = dict(arrays)
    other["mut_pos"] = np.asarray(arrays["mut_pos"]) + 1
    with pytest.raises(UgpError) as e:
        pl.relatives_attach(arrays=other)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    again = pl.relatives_closest(nodes)
    assert (again[0] == got[0]).all() and (again[2] == got[2]).all()        # the state stayed
    pl.close()


def test_error_codes_leave_the_output_untouched():
    arrays = synth.make_case(11, n_leaves=100, n_queries=1)[0]
    pl = Placer(arrays)
    L = pl._L
    nodes = np.array([3, 4, 5], np.uint32)
    info = np.full(3 * 16, 0x5A, np.uint8).view(Placer.REL_INFO)
    off = np.full(4, 77, np.uint64)
    out = np.full(64, 0xABCDEF01, np.uint32)
    n_out = C.c_uint64(7)

    def untouched():
        return (info.view(np.uint8) == 0x5A).all() and (off == 77).all() and (out == 0xABCDEF01).all() and n_out.value == 7

    # before the attach
    assert L.ugp_relatives_closest(pl._h, 3, _ptr(nodes), _ptr(info), _ptr(off), _ptr(out), 64, C.byref(n_out)) == -1
    assert b"ugp_relatives_attach" in L.ugp_last_error() and untouched()
    assert L.ugp_relatives_within(pl._h, 3, _ptr(nodes), 2, _ptr(info), _ptr(off), _ptr(out), 64, C.byref(n_out)) == -1 and untouched()
    # ranks that are no permutation
    with pytest.raises(UgpError):
        pl.relatives_attach(np.zeros(arrays["n"], np.uint32))
    assert L.ugp_relatives_closest(pl._h, 3, _ptr(nodes), _ptr(info), _ptr(off), _ptr(out), 64, C.byref(n_out)) == -1 and untouched()
    pl.relatives_attach()
    bad = np.array([3, arrays["n"], 5], np.uint32)
    assert L.ugp_relatives_closest(pl._h, 3, _ptr(bad), _ptr(info), _ptr(off), _ptr(out), 64, C.byref(n_out)) == -1
    assert L.ugp_last_error() and untouched()
    assert L.ugp_relatives_within(pl._h, 3, _ptr(bad), 2, _ptr(info), _ptr(off), _ptr(out), 64, C.byref(n_out)) == -1 and untouched()
    with pytest.raises(UgpError):
        pl.relatives_closest([arrays["n"]])
    # without ranks there is no best; an empty batch is an empty answer
    got = pl.relatives_closest(nodes)
    assert (got[0]["best"] == R.NONE).all() and got[0]["count"].sum() == len(got[2])
    got = pl.relatives_closest([])
    assert len(got[0]) == 0 and got[1].tolist() == [0] and len(got[2]) == 0
    pl.close()
