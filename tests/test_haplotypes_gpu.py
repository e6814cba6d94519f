"""ugp_haplotype_groups / _sets (Placer.haplotype_*) against the literal restatement of matUtils summary --haplotype
(tests/haplotypes_ref.py) on every hand-shaped case of tests/haplotypes_cases.py, exactly; the scan over segment edges, leaf counts
around a wave, the hash_bits hook that shows the exact comparison is real, the launch windows of the sets, the cap / n_out protocol,
the error codes, and `matutils-amd haplotypes` on the device byte for byte against its own --host output."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import haplotypes_cases as HC
from tests import haplotypes_ref as R
from tests import summary_cases as SC
from tests import test_haplotypes_cpu as CPU
from tests import test_summary_cpu as SCPU
from usher_amd import Placer, UgpError
from usher_amd.placement import _ptr

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in HC.hand_cases()}
FALLBACK = "walking it on the host"


def placer(arrays):
    arrays = dict(arrays, names=arrays.get("names") or ["n%d" % j for j in range(arrays["n"])])
    pl = Placer(SC.topology(arrays))
    pl.haplotypes_attach(arrays)
    return pl


def rows(groups):
    return [(int(g["leaf"]), int(g["count"]), int(g["size"])) for g in groups]


def sets_of(pl, leaves, **kw):
    off, pos, nuc = pl.haplotype_sets(leaves, **kw)
    assert int(off[-1]) == len(pos) == len(nuc) == pl._hp_n_out
    return [list(zip(pos[int(a):int(b)].tolist(), nuc[int(a):int(b)].tolist())) for a, b in zip(off[:-1], off[1:])]


def dirty(n, dtype=Placer.HP_GROUP):
    return np.full(n, 0xA5, np.uint8).repeat(dtype.itemsize).view(dtype)


def refused(pl, hash_bits=128):
    """A groups call that must refuse: (info, n_out) after checking the code and that nothing was written."""
    buf = dirty(8)
    with pytest.raises(UgpError) as e:
        pl.haplotype_groups(hash_bits=hash_bits, out=buf)
    assert e.value.code == -2 and pl._hp_n_out == 0 and (buf.view(np.uint8) == 0xA5).all()
    return pl._hp_info


def against_fast(arrays, chunk_leaves=0):
    F = R.Fast(arrays)
    pl = placer(arrays)
    groups, info = pl.haplotype_groups()
    assert rows(groups) == F.group_records()
    assert (int(info["n_leaves"]), int(info["n_groups"]), int(info["n_collisions"]), int(info["n_duplicate"])) == (F.n_leaves, len(groups), 0, 0)
    off, pos, nuc = pl.haplotype_sets(F.leaf_bfs, chunk_leaves=chunk_leaves)
    w_off, w_pos, w_nuc = F.sets_csr(F.leaf_bfs)
    assert np.array_equal(off, w_off) and np.array_equal(pos, w_pos) and np.array_equal(nuc, w_nuc)
    pl.close()
    return F


@pytest.mark.parametrize("case", HC.hand_cases(), ids=repr)
def test_cases(case):
    T = case.tree()
    pl = placer(case.arrays)
    leaves = T.leaves()
    if case.device:
        groups, info = pl.haplotype_groups()       # returns 0: a refusal would raise, so it cannot hide a wrong answer
        assert rows(groups) == R.group_records(T)
        assert sets_of(pl, leaves) == R.leaf_sets(T, leaves)
        assert (int(info["n_leaves"]), int(info["n_groups"]), int(info["n_collisions"]), int(info["n_duplicate"]), int(info["first_duplicate"])) == \
               (len(leaves), len(groups), 0, 0, R.NONE)
    else:
        info = refused(pl)
        assert (int(info["n_duplicate"]), int(info["first_duplicate"])) == R.duplicates(T) and int(info["n_leaves"]) == len(leaves)
        with pytest.raises(UgpError) as e:
            pl.haplotype_sets(leaves)
        assert e.value.code == -2
        with pytest.raises(UgpError) as e:
            pl.haplotype_time(1)
        assert e.value.code == -2
    pl.close()


def caterpillar_of(n_nodes, every):
    depth = n_nodes // 3
    root = HC.caterpillar(depth, every)
    root.kids += [HC.N(["G5T"]) for _ in range(n_nodes - 3 * depth)]
    return root


@pytest.mark.parametrize("shape,n_nodes", [(s, n) for s in ("star", "caterpillar") for n in (255, 256, 257, 16383, 16384, 16385)])
def test_scan_edges(shape, n_nodes):
    """kBlock = 256 positions per pass of the block scan, kSeg = 16384 per segment."""
    root = HC.star(n_nodes - 1, every=5) if shape == "star" else caterpillar_of(n_nodes, 1 if n_nodes < 1000 else 16)
    arrays, _ = HC.build(root)
    assert arrays["n"] == n_nodes
    F = against_fast(arrays)
    assert len(F.group_count) > 3 and (F.group_count > 1).any()


def test_subtree_ends_on_a_segment_boundary_and_at_n():
    arrays, _ = HC.build(HC.segment_edge_tree())
    F = against_fast(arrays)
    S = F.S
    ends = S.pre + S.size
    carriers = np.flatnonzero(np.diff(arrays["mut_off"]) > 0)
    assert 16384 in ends[carriers].tolist() and arrays["n"] in ends[carriers[carriers != 0]].tolist() and arrays["n"] > 16384
    assert sorted(F.group_size.tolist()) == [0, 1, 1, 1, 2, 2]     # nothing leaked past a subtree: the lone leaf is `reference`


@pytest.mark.parametrize("n_leaves", [1, 63, 64, 65, 16385])
def test_leaf_counts(n_leaves):
    every = 7 if 1 < n_leaves < 100 else 0
    arrays, _ = HC.build(HC.star(n_leaves, every=every))
    F = against_fast(arrays)
    assert F.n_leaves == n_leaves
    if not every:
        assert F.group_records() == [(1, n_leaves, 1)]             # all in one group, named by the first leaf
    else:
        assert len(F.group_count) == 4


def test_hash_bits_show_that_the_comparison_is_real():
    case = CASES["allele_only"]
    want = R.group_records(case.tree())
    assert len(want) >= 3
    pl = placer(case.arrays)
    assert rows(pl.haplotype_groups(hash_bits=128)[0]) == want
    separating = None
    for k in range(2, 65):                                         # some k that happens to separate them
        try:
            got = rows(pl.haplotype_groups(hash_bits=k)[0])
        except UgpError as e:
            assert e.code == -2 and int(pl._hp_info["n_collisions"]) > 0
            continue
        assert got == want
        separating = k
        break
    assert separating is not None and separating < 64
    assert rows(pl.haplotype_groups(hash_bits=100)[0]) == want    # the high lane in part
    for k in (0, 1):                                               # at least two of the four sets share a run: the comparison must say so
        info = refused(pl, hash_bits=k)
        assert int(info["n_collisions"]) > 0 and int(info["n_groups"]) <= 2 and int(info["n_visited"]) > 0
    with pytest.raises(UgpError) as e:
        pl.haplotype_groups(hash_bits=129)
    assert e.value.code == -1
    pl.close()
    # leaves that are equal stay one group however few bits take part
    pl = placer(CASES["no_mutations"].arrays)
    groups, info = pl.haplotype_groups(hash_bits=0)
    assert rows(groups) == R.group_records(CASES["no_mutations"].tree()) and len(groups) == 1 and int(info["n_collisions"]) == 0
    pl.close()
    pl = placer(CASES["star_shared"].arrays)
    assert rows(pl.haplotype_groups(hash_bits=0)[0]) == R.group_records(CASES["star_shared"].tree())
    pl.close()


@pytest.mark.parametrize("name", ["set_sizes", "override_deeper", "caterpillar600", "revert_equals_reference"])
def test_set_windows(name):
    case = CASES[name]
    T = case.tree()
    pl = placer(case.arrays)
    leaves = T.leaves()
    order = leaves[::-1] + leaves[:2]                               # any order, a leaf twice
    want = R.leaf_sets(T, order)
    if name == "set_sizes":
        assert [len(s) for s in R.leaf_sets(T, leaves)] == [63, 0, 64, 65, 300]   # an empty set between two that are not
    if name == "override_deeper":
        assert [(100, 8), (200, 4)] in want and [(100, 2), (200, 4)] in want
    n = len(order)
    for w in sorted({1, 2, n - 1, n, n + 1, 0}):
        assert sets_of(pl, order, chunk_leaves=w) == want, w
    off, pos, nuc = pl.haplotype_sets([])
    assert off.tolist() == [0] and len(pos) == 0
    inner = [v for v in range(case.arrays["n"]) if not T.is_leaf(v)]
    for bad in ([leaves[0], inner[0]], [case.arrays["n"]], [0xFFFFFFFF]):
        with pytest.raises(UgpError) as e:
            pl.haplotype_sets(bad)
        assert e.value.code == -1
    pl.close()


def test_cap_protocol():
    case = CASES["all_distinct"]
    T = case.tree()
    pl = placer(case.arrays)
    full, _ = pl.haplotype_groups()
    n = len(full)
    assert n > 3
    fn = pl._L.ugp_haplotype_groups
    n_out = C.c_uint64(0)
    assert fn(pl._h, None, 0, C.byref(n_out), None) == 0 and n_out.value == n          # cap = 0: the count alone; info may be NULL
    for cap in (n - 1, n, n + 2):
        buf = dirty(n + 2)
        n_out = C.c_uint64(0)
        assert fn(pl._h, _ptr(buf), cap, C.byref(n_out), None) == 0 and n_out.value == n
        k = min(cap, n)
        assert buf[:k].tobytes() == full[:k].tobytes() and (buf[k:].view(np.uint8) == 0xA5).all(), cap
    assert len(pl.haplotype_groups(cap=2)[0]) == 2 and pl._hp_n_out == n
    assert fn(pl._h, None, 3, C.byref(n_out), None) == -1
    # the set entries
    leaves = np.asarray(T.leaves(), np.uint32)
    w_off, w_pos, w_nuc = pl.haplotype_sets(leaves)
    total = len(w_pos)
    assert total == 2 * len(leaves)
    fs = pl._L.ugp_haplotype_sets_chunked
    for cap in (0, 1, total - 1, total, total + 3):
        for chunk in (0, 3):
            off = np.zeros(len(leaves) + 1, np.uint64)
            pos, nuc = dirty(total + 3, np.dtype(np.int32)), dirty(total + 3, np.dtype(np.uint8))
            n_out = C.c_uint64(0)
            assert fs(pl._h, _ptr(leaves), len(leaves), _ptr(off), _ptr(pos), _ptr(nuc), cap, C.byref(n_out), chunk) == 0
            k = min(cap, total)
            assert n_out.value == total and np.array_equal(off, w_off)
            assert np.array_equal(pos[:k], w_pos[:k]) and np.array_equal(nuc[:k], w_nuc[:k])
            assert (pos[k:].view(np.uint8) == 0xA5).all() and (nuc[k:] == 0xA5).all(), (cap, chunk)
    off, pos, nuc = pl.haplotype_sets(leaves, cap=5, chunk_leaves=2)
    assert len(pos) == 5 and pl._hp_n_out == total and np.array_equal(pos, w_pos[:5])
    pl.close()


def test_calls_before_the_attach_name_it():
    case = CASES["allele_only"]
    pl = Placer(SC.topology(case.arrays))
    L = pl._L
    n_out = C.c_uint64(7)
    buf = dirty(4)
    info = np.zeros(1, Placer.HP_INFO)
    assert L.ugp_haplotype_groups(pl._h, _ptr(buf), 4, C.byref(n_out), _ptr(info)) == -1 and b"ugp_haplotypes_attach" in L.ugp_last_error()
    assert n_out.value == 7 and (buf.view(np.uint8) == 0xA5).all()
    leaves = np.asarray([1], np.uint32)
    off = np.zeros(2, np.uint64)
    assert L.ugp_haplotype_sets(pl._h, _ptr(leaves), 1, _ptr(off), None, None, 0, C.byref(n_out)) == -1 and b"ugp_haplotypes_attach" in L.ugp_last_error()
    ms = C.c_double(0)
    assert L.ugp_haplotype_time(pl._h, 1, C.byref(ms), C.byref(ms), C.byref(ms)) == -1 and b"ugp_haplotypes_attach" in L.ugp_last_error()
    pl.haplotypes_attach(case.arrays)
    assert L.ugp_haplotype_time(pl._h, 0, C.byref(ms), C.byref(ms), C.byref(ms)) == -1
    assert L.ugp_haplotype_groups(pl._h, None, 0, None, None) == -1
    assert rows(pl.haplotype_groups()[0]) == R.group_records(case.tree())
    pl.close()


def test_plain_handle_and_shared_tables():
    """A handle made from the tree's own arrays attaches beside the other users of the depth-first tables."""
    from tests import synth
    arrays = synth.make_case(2, n_leaves=250, n_queries=1, n_sites=60, genome_len=500)[0]
    F = R.Fast(arrays)
    assert (F.group_count > 1).sum() > 5
    pl = Placer(arrays)
    pl.nearest_k([3], 2)
    pl.summary_attach()
    pl.haplotypes_attach()
    assert rows(pl.haplotype_groups()[0]) == F.group_records()
    assert len(pl.summary_mutations()) > 0
    w = F.sets_csr(F.leaf_bfs[::3])
    got = pl.haplotype_sets(F.leaf_bfs[::3])
    assert all(np.array_equal(a, b) for a, b in zip(got, w))
    scan_ms, sort_ms, verify_ms = pl.haplotype_time(reps=2)
    assert scan_ms > 0 and sort_ms > 0 and verify_ms > 0
    other = dict(arrays)
    other["mut_pos"] = np.asarray(arrays["mut_pos"]) + 1
    with pytest.raises(UgpError) as e:
        pl.haplotypes_attach(other)
    assert e.value.code == -1 and "other mutation arrays" in str(e.value)
    assert rows(pl.haplotype_groups()[0]) == F.group_records()        # the state stayed
    pl.close()


@pytest.mark.parametrize("name", ["survey", "annotated"] + [c.name for c in HC.cli_cases()])
def test_cli_device_against_host(name, tmp_path):
    if name == "survey":
        pb = CPU.SURVEY_PB
    elif name == "annotated":
        pb = CPU.ANNOTATED_PB
    else:
        pb = SCPU.write_annotated(CASES[name], tmp_path / "case.pb")
    dev = CPU.run(["-i", pb, "-H", "hap.tsv", "-d", tmp_path / "dev"])
    host = CPU.run(["-i", pb, "-H", "hap.tsv", "-d", tmp_path / "host", "--host"])
    got = open(tmp_path / "dev" / "hap.tsv", "rb").read()
    assert got == open(tmp_path / "host" / "hap.tsv", "rb").read() and got.startswith(R.HEADER.encode())
    assert FALLBACK not in host.stderr and FALLBACK not in dev.stderr   # the device path ran
    if name in CASES and CASES[name].text is not None:
        assert got.decode() == R.HEADER + CASES[name].text
    if name in ("survey", "all_distinct", "caterpillar600"):
        # the groups are ordered in pieces on the host threads and merged: pieces of one group each
        env = dict(os.environ, USHER_AMD_GRAIN="1", USHER_AMD_THREADS="5")
        r = subprocess.run([CPU.BIN, "haplotypes", "-i", pb, "-H", "hap.tsv", "-d", str(tmp_path / "pieces")], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and FALLBACK not in r.stderr and open(tmp_path / "pieces" / "hap.tsv", "rb").read() == got
    if name == "duplicate_position":
        # The loader merges two entries at one position of a node (Node::add_mutation, as the reference's does), so the tree AS
        # LOADED has no duplicate node and the device answers it.  No .pb file holds the shape ugp_haplotype_groups refuses; the
        # refusal is tested through the C ABI (test_cases) and the front end's fallback below.
        assert R.duplicates(CPU.load_model(pb)) == (0, R.NONE) and R.duplicates(CASES[name].tree())[0] == 1


@pytest.mark.parametrize("name", ["survey", "allele_only", "caterpillar600"])
def test_cli_falls_back_when_the_device_refuses(name, tmp_path):
    """USHER_AMD_HAPLOTYPE_HASH_BITS=0 puts every leaf into one run of the sort: the exact comparison finds the leaves that differ,
    the library refuses the table, and the front end says so in one line and walks the tree on the host: the same bytes."""
    pb = CPU.SURVEY_PB if name == "survey" else SCPU.write_annotated(CASES[name], tmp_path / "case.pb")
    args = [CPU.BIN, "haplotypes", "-i", pb, "-H", "hap.tsv", "-d"]
    dev = subprocess.run(args + [str(tmp_path / "dev")], capture_output=True, text=True, timeout=600, env=dict(os.environ, USHER_AMD_HAPLOTYPE_HASH_BITS="0"))
    assert dev.returncode == 0, dev.stderr[-2000:]
    CPU.run(["-i", pb, "-H", "hap.tsv", "-d", tmp_path / "host", "--host"])
    assert open(tmp_path / "dev" / "hap.tsv", "rb").read() == open(tmp_path / "host" / "hap.tsv", "rb").read()
    note = [line for line in dev.stderr.split("\n") if FALLBACK in line]
    assert len(note) == 1 and "0 nodes with a position twice" in note[0]
    m = re.search(r"(\d+) fingerprint collisions among (\d+) samples", note[0])
    leaves = len(CPU.load_model(pb).leaves())
    assert m and 0 < int(m.group(1)) < leaves and int(m.group(2)) == leaves
