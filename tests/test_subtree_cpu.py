"""The induced subtree without a GPU: the closed form of tests/subtree_ref.py against the literal restatement of get_subtree on every
hand-shaped case, on random trees and on the seam generators run small (which proves, pair by pair, that a node is kept exactly when
it is selected or two of its children have a selected node at or below them); the hand cases do what they say; the ABI surface of
the ugp_subtree calls; and `matutils-amd subtree --host` byte for byte against `select --host`."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pb_cases
from tests import subtree_cases as SC
from tests import subtree_ref as R
from tests import synth
from tests import test_select_cpu as SEL
from usher_amd import _lib

ROOT, BIN, PB = SEL.ROOT, SEL.BIN, SEL.PB
CASES = SC.all_cases()
SMALL = 128     # the seam of the small runs


def agree(arrays, sel):
    lit, fast = R.literal(arrays, sel), R.closed_form(arrays, sel)
    assert R.same(lit, fast, fast["owner"]), sel[:20]
    return lit


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_closed_form_equals_literal_on_hand_cases(case):
    for sel in case.sels:
        agree(case.arrays, sel)
    if case.arrays["n"] < 100:   # and every selection of up to three nodes, inner ones included
        rng = np.random.default_rng(case.arrays["n"])
        for sel in SC.selections(case.arrays, rng):
            agree(case.arrays, sel)


def test_cases_do_what_they_say():
    for case in CASES:
        res = R.literal(case.arrays, case.sels[0])
        if case.kept is None:
            continue
        names = {v: t for t, v in case.tags.items()}
        assert [names[int(v)] for v in res["kept"]] == case.kept, case.name
        merged = R.strings(case.arrays, res)
        for tag, want in case.merged.items():
            assert merged[case.tags[tag]] == want, (case.name, tag)
        assert res["info"]["n_disagree"] == case.disagree, case.name
    by = SC.by_name()
    # one leaf: the chain is the whole root path, the subtree's root has no parent
    res = R.literal(by["one_leaf"].arrays, by["one_leaf"].sels[0])
    assert res["info"]["longest_chain"] == 3 and res["info"]["n_gathered"] == 4 and res["parent"].tolist() == [R.NIL]
    # the deep common ancestor owns the nodes above it
    c = by["deep_lca"]
    res = R.literal(c.arrays, c.sels[0])
    assert res["owner"][0] == 0 and res["kept"][0] == c.tags["b"] and res["info"]["longest_chain"] == 3
    # a name twice: three names less
    assert R.literal(by["named_twice"].arrays, by["named_twice"].sels[0])["info"]["n_selected"] == 2
    # the opening entry of reverted_and_changed is the third
    c = by["reverted_and_changed"]
    res = R.literal(c.arrays, c.sels[0])
    assert res["first_entry"].tolist() == [int(c.arrays["mut_off"][c.tags["l"]])]
    # the disagreement is reported on the kept node below it, and only where the chain holds both entries
    c = by["disagreement"]
    assert [R.literal(c.arrays, s)["info"]["n_disagree"] for s in c.sels] == [1, 1, 0]
    assert R.literal(c.arrays, c.sels[1])["info"]["first_disagree"] == c.tags["l"]
    # stars: two selected leaves keep the root; all of them keep everything
    for k in (63, 64, 65, 255, 256, 257):
        c = by["sstar%d" % k]
        two, every = R.literal(c.arrays, c.sels[0]), R.literal(c.arrays, c.sels[1])
        assert two["kept"].tolist() == [0, 1, k] and len(every["kept"]) == k + 1 and every["info"]["n_gathered"] == len(c.arrays["mut_pos"])
        assert R.literal(c.arrays, c.sels[2])["kept"].tolist() == [1]
    # the caterpillar: three kept nodes, one chain nearly as long as the tree is deep, and the flips on it cancel in pairs
    c = by["scaterpillar"]
    res = R.literal(c.arrays, c.sels[0])
    assert [int(v) for v in res["kept"]] == [c.tags["v1"], c.tags["deepest"], c.tags["side1"]] and res["info"]["longest_chain"] == 300
    assert R.strings(c.arrays, res)[c.tags["deepest"]] == ["C1A", "G2A", "G3T"]


@pytest.mark.parametrize("seed", range(8))
def test_closed_form_equals_literal_on_random_trees(seed):
    rng = np.random.default_rng(seed)
    for t in range(30):   # 240 trees in all, masked entries among them
        arrays, _, _, _ = synth.random_tree(rng, int(rng.integers(3, 60)), p_masked=0.1 if t % 3 == 0 else 0.0, root_muts=t % 2)
        for sel in SC.selections(arrays, rng):
            agree(arrays, sel)


@pytest.mark.parametrize("variant", SC.VARIANTS)
def test_seam_generators_run_small(variant):
    """The shapes of tests/test_subtree_at_size_gpu.py with the seam at 128, against the literal form; each has the counts and the
    flags at the seam that the test there relies on."""
    for N in (SMALL + 1, SMALL + 100, 500):
        arrays, sel = SC.seam_selection(N, variant, SMALL, 60)
        assert arrays["n"] == N
        res = agree(arrays, sel)
        d2b = np.asarray(R.Tables(arrays).dfs)
        flags = np.isin(d2b[[SMALL - 1, SMALL]], sel)
        assert flags.tolist() == ([True, True] if variant == "11" else [False, False])
        assert len(res["kept"]) > len(set(sel.tolist()))   # common ancestors were added
    for K in (SMALL - 1, SMALL, SMALL + 1, 2 * SMALL + 1):
        arrays, sel = SC.entry_star(K, variant, SMALL)
        res = agree(arrays, sel)
        gone = 2 if variant == "00" and K > SMALL else 1 if variant == "00" and K == SMALL else 0
        assert arrays["n"] == K == len(arrays["mut_pos"]) and len(res["kept"]) == K - gone == res["info"]["n_gathered"] == len(res["pos"])
        arrays, sel = SC.cancel_star(K, variant, SMALL)
        res = agree(arrays, sel)
        assert res["info"]["n_gathered"] == K and len(res["pos"]) == K - (2 if variant == "00" and K > SMALL else 0)
        if variant == "00" and K > SMALL:
            assert int(res["ent_off"][SMALL - 1]) == int(res["ent_off"][SMALL]) == SMALL - 1   # items seam - 1 and seam do not survive


def test_deep_caterpillar_and_half_star_run_small():
    arrays, sel = SC.deep_caterpillar(2 * SMALL + 5)
    res = agree(arrays, sel)
    assert len(res["kept"]) == 3 and res["info"]["longest_chain"] == 2 * SMALL + 5 - 2 + 1 and int(res["kept"][0]) == 3
    arrays, sel = SC.half_star(SMALL + 1)
    res = agree(arrays, sel)
    assert len(res["kept"]) == 1 + (SMALL + 2) // 2 and res["parent"][1:].tolist() == [0] * ((SMALL + 2) // 2)


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    for name in ("ugp_subtree_attach", "ugp_subtree_nodes", "ugp_subtree_nodes_chunked", "ugp_subtree_entries", "ugp_subtree_owner",
                 "ugp_subtree_time"):
        assert re.search(r"\bint %s\(ugp_mat \*mat" % name, hdr) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    L = _lib.lib()   # no handle: an error code, not a crash
    assert L.ugp_subtree_attach(None, None) == -1 and L.ugp_subtree_nodes(None, 0, None, None, None, None, 0, None, None, None) == -1
    assert L.ugp_subtree_nodes_chunked(None, 0, None, None, None, None, 0, None, None, None, 0) == -1
    assert L.ugp_subtree_entries(None, None, None, None, 0, None) == -1 and L.ugp_subtree_owner(None, 0, None, None) == -1
    assert L.ugp_subtree_time(None, 0, None, 1, None, None) == -1


# ---- the command-line tool -------------------------------------------------------------------------------------------------------

def run(args, ok=True, sub="subtree"):
    return SEL.run(args, ok, sub)


OUTPUTS = ("u.txt", "t.nh", "o.pb", "v.vcf")


def outputs(tmp_path, name, sub, pb, opts, extra=("--host",)):
    """The bytes of -u, -t, -o and -v of one run, or the exit code and the last line when it fails."""
    out = tmp_path / ("%s_%s" % (name, sub))
    r = run(["-i", pb, "-d", out, "-u", "u.txt", "-t", "t.nh", "-o", "o.pb", "-v", "v.vcf", "--host-genotypes"] + list(opts) + list(extra), ok=None,
            sub=sub)
    if r.returncode:
        return r.returncode, r.stderr.split("\n")[-2], r
    return {f: open(out / f, "rb").read() for f in OUTPUTS}, SEL.warnings_of(r.stderr), r


@pytest.fixture(scope="module")
def model():
    return SEL.Model()


def test_host_equals_select_on_the_fixture(model, tmp_path):
    ran = 0
    for name, opts, _ in SEL.option_sets(model):
        got, warns, r = outputs(tmp_path, name, "subtree", PB, opts)
        want, wwarns, _ = outputs(tmp_path, name, "select", PB, opts)
        assert got == want and warns == wwarns, name
        if isinstance(got, dict):
            ran += 1
            assert len(got["o.pb"]) > 50 and got["t.nh"].endswith(b";\n") and len(got["v.vcf"]) > 100
            assert "Selection step subtree (host): " in r.stderr or "using full input tree" in r.stderr, name
    assert ran >= 10


def hand_pb(tmp_path, case):
    pb = tmp_path / (case.name + ".pb")
    pb_cases.write_pb_arrays(case.arrays, str(pb))
    from oracle import refio
    return pb, [n.identifier for n in refio.load_mutation_annotated_tree(str(pb)).breadth_first_expansion()]


HAND_CLI = ["siblings", "inner_selected", "all_leaves", "deep_lca", "reverted_and_changed", "one_masked", "disagreement", "sstar65", "scaterpillar"]


@pytest.mark.parametrize("name", HAND_CLI)
def test_host_equals_select_on_hand_cases(tmp_path, name):
    case = SC.by_name()[name]
    pb, names = hand_pb(tmp_path, case)
    for k, sel in enumerate(case.sels[:3]):
        (tmp_path / ("s%d.txt" % k)).write_text("".join(names[v] + "\n" for v in sel))
        got, _, r = outputs(tmp_path, "%s_%d" % (name, k), "subtree", pb, ["-s", tmp_path / ("s%d.txt" % k)])
        want, _, _ = outputs(tmp_path, "%s_%d" % (name, k), "select", pb, ["-s", tmp_path / ("s%d.txt" % k)])
        assert isinstance(got, dict) and got == want, (name, k, r.stderr[-500:])


def test_refusals_and_usage(tmp_path):
    base = ["-i", PB, "-d", tmp_path, "--host"]
    for opt in (["--max-mutation-density", "0.1"], ["-z", "5"], ["-W", "5"], ["-Z"], ["-r", "2"], ["-L", "w.txt"], ["-S", "p.txt"], ["-C", "p.txt"],
                ["-A", "p.txt"], ["-j", "o.json"], ["-N", "5"], ["-X", "5"], ["-x", "5"], ["-y", "n"], ["-R"], ["-M", "m.tsv"], ["-V", "c.tsv"]):
        r = run(base + ["-u", "u.txt"] + opt, ok=False)
        assert r.returncode == 1 and "not supported by matutils-amd extract" in r.stderr, opt
    r = run(base + ["-c", "x"], ok=False)
    assert "No output files requested" in r.stderr
    r = run(base + ["-u", "u.txt", "--bogus"], ok=False)
    assert "unknown option --bogus" in r.stderr and "Usage: matutils-amd subtree" in r.stderr
    help_ = run(["--help"])
    text = help_.stdout + help_.stderr
    assert text.startswith("Usage: matutils-amd subtree")
    for word in ("--host", "select --help", "most recent common ancestor"):
        assert word in text, word
    top = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert top.returncode == 0 and "subtree --help" in top.stdout and "select --help" in top.stdout
    r = subprocess.run([BIN, "introduce"], capture_output=True, text=True)
    assert r.returncode == 1 and "subtree" in r.stderr and "select" in r.stderr
