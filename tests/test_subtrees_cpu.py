"""`matutils-amd subtrees --host` (matUtils extract -N ... -t ...) without a GPU: every file it writes against the literal restatement
of get_minimum_subtrees in tests/subtrees_ref.py on the hand-shaped .pb fixtures of tests/test_subtree_cpu.py; the cover loop's cases;
the refusals and messages; and that extract, select and subtree go on refusing -N."""
import os
import subprocess

import pytest

from tests import nearest_ref as NR
from tests import stdorder
from tests import subtree_cases as SC
from tests import subtrees_ref as R
from tests import test_subtree_cpu as CPU

BIN, PB = CPU.BIN, CPU.PB


def run(args, ok=True, sub="subtrees"):
    return CPU.run(args, ok, sub)


def written(out):
    return {os.path.join(str(out), f): open(os.path.join(str(out), f), "rb").read() for f in sorted(os.listdir(str(out)))}


def check(tmp_path, tag, pb, arrays, names, samples, n, sorter, named=True, extra=("--host",)):
    """One run against the restatement: the same files with the same bytes.  samples: BFS indices; named: pass them with -s (else no
    selector is given and they must be every leaf)."""
    out = tmp_path / tag
    args = ["-i", pb, "-d", out, "-N", n, "-t", "sub"]
    if named:
        (tmp_path / (tag + ".txt")).write_text("".join(names[v] + "\n" for v in samples))
        args += ["-s", tmp_path / (tag + ".txt")]
    r = run(args + list(extra))
    want, sets, seen = R.files(arrays, names, samples, n, os.path.realpath(str(out)) + "/", "sub", sorter)
    got = written(out)
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for path in want:
        assert got[path] == want[path], (tag, path, got[path][:300], want[path][:300])
    for nw in (p for p in want if p.endswith(".nw")):
        assert want[nw].endswith(b";") and b"\n" not in want[nw]
    assert "Selection step cover (%s): " % ("host" if "--host" in extra else "device") in r.stderr
    return want, sets, seen, r


HAND = ["siblings", "inner_selected", "all_leaves", "deep_lca", "reverted_and_changed", "one_masked", "disagreement", "sstar65", "scaterpillar"]


@pytest.mark.parametrize("name", HAND)
def test_files_on_hand_cases(tmp_path, name):
    case = SC.by_name()[name]
    pb, names = CPU.hand_pb(tmp_path, case)
    sorter = stdorder.StdOrder(tmp_path)
    leaves = NR.Tree(case.arrays).leaves_queue(0)   # get_leaves_ids: what no selector means
    made = 0
    for n in (1, 2, 3, 7):
        _, sets, _, _ = check(tmp_path, "all_%d" % n, pb, case.arrays, names, leaves, n, sorter, named=False)
        made += len(sets)
        some = [v for v in case.sels[min(1, len(case.sels) - 1)] if v in set(leaves)][::-1] or leaves[:1]
        check(tmp_path, "some_%d" % n, pb, case.arrays, names, some, n, sorter)
    assert made > 0


def cover_tree():
    """root - {x - {y - {l1, l2}, l3}, z - {l4, l5}, l6}: six leaves; every position has one reference base."""
    N = SC.N
    return SC.Case("cover", N(["A3G"], [N(["A1C"], [N(["C2T"], [N(["G13A"], tag="l1"), N(["G4A", "T5A"], tag="l2")], tag="y"), N(["T6C"], tag="l3")], tag="x"),
                                        N(["A8G"], [N(["C9T"], tag="l4"), N((), tag="l5")], tag="z"), N(["T12C", "T7C", "T18C"], tag="l6")], tag="root"),
                   "the cover loop's cases", [["l1"]])


def test_cover_loop_cases(tmp_path):
    case = cover_tree()
    t = case.tags
    pb, names = CPU.hand_pb(tmp_path, case)
    sorter = stdorder.StdOrder(tmp_path)
    prefix = lambda tag: os.path.realpath(str(tmp_path / tag)) + "/"
    # a sample that an earlier subtree holds is skipped and is assigned to that subtree
    want, sets, seen, _ = check(tmp_path, "covered", pb, case.arrays, names, [t["l1"], t["l2"], t["l4"]], 2, sorter)
    assert sets == [[t["l1"], t["l2"]], [t["l4"], t["l5"]]] and seen[t["l2"]] == 0
    tsv = want[prefix("covered") + "subtree-assignments.tsv"].decode().split("\n")
    assert tsv[1].split("\t") == [names[t["l1"]], prefix("covered") + "sub-subtree-0.nw"] and tsv[2].split("\t")[1] == tsv[1].split("\t")[1]
    assert tsv[3].endswith("sub-subtree-1.nw") and tsv[4] == ""
    # the first subtree that holds a sample owns it, also when a later one holds it too
    want, sets, seen, _ = check(tmp_path, "first_owner", pb, case.arrays, names, [t["l3"], t["l1"], t["l2"]], 2, sorter)
    assert len(sets) >= 1 and all(seen[v] == min(i for i, s in enumerate(sets) if v in s) for v in seen if seen[v] >= 0)
    # no ancestor has more than N leaves: the sample is marked -1, no file is written for it and the table leaves it out
    for n in (6, 7, 50):
        want, sets, seen, _ = check(tmp_path, "none_%d" % n, pb, case.arrays, names, [t["l1"], t["l6"]], n, sorter)
        assert sets == [] and seen == {t["l1"]: -1, t["l6"]: -1}
        assert list(want) == [prefix("none_%d" % n) + "subtree-assignments.tsv"] and want[prefix("none_%d" % n) + "subtree-assignments.tsv"] == b"samples\tnewick_file\n"
    want, sets, _, _ = check(tmp_path, "most", pb, case.arrays, names, [t["l6"]], 5, sorter)   # one less than the tree
    assert len(sets) == 1 and len(sets[0]) == 5
    # names twice in the sample file: searched once, written twice
    want, sets, _, _ = check(tmp_path, "twice", pb, case.arrays, names, [t["l4"], t["l4"], t["l1"], t["l4"], t["l1"]], 2, sorter)
    assert len(sets) == 2 and want[prefix("twice") + "subtree-assignments.tsv"].count(names[t["l4"]].encode() + b"\t") == 3
    # no selector at all: every leaf, in get_leaves_ids' order
    leaves = NR.Tree(case.arrays).leaves_queue(0)
    want, sets, _, r = check(tmp_path, "every", pb, case.arrays, names, leaves, 3, sorter, named=False)
    assert "using full input tree" in r.stderr and len(want) == len(sets) + 1
    # -u is written as select writes it
    out = tmp_path / "used"
    (tmp_path / "used.txt").write_text("".join(names[t[k]] + "\n" for k in ("l5", "l1")))
    run(["-i", pb, "-d", out, "-N", 2, "-t", "sub", "-u", "u.txt", "-s", tmp_path / "used.txt", "--host"])
    assert open(out / "u.txt").read() == "".join(names[t[k]] + "\n" for k in ("l5", "l1")) and os.path.exists(out / "sub-subtree-1.nw")
    # several rounds give the same files
    for rs in (1, 2, 3):
        check(tmp_path, "rounds_%d" % rs, pb, case.arrays, names, leaves[::-1] + leaves, 2, sorter, extra=("--host", "--round-size", rs))


def test_on_the_fixture_with_a_selector(tmp_path):
    """-m and -s on the pinned fixture: the selection runs exactly as in select (its -u file), then the cover."""
    some = tmp_path / "s.txt"
    model = CPU.SEL.Model()
    some.write_text("".join(s + "\n" for s in model.leaves[::7]))
    a, b = tmp_path / "subtrees", tmp_path / "select"
    r = run(["-i", PB, "-d", a, "-N", 20, "-t", "t", "-u", "u.txt", "-s", some, "--host"])
    CPU.SEL.run(["-i", PB, "-d", b, "-u", "u.txt", "-s", some, "--host"])
    assert open(a / "u.txt", "rb").read() == open(b / "u.txt", "rb").read()
    idx = {n: j for j, n in enumerate(model.names)}
    want, sets, _ = R.files(model.arrays, model.names, [idx[s] for s in model.leaves[::7]], 20, os.path.realpath(str(a)) + "/", "t",
                            stdorder.StdOrder(tmp_path))
    got = written(a)
    got.pop(str(a / "u.txt"))
    assert got == want and len(sets) > 3 and "Minimum subtree files written" in r.stderr


def test_refusals_and_usage(tmp_path):
    base = ["-i", PB, "-d", tmp_path, "--host", "-N", "5", "-t", "t"]
    for opt in (["-j", "o.json"], ["-E"], ["-M", "m.tsv"], ["-X", "5"], ["-x", "5"], ["-K", "f:5"], ["-z", "5"], ["-R"], ["-V", "c.tsv"]):
        r = run(base + opt, ok=False)
        assert r.returncode == 1 and "not supported by matutils-amd extract" in r.stderr, opt
    for opt in (["-o", "o.pb"], ["-v", "o.vcf"], ["-n"], ["--write-mat", "o.pb"], ["--write-vcf", "o.vcf"], ["--no-genotypes"]):
        r = run(base + opt, ok=False)
        assert r.returncode == 1 and "the reference exits" in r.stderr and "extract.cpp:723-730" in r.stderr, opt
    r = run(["-i", PB, "-d", tmp_path, "--host", "-N", "5"], ok=False)
    assert r.returncode == 1 and r.stderr.endswith("ERROR: Either JSON (-j) or Newick (-t) output must be requested alongside -N.")
    r = run(["-i", PB, "-d", tmp_path, "--host", "-N", "5", "-u", "u.txt"], ok=False)
    assert r.returncode == 1 and "must be requested alongside -N" in r.stderr
    for opt in ([], ["-N", "0"], ["-N", "-3"]):
        r = run(["-i", PB, "-d", tmp_path, "--host", "-t", "t"] + opt, ok=False)
        assert r.returncode == 1 and "needs -N/--minimum-subtrees-size" in r.stderr and "Usage: matutils-amd subtrees" in r.stderr, opt
    r = run(base[:-4] + ["-N", "x", "-t", "t"], ok=False)
    assert "bad value x for -N" in r.stderr
    r = run(base + ["--bogus"], ok=False)
    assert "unknown option --bogus" in r.stderr and "Usage: matutils-amd subtrees" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".nw") or f.endswith(".tsv")]
    help_ = run(["--help"])
    text = help_.stdout + help_.stderr
    assert text.startswith("Usage: matutils-amd subtrees")
    for word in ("--minimum-subtrees-size", "--write-tree", "--host", "--reference-ties", "select --help", "subtree-assignments.tsv"):
        assert word in text, word
    assert "--round-size" not in text
    top = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert top.returncode == 0 and "subtrees --help" in top.stdout
    r = subprocess.run([BIN, "introduce"], capture_output=True, text=True)
    assert r.returncode == 1 and "subtrees" in r.stderr


@pytest.mark.parametrize("sub", ["extract", "select", "subtree"])
def test_the_other_subcommands_still_refuse_N(tmp_path, sub):
    for opt in (["-N", "5"], ["--minimum-subtrees-size", "5"]):
        r = run(["-i", PB, "-d", tmp_path, "-u", "u.txt", "-t", "t.nh"] + opt, ok=False, sub=sub)
        assert r.returncode == 1 and "%s is not supported by matutils-amd extract" % opt[0] in r.stderr
    assert not os.listdir(tmp_path)
