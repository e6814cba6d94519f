"""matUtils mask without a GPU: the closed forms of tests/mask_ref.py against the literal restatement on every hand-shaped case and
on seeded random trees, the cases' own claims, the ABI surface of the ugp_mask calls, and `matutils-amd mask --host` against the
restated mask_main on the annotated fixture and on hand cases: the written tree node by node, the messages, every error."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import refio
from tests import mask_cases as MC
from tests import mask_ref as R
from tests import pb_cases
from tests import usher_model as UM
from usher_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
PB = os.path.join(ROOT, "tests", "golden", "pb_pinned", "ref_written_annotated.pb")
CASES = MC.all_cases()
REFERENCE = {}   # case name -> the literal answers, computed once


def reference(case):
    if case.name not in REFERENCE:
        sets, lines = MC.leaf_sets(case.arrays), MC.lines(case.arrays)
        ref = {"sets": [(s, R.literal_restricted(case.arrays, s)) for s in sets], "lines": lines,
               "mutations": R.literal_mutations(case.arrays, lines)}
        ref["skip"] = ref["sets"][-1][1][1]   # the entries the last set masks, as -s before -m
        ref["skipped"] = R.literal_mutations(case.arrays, lines, ref["skip"])
        REFERENCE[case.name] = ref
    return REFERENCE[case.name]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_closed_forms_equal_literal(case):
    ref, F = reference(case), R.Fast(case.arrays)
    for s, want in ref["sets"]:
        assert same(F.restricted(s), want), s[:20]
    assert same(F.mutations(ref["lines"]), ref["mutations"])
    assert same(F.mutations(ref["lines"], ref["skip"]), ref["skipped"])
    for l in range(0, len(ref["lines"]) if case.arrays["n"] <= 2000 else 1, 7):   # single lines
        assert same(F.mutations(ref["lines"][l:l + 1]), R.literal_mutations(case.arrays, ref["lines"][l:l + 1])), l


def random_tree(rng, n):
    """Breadth-first arrays of a random tree of n nodes: few positions and alleles, so that keys repeat; some entries masked."""
    parent = np.full(n, -1, np.int64)
    for j in range(1, n):
        parent[j] = rng.integers(max(0, j - 6), j) if rng.random() < 0.7 else rng.integers(0, j)
    parent[1:] = np.sort(parent[1:])   # children in increasing index = breadth-first arrays need parent[] non-decreasing
    rows, off = [], [0]
    for j in range(n):
        for _ in range(int(rng.integers(0, 3))):
            p = int(rng.integers(1, 6)) if rng.random() > 0.08 else -1
            rows.append((p, int(rng.choice([1, 2, 4, 8])), int(rng.choice([1, 2, 4, 8, 5]))))
        off.append(len(rows))
    r = np.asarray(rows, np.int64).reshape(len(rows), 3)
    return {"n": n, "parent": parent, "mut_off": np.asarray(off, np.int64), "mut_pos": r[:, 0].astype(np.int32), "mut_ref": r[:, 1].astype(np.int8),
            "mut_par": r[:, 1].astype(np.int8), "mut_nuc": r[:, 2].astype(np.int8), "names": ["n%d" % j for j in range(n)]}


def test_closed_forms_on_random_trees():
    rng = np.random.default_rng(20)
    inner_roots = partly = excluded = 0
    for trial in range(150):
        arrays = random_tree(rng, int(rng.integers(2, 41)))
        F = R.Fast(arrays)
        _, lv, kids = MC.tables(arrays)
        under = [x for x in MC.below(kids, int(rng.integers(0, arrays["n"]))) if not kids[x]]
        named = sorted(set(under) | set(int(x) for x in rng.choice(lv, int(rng.integers(1, len(lv) + 1)), replace=False)))
        if rng.random() < 0.3:
            named = under
        want = R.literal_restricted(arrays, named)
        assert same(F.restricted(named), want), (trial, named)
        inner_roots += any(kids[int(r)] for r in want[0])
        partly += 0 < want[1].sum() < (np.asarray(arrays["mut_pos"]) >= 0).sum()
        lines = []
        for _ in range(int(rng.integers(1, 8))):
            t = int(rng.integers(0, arrays["n"]))
            excl = [int(x) for x in rng.integers(0, arrays["n"] + 2, int(rng.integers(0, 3)))]
            under_t = MC.below(kids, t)[1:]
            if under_t and rng.random() < 0.7:   # strict descendants of the target: the only exclusions that count
                excl += [int(x) for x in rng.choice(under_t, min(2, len(under_t)), replace=False)]
            lines.append((int(rng.integers(0, 7)), int(rng.choice([1, 2, 15, 15])), int(rng.choice([1, 2, 4, 15, 15, 15])), t, excl))
        got, lit = F.mutations(lines, want[1]), R.literal_mutations(arrays, lines, want[1])
        assert same(got, lit), (trial, lines)
        excluded += not same(lit, R.literal_mutations(arrays, [l[:4] + ([],) for l in lines], want[1]))
    assert inner_roots > 50 and partly > 50 and excluded > 5, (inner_roots, partly, excluded)


def test_cases_do_what_they_say():
    by = MC.by_name()
    # the stars: naming the hub's leaves makes the hub the one root, and the named bits end at 63 .. 129
    for k in (63, 64, 65, 128, 129):
        c = by["mstar%d" % k]
        _, lv, kids = MC.tables(c.arrays)
        hub = c.tags["hub"]
        roots, masked = R.literal_restricted(c.arrays, kids[hub])
        assert roots.tolist() == [hub] and len(kids[hub]) == k and 0 < masked.sum() < len(masked)
        pos = np.asarray(c.arrays["mut_pos"])
        assert masked[pos >= 100].sum() > k // 4 and not masked[np.flatnonzero(pos == 100)[-1]]   # A100C also sits outside the hub
    for m in (255, 256, 257):
        assert len(by["entries%d" % m].arrays["mut_pos"]) == m
    # the straddling root: its depth-first range holds position kSeg, and the tree has more than kSeg nodes
    c = by["straddle"]
    F = R.Fast(c.arrays)
    big = c.tags["big"]
    assert c.arrays["n"] > MC.KSEG and F.pre[big] < MC.KSEG < F.pre[big] + F.size[big]
    _, lv, kids = MC.tables(c.arrays)
    roots, masked = R.literal_restricted(c.arrays, kids[big])
    assert roots.tolist() == [big] and 0 < masked.sum() < len(masked)
    assert any(sorted(s) == sorted(kids[big]) for s in MC.leaf_sets(c.arrays))
    # the caterpillar with every leaf named: one root, the tree's own, although every inner node is full and has a leaf child
    c = by["mcaterpillar"]
    _, lv, kids = MC.tables(c.arrays)
    roots, masked = R.literal_restricted(c.arrays, lv)
    assert roots.tolist() == [0] and masked.sum() == (np.asarray(c.arrays["mut_pos"]) >= 0).sum()
    roots, masked = R.literal_restricted(c.arrays, lv[1:])   # all but the leaf beside the spine: the spine's top is the root
    assert roots.tolist() == [c.tags["v1"]]
    # two entries at one position on one node: a line removes the entry it matches, not the first at the position
    c = by["two_at_one"]
    x = c.tags["x"]
    e0 = int(c.arrays["mut_off"][x])
    first, counts = R.literal_mutations(c.arrays, [(7, 1, 4, x, []), (7, 1, 2, x, [c.tags["y"]])])
    assert first[e0:e0 + 3].tolist() == [1, 0, 1] and counts.tolist() == [1, 3]
    # entries masked before stay as they are
    c = by["masked_before"]
    _, lv, _ = MC.tables(c.arrays)
    roots, masked = R.literal_restricted(c.arrays, lv)
    assert not masked[np.asarray(c.arrays["mut_pos"]) < 0].any() and masked.sum() == (np.asarray(c.arrays["mut_pos"]) >= 0).sum()
    # the codes 0 and 15 print alike: N7C outside keeps N7C (code 0) ... the key of entry 0 is its own
    c = by["code_zero"]
    assert refio.Mutation(7, 1, 0, 2).get_string() == refio.Mutation(7, 1, 15, 2).get_string() == "N7C"
    # a full node without a leaf child is no root: `deep` is, until `mid`'s own leaf is named too
    c = by["nested_full"]
    _, lv, kids = MC.tables(c.arrays)
    deep, mid, top = c.tags["deep"], c.tags["mid"], c.tags["top"]
    assert R.literal_restricted(c.arrays, kids[deep])[0].tolist() == [deep]
    under_mid = [v for v in MC.below(kids, mid) if not kids[v]]
    assert R.literal_restricted(c.arrays, under_mid)[0].tolist() == [mid]
    under_top = [v for v in MC.below(kids, top) if not kids[v]]
    assert R.literal_restricted(c.arrays, under_top)[0].tolist() == [top]
    # a named internal node: the roots nest and the counts go below zero -- the closed form does not hold, the literal walk decides
    roots, masked = R.literal_restricted(c.arrays, [mid] + kids[deep])
    assert sorted(roots.tolist()) == sorted([mid, deep])
    # an excluded node that is no strict descendant of the target changes nothing; a strict descendant does
    c = by["polytomy"]
    poly = c.tags["poly"]
    p = c.arrays["parent"][poly]
    plain = R.literal_mutations(c.arrays, [(4, 15, 15, p, [])])
    assert same(R.literal_mutations(c.arrays, [(4, 15, 15, p, [p, 0, c.arrays["n"] + 1])]), plain)
    assert R.literal_mutations(c.arrays, [(4, 15, 15, p, [poly])])[1][0] < plain[1][0]


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "usher_amd.h")).read()
    for name in ("ugp_mask_attach", "ugp_mask_restricted", "ugp_mask_mutations", "ugp_mask_mutations_chunked", "ugp_mask_time"):
        assert re.search(r"\bint %s\(ugp_mat \*mat" % name, hdr) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    L = _lib.lib()   # no handle: an error code, not a crash
    assert L.ugp_mask_attach(None, None) == -1 and L.ugp_mask_restricted(None, 0, None, None, None, 0, None, None) == -1
    assert L.ugp_mask_mutations(None, 0, None, None, None, None, None, None, None, None, None) == -1
    assert L.ugp_mask_mutations_chunked(None, 0, None, None, None, None, None, None, None, None, None, 1) == -1
    assert L.ugp_mask_time(None, 0, None, 0, None, None, None, None, None, None, 1, None, None) == -1


# ---- the command-line tool -------------------------------------------------------------------------------------------------------

def run(args, ok=True):
    r = subprocess.run([BIN, "mask"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert ok is None or (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


def reloaded(node):
    """The node's entries as a save and a load leave them: the loader enters them one by one with add_mutation, which merges two
    entries at one position -- two masked entries at position -1 cancel."""
    n = refio.Node("", None)
    for m in node.mutations:
        n.add_mutation(m.copy())
    return n.mutations


def tree_dump(T):
    """Everything the tests compare of a tree: per node in depth-first order its level, its name (a leaf's: the loader numbers the
    internal nodes anew, as the reference's does), its entries in stored order (masked ones too) and its annotations, then the
    condensed nodes.  Order and levels fix the topology."""
    return ([(n.level, n.identifier if n.is_leaf() else None, [(m.position, m.par_nuc, m.mut_nuc) if m.position >= 0 else "MASKED" for m in reloaded(n)],
              list(n.clade_annotations)) for n in T.depth_first_expansion()],
            {k: list(v) for k, v in T.condensed_nodes.items()})


CONTRACT = ("Restricted roots size:", "Masking mutation ", "Excluding ", "Masked a total of ", "WARNING:", "ERROR:", "mutation_from_string")


def contract_lines(stderr):
    return [line for line in stderr.split("\n") if line.startswith(CONTRACT)]


def write_files(tmp_path, name, files):
    out = {}
    for key, (fname, text) in files.items():
        path = tmp_path / ("%s_%s" % (name, fname))
        with open(path, "w", newline="") as f:
            f.write(text)
        out[key] = path
    return out


def check_run(tmp_path, pb, name, samples=None, mutations=None, csv=False, rename=None, condense=False, extra=("--host",), long_names=False):
    """One option set through the tool and through the restated mask_main; returns (the run, the restated tree)."""
    files = {}
    if samples is not None:
        files["-s"] = ("s.txt", samples)
    if mutations is not None:
        files["-m"] = ("m.csv" if csv else "m.tsv", mutations)
    if rename is not None:
        files["-r"] = ("r.tsv", rename)
    paths = write_files(tmp_path, name, files)
    long_of = {"-s": "--restricted-samples", "-m": "--mask-mutations", "-r": "--rename-samples"}
    out = tmp_path / (name + ".pb")
    args = ["--input-mat" if long_names else "-i", pb, "--output-mat" if long_names else "-o", out]
    for k, p in paths.items():
        args += [long_of[k] if long_names else k, p]
    if condense:
        args.append("--condense-tree" if long_names else "-c")
    T = refio.load_mutation_annotated_tree(str(pb))
    try:
        log = R.mask_main(T, samples, mutations, csv, rename, condense)
    except R.Exit as e:
        r = run(args + list(extra), ok=False)
        assert r.returncode == 1 and str(e) in r.stderr and not os.path.exists(out), (name, r.stderr[-500:])
        return r, None
    r = run(args + list(extra))
    assert contract_lines(r.stderr) == log, name
    assert tree_dump(refio.load_mutation_annotated_tree(str(out))) == tree_dump(T), name
    return r, T


class Fixture:
    def __init__(self):
        self.T = refio.load_mutation_annotated_tree(PB)
        UM.uncondense_leaves(self.T)
        self.leaves = [n.identifier for n in UM.get_leaves(self.T)]
        inner = [n for n in self.T.depth_first_expansion() if not n.is_leaf() and not n.is_root()]
        self.clade = max((n for n in inner if len(UM.get_leaves(self.T, n)) < 100), key=lambda n: len(UM.get_leaves(self.T, n)))
        self.under = [n.identifier for n in UM.get_leaves(self.T, self.clade)]
        self.child = next(c for c in self.clade.children if not c.is_leaf())
        rng = np.random.default_rng(5)
        self.some = [self.leaves[i] for i in rng.permutation(len(self.leaves))[:60]]
        counts = {}
        for n in self.T.depth_first_expansion():
            for m in n.mutations:
                if m.position >= 0:
                    counts[m.get_string()] = counts.get(m.get_string(), 0) + 1
        self.common = sorted(counts, key=lambda s: -counts[s])[:6]
        below = [m.get_string() for n in self.T.depth_first_expansion(self.clade) for m in n.mutations if m.position >= 0]
        self.local = sorted(set(below), key=lambda s: -below.count(s))[:4]

    def option_sets(self):
        """name -> arguments of check_run."""
        names = "".join(s + "\n" for s in self.under + self.some)
        c, ch = self.clade.identifier, self.child.identifier
        wild = ["N" + s[1:] for s in self.common[:2]] + [s[:-1] + "N" for s in self.common[2:4]]
        tsv = "".join(s + "\n" for s in self.common[:2] + wild) + "".join("%s\t%s\n" % (s, c) for s in self.local[:2]) + \
            "".join("%s\t%s\t%s;no_such_node;%s\n" % (s, c, ch, c) for s in ["N" + self.local[0][1:-1] + "N"] + self.local[2:]) + self.common[0] + "\n" + \
            "N%sN\r\n" % self.common[4][1:-1] + "A1C\n"
        return {
            "samples": dict(samples=names),
            "samples_few": dict(samples="".join(s + "\n" for s in self.some[:7])),
            "samples_internal": dict(samples=c + "\n" + "".join(s + "\n" for s in self.some[:5]) + ch + "\n"),
            "mutations": dict(mutations=tsv),
            "mutations_csv": dict(mutations=tsv.replace("\t", ","), csv=True),
            "samples_mutations": dict(samples=names, mutations=tsv),
            "rename": dict(rename="%s\tnew_name\nno_such_node\tx\n%s\tinner_renamed\n" % (self.leaves[3], c)),
            "condense": dict(condense=True),
            "everything": dict(samples=names, mutations=tsv, rename="%s\trenamed\n" % self.leaves[0], condense=True),
        }


@pytest.fixture(scope="module")
def fixture():
    return Fixture()


OPTION_SETS = ("samples", "samples_few", "samples_internal", "mutations", "mutations_csv", "samples_mutations", "rename", "condense", "everything")


@pytest.mark.parametrize("name", OPTION_SETS)
def test_host_on_the_fixture(fixture, tmp_path, name):
    sets = fixture.option_sets()
    assert tuple(sets) == OPTION_SETS
    r, T = check_run(tmp_path, PB, name, long_names=name == "everything", **sets[name])
    assert T is not None
    log = contract_lines(r.stderr)
    if "samples" in name:
        assert name == "samples_few" or sum(l.startswith("Masking mutation") for l in log) > 10, name
    if name == "samples":
        assert int([l for l in log if l.startswith("Restricted roots size:")][0].split()[-1]) >= 2   # the clade's root and lone leaves
    if "mutations" in name:
        total = int([l for l in log if l.startswith("Masked a total of")][0].split()[4])
        assert total > 20 and sum(l.startswith("Excluding %s " % fixture.child.identifier) for l in log) == 3
    if name == "samples_mutations":   # what -s masked is no longer there for -m
        assert total < int([l for l in contract_lines(check_run(tmp_path, PB, "again", **sets["mutations"])[0].stderr) if l.startswith("Masked")][0].split()[4])
    if name == "rename":
        assert T.get_node("new_name") is not None and T.get_node("inner_renamed") is not None and "WARNING: Node no_such_node not found in the MAT." in log
    if name == "condense":
        assert len(T.condensed_nodes) > 0


def hand_pb(tmp_path, name):
    case = MC.by_name()[name]
    pb = tmp_path / (name + ".pb")
    pb_cases.write_pb_arrays(case.arrays, str(pb))
    T = refio.load_mutation_annotated_tree(str(pb))
    return case, pb, [n.identifier for n in T.breadth_first_expansion()]


@pytest.mark.parametrize("name", ["two_at_one", "masked_before", "nested_full", "mstar65", "polytomy"])
def test_host_on_hand_cases(tmp_path, name):
    case, pb, names = hand_pb(tmp_path, name)
    ran = 0
    for k, s in enumerate(MC.leaf_sets(case.arrays)[:6]):
        r, T = check_run(tmp_path, pb, "%s_s%d" % (name, k), samples="".join(names[v] + "\n" for v in s))
        ran += T is not None
    lines = [l for l in MC.lines(case.arrays) if l[0] > 0 and all(x < len(names) for x in l[4])]
    text = "".join("%s%d%s\t%s\t%s\n" % (refio.get_nuc(a), p, refio.get_nuc(b), names[t], ";".join(names[x] for x in ex)) for p, a, b, t, ex in lines)
    r, T = check_run(tmp_path, pb, name + "_m", mutations=text)
    s = MC.leaf_sets(case.arrays)[-1]
    r, T2 = check_run(tmp_path, pb, name + "_sm", samples="".join(names[v] + "\n" for v in s), mutations=text, condense=True)
    assert ran >= 2 and T is not None and T2 is not None


def test_errors_and_refused_options(fixture, tmp_path):
    ok_m = fixture.common[0] + "\n"
    for name, kw, word in [
            ("unknown_sample", dict(samples=fixture.leaves[0] + "\nno_such_sample\n"), "ERROR: Sample missing in input MAT!"),
            ("empty_samples", dict(samples=""), "names no sample"),
            ("unknown_target", dict(mutations=ok_m + "%s\tno_such_node\n" % fixture.common[1]), "ERROR: Internal node no_such_node requested for masking does not exist in the tree. Exiting"),
            ("bad_mutation", dict(mutations=ok_m + "11083T\n"), R.FROM_STRING % "11083T"),
            ("bad_tail", dict(mutations="G11083Tx\n"), R.FROM_STRING_TAIL % "G11083Tx"),
            ("negative", dict(mutations="G-5T\n"), R.FROM_STRING_TAIL % "G-5T"),
            ("empty_line", dict(mutations=ok_m + "\n" + ok_m), "ERROR: Empty line in the mutations file"),
            ("rename_taken", dict(rename="%s\t%s\n" % (fixture.leaves[0], fixture.leaves[1])), "ERROR: rename_node: node with id '%s' already exists." % fixture.leaves[1]),
            ("rename_words", dict(rename="%s\n" % fixture.leaves[0]), "ERROR: Incorrect format for the renaming file"),
            ("rename_three", dict(rename="a\tb\tc\n"), "ERROR: Incorrect format for the renaming file")]:
        r, T = check_run(tmp_path, PB, name, **kw)
        assert T is None and r.returncode == 1 and word in r.stderr, name
    out = tmp_path / "o.pb"
    for opts, word in [(["-o", out], "'--input-mat' is required"), (["-i", PB], "'--output-mat' is required"), (["-i", PB, "-o", out, "-s"], "needs a value"),
                       (["-i", PB, "-o", out, "--bogus"], "unknown option --bogus"), (["-i", PB, "-o", out, "-s", tmp_path / "none.txt"], "Could not open"),
                       (["-i", PB, "-o", out, "-m", tmp_path / "none.txt"], "Could not open"), (["-i", PB, "-o", out, "-r", tmp_path / "none.txt"], "Could not open")]:
        r = run(["--host"] + list(opts), ok=False)
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(out), opts
    for opt in (["-S"], ["--simplify"], ["-M", "m.tsv"], ["--move-nodes", "m.tsv"], ["-D", "3"], ["--max-snp-distance", "3"], ["-f", "d.maple"], ["--maple-file", "d.maple"]):
        r = run(["-i", PB, "-o", out] + opt, ok=False)
        assert r.returncode == 1 and r.stderr == "ERROR: %s is not supported by matutils-amd mask (use the reference matUtils)\n" % opt[0] and not os.path.exists(out)
    help_ = run(["--help"])
    assert help_.stdout.startswith("Usage: matutils-amd mask")
    for word in ("--restricted-samples", "--mask-mutations", "--rename-samples", "--condense-tree", "--host", "depth-first order", "--simplify"):
        assert word in help_.stdout, word
    top = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert top.returncode == 0 and "mask --help" in top.stdout
    r = subprocess.run([BIN, "introduce"], capture_output=True, text=True)
    assert r.returncode == 1 and "select, mask)" in r.stderr
    # the other subcommands keep refusing what they refuse
    r = subprocess.run([BIN, "extract", "-i", PB, "-u", "x.txt", "-d", str(tmp_path), "-c", "x"], capture_output=True, text=True)
    assert r.returncode == 1 and "not supported by matutils-amd extract" in r.stderr
    r = subprocess.run([BIN, "summarize", "-i", PB, "-t", "x.tsv"], capture_output=True, text=True)
    assert r.returncode == 1 and "not supported by matutils-amd summarize" in r.stderr


def test_no_option_is_a_copy(tmp_path):
    """Nothing asked: the tree is loaded, uncondensed and written."""
    r, T = check_run(tmp_path, PB, "copy")
    assert T is not None and contract_lines(r.stderr) == []
