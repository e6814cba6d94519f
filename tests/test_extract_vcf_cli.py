"""`matutils-amd extract -v` end to end on the survey tree: the written VCF byte for byte against the literal restatement of make_vcf
(tests/genotypes_ref.py) run, as the reference does, on the subtree extract_main hands to make_vcf with the selected samples.  The
--host-genotypes cases need no GPU."""
import gzip
import os
import re
import subprocess

import pytest

from oracle import refio
from tests import genotypes_ref as G
from tests import nearest_ref as NR
from tests import usher_model as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
PB = os.path.join(ROOT, "tests", "golden", "survey_ref", "global", "global_assignments.pb")


class Model:
    def __init__(self):
        self.T = refio.load_mutation_annotated_tree(PB)
        UM.uncondense_leaves(self.T)
        self.arrays = refio.tree_to_bfs_arrays(self.T)
        self.leaves = [n.identifier for n in UM.get_leaves(self.T)]
        self.chrom = next(m.chrom for n in self.T.depth_first_expansion() for m in n.mutations)

    def vcf(self, samples=None, genotypes=True):
        """make_vcf(subtree, ..., samples): the whole tree when nothing is selected."""
        S = UM.get_subtree(self.T, samples) if samples else self.T
        arrays = refio.tree_to_bfs_arrays(S)
        index = {s: j for j, s in enumerate(arrays["names"])}
        return G.literal(arrays, [index[s] for s in samples] if samples else None, genotypes, self.chrom).text

    def nearby(self, name, k):
        index = {s: j for j, s in enumerate(self.arrays["names"])}
        return [self.arrays["names"][v] for v in NR.literal(NR.Tree(self.arrays), index[name], k)["nodes"]]


@pytest.fixture(scope="module")
def model():
    return Model()


def _run(args, tmp_path, ok=True):
    r = subprocess.run([BIN, "extract", "-i", PB, "-d", str(tmp_path)] + args, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


def _cases(model, tmp_path, extra):
    some = model.leaves[4::9]
    (tmp_path / "samples.txt").write_text("\n".join(some) + "\n")
    _run(["-v", "out.vcf"] + extra, tmp_path)                       # -v alone satisfies the output-file check
    assert open(tmp_path / "out.vcf").read() == model.vcf()
    _run(["-v", "n.vcf", "-n"] + extra, tmp_path)
    assert open(tmp_path / "n.vcf").read() == model.vcf(genotypes=False)
    _run(["--write-vcf", "out.vcf.gz"] + extra, tmp_path)
    raw = open(tmp_path / "out.vcf.gz", "rb").read()
    assert raw[:2] == b"\x1f\x8b" and gzip.decompress(raw).decode() == model.vcf()
    _run(["-s", str(tmp_path / "samples.txt"), "-v", "s.vcf", "-u", "u.txt"] + extra, tmp_path)
    assert open(tmp_path / "s.vcf").read() == model.vcf(some)
    _run(["-s", str(tmp_path / "samples.txt"), "-v", "sn.vcf", "--no-genotypes"] + extra, tmp_path)
    assert open(tmp_path / "sn.vcf").read() == model.vcf(some, genotypes=False)


def test_host_genotypes(model, tmp_path):
    _cases(model, tmp_path, ["--host-genotypes"])


@pytest.mark.gpu
def test_device_genotypes(model, tmp_path):
    _cases(model, tmp_path, [])
    for f in ("out.vcf", "n.vcf", "s.vcf", "sn.vcf"):
        os.rename(tmp_path / f, tmp_path / ("dev_" + f))
    _cases(model, tmp_path, ["--host-genotypes"])
    for f in ("out.vcf", "n.vcf", "s.vcf", "sn.vcf"):
        assert open(tmp_path / f, "rb").read() == open(tmp_path / ("dev_" + f), "rb").read(), f
    said = [re.search(r"VCF of (\d+) sites x (\d+) samples", _run(["-v", "m.vcf"] + extra, tmp_path).stderr).groups() for extra in ([], ["--host-genotypes"])]
    assert said[0] == said[1] == (str(len(model.vcf().splitlines()) - 2), str(len(model.leaves)))


@pytest.mark.gpu
def test_nearest_k_neighbourhood(model, tmp_path):
    s = model.leaves[len(model.leaves) // 3]
    want = model.nearby(s, 20)
    _run(["-k", s + ":20", "-v", "near.vcf", "-u", "u.txt"], tmp_path)
    text = open(tmp_path / "near.vcf").read()
    cols = text.splitlines()[1].split("\t")[9:]
    used = open(tmp_path / "u.txt").read().split()
    assert used == want and sorted(cols) == sorted(used)
    S = UM.get_subtree(model.T, want)
    order = [n.identifier for n in S.depth_first_expansion() if n.identifier in set(want)]
    assert cols == order
    assert text == model.vcf(want)


def _two_chromosomes(model, tmp_path, extras):
    raw = open(PB, "rb").read()
    name = model.chrom.encode()
    assert raw.count(name) > 1 and len(name) > 2
    other = name[:-1] + (b"X" if name[-1:] != b"X" else b"Y")   # the same length: the message stays well-formed
    (tmp_path / "two.pb").write_bytes(raw.replace(name, other, 1))
    for extra in extras:
        r = subprocess.run([BIN, "extract", "-i", str(tmp_path / "two.pb"), "-d", str(tmp_path), "-v", "x.vcf"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "more than one chromosome" in r.stderr, r.stderr[-1000:]


def test_two_chromosomes_are_rejected(model, tmp_path):
    _two_chromosomes(model, tmp_path, (["--host-genotypes"], ["--host-genotypes", "-n"]))


@pytest.mark.gpu
def test_two_chromosomes_are_rejected_on_the_device_path(model, tmp_path):
    _two_chromosomes(model, tmp_path, ([], ["-n"]))


def test_output_file_check(tmp_path):
    r = subprocess.run([BIN, "extract", "-i", PB, "-d", str(tmp_path), "-n"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "No output files requested" in r.stderr
