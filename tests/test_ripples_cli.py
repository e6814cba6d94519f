"""usher_amd/bin/ripples-amd against the restatement of ripples/main.cpp (tests/ripples_ref.render): descendants.tsv and
recombination.tsv byte for byte, the branch order of std::sort + std::shuffle, -S/-E, -s (CRLF lines included), and the
argument and sample-file errors."""
import os
import subprocess

import numpy as np
import pytest

from tests import pb_cases
from tests import ripples_ref as RR
from tests.stdorder import StdOrder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "ripples-amd")
SYN = os.path.join(ROOT, "tests", "golden", "survey_ref", "syn", "tree.pb")


def _run(args, cwd=None):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300, cwd=cwd)


def _files(d):
    with open(os.path.join(d, "descendants.tsv")) as f1, open(os.path.join(d, "recombination.tsv")) as f2:
        return f1.read(), f2.read()


@pytest.fixture(scope="module")
def planted_pb(tmp_path_factory):
    d = tmp_path_factory.mktemp("ripples_pb")
    arrays = RR.planted(11, n_leaves=160)
    path = str(d / "planted.pb")
    pb_cases.write_pb_arrays(arrays, path)
    return path, RR.node_named(arrays, "recomb_11")


# ---- no device needed ------------------------------------------------------------------------------------------------

def test_help_and_missing_input():
    p = _run(["-h"])
    assert p.returncode == 0 and "--input-mat" in p.stdout
    p = _run(["-l", "3"])
    assert p.returncode == 1 and "input-mat" in p.stderr


def test_sample_file_errors(tmp_path):
    bad = tmp_path / "bad.txt"
    bad.write_text("node_1 node_2\n")
    p = _run(["-i", SYN, "-s", str(bad), "-d", str(tmp_path / "o")])
    assert p.returncode == 1 and "ERROR: Incorrect format for samples file: %s!" % bad in p.stderr
    unk = tmp_path / "unk.txt"
    unk.write_text("no_such_node\n")
    p = _run(["-i", SYN, "-s", str(unk), "-d", str(tmp_path / "o")])
    assert p.returncode == 1 and "ERROR: Node id no_such_node not found!" in p.stderr
    p = _run(["-i", SYN, "-s", str(tmp_path / "missing.txt")])
    assert p.returncode == 1 and "Could not open the samples file" in p.stderr


def test_empty_slice_writes_headers_and_creates_outdir(tmp_path):
    out = tmp_path / "new_dir"
    p = _run(["-i", SYN, "-d", str(out), "-S", "0", "-E", "0"])
    assert p.returncode == 0, p.stderr
    d, r = _files(str(out))
    assert d == "#node_id\tdescendants\n" and r.startswith("#recomb_node_id\tbreakpoint-1_interval\t") and r.count("\n") == 1


# ---- on the device ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_planted_tree_byte_for_byte(planted_pb, tmp_path):
    path, _ = planted_pb
    so = StdOrder(tmp_path)
    arrays = RR.load_uncondensed(path)
    order = RR.branch_order(arrays, so)
    want = RR.render(arrays, order, so)
    p = _run(["-i", path, "-d", str(tmp_path / "o")])
    assert p.returncode == 0, p.stderr
    got = _files(str(tmp_path / "o"))
    assert got == want
    assert want[1].count("\n") > 1   # the planted recombinant is reported


@pytest.mark.gpu
def test_syn_tree_byte_for_byte_and_slice(tmp_path):
    so = StdOrder(tmp_path)
    arrays = RR.load_uncondensed(SYN)
    opts = dict(l=2, r=100, R=10 ** 7, p=1, n_desc=5)
    cli = ["-l", "2", "-r", "100", "-p", "1", "-n", "5", "-T", "4"]
    order = RR.branch_order(arrays, so, l=2, n_desc=5)
    want = RR.render(arrays, order, so, **opts)
    p = _run(["-i", SYN, "-d", str(tmp_path / "all")] + cli)
    assert p.returncode == 0, p.stderr
    assert _files(str(tmp_path / "all")) == want and want[1].count("\n") > 1
    want = RR.render(arrays, order, so, S=5, E=30, **opts)
    p = _run(["-i", SYN, "-d", str(tmp_path / "part"), "-S", "5", "-E", "30"] + cli)
    assert p.returncode == 0, p.stderr
    assert _files(str(tmp_path / "part")) == want


@pytest.mark.gpu
def test_samples_file_with_crlf(planted_pb, tmp_path):
    path, X = planted_pb
    so = StdOrder(tmp_path)
    arrays = RR.load_uncondensed(path)
    par = np.asarray(arrays["parent"])
    leaf = [j for j in range(arrays["n"]) if par[j] == X][0]
    other = int(np.flatnonzero(par >= 0)[-1])
    names = [arrays["names"][leaf], arrays["names"][other]]
    f = tmp_path / "s.txt"
    f.write_bytes(("\r\n".join(names) + "\r\n").encode())
    want = RR.render(arrays, RR.branch_order(arrays, so, samples=names), so)
    p = _run(["-i", path, "-s", str(f), "-d", str(tmp_path / "o")])
    assert p.returncode == 0, p.stderr
    assert _files(str(tmp_path / "o")) == want and want[1].count("\n") > 1
