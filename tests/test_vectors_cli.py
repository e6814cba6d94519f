"""usher-amd -n and -p with the placement nodes' vectors from the device (--device-vectors: Backend::vectors, one call per batch)
and on the host (--host-vectors): byte for byte the same files, and the reference's recorded placement_stats.tsv /
parsimony-scores.tsv.  Without a GPU the oracle backend has no such hook, and the option must leave the host path as it is."""
import gzip
import os
import re
import subprocess

import pytest

from tests.host_harness import run_usher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "usher-amd")
SURVEY = os.path.join(ROOT, "tests", "golden", "survey_ref")
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures")
RUNS = {"syn-n": (["-i", os.path.join(SURVEY, "syn", "tree.pb"), "-v", os.path.join(SURVEY, "syn", "query.vcf"), "-n"], "placement_stats.tsv",
                  os.path.join(SURVEY, "syn", "o3", "placement_stats.tsv")),
        "global-p": (["-i", os.path.join(SURVEY, "global", "global_assignments.pb"), "-v", os.path.join(FIX, "new_samples.vcf"), "-p"],
                     "parsimony-scores.tsv", os.path.join(SURVEY, "global", "out4", "parsimony-scores.tsv.gz"))}


def _read(path):
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        return f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("run", sorted(RUNS))
def test_device_and_host_vectors_write_the_reference_files(run, tmp_path):
    args, name, gold = RUNS[run]
    out = {}
    for flag in ("--device-vectors", "--host-vectors"):
        d = tmp_path / flag.strip("-")
        d.mkdir()
        r = subprocess.run([BIN] + args + [flag, "-d", str(d)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, USHER_AMD_PROFILE="1"))
        assert r.returncode == 0, r.stderr[-2000:]
        out[flag] = {f: _read(str(d / f)) for f in sorted(os.listdir(str(d)))}
        # the profile says which path answered: the device's calls, the pairs they carried and how many of them were used
        m = re.search(r"vectors from the device: (\d+) calls, (\d+) pairs in [0-9.]+ s, (\d+) of them used", r.stderr)
        if flag == "--device-vectors":
            assert m and int(m.group(1)) >= 1 and int(m.group(2)) >= int(m.group(3)) >= 5, r.stderr[-1500:]
        else:
            assert m is None
    assert out["--device-vectors"] == out["--host-vectors"]
    assert out["--device-vectors"][name] == _read(gold)
    if run == "syn-n":   # the fixture has imputed mutations: the column the device answered is not empty
        assert any(len(l.split(b"\t")) > 3 and l.split(b"\t")[3].strip() for l in out["--device-vectors"][name].splitlines())


@pytest.mark.gpu
def test_help_names_both_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=120)
    assert "--device-vectors" in r.stdout + r.stderr and "--host-vectors" in r.stdout + r.stderr


@pytest.mark.parametrize("run", sorted(RUNS))
@pytest.mark.parametrize("flag", ["--device-vectors", "--host-vectors"])
def test_a_backend_without_the_hook_stays_on_the_host(run, flag, tmp_path):
    args, name, gold = RUNS[run]
    assert run_usher(args + [flag, "-d", str(tmp_path)]) == 0
    assert _read(str(tmp_path / name)) == _read(gold)
