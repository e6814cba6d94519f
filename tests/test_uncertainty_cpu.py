"""matutils-amd's argument handling (no device needed) and a self-check of the tests' neighborhood oracle: the literal
restatement of get_neighborhood_size against its closed form on random tie sets."""
import os
import subprocess

import numpy as np
import pytest

from tests import synth
from tests import uncertainty_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "usher_amd", "bin", "matutils-amd")
MAT = os.path.join(ROOT, "tests", "golden", "survey_ref", "syn", "tree.pb")


def _run(*args):
    if not os.path.exists(BIN):
        pytest.fail("matutils-amd is not built (run __graft_entry__.build())")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)


def test_missing_input_mat_is_an_error():
    r = _run("uncertainty", "-s", "x.txt")
    assert r.returncode == 1 and "--input-mat" in r.stderr


def test_dropout_mutations_are_rejected():
    r = _run("uncertainty", "-i", MAT, "-d", "drop.tsv")
    assert r.returncode == 1 and "dropout" in r.stderr


def test_without_samples_nothing_is_computed(tmp_path):
    e = tmp_path / "e.tsv"
    r = _run("uncertainty", "-i", MAT, "-e", str(e))
    assert r.returncode == 0 and not e.exists() and "Processing" not in r.stderr


def test_unknown_subcommand():
    r = _run("summary", "-i", MAT)
    assert r.returncode == 1 and "uncertainty" in r.stderr


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_neighborhood_oracle_matches_closed_form(seed):
    arrays, _ = synth.make_case(700 + seed, n_leaves=150, n_queries=1, n_sites=50, p_masked=0.02 * (seed - 1))
    rng = np.random.default_rng(seed)
    n = arrays["n"]
    for _ in range(60):
        k = int(rng.integers(2, 9))
        ties = rng.choice(n, k, replace=rng.random() < 0.2).tolist()
        if rng.random() < 0.2:
            ties[0] = 0
        assert U.neighborhood_literal(arrays, ties) == U.neighborhood_closed(arrays, ties), ties
