"""bench.py on one device.  A plain run prints the headline line and measures nothing beyond its timed steps; `--dump-outputs`
writes the placements of the last timed step.  `--full` adds the keys of every other figure and check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config", "windows"}
FULL_KEYS = {"value_pcie_inclusive", "per_rank", "other_configs", "roofline", "cpu_baseline", "host_buffer_path"}
NODES, QUERIES = 300_000, 2000


def _bench(*flags):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--nodes", str(NODES), "--queries", str(QUERIES)] + list(flags),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    from usher_amd import Placer, QueryBatch, synth
    from bench import RESULT_FIELDS
    steps, warmup, qsets = 2, 1, 4
    d = _bench("--steps", str(steps), "--warmup", str(warmup), "--qsets", str(qsets), "--dump-outputs", str(tmp_path))
    assert HEADLINE_KEYS <= set(d) and not FULL_KEYS & set(d), sorted(d)
    assert "last_step_equals_stream_ordered_call" not in d["config"]
    assert d["unit"] == "placements/s" and d["higher_is_better"] is True and d["steps"] == steps and d["warmup"] == warmup
    assert d["config"]["queries_total"] == QUERIES
    assert d["value"] > 0 and d["value"] == d["windows"]["value_median"] and [d["ms_per_step"]] == d["windows"]["ms_per_step"]
    # the last timed step placed query set (warmup + steps - 1) mod qsets, drawn as bench.py draws it; one handle places it here
    st = synth.SynthTree(NODES, n_sites=1500, seed=1)
    q = st.queries(QUERIES, seed=1000 + 17 + 7919 * ((warmup + steps - 1) % qsets))
    pl = Placer(st.arrays)
    want = pl.place(QueryBatch.from_csr(q["ent_off"], q["pos"], q["ref"], q["nuc"], q["is_missing"]))
    assert d["config"]["nodes"] == pl.info()["n_nodes"]
    pl.close()
    assert not os.path.exists(str(tmp_path / "row_index.npy"))
    for f in RESULT_FIELDS:
        got = np.load(str(tmp_path / (f + ".npy")))
        assert got.dtype == np.float64 and (got == want[f].astype(np.float64)).all(), f


def test_full_run_adds_every_other_figure_and_check():
    d = _bench("--steps", "2", "--warmup", "1", "--cpu-queries", "4", "--full")
    assert HEADLINE_KEYS | FULL_KEYS <= set(d), sorted(d)
    assert d["config"]["last_step_equals_stream_ordered_call"] is True
    assert d["host_buffer_path"]["identical_to_device_path"] is True and d["host_buffer_path"]["two_in_flight"]["identical_to_device_path"] is True
    assert d["roofline"]["kernel_ms_alone"] > 0 and d["cpu_baseline"]["mismatches_vs_gpu"] == 0
    assert d["other_configs"] is None   # (the extra configurations belong to the default 10M-node workload only)
