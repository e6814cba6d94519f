"""A tree without any mutation through a front end on the device: the one input on which the front ends' former copies of the
tree-to-arrays step differed in what they handed to the library (a padded entry array or an empty one).  uh::TreeArrays always
pads; `matutils-amd summarize` on three nodes with no entry must write what its own --host walk writes, byte for byte."""
import os

import pytest

from tests import pb_cases
from tests import test_summary_cpu as CPU
from tests.test_tree_arrays_cpu import CASES

pytestmark = pytest.mark.gpu


def test_summarize_on_a_tree_without_entries(tmp_path):
    pb = str(tmp_path / "t.pb")
    pb_cases.write_pb_arrays(CASES["three_nodes_no_entry"], pb)
    args = ["-i", pb, "-A", "-R", "roho.tsv", "-C", "sample-clades.tsv"]   # as tests/test_summary_gpu.py runs its cases
    CPU.run(args + ["-d", tmp_path / "dev"])
    CPU.run(args + ["-d", tmp_path / "host", "--host"])
    for f in CPU.TABLES:
        assert open(tmp_path / "dev" / f, "rb").read() == open(tmp_path / "host" / f, "rb").read(), f
    assert sorted(os.listdir(tmp_path / "dev")) == sorted(CPU.TABLES)
    assert open(tmp_path / "dev" / "samples.tsv").read().count("\n") == 3   # the header and the two leaves
