"""`matutils-amd subtrees` on the device against its own --host output, byte for byte: on the hand-shaped .pb fixtures without
--reference-ties, with a neighbourhood size per fixture at which Placer.nearest_k says that every sample's nearest set is unique (the
n_at_cut rule of ugp_nearest_k), so that no query needs leaving out; on a random tree with --reference-ties on both sides; and with
the cover's round size forced small, so that one run crosses several rounds."""
import os
import types

import numpy as np
import pytest

from tests import nearest_ref as NR
from tests import subtree_cases as SC
from tests import summary_cases as SMC
from tests import synth
from tests import test_subtree_cpu as CPU
from tests import test_subtrees_cpu as TC
from usher_amd import Placer

pytestmark = pytest.mark.gpu

# fixture -> neighbourhood sizes at which every leaf's nearest set is unique (asserted below through the device's own counts)
SIZES = {"siblings": (1,), "inner_selected": (2, 3), "all_leaves": (2,), "deep_lca": (1, 2), "reverted_and_changed": (1,), "one_masked": (1,),
         "disagreement": (1,), "sstar65": (6,), "scaterpillar": (3, 7), "cover": (2,)}


def both(tmp_path, tag, pb, opts, device=(), host=("--host",)):
    """The files of the device run and of the --host run into the same directory (the table holds the files' paths)."""
    out = tmp_path / tag
    rd = TC.run(["-i", pb, "-d", out, "-t", "sub"] + list(opts) + list(device))
    dev = TC.written(out)
    for f in dev:
        os.remove(f)
    rh = TC.run(["-i", pb, "-d", out, "-t", "sub"] + list(opts) + list(host))
    return dev, TC.written(out), rd, rh


def every_set_is_unique(arrays, nodes, n):
    pl = Placer(SMC.topology(arrays))   # the handle takes the bare topology, the nearest tables the entries as they are stored
    pl.nearest_attach(arrays)
    out, dist, info = pl.nearest_k(np.asarray(nodes, np.uint32), n)
    pl.close()
    nleaves = NR.Tree(arrays).nleaves
    for i in range(len(nodes)):
        if not int(info[i]["count"]):
            continue
        taken = dist[i, int(nleaves[int(info[i]["last_anc"])]):int(info[i]["count"])]
        if int(info[i]["n_at_cut"]) != int((taken == int(info[i]["cut_dist"])).sum()):
            return False
    return True


@pytest.mark.parametrize("name", sorted(SIZES))
def test_device_against_host_on_hand_fixtures(tmp_path, name):
    case = TC.cover_tree() if name == "cover" else SC.by_name()[name]
    pb, names = CPU.hand_pb(tmp_path, case)
    leaves = NR.Tree(case.arrays).leaves_queue(0)
    (tmp_path / "rev.txt").write_text("".join(names[v] + "\n" for v in leaves[::-1] + leaves[:3]))
    for n in SIZES[name]:
        assert every_set_is_unique(case.arrays, leaves, n), (name, n)
        dev, host, rd, _ = both(tmp_path, "all_%d" % n, pb, ["-N", n])
        assert dev == host and len(dev) >= 2, (name, n, rd.stderr[-800:])
        assert "Selection step cover (device): " in rd.stderr and "Selection step subtrees (device): " in rd.stderr
        assert ("consecutive mutations at one position disagree" in rd.stderr) == (name == "disagreement")
        dev, host, rd, _ = both(tmp_path, "rev_%d" % n, pb, ["-N", n, "-s", tmp_path / "rev.txt", "-u", "u.txt"], device=("--round-size", 2))
        assert dev == host and len(dev) >= 3, (name, n, rd.stderr[-800:])
        if len(leaves) > 4:
            assert " in 1 rounds" not in rd.stderr


def test_device_against_host_with_reference_ties_on_a_random_tree(tmp_path):
    rng = np.random.default_rng(41)
    arrays, _, _, _ = synth.random_tree(rng, 150, p_masked=0.1, root_muts=1)
    pb, names = CPU.hand_pb(tmp_path, types.SimpleNamespace(name="random150", arrays=arrays))
    ran = 0
    for k, sel in enumerate(SC.selections(arrays, rng)):
        (tmp_path / ("s%d.txt" % k)).write_text("".join(names[int(v)] + "\n" for v in sel))
        for n in ((2, 9) if k % 2 else (5,)):
            dev, host, rd, rh = both(tmp_path, "r%d_%d" % (k, n), pb, ["-N", n, "-s", tmp_path / ("s%d.txt" % k), "--reference-ties"],
                                     device=("--round-size", 3))
            assert dev == host, (k, n, rd.stderr[-800:])
            ran += len(dev) > 1
    dev, host, rd, _ = both(tmp_path, "every", pb, ["-N", 6, "--reference-ties"])
    assert dev == host and len(dev) > 5 and "using full input tree" in rd.stderr
    assert ran >= 6
