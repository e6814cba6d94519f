"""The kernels of the dense searches (ugp_annotate.hip, ugp_uncertainty.hip) and of RIPPLES (ugp_ripples.hip) do not spill, and
the annotate and RIPPLES kernels use no scratch: read from the compiler's own resource report."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")


def _resources(src, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-structurizecfg-skip-uniform-regions=1",
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, src), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "a.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[b.split()[0]] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", b)}
    return seen


def _check(seen, kernels, no_scratch):
    names = " ".join(seen)
    for k in kernels:
        assert k in names, (k, list(seen))
    for name, v in seen.items():
        if no_scratch:
            assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (name, v)


def test_annotate_kernels_do_not_spill(tmp_path):
    _check(_resources("ugp_annotate.hip", tmp_path), ("k_walk", "k_count", "k_desc", "k_events", "k_segsum", "k_score", "k_tiewrite"), True)


@pytest.mark.parametrize("src,kernels,no_scratch", [
    ("ugp_uncertainty.hip", ("k_gather", "k_events", "k_segsum", "k_score", "k_tiecount", "k_tiewrite", "k_final"), False),
    ("ugp_ripples.hip", ("k_count", "k_pairs", "k_merge", "k_fetch"), True),
])
def test_dense_and_ripples_kernels_do_not_spill(src, kernels, no_scratch, tmp_path):
    _check(_resources(src, tmp_path), kernels, no_scratch)
