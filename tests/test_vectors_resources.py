"""The kernels of ugp_vectors.hip do not spill and use no scratch; only the prefix sum holds LDS (its block scan), read from the
compiler's own resource report; the list of the file's kernels is complete."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")
LDS = {"k_vec_count": 0, "k_vec_scan": 32, "k_vec_fill": 0, "k_vec_order": 0}


def test_vectors_kernels_do_not_spill(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-structurizecfg-skip-uniform-regions=1",
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, "ugp_vectors.hip"), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "a.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[b.split()[0]] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[a-z/]+\])?: (\d+)", b)}
    for kernel, lds in LDS.items():
        hits = [v for name, v in seen.items() if re.search(kernel + r"(?![a-z_])", name)]
        assert len(hits) == 1, (kernel, list(seen))
        assert hits[0]["LDS Size"] == lds, (kernel, hits[0])
    assert len(seen) == len(LDS), list(seen)
    for name, v in seen.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
