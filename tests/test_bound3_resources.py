"""The kernels of ugp_bound3.hip do not spill and use no scratch, and their LDS is what DESIGN section 7.2 reasons with when it asks
what fits beside the persistent walks on a CU: the table kernel's counters for 32 tiles (32 rows of 257 words), three arrays of one
word per thread and the 32 open counts; one word per wave in the levels kernel; none in the pairmask kernel.  Read from the compiler's
own resource report.  Every kernel of the file is listed.
(The one-wave table kernel of profiles/b3_one_wave.txt -- 8 256 bytes, 36 VGPRs -- met the bounds set for it, 12 288 bytes and 64 VGPRs,
and lost on speed; it is not in the tree, so there is nothing here to hold to those bounds.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")
LDS = {"k_b3_pairmask": 0, "k_b3_group_tables": 4 * (32 * 257 + 3 * 512 + 32), "k_b3_levels": 4 * 4}


def test_table_kernels_do_not_spill(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-structurizecfg-skip-uniform-regions=1",
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, "ugp_bound3.hip"), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "a.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[b.split()[0]] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[a-z/]+\])?: (\d+)", b)}
    for kernel, lds in LDS.items():
        hits = [v for name, v in seen.items() if kernel in name]
        assert len(hits) == 1, (kernel, list(seen))
        v = hits[0]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (kernel, v)
        assert v["LDS Size"] == lds, (kernel, v)
    assert len(seen) == len(LDS), list(seen)
