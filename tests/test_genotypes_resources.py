"""The kernels of ugp_genotypes.hip do not spill, use no scratch and hold no LDS beyond the block scan's per-wave sums: read from
the compiler's own resource report.  Every kernel of the file is listed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")
SCAN = 4 * 4   # block_incl_scan: one int per wave
LDS = {"k_gt_e2x": 0, "k_gt_owner": 0, "k_gt_mark": 0, "k_flag_segsum": SCAN, "k_gt_rank": SCAN, "k_gt_count": 0, "k_gt_flag": 0,
       "k_gt_compact": SCAN, "k_gt_table": 0, "k_gt_rows": 0}


def test_genotype_kernels_do_not_spill(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-structurizecfg-skip-uniform-regions=1",
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, "ugp_genotypes.hip"), "--cuda-device-only",
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
