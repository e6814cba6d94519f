"""The kernels of ugp_nearest.hip do not spill, use no scratch and stay within the LDS they declare (the 2048-bin histogram, the
4096-pair sort buffer, the block scan's per-wave sums): read from the compiler's own resource report."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")
SCAN = 4 * 4   # block_incl_scan: one int per wave
LDS = {"k_flag_segsum": SCAN, "k_flag_scan": SCAN, "k_nk_anchor": 0, "k_nk_hist": 2048 * 4, "k_nk_pick": SCAN, "k_nk_count": SCAN, "k_nk_offsets": 0,
       "k_nk_write": SCAN, "k_nk_sortILb1": 4096 * 8, "k_nk_sortILb0": 0, "k_nk_tobfs": 0}


def test_nearest_kernels_do_not_spill(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-structurizecfg-skip-uniform-regions=1",
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, "ugp_nearest.hip"), "--cuda-device-only",
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
