"""The kernels of ugp_mask.hip do not spill, use no scratch and hold no LDS beyond the four partial sums of a block scan, read from
the compiler's own resource report; the list of the file's kernels is complete (k_msk_segsum is compiled for two inputs)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")
SCAN = 4 * 4   # block_incl_scan: one int per wave
LDS = {"k_msk_names": (1, 0), "k_msk_segsum": (2, SCAN), "k_msk_wordscan": (1, SCAN), "k_msk_full": (1, 0), "k_msk_cover": (1, SCAN),
       "k_msk_mark": (1, 0), "k_msk_read": (1, 0), "k_msk_mutations": (1, 0)}   # kernel -> (instances, LDS bytes)


def test_mask_kernels_do_not_spill(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-structurizecfg-skip-uniform-regions=1",
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, "ugp_mask.hip"), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "a.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[b.split()[0]] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[a-z/]+\])?: (\d+)", b)}
    for kernel, (count, lds) in LDS.items():
        hits = [v for name, v in seen.items() if re.search(kernel + r"(?![a-z_])", name)]
        assert len(hits) == count, (kernel, list(seen))
        assert all(h["LDS Size"] == lds for h in hits), (kernel, hits)
    assert len(seen) == sum(c for c, _ in LDS.values()), list(seen)
    for name, v in seen.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
