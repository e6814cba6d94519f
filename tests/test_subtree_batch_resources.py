"""The kernels of ugp_subtree_batch.hip do not spill, use no scratch and hold exactly the LDS they declare (none; the flag scans of
ugp_scan.hpp, compiled here, hold the block scan's per-wave sums), read from the compiler's own resource report; the list of the
file's own kernels is complete.  The device radix sort's kernels (rocprim, instantiated in this file) are the library's code: they
are held to no register spills; scratch of theirs (a private digit array, by design) is no spill."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")
SCAN32 = 4 * 4   # one sum per wave
LDS = {"k_sbat_lca": 0, "k_sbat_wid": 0, "k_sbat_mark": 0, "k_sbat_kept": 0, "k_sbat_list": 0, "k_sbat_chains": 0, "k_sbat_eflag": 0,
       "k_sbat_winfo": 0, "k_sbat_rootpath": 0, "k_sbat_gather": 0, "k_sbat_merge": 0, "k_sbat_compact": 0, "k_sbat_entoff": 0,
       "k_flag_segsum": SCAN32, "k_flag_scan": SCAN32}


def test_subtree_batch_kernels_do_not_spill(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-structurizecfg-skip-uniform-regions=1",
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, "ugp_subtree_batch.hip"), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "a.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        seen[b.split()[0]] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[a-z/]+\])?: (\d+)", b)}
    own = {name: v for name, v in seen.items() if re.search("k_sbat_|k_flag_", name)}   # the scans of ugp_scan.hpp are compiled here
    assert not [name for name in seen if "k_sub_" in name], "the single call's kernels belong to ugp_subtree.hip"
    for kernel, lds in LDS.items():
        hits = [v for name, v in own.items() if re.search(kernel + r"(?![a-z_])", name)]
        assert len(hits) == 1, (kernel, list(own))
        assert hits[0]["LDS Size"] == lds, (kernel, hits[0])
    assert len(own) == len(LDS), list(own)
    assert len(seen) > len(own), "the radix sort's kernels are missing from the report"
    for name, v in seen.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["ScratchSize"] == 0 or name not in own, (name, v)
