"""The attach scaffold and the stage timer of usher_amd/csrc/ugp_query.hpp on the host alone: tests/query_scaffold_host.cpp drives
query_attach with a stub state whose build fails after the state exists (the old state stays, the new one, its stream and tables the
attach made are gone) and timed with a run that fails in the warm-up only; the HIP calls are stand-ins, so no device is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scaffold_and_timer_on_the_host(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "query_scaffold_host")
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-x", "hip", "--cuda-host-only",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "usher_amd", "csrc"),
                        os.path.join(ROOT, "tests", "query_scaffold_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 20 and all(l.startswith("ok  ") for l in lines), r.stdout + r.stderr[-1000:]
