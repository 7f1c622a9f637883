"""The interleaved camera map in closed form (csrc/pg_kernels.h pg_camera_slot), compiled for the host as a stand-alone
program (tests/csrc/camera_map_check.cpp): over the chunk sizes the fused first launch is tested at, every size up to
three 64 x 64 blocks of the map and layered chunks up to 2^27 paths, (shard, entry) -> slot is a bijection onto
[0, npix * nlayers) with the shard counts of pg_camera_count, and it is the inverse of the map k_camera stores."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "camera_map_check.cpp")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_camera_map_on_the_host(tmp_path):
    exe = str(tmp_path / "camera_map_check")
    # pg_kernels.h declares the launchers too: the HIP headers, host side only (as the Makefile's host objects)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE,
                           "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 4
