"""The shadow-blocker helpers (csrc/pg_layout.h "Shadow blockers"), compiled for the host as a stand-alone program
(tests/csrc/blocker_check.cpp): on 10^6 random rays against random TriAccel records, whenever pg_ray_hits_blockers
accepts, the plain TriAccel test of the same record accepts too, with t, u, v inside the unshrunk bounds -- the margins
only ever remove answers; the margin cases (a zero direction component, a grazing ray, a ray that ends within 2^-10 of
the blocker, a triangle too small for the scene) are refused; and pg_select_blockers keeps the 1/64 threshold, the cap
at 8, an empty list for empty counts or when the listed triangles blocked less than half of all shadow rays, and
sends ties to the lower triangle id."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "blocker_check.cpp")


def test_blocker_helpers_on_the_host(tmp_path):
    exe = str(tmp_path / "blocker_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 10
