"""The probe-occluder helpers (csrc/pg_layout.h "Probe occluders") on the host.

tests/csrc/probe_list_check.cpp, a stand-alone program: on 10^6 random rays against random TriAccel records, whenever
pg_ray_hits_occluders accepts, the plain TriAccel test of the record it names accepts too with tmax = inf, at least
2^-15 E / max|d| past tmin -- the margins only ever remove answers; the margin cases are refused; a long shadow ray's
certain hit (pg_ray_hits_blockers) is always a probe's; and pg_select_listed keeps the 1/64 threshold, the half-share
rule, the cap (16 here, 8 through pg_select_blockers) and sends ties to the lower id.  The same program is what a
sanitizer build runs (g++ -fsanitize=address,undefined -o check tests/csrc/probe_list_check.cpp && ./check).

The factored selection through a shim (tests/csrc/occluder_shim.cpp): given count arrays, the expected ids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")


def test_probe_list_helpers_on_the_host(tmp_path):
    exe = str(tmp_path / "probe_list_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(CSRC, "probe_list_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 12


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("occshim") / "liboccshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out,
                           os.path.join(CSRC, "occluder_shim.cpp")])
    L = C.CDLL(out)
    L.occluder_shim_select.restype = C.c_uint32
    L.occluder_shim_list_max.restype = C.c_uint32

    def run(counts, total, cap=None):
        counts = np.ascontiguousarray(counts, np.uint32)
        cap = L.occluder_shim_list_max() if cap is None else cap
        ids = np.full(cap, 0xFFFFFFFF, np.uint32)
        n = L.occluder_shim_select(counts.ctypes.data_as(C.c_void_p), C.c_uint32(len(counts)), C.c_uint64(total),
                                   C.c_uint32(cap), ids.ctypes.data_as(C.c_void_p))
        return ids[:n].tolist()
    run.list_max = L.occluder_shim_list_max()
    return run


def _expected(counts, total, cap):
    """The rule in plain Python: each >= total / 64, descending by count then ascending by id, the first cap of them,
    kept only if together >= half of total."""
    if total == 0:
        return []
    ids = [t for t, c in enumerate(counts) if c > 0 and c * 64 >= total]
    ids.sort(key=lambda t: (-int(counts[t]), t))
    ids = ids[:cap]
    return ids if 2 * sum(int(counts[t]) for t in ids) >= total else []


def test_selection_returns_the_expected_ids(select):
    assert select.list_max == 16
    # a room: six walls of two triangles take nearly everything, clutter the rest
    counts = np.zeros(5000, np.uint32)
    walls = [17, 18, 400, 401, 1200, 1201, 3000, 3001, 3002, 3003, 4998, 4999]
    counts[walls] = [900, 850, 700, 700, 640, 600, 500, 450, 300, 300, 200, 150]
    rng = np.random.default_rng(3)
    clutter = rng.choice(np.setdiff1d(np.arange(5000), walls), 300, replace=False)
    counts[clutter] = 10
    total = int(counts.sum()) + 710  # 710 probes escaped
    assert total == 10000  # the threshold is 156.25
    got = select(counts, total)
    assert got == _expected(counts, total, 16)
    assert got == [17, 18, 400, 401, 1200, 1201, 3000, 3001, 3002, 3003, 4998]  # 150 * 64 < total: 4999 is out
    assert select(counts, total, cap=8) == got[:8]
    # listed triangles that took less than half: nothing
    assert select(counts, 4 * total) == []
    assert select(np.zeros(10, np.uint32), 0) == [] and select(np.zeros(10, np.uint32), 4096) == []
    # random counts at both capacities agree with the rule
    for seed in range(20):
        rng = np.random.default_rng(seed)
        c = np.where(rng.random(2000) < 0.02, rng.integers(1, 2000, 2000), rng.integers(0, 3, 2000)).astype(np.uint32)
        tot = int(c.sum() * rng.choice([1.0, 1.5, 2.5]))
        for cap in (8, 16):
            assert select(c, tot, cap) == _expected(c, tot, cap), (seed, cap)
