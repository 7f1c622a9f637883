"""CPU figures for the reinsertion pass of the BVH builder (pg_bvh.cpp, PG_BVH_REINSERT), through the test shim
tests/csrc/bvh_reinsert_shim.cpp: the binary tree's SAH cost with the pass off and on, buildBvh wall time, and on
C3 the node visits and triangle tests per ray of the closest-hit walk over rays of the kind the dense bounces
trace (origins uniform on the surface area, cosine-distributed about the normal, tmin the ray epsilon).

    python tools/bvh_reinsert_stats.py [--rays 200000]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def load_shim():
    out = os.path.join(tempfile.mkdtemp(prefix="bvhreinsert"), "libbvhreinsert.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out,
                           os.path.join(ROOT, "tests", "csrc", "bvh_reinsert_shim.cpp"),
                           os.path.join(ROOT, "mitsuba-path-guiding_amd", "csrc", "pg_bvh.cpp"), "-lpthread"])
    L = C.CDLL(out)
    L.shim_build.restype = C.c_int
    L.shim_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.shim_sah_cost.restype = C.c_float
    L.shim_visits.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def surface_rays(V, F, n, seed=1):
    rng = np.random.default_rng(seed)
    P = V[F].astype(np.float64)
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    area = 0.5 * np.linalg.norm(nrm, axis=1)
    t = rng.choice(len(F), n, p=area / area.sum())
    u, v = rng.random(n), rng.random(n)
    su = np.sqrt(u)
    o = (1 - su)[:, None] * P[t, 0] + (su * (1 - v))[:, None] * P[t, 1] + (su * v)[:, None] * P[t, 2]
    N = nrm[t] / np.maximum(np.linalg.norm(nrm[t], axis=1, keepdims=True), 1e-300)
    a = np.where(np.abs(N[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    T = np.cross(N, a)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    B = np.cross(N, T)
    r1, r2 = rng.random(n), rng.random(n)
    sr, ph = np.sqrt(r1), 2 * np.pi * r2
    d = (sr * np.cos(ph))[:, None] * T + (sr * np.sin(ph))[:, None] * B + np.sqrt(1 - r1)[:, None] * N
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 7] = o, d, np.inf
    r[:, 3] = 1e-4 * np.maximum(np.abs(r[:, 0:3]).max(1), 1e-4)  # pg_ray_tmin
    return r


def build(L, V, F, mode):
    os.environ["PG_BVH_REINSERT"] = str(mode)
    t0 = time.perf_counter()
    assert L.shim_build(V.ctypes.data, len(V), F.ctypes.data, len(F)) == 1
    return time.perf_counter() - t0, L.shim_sah_cost()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=200000)
    a = ap.parse_args()
    import pgload
    import test_bvh4_build as T
    pg = pgload.load()
    L = load_shim()
    meshes = [("C3 ajar_door", pg.scenes.ajar_door()), ("kitchen 1 M", pg.scenes.kitchen()),
              ("kitchen 334 k", pg.scenes.kitchen(target_tris=334_000)),
              ("courtyard", pg.scenes.sky_courtyard())]
    meshes = [(k, (s.positions.reshape(-1, 3), s.indices.reshape(-1, 3))) for k, s in meshes]
    meshes += [(k, T.geometry(pg, k)) for k in ("ajar", "cornell", "bunny", "strip", "dups", "single")]
    print("%-16s %9s  %9s %9s %7s  %8s %8s" % ("mesh", "tris", "sah off", "sah on", "change", "s off", "s on"))
    for name, (V, F) in meshes:
        V, F = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(F, np.uint32)
        t0, c0 = build(L, V, F, 0)
        t1, c1 = build(L, V, F, 1)
        print("%-16s %9d  %9.3f %9.3f %+6.1f%%  %8.3f %8.3f" % (name, len(F), c0, c1, 100 * (c1 / c0 - 1) if c0 else 0, t0, t1),
              flush=True)
        if name.startswith("C3") and a.rays:
            rays = surface_rays(V, F, a.rays)
            for mode in (0, 1):
                build(L, V, F, mode)
                out = np.zeros(3, np.uint64)
                L.shim_visits(rays.ctypes.data, len(rays), out.ctypes.data)
                print("    reinsert=%d: %.3f node visits, %.3f triangle tests per ray (%.1f %% hit)"
                      % (mode, out[0] / len(rays), out[1] / len(rays), 100.0 * out[2] / len(rays)), flush=True)


if __name__ == "__main__":
    main()
