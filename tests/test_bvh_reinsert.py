"""The reinsertion pass of the BVH builder (pg_bvh.cpp Reinserter, switch PG_BVH_REINSERT) on the CPU, through
tests/csrc/bvh_reinsert_shim.cpp (bvh_shim.cpp plus the tree's SAH cost and the built arrays).

With the pass on, on the six geometries of test_bvh4_build, the empty mesh, a one-triangle mesh and 64 coincident
triangles: the structural checks of both collapsed trees (shim_check, shim_check_wide), the restated closest-hit walk
equal to brute force bit for bit on the rays of test_bvh4_build, and the restated any-hit walk against brute force on
the ray families and with the exclusion rule and cap of test_bvh8_build (its check_family); on the strip and the
coincident mesh more axis-parallel rays with +0.0 / -0.0 components through the any-hit walk.  The cost does not rise, two
builds give the same bytes, PG_BVH_REINSERT=0 gives the arrays of the builder as it was before the pass (their
SHA-256, recorded from that builder, in tests/golden/bvh_unoptimised_sha256.json), deep meshes stay within the depth
bound, and the fallback (PG_BVH_REINSERT=2: the optimised tree dropped as if a collapse had refused it) builds the
unoptimised arrays."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import test_bvh4_build as T
import test_bvh8_build as T8

ROOT = T.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "bvh_unoptimised_sha256.json")
NAMES = T8.NAMES + ["empty", "one", "coincident64"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bvhreinsert") / "libbvhreinsert.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out,
                           os.path.join(ROOT, "tests", "csrc", "bvh_reinsert_shim.cpp"), T.SHIM_SOURCES[1], "-lpthread"])
    L = C.CDLL(out)
    L.shim_build.restype = C.c_int
    L.shim_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.shim_check.argtypes = [C.c_uint32, C.c_void_p]
    L.shim_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    L.shim_order.argtypes = [C.c_void_p]
    L.shim_check_wide.argtypes = [C.c_uint32, C.c_void_p]
    L.shim_trace_any.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    L.shim_sah_cost.restype = C.c_float
    L.shim_max_depth.restype = C.c_uint32
    L.shim_sizes.argtypes = [C.c_void_p]
    L.shim_arrays.argtypes = [C.c_void_p] * 4
    return L


def geometry(pg, name):
    if name == "empty":
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    if name == "one":
        return np.array([[0.3, -1, 2], [1.5, 0.25, 2.5], [-0.5, 1, 3]], np.float32), np.array([[0, 1, 2]], np.uint32)
    if name == "coincident64":
        V = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5]], np.float32)
        return V, np.tile(np.array([[0, 1, 2]], np.uint32), (64, 1))
    V, F = T.geometry(pg, name)
    return np.ascontiguousarray(V, np.float32), np.ascontiguousarray(F, np.uint32)


def nested_shells(n=4096):
    """n concentric tetrahedra, each 0.2 % larger than the one inside it: every box contains all the smaller ones"""
    tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    V = (tet[None] * (1.002 ** np.arange(n))[:, None, None]).reshape(-1, 3).astype(np.float32)
    F = (np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])[None] + 4 * np.arange(n)[:, None, None]).reshape(-1, 3)
    return V, F.astype(np.uint32)


def build(shim, V, F, mode):
    """the arrays (nodes, wnodes, order, tris as bytes), the binary tree's cost and its depth"""
    old = os.environ.get("PG_BVH_REINSERT")
    os.environ["PG_BVH_REINSERT"] = str(mode)
    try:
        assert shim.shim_build(V.ctypes.data, len(V), F.ctypes.data, len(F)) == 1
    finally:
        if old is None:
            del os.environ["PG_BVH_REINSERT"]
        else:
            os.environ["PG_BVH_REINSERT"] = old
    size = np.zeros(4, np.uint64)
    shim.shim_sizes(size.ctypes.data)
    arr = [np.zeros(int(s), np.uint8) for s in size]
    shim.shim_arrays(*[a.ctypes.data for a in arr])
    return [a.tobytes() for a in arr], float(shim.shim_sah_cost()), int(shim.shim_max_depth())


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(len(a).to_bytes(8, "little"))
        h.update(a)
    return h.hexdigest()


def closest_equal(shim, rays, nt):
    rays = np.ascontiguousarray(rays, np.float32)
    walk, brute = np.zeros((len(rays), 2), np.uint32), np.zeros((len(rays), 2), np.uint32)
    shim.shim_trace(rays.ctypes.data, len(rays), walk.ctypes.data, brute.ctypes.data, nt)
    np.testing.assert_array_equal(walk, brute)
    return brute


def any_hit(shim, label, rays, nt):
    rays = np.ascontiguousarray(rays, np.float32)
    walk, brute = np.zeros(len(rays), np.uint32), np.zeros((len(rays), 3), np.uint32)
    shim.shim_trace_any(rays.ctypes.data, len(rays), walk.ctypes.data, brute.ctypes.data, nt)
    T8.check_family(label, walk != 0xFFFFFFFF, brute, brute[:, 2] == 1)
    return brute


@pytest.mark.parametrize("name", NAMES)
def test_optimised_trees_structure_and_walks(pg, shim, name):
    V, F = geometry(pg, name)
    nt = len(F)
    build(shim, V, F, 1)
    info = np.zeros(5, np.uint32)
    shim.shim_check(nt, info.ctypes.data)
    nodes, need, once, bad, depth = (int(x) for x in info)
    assert once == nt, "every triangle in exactly one leaf"
    assert bad == 0, "child boxes contain their subtrees"
    assert need <= T.QSTACK_DEPTH
    T8.check_structure(shim, nt)
    if nt == 0:
        rays = np.array([[0, 0, -1, 1e-5, 0, 0, 1, np.inf], [1, 2, 3, 1e-5, 0, -0.0, -1, 5.0]], np.float32)
        assert (closest_equal(shim, rays, 0)[:, 1] == 0xFFFFFFFF).all()
        assert not any_hit(shim, name, rays, 0).any()
        return
    # closest hits: the rays of test_bvh4_build, none excluded
    brute = closest_equal(shim, T.rays_through(V, F, 2000 if nt > 20000 else 4000, nt), nt)
    assert (brute[:, 1] != 0xFFFFFFFF).mean() > (0.0 if nt == 1 else 0.2)
    # any hit: 20 000 per family on the strip (the unpadded walk missed about 2 rays in 10 000 there), 500 on the
    # large meshes: the brute force is the cost of this test
    fams = T8.ray_families(V, F, 20000 if name == "strip" else (500 if nt > 20000 else 4000))
    if name in ("strip", "coincident64"):
        fams["axis"] = T8.axis_parallel(V, F, 4000, nt + 12)
    for fam, rays in fams.items():
        b = any_hit(shim, f"{name}/{fam}", rays, nt)
        if name in T8.NAMES and nt > 1:  # the families do test the walk
            assert (b[:, 0] > 0).mean() > 0.2, fam


@pytest.mark.parametrize("name", NAMES)
def test_cost_reproducible_and_switch(pg, shim, name):
    V, F = geometry(pg, name)
    off, cost_off, depth_off = build(shim, V, F, 0)
    on, cost_on, depth_on = build(shim, V, F, 1)
    again, cost_again, _ = build(shim, V, F, 1)
    print(f"{name}: SAH cost {cost_off:.4f} -> {cost_on:.4f}, depth {depth_off} -> {depth_on}")
    assert cost_on <= cost_off
    assert on == again and cost_on == cost_again, "two builds of one mesh differ"
    assert depth_on <= max(depth_off, 40)
    with open(GOLDEN) as f:
        assert digest(off) == json.load(f)[name], "PG_BVH_REINSERT=0 is not the builder without the pass"
    if name in ("ajar", "strip"):
        assert cost_on < cost_off and on != off  # the pass does something where there is something to do


@pytest.mark.parametrize("name", ["strip", "shells"])
def test_deep_meshes_and_fallback(pg, shim, name):
    """the strip spans 1 to 1.6e5 and drives the binned build to its depth-32 median fallback; the shells nest 4096
    deep.  The optimised tree stays within the depth bound and passes the collapses' stack checks; with the
    optimised tree dropped (mode 2) the build succeeds with the unoptimised arrays."""
    V, F = T.geometric_strip() if name == "strip" else nested_shells()
    V, F = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(F, np.uint32)
    assert V.max() / np.abs(V[V != 0]).min() > 1e3
    off, cost_off, depth_off = build(shim, V, F, 0)
    on, cost_on, depth_on = build(shim, V, F, 1)
    print(f"{name}: SAH cost {cost_off:.4f} -> {cost_on:.4f}, depth {depth_off} -> {depth_on}")
    assert cost_on <= cost_off and depth_on <= max(depth_off, 40)
    info = np.zeros(5, np.uint32)
    shim.shim_check(len(F), info.ctypes.data)
    assert int(info[2]) == len(F) and int(info[3]) == 0 and int(info[1]) <= T.QSTACK_DEPTH
    T8.check_structure(shim, len(F))
    fallback, cost_fb, depth_fb = build(shim, V, F, 2)
    assert fallback == off and cost_fb == cost_off and depth_fb == depth_off
