"""The library's shadow-ray BVH (pg_bvh.cpp buildWide: 8-wide nodes with quantised child boxes, pg_layout.h "8-wide
BVH node") built and walked on the CPU through the test-only shim (tests/csrc/bvh_shim.cpp).

Structure (shim_check_wide): every triangle in exactly one leaf slot, every decoded child box containing its subtree,
leaf slots within the walk's 24-bit triangle mask, no slot both inner and leaf, inner children consecutive in slot
order, and the depth the builder reports within the stack limit.

Walk (shim_trace_any): a scalar restatement of the device's any-hit walk (pg_trace.h traverseWide<true>) against a
brute-force loop over the same triangle records, on rays through the scene with tmax = inf, the same rays cut to a
finite tmax, surface-to-surface segments with the shadow rays' epsilons, and axis-parallel rays.  Exact in both
directions: an "occluded" of the walk names a triangle the brute force accepts (every ray), and where the brute force
accepts a triangle at a t inside that triangle's own box the walk says occluded.  Rays whose accepted triangles all
lie outside their own boxes (test_bvh4_build.consistent_hits: an fp32 TriAccel t of a grazing ray far from the origin
can be ~100 ulps off, and no box walk can be required to open that box) are excluded from the second assertion only
and counted.  The GPU walk is held to the same references in test_gpu_parity.test_any_hit_matches_bruteforce."""
import numpy as np
import pytest

import test_bvh4_build as T

STACK_DEPTH = 48  # pg_trace.h STACK_DEPTH, the limit the library passes to buildBvh
NAMES = ["ajar", "cornell", "bunny", "strip", "dups", "single"]
# Share of the occluded rays of a family that may be excluded (no box-consistent accepted triangle).  The bar of the
# 4-wide test for the same geometries is 3 % (test_gpu_parity.test_trace_matches_bruteforce); measured here, with the
# rays below, no ray of any geometry or family (inf / finite / segment / axis) is excluded -- an any-hit ray needs
# only one of its accepted triangles to be consistent -- so the cap is that 0 rounded up to the next 0.1 %.  The
# share depends on the rays and the brute force only, not on the walk under test: the GPU test sees the same one.
EXCLUDED_CAP = 0.001

_cache = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return T.build_shim(tmp_path_factory)


def build(shim, V, F):
    V, F = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(F, np.uint32)
    assert shim.shim_build(V.ctypes.data, len(V), F.ctypes.data, len(F)) == 1
    return V, F


def ray_count(name, nt):
    """100 000 per family on the strip: about 2 unpadded walks in 10 000 missed their triangle there, and the
    test has to see that rate; the other geometries as the 4-wide test"""
    return 100_000 if name == "strip" else (2000 if nt > 20000 else 4000)


def segments(V, F, n, seed):
    """surface-to-surface segments, the shape of a next-event shadow ray: from a random point of a random triangle to
    a random point of another, tmin = 1e-4 max|o|, tmax = dist (1 - 1e-3) (DESIGN.md section 4 "Epsilons")"""
    rng = np.random.default_rng(seed)
    nt = len(F)
    i = rng.integers(0, nt, n)
    j = (i + 1 + rng.integers(0, max(nt - 1, 1), n)) % nt

    def point(t):
        u, v = rng.random(n), rng.random(n)
        flip = u + v > 1
        u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
        P = V[F[t]].astype(np.float64)
        return P[:, 0] * (1 - u - v)[:, None] + P[:, 1] * u[:, None] + P[:, 2] * v[:, None]

    a, b = point(i), point(j)
    dist = np.linalg.norm(b - a, axis=1)
    ok = dist > 0
    d = np.zeros_like(a)
    d[ok] = (b - a)[ok] / dist[ok, None]
    d[~ok] = (1.0, 0.0, 0.0)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 4:7] = a, d
    r[:, 3] = np.float32(1e-4) * np.abs(r[:, 0:3]).max(1)
    r[:, 7] = (dist * (1 - 1e-3)).astype(np.float32)
    return r


def axis_parallel(V, F, n, seed):
    """rays with one or two direction components exactly zero (+0.0 and -0.0), through a triangle centroid, from
    inside and outside the scene box: the walk's copysignf(eps, d) reciprocals"""
    rng = np.random.default_rng(seed)
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    rad = np.linalg.norm(hi - lo) / 2 + 1e-3
    c = V[F[rng.integers(0, len(F), n)]].astype(np.float64).mean(1)
    d = rng.normal(size=(n, 3))
    zero = np.zeros((n, 3), bool)
    zero[np.arange(n), rng.integers(0, 3, n)] = True  # one zero component ...
    two = rng.random(n) < 0.5
    zero[np.arange(n), rng.integers(0, 3, n)] |= two  # ... and for about a third of the rays a second one
    d[zero] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = c - d * (rad * 2.0 * rng.random(n))[:, None]  # up to a scene diameter back: inside and outside the box
    d[zero & (rng.random((n, 3)) < 0.5)] = -0.0
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 1e-5, d, np.inf
    assert (r[:, 4:7] == 0).any(1).all()
    return r


def ray_families(V, F, n):
    """{family: rays} of one geometry, n rays each: (a) rays_through with tmax = inf, (b) the same rays with tmax
    uniform in 0.5 to 1.5 times the distance to the centroid they were aimed at, (c) surface-to-surface segments; and
    300 axis-parallel rays"""
    nt = len(F)
    inf, target = T.rays_through(V, F, n, nt + 8, targets=True)
    finite = inf.copy()
    dist = np.linalg.norm(target - inf[:, 0:3].astype(np.float64), axis=1)
    finite[:, 7] = dist * (0.5 + np.random.default_rng(nt + 9).random(n))
    return {"inf": inf, "finite": finite, "segment": segments(V, F, n, nt + 10), "axis": axis_parallel(V, F, 300, nt + 11)}


def references(pg, shim, name, n=None):
    """(V, F, {family: (rays, walk, brute)}) of one geometry with n rays per family (default: ray_count), computed
    once per session: walk[i] = the restated walk's BVH-order triangle or ~0; brute[i] = (accepted triangles, 1 if
    one of them is box-consistent, 1 if the walk's triangle is accepted)"""
    V, F = T.geometry(pg, name)
    n = n or ray_count(name, len(F))
    if (name, n) not in _cache:
        V, F = build(shim, V, F)
        out = {}
        for fam, rays in ray_families(V, F, n).items():
            rays = np.ascontiguousarray(rays, np.float32)
            walk = np.zeros(len(rays), np.uint32)
            brute = np.zeros((len(rays), 3), np.uint32)
            shim.shim_trace_any(rays.ctypes.data, len(rays), walk.ctypes.data, brute.ctypes.data, len(F))
            for a in (rays, walk, brute):
                a.setflags(write=False)
            out[fam] = (rays, walk, brute)
        _cache[name, n] = (V, F, out)
    return _cache[name, n]


def check_family(label, occ, brute, accepted_ok):
    """The assertions of both the CPU and the GPU test.  occ: the walk's answers; accepted_ok: where occ, whether
    what the walk accepted is accepted by brute force.  Returns the printed figures."""
    hit, consistent = brute[:, 0] > 0, brute[:, 1] == 1
    excluded = hit & ~consistent
    false_pos = int((occ & ~accepted_ok).sum())
    false_miss = int((consistent & ~occ).sum())
    share = excluded.sum() / max(int(hit.sum()), 1)
    print(f"{label}: {len(occ)} rays, {int(hit.sum())} occluded by brute force, walk occluded {int(occ.sum())}, "
          f"false positives {false_pos}, false misses {false_miss}, excluded {int(excluded.sum())} ({share:.5f})")
    assert false_pos == 0, f"{label}: the walk accepted what brute force does not on {false_pos} rays"
    assert false_miss == 0, f"{label}: {false_miss} rays with a box-consistent accepted triangle walked free"
    assert share < EXCLUDED_CAP, f"{label}: {share:.5f} of the occluded rays excluded"
    return false_pos, false_miss, share


def check_structure(shim, nt):
    info = np.zeros(9, np.uint32)
    shim.shim_check_wide(nt, info.ctypes.data)
    nodes, once, bad_box, bad_leaf, bad_both, bad_ref, depth, wide_depth, limit = (int(x) for x in info)
    print(f"8-wide tree: {nodes} nodes, depth {depth}")
    assert once == nt, "every triangle in exactly one leaf slot"
    assert bad_box == 0, "decoded child boxes contain their subtrees"
    assert bad_leaf == 0, "leaf slots: count 1..3, offset + count <= 24"
    assert bad_both == 0, "no slot both inner and leaf"
    assert bad_ref == 0, "inner children consecutive in slot order, triangles in range"
    assert depth == wide_depth, "BvhOut::wide_depth is the tree's depth"
    assert limit == STACK_DEPTH and wide_depth + 1 <= limit
    return nodes, depth


@pytest.mark.parametrize("name", NAMES)
def test_bvh8_structure(pg, shim, name):
    V, F = build(shim, *T.geometry(pg, name))
    nodes, depth = check_structure(shim, len(F))
    assert nodes >= 1
    if name == "single":
        assert (nodes, depth) == (1, 1)
    if name == "strip":
        assert depth > 8  # deeper than the walk's LDS stack (pg_trace.h WIDE_LDS_STACK): the overflow ring is used


def test_bvh8_structure_empty(shim):
    """no triangles: one childless node, every ray free"""
    V, F = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    assert shim.shim_build(V.ctypes.data, 0, F.ctypes.data, 0) == 1
    assert check_structure(shim, 0) == (1, 1)
    rays = np.array([[0, 0, -1, 1e-5, 0, 0, 1, np.inf], [1, 2, 3, 1e-5, 0, -0.0, -1, 5.0]], np.float32)
    walk, brute = np.zeros(2, np.uint32), np.zeros((2, 3), np.uint32)
    shim.shim_trace_any(rays.ctypes.data, 2, walk.ctypes.data, brute.ctypes.data, 0)
    assert (walk == 0xFFFFFFFF).all() and not brute.any()


@pytest.mark.parametrize("name", NAMES)
def test_bvh8_walk_matches_bruteforce(pg, shim, name):
    """Measured: no false positive, no false miss and an excluded share of 0 on every geometry and family.  The
    walk as it was before wideRay's padding missed 16 (tmax = inf) and 10 (finite tmax) of the strip's 57 752 and
    33 234 occluded rays, and 93 to 187 of each geometry's 300 axis-parallel rays (the -0.0 components)."""
    V, F, fams = references(pg, shim, name)
    failed = []
    for fam, (rays, walk, brute) in fams.items():
        try:
            check_family(f"{name}/{fam}", walk != 0xFFFFFFFF, brute, brute[:, 2] == 1)
        except AssertionError as e:  # every family's figures are printed before the test fails
            failed.append(str(e))
        # the families do test the walk: they hit, and the finite ones also end in front of what they were aimed at
        if name != "single":
            assert (brute[:, 0] > 0).mean() > 0.2, fam
        if fam == "finite":
            assert (brute[:, 0] == 0).mean() > 0.01, fam
    assert not failed, failed
