"""The doom probe's emitter bounds (csrc/pg_layout.h pg_emitter_boxes / pg_ray_misses_boxes), on the CPU: every emitter
triangle's vertices lie inside some box, a ray aimed at an emitter triangle from anywhere passes the slab test (the
test must never reject a ray the closest-hit walk could return an emitter for), rays that point away are rejected
(the test is not vacuous), one box per emitter up to PG_EMBOX_MAX and one union beyond."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "embox_shim.cpp")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emboxshim") / "libemboxshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, SRC])
    L = C.CDLL(out)
    L.embox_max.restype = C.c_int
    L.embox_build.restype = C.c_uint32
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _boxes(shim, sc):
    tri_em = np.zeros(len(sc.indices), np.uint32)
    for sh in sc.shapes:
        tri_em[sh.tri_begin:sh.tri_begin + sh.tri_count] = sh.emitter + 1
    boxes = np.zeros((shim.embox_max(), 6), np.float32)
    absmax = C.c_float()
    n = shim.embox_build(_p(sc.positions, C.c_float), _p(sc.indices, C.c_uint32), _p(tri_em, C.c_uint32),
                         C.c_uint32(len(sc.indices)), C.c_uint32(len(sc.emitters)), _p(boxes, C.c_float), C.byref(absmax))
    return boxes[:n], absmax.value, tri_em


def _misses(shim, boxes, absmax, o, d, tmin):
    rays = np.ascontiguousarray(np.concatenate([o, d, tmin[:, None]], 1), np.float32)
    out = np.zeros(len(rays), np.uint8)
    b = np.ascontiguousarray(boxes, np.float32)
    shim.embox_misses(_p(b, C.c_float), C.c_uint32(len(b)), C.c_float(absmax), _p(rays, C.c_float), C.c_uint32(len(rays)),
                      _p(out, C.c_uint8))
    return out.astype(bool)


def _many_lights(S, n):
    sc = S.cornell(32, 32)
    for k in range(n - 1):
        x = 0.3 + 0.5 * k
        V, F = S.quad((x, 1.0, 5.58), (x + 0.2, 1.0, 5.58), (x + 0.2, 1.5, 5.58), (x, 1.5, 5.58), facing=(0, 0, -1))
        sc.add_mesh(V, F, material=3, radiance=(1.0, 1.0, 1.0))
    return sc.finalize()


@pytest.mark.parametrize("scene", ["cornell", "ajar", "kitchen", "two", "ten"])
def test_boxes_hold_the_emitters_and_pass_rays_at_them(pg, shim, scene):
    S = pg.scenes
    sc = {"cornell": lambda: S.cornell(32, 32), "ajar": lambda: S.ajar_door(32, 18, sphere_res=(16, 8)),
          "kitchen": lambda: S.kitchen(32, 18, target_tris=20000), "two": lambda: _many_lights(S, 2),
          "ten": lambda: _many_lights(S, 10)}[scene]()
    boxes, absmax, tri_em = _boxes(shim, sc)
    nem = len(sc.emitters)
    assert len(boxes) == (nem if nem <= shim.embox_max() else 1)
    tris = sc.positions[sc.indices[tri_em > 0]]  # (T, 3, 3)
    assert len(tris) > 0
    V = tris.reshape(-1, 3)
    inside = ((V[:, None, :] >= boxes[None, :, :3]) & (V[:, None, :] <= boxes[None, :, 3:])).all(-1).any(-1)
    assert inside.all()
    # the padding the kernels rely on: 1e-3 of the largest extent plus 1e-3 of the largest |coordinate|, per box
    if len(boxes) == nem:
        for b, e in zip(boxes, range(nem)):
            v = sc.positions[sc.indices[tri_em == e + 1]].reshape(-1, 3)
            pad = 1e-3 * (v.max(0) - v.min(0)).max() + 1e-3 * np.abs(v).max()
            assert (v.min(0) - b[:3] >= 0.999 * pad).all() and (b[3:] - v.max(0) >= 0.999 * pad).all()
    rng = np.random.default_rng(7)
    lo, hi = sc.bounds()
    ctr = tris.mean(1)
    pick = rng.integers(0, len(ctr), 20000)
    # origins all over the scene box, some far outside it, some a hair off the emitter itself
    o = lo + (hi - lo) * rng.uniform(-0.5, 1.5, (len(pick), 3))
    o[::7] *= 1000.0
    o[1::7] = ctr[pick[1::7]] + rng.normal(0, 1e-4, (len(pick[1::7]), 3))
    o = o.astype(np.float32)
    d = ctr[pick] - o
    ln = np.linalg.norm(d, axis=1)
    ok = ln > 0
    d = (d[ok] / ln[ok, None]).astype(np.float32)
    o = o[ok]
    tmin = (1e-4 * np.maximum(np.abs(o).max(1), 1e-4)).astype(np.float32)
    reach = ln[ok] >= tmin  # the centroid lies at t >= tmin
    miss = _misses(shim, boxes, absmax, o, d, tmin)
    assert not miss[reach].any()
    # axis-parallel rays at the centroids (zero direction components)
    for a in range(3):
        oa = ctr.copy()
        oa[:, a] -= 1.0
        da = np.zeros_like(ctr)
        da[:, a] = 1.0
        assert not _misses(shim, boxes, absmax, oa.astype(np.float32), da.astype(np.float32),
                           np.full(len(ctr), 1e-4, np.float32)).any()
    # and the test rejects: from outside every box, pointing away from all of them
    c = 0.5 * (boxes[:, :3].min(0) + boxes[:, 3:].max(0))
    far = hi + (hi - lo)  # beyond the scene's upper corner, hence beyond every box
    away = np.tile((far - c) / np.linalg.norm(far - c), (8, 1)).astype(np.float32)
    assert _misses(shim, boxes, absmax, np.tile(far, (8, 1)).astype(np.float32), away, np.full(8, 1e-4, np.float32)).all()
