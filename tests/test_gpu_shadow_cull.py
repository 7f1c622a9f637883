"""Shadow blockers (pg_layout.h "Shadow blockers"): the recording passes count which triangles block the next-event
shadow rays, the host lists up to 8 of them, and the shader resolves a shadow ray that certainly hits a listed
triangle before it is stored, queued or walked.  The list only decides which rays are resolved early, so films, sums
of squares, the serialized SD-tree, the training records and the path statistics are bit-identical with
PG_NO_SHADOW_CULL=1 -- for the fused launches, the unfused ones, and with the tail forced from the second bounce.
On the ajar door (the emitter is in the other room: nearly every shadow ray fails) something must be resolved after
the second pass, so the comparison cannot pass on an idle switch; with the switch off, before any recording pass and
with an environment emitter nothing may be.

The test itself against the walk: wherever pg_blocker_test answers "certainly occluded" for the ajar door's chosen
blockers, pg_trace_rays(any_hit=1) answers occluded -- on random segments from room A to the light, rays aimed at the
blockers' edges and vertices displaced by 1 to 64 ulps, rays that end at the blocker's t (1 +- k 2^-20), k <= 2^12
(both sides of the 2^-10 margin), and rays that start on one.

Measured on an MI355X (profiles/r11_shadow_blockers/tests_shadow.log): ajar door 96 x 54, training 1 + 2 + 4 spp and
an 8-spp final render, 126,598 of 144,238 shadow rays (87.8 %) resolved in the shader, the same in all three launch
variants; Cornell box and courtyard 0 (empty lists).  Blocker test against the walk, 25,000 rays a family, device
test / host helper / walk answering occluded: segments 24,585 / 19,243 / 24,987, edges 967 / 10,225 / 24,545, tmax
9,245 / 7,003 / 16,305, rays starting on a blocker 21 / 1,022 / 13,354 (the host helper tests all eight triangles
whatever their size); no ray where the device test said occluded and the walk did not."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

COUNTED = ("segments", "escaped", "shadow_rays", "records", "culled", "probes")
VARIANTS = {
    "fused": ({}, ()),
    "unfused": ({}, ("PG_NO_RAYS_FUSION", "PG_NO_SHADE_FUSION")),
    "tail": ({"tail_paths": 1 << 30}, ()),
}


def _scene(S, name):
    if name == "ajar":
        return S.ajar_door(96, 54)
    if name == "cornell":
        return S.cornell(96, 96)
    return S.sky_courtyard(64, 48, env=S.sky_envmap(128, 64, sun_radiance=20.0))


def _job(pg, sc, cfg):
    """3 training iterations (1, 2, 4 spp), then an 8-spp final render; everything the job produced"""
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(guiding=1, s_tree_threshold=400.0, **cfg))
    d.upload(sc)
    assert d.stats()["shadow_culled"] == 0
    off, recs, after = 0, [], []
    for it in range(3):
        d.render_pass(2 ** it, off, True)
        rec = d.get_records().reshape(-1, 32)  # in commit order, which no run fixes: compare them sorted
        recs.append(rec[np.lexsort(rec.T[::-1])])
        d.splat_local()
        d.refit(it)
        off += 2 ** it
        after.append(d.stats()["shadow_culled"])
    train_film = d.read_film()
    d.reset_film()
    d.render_pass(8, off)
    out = dict(film=d.read_film(), train_film=train_film, tree=d.get_sdtree(), recs=recs, stats=d.stats(), after=after,
               blockers=d.blockers())
    d.close()
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("scene", ["ajar", "cornell", "courtyard"])
def test_shadow_cull_is_bit_identical(pg, monkeypatch, scene, variant):
    sc = _scene(pg.scenes, scene)
    cfg, env = VARIANTS[variant]
    for name in env:
        monkeypatch.setenv(name, "1")
    monkeypatch.delenv("PG_NO_SHADOW_CULL", raising=False)
    on = _job(pg, sc, cfg)
    monkeypatch.setenv("PG_NO_SHADOW_CULL", "1")
    off = _job(pg, sc, cfg)
    s = on["stats"]
    print(scene, variant, "shadow rays", s["shadow_rays"], "resolved in the shader", s["shadow_culled"],
          "(%.1f %%)" % (100.0 * s["shadow_culled"] / max(1, s["shadow_rays"])), "after each training pass", on["after"],
          "blockers", on["blockers"][1].tolist())
    assert off["stats"]["shadow_culled"] == 0 and off["after"] == [0, 0, 0] and len(off["blockers"][0]) == 0
    assert on["after"][0] == 0  # nothing is listed before the first recording pass has been counted
    if scene == "ajar":
        assert on["after"][1] > 0 and s["shadow_culled"] > on["after"][2]
    if scene == "courtyard":  # an environment emitter: never
        assert s["shadow_culled"] == 0 and len(on["blockers"][0]) == 0
    for k in ("film", "train_film"):
        assert np.array_equal(on[k][0], off[k][0]) and np.array_equal(on[k][1], off[k][1]), k
    assert on["film"][0][..., 3].sum() > 0
    assert np.array_equal(on["tree"], off["tree"])
    assert all(len(a) > 0 and np.array_equal(a, b) for a, b in zip(on["recs"], off["recs"]))
    for k in COUNTED:
        assert on["stats"][k] == off["stats"][k], k


def test_nothing_is_resolved_before_a_recording_pass(pg, monkeypatch):
    from mitsuba_path_guiding_amd.integrator import Device
    monkeypatch.delenv("PG_NO_SHADOW_CULL", raising=False)
    d = Device(pg.capi.default_config(guiding=1))
    d.upload(pg.scenes.ajar_door(96, 54))
    d.render_pass(2, 0)
    st = d.stats()
    assert st["shadow_rays"] > 0 and st["shadow_culled"] == 0 and len(d.blockers()[0]) == 0
    # a tree from outside starts a new job: the list is emptied again
    d.render_pass(2, 2, True)
    assert len(d.blockers()[0]) > 0
    d.put_sdtree(d.get_sdtree())
    assert len(d.blockers()[0]) == 0
    d.close()


def _ulps(x, k):
    """x moved by k ulps (float32, elementwise; k integer array)"""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def host_helper(tmp_path_factory):
    """pg_ray_hits_blockers compiled for the host (tests/csrc/blocker_shim.cpp): (triangles k x 3 x 3, absmax, rays)
    -> the rays it fires on"""
    out = str(tmp_path_factory.mktemp("blkshim") / "libblkshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out,
                           os.path.join(ROOT, "tests", "csrc", "blocker_shim.cpp")])
    L = C.CDLL(out)
    L.blocker_shim_test.restype = C.c_int

    def run(tris, absmax, rays):
        tris = np.ascontiguousarray(tris, np.float32)
        rays = np.ascontiguousarray(rays, np.float32)
        res = np.zeros(len(rays), np.uint32)
        n = L.blocker_shim_test(tris.ctypes.data_as(C.c_void_p), C.c_uint32(len(tris)), C.c_float(absmax),
                                rays.ctypes.data_as(C.c_void_p), C.c_uint32(len(rays)), res.ctypes.data_as(C.c_void_p))
        assert n >= 0
        return res
    return run


def test_blocker_test_implies_the_walk(pg, monkeypatch, host_helper):
    from mitsuba_path_guiding_amd.integrator import Device
    monkeypatch.delenv("PG_NO_SHADOW_CULL", raising=False)
    sc = pg.scenes.ajar_door(96, 54)
    d = Device(pg.capi.default_config(guiding=1, s_tree_threshold=400.0))
    d.upload(sc)
    off = 0
    for it in range(3):
        d.render_pass(2 ** it, off, True)
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    ids, orig = d.blockers()
    assert len(ids) > 0
    tri = sc.positions[sc.indices.reshape(-1, 3)[orig]].astype(np.float64)  # (k, 3 vertices, xyz)
    rng = np.random.default_rng(5)
    n = 25000

    def room_a(m):
        return rng.uniform((0.1, 0.1, 0.1), (4.9, 2.9, 4.9), (m, 3))

    def rays(o, target, tmax):
        o = np.asarray(o, np.float32)
        dd = (np.asarray(target, np.float32) - o).astype(np.float32)  # unnormalised: the target sits at t = 1
        tmin = (np.float32(1e-4) * np.abs(o).max(1)).astype(np.float32)
        return np.concatenate([o, tmin[:, None], dd, np.asarray(tmax, np.float32)[:, None]], 1).astype(np.float32)

    fam = {}
    # random segments between points of room A and the light
    light = np.stack([rng.uniform(6.5, 8.5, n), np.full(n, 2.99), rng.uniform(1.5, 3.5, n)], 1)
    fam["segments"] = rays(room_a(n), light, np.full(n, 1.0 - 1e-3))
    # aimed at the blockers' edges and vertices, displaced by +-1 to 64 ulps per coordinate
    t = tri[rng.integers(0, len(tri), n)]
    e = rng.integers(0, 3, n)
    s = np.where(rng.random(n) < 0.3, 0.0, rng.random(n))[:, None]  # 30 %: the vertex itself
    a, b = t[np.arange(n), e], t[np.arange(n), (e + 1) % 3]
    tgt = _ulps((a + s * (b - a)).astype(np.float32), rng.integers(1, 65, (n, 3)) * rng.choice([-1, 1], (n, 3)))
    fam["edges"] = rays(room_a(n), tgt, np.full(n, 2.0))
    # ending at the blocker's t times (1 +- k 2^-20), k up to 2^12: both sides of the 2^-10 margin
    t = tri[rng.integers(0, len(tri), n)]
    w = rng.uniform(0.15, 0.4, (n, 2))
    tgt = t[:, 0] + w[:, :1] * (t[:, 1] - t[:, 0]) + w[:, 1:] * (t[:, 2] - t[:, 0])
    k = rng.integers(0, 4097, n) * rng.choice([-1, 1], n)
    fam["tmax"] = rays(room_a(n), tgt, 1.0 + k * 2.0 ** -20)
    # starting on a blocker
    t = tri[rng.integers(0, len(tri), n)]
    w = rng.uniform(0.05, 0.45, (n, 2))
    on = t[:, 0] + w[:, :1] * (t[:, 1] - t[:, 0]) + w[:, 1:] * (t[:, 2] - t[:, 0])
    other = np.where(rng.random(n)[:, None] < 0.5, light, room_a(n))
    fam["on_blocker"] = rays(on, other, np.full(n, 1.0 - 1e-3))

    absmax = float(np.abs(sc.positions).max())
    for name, r in fam.items():
        assert np.isfinite(r).all()
        # a condition on the inputs, checked on the host helper: every family but the last holds rays it fires on
        host = host_helper(tri, absmax, r)
        if name != "on_blocker":
            assert host.sum() > 0, name
        fast = d.blocker_test(r, ids)
        walk = d.trace_rays(r, any_hit=True)[:, 0]
        bad = np.flatnonzero((fast == 1) & (walk != 1.0))
        print(name, len(r), "rays: blocker test", int(fast.sum()), "on the host", int(host.sum()), "walk", int(walk.sum()))
        assert len(bad) == 0, (name, r[bad[:4]])
        if name != "on_blocker":
            assert fast.sum() > 0, name
    assert (d.blocker_test(fam["segments"], ids[:0]) == 0).all()  # an empty list answers nothing
    d.close()
