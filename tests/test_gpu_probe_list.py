"""Probe occluders (pg_layout.h "Probe occluders"): the probe rows of the recording passes count which triangles the
doom probes end on, the host lists up to 16 of them, and the tracing kernels answer a probe that certainly hits a
listed triangle without walking the tree.  The list only decides which probes skip the walk, so films, sums of squares,
the serialized SD-tree, the training records and segments / escaped / culled / shadow_rays / records / probes are
bit-identical with PG_NO_PROBE_LIST=1 -- for the fused launches, the unfused ones, and with the tail forced from the
second bounce (k_tail's inline probe always walks and counts nothing, so there the list stays empty).  Every job has
five training iterations and an 8-spp render in chunks of at most 1073 paths, no multiple of the wave.  The fused and
unfused jobs run with the tail off: a chunk this small would otherwise finish in k_tail after its first bounce.

Scenes: the ajar door at 160 x 90 (something must be resolved, so the comparison cannot pass on an idle switch), the
Cornell box at 64 x 64, and a box with its front face removed, lit by a panel under its ceiling, seen from inside: rays
leave through the opening (escaped > 0) while the five faces are listed.

The predicate against the walk (pg_occluder_test), where the walk really misses: one listed triangle in empty space
(rays inside and just outside its edges and vertices, hits on both sides of tmin and of the distance margin, grazing
directions, origins far outside the scene, +-0 components; every margin's refusal asserted from the inputs), and the
open box's learned list (rays that leave through the opening or pass the box by).  Wherever the device predicate says
hit the probe walk says hit, and the device predicate agrees with its host build (tests/csrc/occluder_shim.cpp) on all
but 0.1 % of the rays of a family: the same fp32 arithmetic on the same records, so only a ray within an ulp of a
margin may differ.  Floors on the resolved share are conditions on the inputs, met by the host build first."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

COUNTED = ("segments", "escaped", "shadow_rays", "records", "culled", "probes")
CHUNK = 1073
VARIANTS = {
    "fused": ({"tail_paths": -1}, ()),
    "unfused": ({"tail_paths": -1}, ("PG_NO_RAYS_FUSION",)),
    "tail": ({"tail_paths": 1 << 30}, ()),
}
ITERATIONS = 5


def open_box(pg, width=48, height=48):
    """A 4 x 3 x 4 box without its z = 0 face, a light panel under the ceiling, the camera inside looking at the back
    wall: paths leave through the opening behind the camera."""
    S = pg.scenes
    s = S.Scene()
    s.name = "open_box"
    white = s.add_material(S.material("diffuse", reflectance=(0.7, 0.7, 0.7)))
    V, F = S.box((0, 0, 0), (4, 3, 4), inward=True)
    keep = np.array([i for i in range(6) if i != 4])  # face 4 is z = z0
    s.add_mesh(V, np.concatenate([F[2 * i: 2 * i + 2] for i in keep]), material=white)
    LV, LF = S.quad((1.5, 2.99, 1.5), (2.5, 2.99, 1.5), (2.5, 2.99, 2.5), (1.5, 2.99, 2.5), facing=(0, -1, 0))
    s.add_mesh(LV, LF, material=white, radiance=(10.0, 10.0, 10.0))
    s.set_camera((2.0, 1.5, 0.5), (2.0, 1.5, 4.0), (0, 1, 0), 70.0, width, height)
    return s.finalize()


def _scene(pg, name):
    if name == "ajar":
        return pg.scenes.ajar_door(160, 90)
    if name == "cornell":
        return pg.scenes.cornell(64, 64)
    if name == "open_box":
        return open_box(pg)
    return pg.scenes.sky_courtyard(64, 48, env=pg.scenes.sky_envmap(128, 64, sun_radiance=20.0))


def _u64(d, fn):
    n = C.c_uint64()
    d._chk(fn(d.h, C.byref(n)))
    return n.value


def resolved(d):
    return _u64(d, d.lib.pg_get_probes_resolved)


def occluders(d):
    ids, orig = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    n = C.c_uint32()
    d._chk(d.lib.pg_get_occluders(d.h, ids.ctypes.data_as(C.c_void_p), orig.ctypes.data_as(C.c_void_p), C.byref(n)))
    return ids[: n.value].copy(), orig[: n.value].copy()


def occluder_test(d, rays, tri_ids):
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    ids = np.ascontiguousarray(tri_ids, np.uint32)
    out = np.zeros((len(rays), 2), np.uint32)
    d._chk(d.lib.pg_occluder_test(d.h, rays.ctypes.data_as(C.c_void_p), C.c_uint64(len(rays)),
                                  ids.ctypes.data_as(C.c_void_p), C.c_uint32(len(ids)), out.ctypes.data_as(C.c_void_p)))
    return out[:, 0], out[:, 1]


def _train(d, iterations=ITERATIONS, after=None, recs=None):
    off = 0
    for it in range(iterations):
        d.render_pass(2 ** it, off, True)
        if recs is not None:
            rec = d.get_records().reshape(-1, 32)  # in commit order, which no run fixes: compare them sorted
            recs.append(rec[np.lexsort(rec.T[::-1])])
        d.splat_local()
        d.refit(it)
        off += 2 ** it
        if after is not None:
            after.append(resolved(d))
    return off


def _job(pg, sc, cfg):
    """5 training iterations (1 .. 16 spp), then an 8-spp final render; everything the job produced"""
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(guiding=1, s_tree_threshold=400.0, max_paths_in_flight=CHUNK, **cfg))
    d.upload(sc)
    assert resolved(d) == 0 and len(occluders(d)[0]) == 0
    recs, after = [], []
    off = _train(d, after=after, recs=recs)
    train_film = d.read_film()
    d.reset_film()
    d.render_pass(8, off)
    out = dict(film=d.read_film(), train_film=train_film, tree=d.get_sdtree(), recs=recs, stats=d.stats(), after=after,
               resolved=resolved(d), occluders=occluders(d))
    d.close()
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("scene", ["ajar", "cornell", "open_box"])
def test_probe_list_is_bit_identical(pg, monkeypatch, scene, variant):
    sc = _scene(pg, scene)
    cfg, env = VARIANTS[variant]
    for name in ("PG_NO_RAYS_FUSION", "PG_NO_SHADE_FUSION", "PG_NO_DOOM_PROBE", "PG_NO_PATH_CULL", "PG_NO_PROBE_LIST"):
        monkeypatch.delenv(name, raising=False)
    for name in env:
        monkeypatch.setenv(name, "1")
    on = _job(pg, sc, cfg)
    monkeypatch.setenv("PG_NO_PROBE_LIST", "1")
    off = _job(pg, sc, cfg)
    s = on["stats"]
    print(scene, variant, "probes", s["probes"], "resolved", on["resolved"],
          "(%.1f %%)" % (100.0 * on["resolved"] / max(1, s["probes"])), "after each training pass", on["after"],
          "escaped", s["escaped"], "culled", s["culled"], "occluders", on["occluders"][1].tolist())
    assert off["resolved"] == 0 and off["after"] == [0] * ITERATIONS and len(off["occluders"][0]) == 0
    assert on["after"][0] == 0  # nothing is listed before the first recording pass has been counted
    assert on["resolved"] <= s["probes"]
    if variant == "tail":  # k_tail's probes always walk and are not counted: nothing is ever listed
        assert on["resolved"] == 0 and len(on["occluders"][0]) == 0
    elif scene == "ajar":
        assert on["resolved"] > 0 and len(on["occluders"][0]) > 0
    elif scene == "open_box":  # rays really leave, and a list is selected in the same run
        assert s["escaped"] > 0 and len(on["occluders"][0]) > 0 and on["resolved"] > 0
    if scene == "open_box":
        assert s["escaped"] > 0
    for k in ("film", "train_film"):
        assert np.array_equal(on[k][0], off[k][0]) and np.array_equal(on[k][1], off[k][1]), k
    assert on["film"][0][..., 3].sum() > 0
    assert np.array_equal(on["tree"], off["tree"])
    assert all(len(a) > 0 and np.array_equal(a, b) for a, b in zip(on["recs"], off["recs"]))
    for k in COUNTED:
        assert on["stats"][k] == off["stats"][k], k
    assert s["probes"] > 0


def test_the_list_is_empty_where_it_must_be(pg, monkeypatch):
    from mitsuba_path_guiding_amd.integrator import Device
    for name in ("PG_NO_RAYS_FUSION", "PG_NO_DOOM_PROBE", "PG_NO_PATH_CULL", "PG_NO_PROBE_LIST"):
        monkeypatch.delenv(name, raising=False)
    cfg = dict(guiding=1, s_tree_threshold=400.0, tail_paths=-1)
    d = Device(pg.capi.default_config(**cfg))
    d.upload(_scene(pg, "ajar"))
    assert len(occluders(d)[0]) == 0 and resolved(d) == 0  # after upload
    d.render_pass(2, 0)  # a pass that records nothing lists nothing
    assert d.stats()["probes"] > 0 and len(occluders(d)[0]) == 0 and resolved(d) == 0
    _train(d, 3)
    assert len(occluders(d)[0]) > 0
    d.put_sdtree(d.get_sdtree())  # a tree from outside starts a new job
    assert len(occluders(d)[0]) == 0
    before = resolved(d)
    d.render_pass(2, 16)
    assert resolved(d) == before
    d.close()
    # an environment emitter: no probes, no list
    d = Device(pg.capi.default_config(**cfg))
    d.upload(_scene(pg, "courtyard"))
    _train(d, 3)
    assert d.stats()["probes"] == 0 and len(occluders(d)[0]) == 0 and resolved(d) == 0
    d.close()
    # a scene where nothing qualifies: a sphere of 4608 triangles around the camera and a small light, every triangle
    # far below 1/64 of the probes
    S = pg.scenes
    s = S.Scene()
    s.name = "in_sphere"
    white = s.add_material(S.material("diffuse", reflectance=(0.7, 0.7, 0.7)))
    V, F, N = S.uv_sphere((0, 0, 0), 2.0, nu=96, nv=48)
    s.add_mesh(V, F[:, ::-1].copy(), material=white)
    LV, LF = S.quad((-0.3, 1.2, -0.3), (0.3, 1.2, -0.3), (0.3, 1.2, 0.3), (-0.3, 1.2, 0.3), facing=(0, -1, 0))
    s.add_mesh(LV, LF, material=white, radiance=(10.0, 10.0, 10.0))
    s.set_camera((0, 0, -1.0), (0, 0, 1.0), (0, 1, 0), 60.0, 64, 64)
    d = Device(pg.capi.default_config(**cfg))
    d.upload(s.finalize())
    _train(d, 4)
    assert d.stats()["probes"] > 4096 and len(occluders(d)[0]) == 0 and resolved(d) == 0
    d.close()


def _ulps(x, k):
    """x moved by k ulps (float32, elementwise; k integer array)"""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def host_helper(tmp_path_factory):
    """pg_ray_hits_occluders compiled for the host (tests/csrc/occluder_shim.cpp): (triangles k x 3 x 3, absmax, rays)
    -> the rays it fires on"""
    out = str(tmp_path_factory.mktemp("occshim") / "liboccshim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out,
                           os.path.join(ROOT, "tests", "csrc", "occluder_shim.cpp")])
    L = C.CDLL(out)
    L.occluder_shim_test.restype = C.c_int

    def run(tris, absmax, rays):
        tris = np.ascontiguousarray(tris, np.float32)
        rays = np.ascontiguousarray(rays, np.float32)
        res = np.zeros(len(rays), np.uint32)
        n = L.occluder_shim_test(tris.ctypes.data_as(C.c_void_p), C.c_uint32(len(tris)), C.c_float(absmax),
                                 rays.ctypes.data_as(C.c_void_p), C.c_uint32(len(rays)), res.ctypes.data_as(C.c_void_p))
        assert n >= 0
        return res
    return run


def _rays(o, d, tmin=None):
    o = np.asarray(o, np.float32)
    d = np.asarray(d, np.float32)
    if tmin is None:
        tmin = np.float32(1e-4) * np.maximum(np.abs(o).max(1), np.float32(1e-4))
    tmin = np.asarray(tmin, np.float32)
    return np.concatenate([o, tmin[:, None], d, np.zeros((len(o), 1), np.float32)], 1).astype(np.float32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=1)[:, None]


def _compare(d, host_helper, tri, absmax, ids, name, r):
    """host helper, device predicate and probe walk on rays r; the implication and the agreement hold for every family"""
    assert np.isfinite(r).all()
    host = host_helper(tri, absmax, r)
    fast, walk = occluder_test(d, r, ids)
    print(name, len(r), "rays: occluder test", int(fast.sum()), "on the host", int(host.sum()), "walk", int(walk.sum()),
          "host != device", int((host != fast).sum()))
    bad = np.flatnonzero((fast == 1) & (walk != 1))
    assert len(bad) == 0, (name, r[bad[:4]])
    # one test, one arithmetic (fp32, no contraction, the same records): only a ray within an ulp of a margin may differ
    assert (host != fast).mean() <= 1e-3, (name, int((host != fast).sum()))
    return host, fast, walk


def test_occluder_test_implies_the_walk_single_triangle(pg, monkeypatch, host_helper):
    """One listed triangle in empty space, so the walk misses whatever misses the triangle: rays aimed inside and just
    outside its edges and vertices, hits on both sides of tmin and of the distance margin, grazing directions on both
    sides of the 1/16 bound, origins so far out that the triangle is too small for E, +-0 components.  Every margin's
    refusal is asserted from the inputs, and the floor on plain hits is taken on the host first."""
    from mitsuba_path_guiding_amd.integrator import Device
    monkeypatch.delenv("PG_NO_PROBE_LIST", raising=False)
    S = pg.scenes
    s = S.Scene()
    s.name = "one_triangle"
    white = s.add_material(S.material("diffuse", reflectance=(0.7, 0.7, 0.7)))
    A, B, Cc = np.array((0.0, 0.0, 0.0)), np.array((4.0, 0.0, 0.0)), np.array((0.0, 4.0, 0.0))
    s.add_mesh(np.array([A, B, Cc], np.float32), np.array([[0, 1, 2]], np.uint32), material=white)
    LV, LF = S.quad((5.0, 5.0, 3.0), (5.2, 5.0, 3.0), (5.2, 5.2, 3.0), (5.0, 5.2, 3.0), facing=(0, 0, -1))
    s.add_mesh(LV, LF, material=white, radiance=(10.0, 10.0, 10.0))
    s.set_camera((1.0, 1.0, 3.0), (1.0, 1.0, 0.0), (0, 1, 0), 60.0, 16, 16)
    sc = s.finalize()
    d = Device(pg.capi.default_config(guiding=1))
    d.upload(sc)
    aim = _rays([(1.0, 1.0, 2.0)], [(0.0, 0.0, -1.0)])
    aim[:, 7] = 1e30  # pg_trace_rays takes a tmax; the probe rows of _rays carry none
    hit = d.trace_rays(aim)
    ids = hit[:, 1].copy().view(np.uint32)[:1]  # the triangle's BVH-order id
    assert ids[0] != 0xFFFFFFFF
    tri = np.array([[A, B, Cc]], np.float64)
    absmax = float(np.abs(sc.positions).max())
    rng = np.random.default_rng(17)
    n = 100000 // 8

    def point(w0, w1):
        return A + np.asarray(w0)[:, None] * (B - A) + np.asarray(w1)[:, None] * (Cc - A)

    def front(m):  # origins 0.5 to 3 above or below the triangle's plane, over it
        o = point(rng.uniform(0.1, 0.5, m), rng.uniform(0.1, 0.4, m))
        o[:, 2] = rng.uniform(0.5, 3.0, m) * rng.choice([-1, 1], m)
        return o

    # plain hits: aimed well inside, steep enough
    o = front(n)
    r = _rays(o, _unit(point(rng.uniform(0.05, 0.45, n), rng.uniform(0.05, 0.45, n)) - o))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "inside", r)
    steep = np.abs(r[:, 6]) * 16 >= np.abs(r[:, 4:7]).max(1)
    assert steep.mean() > 0.9 and host[steep].mean() >= 0.99 and fast[steep].mean() >= 0.99 and walk.all()
    # around the edges and vertices: weights from -2^-9 to 2^-9, and targets displaced by ulps
    o = front(n)
    w0 = rng.integers(-4096, 4097, n) * 2.0 ** -21
    w1 = np.where(rng.random(n) < 0.3, rng.integers(-4096, 4097, n) * 2.0 ** -21, rng.uniform(0.05, 0.9, n))
    swap = rng.random(n) < 0.5
    w0, w1 = np.where(swap, w1, w0), np.where(swap, w0, w1)
    third = rng.random(n) < 0.33  # the hypotenuse: w0 + w1 around 1
    w1 = np.where(third, 1.0 - w0 - rng.integers(-4096, 4097, n) * 2.0 ** -21, w1)
    tgt = _ulps(point(w0, w1).astype(np.float32), rng.integers(-64, 65, (n, 3)))
    tgt[:, 2] = 0.0
    r = _rays(o, _unit(tgt.astype(np.float64) - o))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "edges", r)
    # the aimed weights: whatever is outside, or inside by less than half the 2^-10 margin, must be refused
    wmin = np.minimum(np.minimum(w0, w1), 1.0 - w0 - w1)
    assert (walk == 0).sum() > n // 10  # the walk really misses here
    assert (wmin < 2.0 ** -11).sum() > n // 4 and fast[wmin < 2.0 ** -11].sum() == 0
    assert host[wmin > 1.5 * 2.0 ** -10].sum() > 0  # inside by one and a half margins: accepted unless grazing
    # the hit on both sides of tmin and of the distance margin 2^-15 E / max|d|: t = tmin + k 2^-17 E, k in [-16, 16]
    o = front(n)
    dd = _unit(point(rng.uniform(0.1, 0.4, n), rng.uniform(0.1, 0.4, n)) - o)
    t = np.abs(o[:, 2] / dd[:, 2])
    E = absmax + np.abs(o).max(1)
    k = rng.integers(-16, 17, n)
    r = _rays(o, dd, t - k * 2.0 ** -17 * E)
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "tmin", r)
    assert (walk == 0).sum() > n // 4  # t < tmin: a miss
    assert fast[k <= 1].sum() == 0  # behind tmin, or past it by less than half the margin
    assert host[k >= 8].sum() > 0
    # grazing: |d_k| on both sides of max|d| / 16
    p = point(rng.uniform(0.2, 0.3, n), rng.uniform(0.2, 0.3, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    dxy = np.stack([np.cos(ang), np.sin(ang)], 1)
    dz = rng.uniform(0.01, 0.12, n) * rng.choice([-1, 1], n)
    dd = _unit(np.concatenate([dxy, dz[:, None]], 1))
    o = p - dd * rng.uniform(0.5, 1.5, (n, 1))
    r = _rays(o, dd)
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "grazing", r)
    shallow = np.abs(r[:, 6]) * np.float32(16) < np.abs(r[:, 4:7]).max(1)
    assert shallow.sum() > n // 4 and fast[shallow].sum() == 0 and host[~shallow].sum() > 0
    # origins far out: the triangle (4 wide) is too small once E = absmax + max|o| > 128
    far = _unit(rng.normal(size=(n, 3))) * (10.0 ** rng.uniform(1.0, 4.0, (n, 1)))
    far[:, 2] = np.where(np.abs(far[:, 2]) < 0.3 * np.abs(far).max(1), 0.3 * np.abs(far).max(1), far[:, 2])
    r = _rays(far, _unit(point(rng.uniform(0.1, 0.4, n), rng.uniform(0.1, 0.4, n)) - far))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "far", r)
    small = np.float32(128.0) < np.float32(absmax) + np.abs(r[:, :3]).max(1)
    assert small.sum() > n // 4 and fast[small].sum() == 0 and host[~small].sum() > 0
    # +-0 direction components
    o = front(n)
    r = _rays(o, _unit(point(rng.uniform(0.1, 0.4, n), rng.uniform(0.1, 0.4, n)) - o))
    ax = rng.integers(0, 2, n)
    r[np.arange(n), 4 + ax] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "zero", r)
    assert fast.sum() == 0 and host.sum() == 0
    # aimed past the triangle altogether
    o = front(n)
    r = _rays(o, _unit(point(rng.uniform(1.1, 3.0, n), rng.uniform(-2.0, 3.0, n)) - o))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "outside", r)
    assert fast.sum() == 0 and walk.sum() < n // 10
    # and away from it
    r = _rays(o, -r[:, 4:7])
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "away", r)
    assert fast.sum() == 0
    assert (occluder_test(d, r, ids[:0])[0] == 0).all()  # an empty list answers nothing
    d.close()


def test_occluder_test_implies_the_walk_open_box(pg, monkeypatch, host_helper):
    """The learned list of the open box against its walk: rays from inside and outside the box, a third of which leave
    through the missing face or never reach the box, so a predicate that answers too often is caught by the walk."""
    from mitsuba_path_guiding_amd.integrator import Device
    for name in ("PG_NO_RAYS_FUSION", "PG_NO_DOOM_PROBE", "PG_NO_PATH_CULL", "PG_NO_PROBE_LIST"):
        monkeypatch.delenv(name, raising=False)
    sc = open_box(pg)
    d = Device(pg.capi.default_config(guiding=1, s_tree_threshold=400.0, tail_paths=-1))
    d.upload(sc)
    _train(d, 4)
    ids, orig = occluders(d)
    assert len(ids) >= 6
    tri = sc.positions[sc.indices.reshape(-1, 3)[orig]].astype(np.float64)
    absmax = float(np.abs(sc.positions).max())
    rng = np.random.default_rng(23)
    n = 20000
    inside = rng.uniform((0.05, 0.05, 0.05), (3.95, 2.95, 3.95), (n, 3))
    r = _rays(inside, _unit(rng.normal(size=(n, 3))))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "from inside", r)
    # at least three of the five faces are listed, and each fills about a sixth of the directions
    assert (walk == 0).sum() > n // 20 and host.mean() >= 0.3 and fast.mean() >= 0.3
    # towards the opening's rim: z = 0, on and around the edges of the missing face
    rim = np.stack([rng.uniform(-0.05, 4.05, n), np.where(rng.random(n) < 0.5, rng.uniform(-0.01, 0.01, n), 3.0 +
                    rng.uniform(-0.01, 0.01, n)), rng.uniform(-0.01, 0.01, n)], 1)
    r = _rays(inside, _unit(rim - inside))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "rim", r)
    assert (walk == 0).sum() > n // 20
    # from outside, in front of the opening and around the box
    outside = _unit(rng.normal(size=(n, 3))) * rng.uniform(5.0, 30.0, (n, 1)) + (2.0, 1.5, 2.0)
    r = _rays(outside, _unit(rng.uniform((-1, -1, -1), (5, 4, 5), (n, 3)) - outside))
    host, fast, walk = _compare(d, host_helper, tri, absmax, ids, "from outside", r)
    assert (walk == 0).sum() > n // 50
    d.close()
