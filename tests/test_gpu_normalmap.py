"""Normal maps on the GPU (pg_set_normal_maps / pg_hit_frames) against tests/normalmap_ref.py and closed forms."""
import numpy as np
import pytest

import normalmap_ref as R
import texture_ref as T
from test_gpu_textures import VARIANTS, make_dev, quad_scene

pytestmark = pytest.mark.gpu
F = np.float32
FLAT = np.tile(np.array([0.5, 0.5, 1.0], F), (1, 1, 1))


def run(pg, sc, passes, spp, hook=None, offset=0, **cfg):
    """`passes` training iterations, then `spp` samples; hook(device) runs after the upload."""
    d = make_dev(pg, **dict(dict(guiding=1, s_tree_threshold=300.0), **cfg))
    d.upload(sc)
    if hook is not None:
        hook(d)
    off = offset
    for it in range(passes):
        d.render_pass(2 ** it, off, True)
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    d.reset_film()
    d.render_pass(spp, off)
    out = dict(film=d.read_film(), tree=d.get_sdtree(), stats=d.stats())
    d.close()
    return out


def same(a, b):
    return (np.array_equal(a["film"][0], b["film"][0]) and np.array_equal(a["film"][1], b["film"][1])
            and np.array_equal(a["tree"], b["tree"]))


def bumpy(seed=7, n=4):
    rgb = np.random.default_rng(seed).uniform(0.25, 0.75, (n, n, 3)).astype(F)
    rgb[..., 2] = np.random.default_rng(seed + 1).uniform(0.8, 1.0, (n, n)).astype(F)
    return rgb


# ---- 1. frames --------------------------------------------------------------------------------------------------------
def frames_scene(pg):
    S = pg.scenes
    s = S.Scene()
    m = s.add_material(S.material("diffuse", reflectance=(0.5, 0.5, 0.5)))
    plain = s.add_material(S.material("diffuse", reflectance=(0.5, 0.5, 0.5)))
    Fi = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    nrm = lambda a: (np.asarray(a, np.float64) / np.linalg.norm(a, axis=1, keepdims=True)).astype(F)
    # quad A: texcoords rotated by 35 degrees and scaled (3, 0.4) against the edges
    VA = np.array([[-1.5, -1, 1], [0, -1, 1.2], [0, 1, 1.1], [-1.5, 1, 0.9]], F)
    NA = nrm([[0.1, 0, -1], [0, 0.2, -1], [-0.15, 0.1, -1], [0.05, -0.1, -1]])
    c, sn = np.cos(np.radians(35.0)), np.sin(np.radians(35.0))
    uvA = np.stack([3.0 * (c * VA[:, 0] + sn * VA[:, 1]), 0.4 * (-sn * VA[:, 0] + c * VA[:, 1])], 1).astype(F)
    # quad B: triangle (0, 2, 3) has a degenerate uv (t3 = t0)
    VB = np.array([[0, -1, 1.2], [1.5, -1, 1], [1.5, 1, 1.3], [0, 1, 1.1]], F)
    NB = nrm([[0, 0.1, -1], [0.2, 0, -1], [0.1, 0.1, -1], [-0.1, 0, -1]])
    uvB = np.array([[0.2, 0.1], [1.3, 0.4], [0.9, 1.7], [0.2, 0.1]], F)
    s.add_mesh(VA, Fi, NA, material=m, uv=uvA)
    s.add_mesh(VB, Fi, NB, material=m, uv=uvB)
    # quad C, behind the camera: no map
    VC = VA * np.array([1, 1, -1], F)
    s.add_mesh(VC, Fi[:, ::-1], NA * np.array([1, 1, -1], F), material=plain, uv=uvA)
    s.set_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 40.0, 8, 8)
    return s.finalize()


def frame_rays(n=256, seed=3):
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.zeros((n, 1))], 1)
    d = np.concatenate([rng.uniform(-1.3, 1.3, (n, 2)), np.where(np.arange(n) % 8 == 7, -1.0, 1.0)[:, None]], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.full((n, 1), 1e-4), d, np.full((n, 1), np.inf)], 1).astype(F)


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_hit_frames_match_the_reference(pg, filt):
    sc = frames_scene(pg)
    rgb = bumpy()
    kw = dict(filter=filt, wrap_u="repeat", uscale=1.5, vscale=0.75, uoffset=0.125, voffset=-0.25)
    sc.bind_normal_map(0, sc.add_normal_map(rgb, filter=filt, wrap="repeat", uscale=1.5, vscale=0.75, uoffset=0.125,
                                            voffset=-0.25))
    rays = frame_rays()
    d = make_dev(pg, sc)
    hits, rec, got = d.trace_rays(rays), d.hit_records(rays), d.hit_frames(rays)
    d.close()
    tri = hits[:, 1].view(np.uint32)
    hit = tri != 0xFFFFFFFF
    assert 0.5 < hit.mean() < 1.0 and not got[~hit].any()
    P, N, UV, I = sc.positions, sc.normals, sc.texcoords, sc.indices.reshape(-1, 3)
    want = np.zeros_like(got)
    seen = set()
    for k in np.flatnonzero(hit):
        f, u, v = I[tri[k]], hits[k, 2], hits[k, 3]
        b0 = F(1) - u - v
        shN = R.normalize(N[f[0]] * b0 + N[f[1]] * u + N[f[2]] * v)
        wd = -rays[k, 4:7]
        if tri[k] >= 4:  # the unmapped quad: the base frame on p1 - p0
            fr = R.shading_frame(shN, P[f[1]] - P[f[0]])
        else:
            dpdu = R.tangent(P[f[0]], P[f[1]], P[f[2]], UV[f[0]], UV[f[1]], UV[f[2]])
            uv = T.hit_uv(UV[f[0]], UV[f[1]], UV[f[2]], [u], [v])
            fr = R.perturbed_frame(shN, dpdu, R.lookup(rgb, uv, **kw)[0])
        seen.add(int(tri[k]))
        want[k] = np.concatenate([fr[2], fr[0], fr[1], R.to_local(fr, wd)])
    assert seen == set(range(6))  # every triangle, the degenerate-uv one (3) and the unmapped ones (4, 5)
    err = np.abs(got - want).max()
    print(f"{filt}: max |frame - ref| = {err:.3g} over {hit.sum()} hits")
    assert err <= 1e-6
    # unmapped hits are hit_records' frame bit for bit
    un = hit & (tri >= 4)
    np.testing.assert_array_equal(got[un][:, 0:3], rec[un][:, 7:10])
    np.testing.assert_array_equal(got[un][:, 3:6], rec[un][:, 10:13])
    np.testing.assert_array_equal(got[un][:, 9:12], rec[un][:, 13:16])
    # and a mapped frame is not the base one
    assert np.abs(got[hit & (tri < 4)][:, 0:3] - rec[hit & (tri < 4)][:, 7:10]).max() > 1e-2


# ---- 2. a flat map is a no-op, bit for bit ----------------------------------------------------------------------------
def test_flat_map_is_a_no_op(pg):
    """The 32 x 32 Cornell box with a constant (0.5, 0.5, 1) map and no texcoords renders the no-map film, sum of
    squares and tree exactly.  n' = normalize(n) returns n only where |n| rounds to 1, which holds for axis-aligned
    normals; the Cornell data's left wall and its blocks are slanted, so the map goes on every diffuse wall material
    all of whose normals renormalise to themselves in float32 (checked here with the restatement; the blocks get
    material records of their own so that the white of floor, ceiling and back wall qualifies).  The filter is nearest:
    the bilinear sum of four equal texels, v dx2 dy2 + v dx2 dy1 + v dx1 dy2 + v dx1 dy1, returns v only within an
    ulp (on the MI355X a bilinear flat map moved the film in the eighth digit)."""
    S = pg.scenes
    white = dict(reflectance=(0.725, 0.71, 0.68))
    sc = S.cornell(32, 32, short_material=S.material("diffuse", **white), tall_material=S.material("diffuse", **white))
    sc.finalize()
    I, N = sc.indices.reshape(-1, 3), sc.normals
    stable = []
    for m in (0, 1, 2):
        n = np.concatenate([N[I[sh.tri_begin:sh.tri_begin + sh.tri_count]].reshape(-1, 3) for sh in sc.shapes if sh.material == m])
        if np.array_equal(R.normalize(n).view(np.uint32), n.view(np.uint32)):
            stable.append(m)
    assert 0 in stable and len(stable) >= 2, stable  # floor, ceiling, back wall and the x = 0 wall at least
    never = run(pg, sc, 2, 4)
    k = sc.add_normal_map(np.tile(FLAT, (2, 3, 1)), filter="nearest")
    for m in stable:
        sc.bind_normal_map(m, k)
    assert sc.texcoords is None
    mapped = run(pg, sc, 2, 4)
    assert never["film"][0][..., :3].sum() > 0
    assert same(mapped, never)


# ---- 3. / 4. analytic direct light; the hemisphere rule ------------------------------------------------------------
RHO, E = 0.5, 3.0
LIGHT = np.array([-0.2, 0.3, 1.0])  # the direction the light travels; l = -LIGHT / |LIGHT|


def light_quad(pg, uv, tilt_deg, about, light=LIGHT, twosided=False, camera=((0, 0, 0), (0, 0, 1), 40.0)):
    mat = pg.scenes.material("diffuse", reflectance=(RHO, RHO, RHO), twosided=twosided)
    sc = quad_scene(pg, uv, mat, 16, 16)
    sc.set_camera(camera[0], camera[1], (0, 1, 0), camera[2], 16, 16)
    sc.add_directional_light(tuple(light), (E, E, E))
    a = np.radians(tilt_deg)
    nl = np.array([0.0, np.sin(a), np.cos(a)] if about == "s" else [np.sin(a), 0.0, np.cos(a)])
    c = ((nl + 1) / 2).astype(F)
    sc.bind_normal_map(0, sc.add_normal_map(c.reshape(1, 1, 3), filter="nearest"))
    return sc.finalize(), c


def radiance(pg, sc):
    d = make_dev(pg, sc, max_depth=2, guiding=0)
    d.render_pass(4, 0)
    rgbw, _ = d.read_film()
    d.close()
    np.testing.assert_array_equal(rgbw[..., 3], 4.0)
    return rgbw[..., :3] / rgbw[..., 3:4]


def expected(sc, c, tri):
    """rho / pi E max(0, n' . l) of triangle `tri` (float64 of the float32 frame)"""
    P, I, UV = sc.positions, sc.indices.reshape(-1, 3), sc.texcoords
    f = I[tri]
    tc = (None, None, None) if UV is None else (UV[f[0]], UV[f[1]], UV[f[2]])
    dpdu = R.tangent(P[f[0]], P[f[1]], P[f[2]], *tc)
    _, _, n2 = R.perturbed_frame(sc.normals[f[0]], dpdu, c)
    l = -LIGHT / np.linalg.norm(LIGHT)
    return RHO / np.pi * E * max(0.0, float(np.dot(n2.astype(np.float64), l))), n2


def test_analytic_direct_light_barycentric_tangent(pg):
    """no texcoords: dpdu = p1 - p0, which differs between the quad's two triangles ((2, 0, 0) and (2, 2, 0)); each
    side of the diagonal carries its triangle's value"""
    sc, c = light_quad(pg, None, 30.0, "s")
    img = radiance(pg, sc)
    e0, n0 = expected(sc, c, 0)
    e1, n1 = expected(sc, c, 1)
    flat = RHO / np.pi * E * float(np.dot([0, 0, -1.0], -LIGHT / np.linalg.norm(LIGHT)))
    assert abs(e0 - e1) > 0.01 * e0 and abs(e0 - flat) > 0.01 * flat and abs(e1 - flat) > 0.01 * flat
    py, px = np.mgrid[0:16, 0:16]
    sides = [img[py > px], img[py < px]]
    print("triangle values", e0, e1, "film", sides[0].mean(), sides[1].mean())
    a, b = (sides if abs(sides[0].mean() - e0) < abs(sides[0].mean() - e1) else sides[::-1])
    assert np.abs(a - e0).max() <= 1e-4 * e0 and np.abs(b - e1).max() <= 1e-4 * e1


def test_analytic_direct_light_rotated_texcoords(pg):
    """texcoords rotated by 50 degrees against the edges: one tangent for both triangles, another tilt direction"""
    V = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64)
    cs, sn = np.cos(np.radians(50.0)), np.sin(np.radians(50.0))
    uv = np.stack([0.5 * (cs * V[:, 0] + sn * V[:, 1]), 2.0 * (-sn * V[:, 0] + cs * V[:, 1])], 1).astype(F)
    sc, c = light_quad(pg, uv, 30.0, "s")
    img = radiance(pg, sc)
    e0, n0 = expected(sc, c, 0)
    e1, _ = expected(sc, c, 1)
    plain, _ = expected(light_quad(pg, None, 30.0, "s")[0], c, 0)
    assert abs(e0 - e1) <= 1e-6 * e0 and abs(e0 - plain) > 0.01 * e0
    np.testing.assert_allclose(n0[:2] / np.linalg.norm(n0[:2]), [sn, -cs], atol=1e-5)  # tilted along t = cross(n, s)
    print("expected", e0, "film", img.min(), img.max())
    assert np.abs(img - e0).max() <= 1e-4 * e0


def test_hemisphere_rule(pg):
    """normalmap{twosided{diffuse}}, camera and light grazing from +y: above the base plane (n = -z), below the plane
    tilted by 60 degrees towards -y.  Without the rule the two-sided flip would give rho / pi E |n' . l|."""
    V = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], F)
    light = np.array([0.0, -3.0, 0.5])
    cam = ((0, 3.0, 0.7), (0, 0, 1), 4.0)
    sc, c = light_quad(pg, V, 60.0, "s", light=light, twosided=True, camera=cam)
    _, _, n2 = R.perturbed_frame(np.array([0, 0, -1], F), R.tangent(*sc.positions[:3], *V[:3]), c)
    l, w = -light / np.linalg.norm(light), np.array(cam[0]) - np.array([0, 0, 1.0])
    assert l[2] < 0 and w[2] < 0 and np.dot(n2, l) < -0.5 and np.dot(n2, w) < -0.5  # above n = -z, below n'
    img = radiance(pg, sc)
    assert not img.any()
    sc.normal_map_bindings = []
    lit = radiance(pg, sc)  # the camera does see the lit quad
    assert (lit[..., 0] > 0).mean() > 0.5


# ---- 5. guiding stays unbiased ----------------------------------------------------------------------------------------
def z_test(a, b):
    total, var = 0.0, 0.0
    for (rgbw, sq), s in ((a, 1), (b, -1)):
        n = rgbw[..., 3:4].astype(np.float64)
        mean = rgbw[..., :3] / n
        total = total + s * mean
        var = var + np.maximum(sq[..., :3] / n - mean * mean, 0) / n
    ok = var > 0
    z = np.abs(total[ok]) / np.sqrt(var[ok])
    return (z < 5).mean(), z.max()


def test_guiding_stays_unbiased(pg):
    """Cornell 32 x 32 with a bumpy 4 x 4 map on the white walls (floor, ceiling, back) and the blocks: guided against
    unguided at 256 spp, per-pixel z-test (|z| < 5 on >= 99.9 %).  The spp is one at which two unguided runs on
    different sample streams pass the same test, which is asserted first."""
    sc = pg.scenes.cornell(32, 32)
    sc.bind_normal_map(0, sc.add_normal_map(bumpy(), filter="bilinear"))
    spp = 256
    u0 = run(pg, sc, 0, spp, guiding=0, max_depth=5)["film"]
    u1 = run(pg, sc, 0, spp, offset=100000, guiding=0, max_depth=5)["film"]
    frac, zmax = z_test(u0, u1)
    print(f"unguided vs unguided at {spp} spp: |z| < 5 for {frac:.5f}, max {zmax:.2f}")
    assert frac >= 0.999
    g = run(pg, sc, 4, spp, max_depth=5)["film"]
    frac, zmax = z_test(g, u0)
    print(f"guided vs unguided at {spp} spp: |z| < 5 for {frac:.5f}, max {zmax:.2f}")
    assert frac >= 0.999


# ---- 6. launch variants and shards ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def variant_job(pg):
    S = pg.scenes
    sc = S.cornell(32, 32, short_material=S.material("roughconductor", alpha=0.2),
                   tall_material=S.material("roughplastic", reflectance=(0.6, 0.25, 0.4), alpha=0.2))
    k = sc.add_normal_map(bumpy(), filter="bilinear", uscale=2.0, vscale=3.0)
    for m in (0, 1, 4, 5):
        sc.bind_normal_map(m, k)
    sc.bind_texture(1, sc.add_texture("checkerboard", color0=(0.9, 0.1, 0.1), color1=(0.1, 0.1, 0.9), uscale=4.0, vscale=4.0))
    return sc, run(pg, sc, 2, 4)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_launch_variants_are_bit_identical(pg, monkeypatch, variant_job, variant):
    sc, base = variant_job
    cfg, env = VARIANTS[variant]
    for name in env:
        monkeypatch.setenv(name, "1")
    out = run(pg, sc, 2, 4, **cfg)
    assert base["film"][0][..., :3].sum() > 0
    assert same(out, base)


def test_shard_union_is_bit_identical(pg, variant_job):
    sc, base = variant_job
    parts = [make_dev(pg, sc, guiding=1, s_tree_threshold=300.0, rank=r, world_size=2, tile_size=16) for r in range(2)]
    full = make_dev(pg, sc, guiding=1, s_tree_threshold=300.0, tile_size=16)
    off = 0
    for it in range(2):
        full.render_pass(2 ** it, off, True)
        full.splat_local()
        full.refit(it)
        for d in parts:
            d.render_pass(2 ** it, off, True)
            d.splat_local()
        total = parts[0].get_tree_stats() + parts[1].get_tree_stats()
        for d in parts:
            d.put_tree_stats(total)
            d.refit(it)
        off += 2 ** it
    films = []
    for d in parts + [full]:
        d.reset_film()
        d.render_pass(4, off)
        films.append(d.read_film())
    assert all(np.array_equal(d.get_sdtree(), base["tree"]) for d in parts + [full])
    for k in range(2):
        assert np.array_equal(films[0][k] + films[1][k], films[2][k])
        assert np.array_equal(films[2][k], base["film"][k])
    for d in parts + [full]:
        d.close()


# ---- 7. life cycle and errors -----------------------------------------------------------------------------------------
def test_life_cycle(pg):
    sc = pg.scenes.cornell(32, 32)
    never = run(pg, sc, 2, 4)
    maps, bind = [pg.scenes.make_texture("bitmap", bumpy())], [(0, 0), (2, 0)]
    on = run(pg, sc, 2, 4, hook=lambda d: d.set_normal_maps(maps, bind, None))
    assert not np.array_equal(on["film"][0], never["film"][0])

    def off(d):
        d.set_normal_maps(maps, bind, None)
        d.set_normal_maps(maps, [], None)
    assert same(run(pg, sc, 2, 4, hook=off), never)

    def reupload(d):
        d.set_normal_maps(maps, bind, None)
        d.upload(sc)
    assert same(run(pg, sc, 2, 4, hook=reupload), never)

    def textures_come_and_go(d):  # the maps survive pg_set_textures turning its own set on and off
        d.set_normal_maps(maps, bind, None)
        d.set_textures([pg.scenes.make_texture("checkerboard")], [(1, 0)], None)
        d.set_textures([], [], None)
    assert same(run(pg, sc, 2, 4, hook=textures_come_and_go), on)


def test_errors(pg):
    from mitsuba_path_guiding_amd.integrator import PGError
    S, c = pg.scenes, pg.capi
    good = S.make_texture("bitmap", bumpy())

    def fails(d, status, word, *args, call="set_normal_maps"):
        with pytest.raises(PGError) as e:
            getattr(d, call)(*args)
        assert e.value.status == status, e.value
        assert word in d.lib.pg_last_error(d.h).decode(), d.lib.pg_last_error(d.h)

    d = make_dev(pg)
    fails(d, c.PG_ERR_STATE, "no scene", [good], [(0, 0)], None)
    sc = S.cornell(16, 16, short_material=S.material("dielectric"), tall_material=S.material("null"))
    d.upload(sc)
    nv = sc.desc().num_vertices
    tc = np.random.default_rng(1).uniform(0, 1, (nv, 2)).astype(F)
    d.set_normal_maps([good], [(0, 0)], tc)
    fails(d, c.PG_ERR_INVALID, "out of range", [good], [(0, 1)], None)
    fails(d, c.PG_ERR_INVALID, "out of range", [good], [(len(sc.materials), 0)], None)
    fails(d, c.PG_ERR_INVALID, "dielectric", [good], [(4, 0)], None)
    fails(d, c.PG_ERR_INVALID, "null", [good], [(5, 0)], None)
    fails(d, c.PG_ERR_INVALID, "twice", [good, good], [(0, 0), (0, 1)], None)
    bad = bumpy()
    bad[0, 0, 0] = np.nan
    fails(d, c.PG_ERR_INVALID, "texel", [S.make_texture("bitmap", bad)], [(0, 0)], None)
    other = tc.copy()
    other[3, 1] += 0.5
    fails(d, c.PG_ERR_INVALID, "texcoords differ", [S.make_texture("checkerboard")], [(1, 0)], other, call="set_textures")
    d.set_textures([S.make_texture("checkerboard")], [(1, 0)], tc)  # equal: fine
    fails(d, c.PG_ERR_INVALID, "texcoords differ", [good], [(0, 0)], other)
    d.set_normal_maps([good], [(0, 0)], None)  # NULL reads the other call's
    d.render_pass(1, 0)
    fails(d, c.PG_ERR_STATE, "render pass", [good], [(0, 0)], None)
    d.upload(sc)
    d.set_normal_maps([good], [(0, 0)], None)
    d.close()
    v = make_dev(pg, integrator=c.PG_INTEGRATOR_VOLPATH)
    v.upload(S.smoke(8, 8, res=32))
    fails(v, c.PG_ERR_INVALID, "volumetric", [good], [(0, 0)], None)
    v.close()


# ---- 8. XML end to end -----------------------------------------------------------------------------------------------
def test_xml_end_to_end(pg, tmp_path):
    from test_normalmap import GOOD, nmap_xml
    S = pg.scenes
    p, rgb = nmap_xml(tmp_path, GOOD)
    a = pg.mitsuba_xml.load(str(p)).scene
    b = S.Scene()
    m0 = b.add_material(S.material("roughconductor", conductor="Al", alpha=0.2, twosided=True))
    assert bytes(b.materials[m0]) == bytes(a.materials[0])
    for k, sh in enumerate(a.shapes):
        sl = slice(sh.tri_begin, sh.tri_begin + sh.tri_count)
        v0, v1 = int(a.indices[sl].min()), int(a.indices[sl].max()) + 1
        if k == 0:
            b.add_mesh(a.positions[v0:v1], a.indices[sl] - v0, a.normals[v0:v1], material=m0, uv=a.texcoords[v0:v1])
        else:
            e = b.add_material(S.material("diffuse", reflectance=(0.0, 0.0, 0.0)))
            b.add_mesh(a.positions[v0:v1], a.indices[sl] - v0, a.normals[v0:v1], material=e, radiance=(5.0, 5.0, 5.0))
    b.bind_normal_map(m0, b.add_normal_map(rgb, filter="nearest", uscale=3.0))
    cam = a.camera
    for s in (a, b):
        s.set_camera(list(cam.origin), list(cam.target), list(cam.up), cam.fov_x_deg, 32, 32, cam.near_clip, cam.far_clip)
        s.finalize()
    ja, jb = run(pg, a, 2, 4), run(pg, b, 2, 4)
    assert ja["film"][0][..., :3].sum() > 0 and same(ja, jb)
    a.normal_map_bindings = []
    assert not np.array_equal(run(pg, a, 2, 4)["film"][0], ja["film"][0])
