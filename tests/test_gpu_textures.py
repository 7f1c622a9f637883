"""Textures (pg_set_textures) on the GPU.

The oracle renders no textures, so the yardsticks are the numpy float32 restatement of the lookups
(tests/texture_ref.py, checked by hand in test_textures.py) -- bit for bit -- and exact identities: a constant
texture is the constant material, a power-of-two reflectance scales every float product and sum exactly, and no
bindings is the library without the feature.  There is no tolerance in any of them."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import texture_ref as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNTED = ("segments", "escaped", "shadow_rays", "records")
SIZES = {"1x1": (1, 1), "2x3": (2, 3), "5x4": (5, 4)}  # (width, height)
XFORM = dict(uscale=1.75, vscale=-0.625, uoffset=0.3125, voffset=1.5)


def make_dev(pg, scene=None, **cfg):
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(**cfg))
    if scene is not None:
        d.upload(scene)
    return d


def texels(w, h, seed=3):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)


def query_points(w, h, n=4096, seed=5):
    """uv in [-3, 3], exact texel-boundary values of the transformed coordinate, +-0, and NaN / inf rows"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-3.0, 3.0, (n, 2)).astype(np.float32)
    # raw uv whose transform lands on texel boundaries k / W (the transform is exact for these dyadic constants
    # wherever (k / W - offset) / scale is representable; the others land next to the boundary, as good a probe)
    k = np.arange(-2 * w, 2 * w + 1, dtype=np.float32)
    bu = (k / np.float32(w) - np.float32(XFORM["uoffset"])) / np.float32(XFORM["uscale"])
    k = np.arange(-2 * h, 2 * h + 1, dtype=np.float32)
    bv = (k / np.float32(h) - np.float32(XFORM["voffset"])) / np.float32(XFORM["vscale"])
    m = min(len(bu), len(bv))
    uv[:m, 0], uv[:m, 1] = bu[:m], bv[::-1][:m]
    uv[m:m + 4] = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    uv[m + 4:m + 10] = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (np.nan, np.nan), (-np.inf, np.inf)]
    return uv


@pytest.fixture(scope="module")
def dev(pg):
    d = make_dev(pg)  # the lookup needs a context only
    yield d
    d.close()


# ---- 3. lookup parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("wrap", T.WRAPS)
@pytest.mark.parametrize("size", list(SIZES))
def test_bitmap_lookup_bit_for_bit(pg, dev, size, wrap, filt):
    w, h = SIZES[size]
    rgb = texels(w, h)
    wrap_v = T.WRAPS[(T.WRAPS.index(wrap) + 2) % len(T.WRAPS)]  # each axis on its own mode
    uv = query_points(w, h)
    assert np.abs(uv[np.isfinite(uv).all(1)]).max() * 2 * max(w, h) < 2 ** 23
    tex = pg.scenes.make_texture("bitmap", rgb, filter=filt, wrap=wrap, wrap_v=wrap_v, **XFORM)
    got = dev.texture_query(tex, uv)
    want = T.bitmap(rgb, uv, filt, wrap, wrap_v, **XFORM)
    bad = ~np.isfinite(uv).all(1)
    assert bad.sum() == 6 and not got[bad].any()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # the same mode on both axes too
    tex = pg.scenes.make_texture("bitmap", rgb, filter=filt, wrap=wrap, **XFORM)
    np.testing.assert_array_equal(dev.texture_query(tex, uv).view(np.uint32),
                                  T.bitmap(rgb, uv, filt, wrap, **XFORM).view(np.uint32))


def test_checkerboard_lookup_bit_for_bit(pg, dev):
    c0, c1 = (0.9, 0.5, 0.1), (0.05, 0.2, 0.7)
    uv = query_points(2, 2)  # boundaries at multiples of 1/2
    for xf in (XFORM, dict(uscale=1.0, vscale=1.0, uoffset=0.0, voffset=0.0)):
        tex = pg.scenes.make_texture("checkerboard", color0=c0, color1=c1, **xf)
        got = dev.texture_query(tex, uv)
        np.testing.assert_array_equal(got.view(np.uint32), T.checkerboard(c0, c1, uv, **xf).view(np.uint32))
        assert len(np.unique(got[:, 0])) == 3  # both colours and the non-finite rows' 0


def test_huge_uv_is_safe(pg, dev):
    """+-3e38 (finite): the colour is unspecified, the call succeeds with finite output (the texel address is clamped)"""
    uv = np.array([(3e38, 3e38), (-3e38, 3e38), (3e38, -3e38), (-3e38, -3e38), (3e38, 0.5), (0.5, -3e38)], np.float32)
    rgb = texels(5, 4)
    for filt in ("nearest", "bilinear"):
        for wrap in T.WRAPS:
            out = dev.texture_query(pg.scenes.make_texture("bitmap", rgb, filter=filt, wrap=wrap), uv)
            assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1
    assert np.isfinite(dev.texture_query(pg.scenes.make_texture("checkerboard"), uv)).all()


# ---- 4. hit uv ---------------------------------------------------------------------------------------------------------
def test_hit_uv_dgeom_kat(pg):
    from test_oracle_kat import dgeom_scene
    kat = json.load(open(os.path.join(GOLDEN, "dgeom_kat.json")))
    want = [(0.1, 0.2), (0.2, 0.26), (0.2, 0.1)]
    assert len(kat["cases"]) == 3
    tex = [pg.scenes.make_texture("checkerboard")]
    for case, uv in zip(kat["cases"], want):
        assert np.allclose(case["uv"], uv)
        d = make_dev(pg, dgeom_scene(pg, case))
        r = np.array([[*case["ray_o"], 1e-4, *case["ray_d"], np.inf]], np.float32)
        tc = None if case["texcoords"] is None else np.array(case["texcoords"], np.float32)
        d.set_textures(tex, [(0, 0)], tc)
        got = d.hit_uvs(r)[0]
        d.close()
        assert np.allclose(got, uv, atol=case["eps"]), (case["name"], got)


def quad_scene(pg, uv=None, material=None, width=8, height=8):
    S = pg.scenes
    s = S.Scene()
    m = s.add_material(material if material is not None else S.material("diffuse", reflectance=(0.5, 0.5, 0.5)))
    V = np.array([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float32)
    F = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    N = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    s.add_mesh(V, F, N, material=m, uv=uv)
    s.set_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 40.0, width, height)
    return s.finalize()


def test_hit_uv_is_the_float32_formula(pg):
    tc = np.array([[0.25, -1.5], [3.0, 0.125], [1.75, 2.5], [-0.5, 0.875]], np.float32)
    sc = quad_scene(pg)
    rng = np.random.default_rng(11)
    n = 4096
    o = np.concatenate([rng.uniform(-1.2, 1.2, (n, 2)), np.full((n, 1), -1.0)], 1)
    dd = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.ones((n, 1))], 1)
    rays = np.concatenate([o, np.full((n, 1), 1e-4), dd, np.full((n, 1), np.inf)], 1).astype(np.float32)
    d = make_dev(pg, sc)
    hits = d.trace_rays(rays)
    hit = hits[:, 1].view(np.uint32) != 0xFFFFFFFF
    assert 0.3 < hit.mean() < 1.0  # hits and misses
    np.testing.assert_array_equal(d.hit_uvs(rays)[hit], hits[hit, 2:4])  # no textures set: the barycentrics
    tex = [pg.scenes.make_texture("checkerboard")]
    d.set_textures(tex, [(0, 0)], None)  # texcoords = NULL: (u, v) too
    got = d.hit_uvs(rays)
    np.testing.assert_array_equal(got[hit], hits[hit, 2:4])
    assert not got[~hit].any()
    d.set_textures(tex, [(0, 0)], tc)
    got = d.hit_uvs(rays)
    F = sc.indices.reshape(-1, 3)[hits[hit, 1].view(np.uint32)]
    want = np.stack([T.hit_uv(tc[f[0]], tc[f[1]], tc[f[2]], [u], [v])[0] for f, u, v in zip(F, hits[hit, 2], hits[hit, 3])])
    np.testing.assert_array_equal(got[hit].view(np.uint32), want.view(np.uint32))
    assert not got[~hit].any()
    d.close()


# ---- 5 / 6. off is off; a constant texture is the constant material ----------------------------------------------------
def job(pg, sc, passes, spp, textures=None, reupload=False, **cfg):
    """`passes` training iterations (1, 2, 4, ... spp), then `spp` samples; textures: what set_textures gets after
    the upload (None: never called).  Everything the job produced."""
    d = make_dev(pg, **dict(dict(guiding=1, s_tree_threshold=300.0), **cfg))
    d.upload(sc)
    if textures is not None:
        d.set_textures(*textures)
    if reupload:
        d.upload(sc)
    off, recs = 0, []
    for it in range(passes):
        d.render_pass(2 ** it, off, True)
        rec = d.get_records().reshape(-1, 32)  # commit order is not fixed: compare sorted
        recs.append(rec[np.lexsort(rec.T[::-1])])
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    d.reset_film()
    d.render_pass(spp, off)
    out = dict(film=d.read_film(), tree=d.get_sdtree(), recs=recs, stats=d.stats())
    d.close()
    return out


def assert_same_job(a, b, records=True):
    assert np.array_equal(a["film"][0], b["film"][0]) and np.array_equal(a["film"][1], b["film"][1])
    assert a["film"][0][..., :3].sum() > 0
    assert np.array_equal(a["tree"], b["tree"])
    if records:
        assert all(len(x) > 0 and np.array_equal(x, y) for x, y in zip(a["recs"], b["recs"]))
    for k in COUNTED:
        assert a["stats"][k] == b["stats"][k], k


@pytest.fixture(scope="module")
def cornell32(pg):
    sc = pg.scenes.cornell(32, 32)
    return sc, job(pg, sc, 2, 4)


def test_no_bindings_is_off(pg, cornell32):
    sc, never = cornell32
    tex = [pg.scenes.make_texture("checkerboard")]
    assert_same_job(job(pg, sc, 2, 4, textures=(tex, [], None)), never)


def test_reupload_clears_textures(pg, cornell32):
    sc, never = cornell32
    tex = [pg.scenes.make_texture("checkerboard", color0=(0.9, 0.1, 0.1), color1=(0.0, 0.0, 0.9))]
    assert_same_job(job(pg, sc, 2, 4, textures=(tex, [(0, 0), (1, 0)], None), reupload=True), never)
    # ... and they were on before: the same textures without the re-upload render another image
    other = job(pg, sc, 2, 4, textures=(tex, [(0, 0), (1, 0)], None))
    assert not np.array_equal(other["film"][0], never["film"][0])


def constant_textures(pg, sc, mats, with_average):
    """every material of `mats` bound to a texture that is its own reflectance everywhere; random texcoords"""
    S = pg.scenes
    tex, bind = [], []
    for k, m in enumerate(mats):
        c = np.array(list(sc.materials[m].diffuse_reflectance)[:3], np.float32)
        avg = tuple(float(x) for x in c) if with_average else None
        if k % 2 == 0:
            tex.append(S.make_texture("bitmap", np.tile(c, (2, 3, 1)), filter="nearest", wrap="mirror", average=avg, **XFORM))
        else:
            tex.append(S.make_texture("checkerboard", color0=c, color1=c, average=avg, **XFORM))
        bind.append((m, k))
    tc = np.random.default_rng(2).uniform(-2, 2, (sc.desc().num_vertices, 2)).astype(np.float32)
    return tex, bind, tc


def test_constant_texture_is_the_constant_material(pg):
    sc = pg.scenes.cornell(48, 48)
    cfg = dict(bsdf_fraction_bound=pg.capi.PG_FRACTION_ALBEDO)
    plain = job(pg, sc, 3, 8, **cfg)
    textured = job(pg, sc, 3, 8, textures=constant_textures(pg, sc, [0, 1, 2], False), **cfg)
    assert_same_job(textured, plain)


def test_constant_texture_plastic(pg):
    S = pg.scenes
    sc = S.cornell(48, 48, short_material=S.material("plastic", reflectance=(0.3, 0.5, 0.2)),
                   tall_material=S.material("roughplastic", reflectance=(0.6, 0.25, 0.4), alpha=0.2))
    cfg = dict(bsdf_fraction_bound=pg.capi.PG_FRACTION_ALBEDO)
    plain = job(pg, sc, 3, 8, **cfg)
    textured = job(pg, sc, 3, 8, textures=constant_textures(pg, sc, [4, 5, 0], True), **cfg)
    assert_same_job(textured, plain)


# ---- 7 / 8 / 9. the texture reaches the shader ---------------------------------------------------------------------------
W = 64
TAN = np.float32(np.tan(np.float32(40.0) * np.float32(np.pi) / np.float32(360.0)))


def lit_quad(pg, reflectance=(1.0, 1.0, 1.0)):
    """A two-sided diffuse quad at z = 1, perpendicular to the optical axis and larger than the frustum, under a
    constant environment of radiance 1.  The camera (origin, +z, fov 40, square film) sees x, y = (1 - 2 s) tan(20 deg)
    at film position s in [0, 1]^2 (k_camera), so the texcoords u = (1 - x / tan) / 2 (v alike), affine in the
    position, make uv the film position: the visible part spans [0, 1]^2 and pixel (px, py) covers
    [px, px + 1] x [py, py + 1] / 64."""
    corner = lambda x: (1.0 - x / float(TAN)) / 2.0
    uv = np.array([[corner(-1), corner(-1)], [corner(1), corner(-1)], [corner(1), corner(1)], [corner(-1), corner(1)]],
                  np.float32)
    sc = quad_scene(pg, uv, pg.scenes.material("diffuse", reflectance=reflectance, twosided=True), W, W)
    sc.set_envmap(np.ones((8, 16, 3), np.float32))
    return sc.finalize()


def render(pg, sc, spp, textures=None, passes=0, **cfg):
    d = make_dev(pg, **cfg)
    d.upload(sc)
    if textures is not None:
        d.set_textures(*textures)
    off = 0
    for it in range(passes):
        d.render_pass(2 ** it, off, True)
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    d.reset_film()
    d.render_pass(spp, off)
    out = dict(film=d.read_film(), aov=d.read_aovs() if cfg.get("aovs") else None, tree=d.get_sdtree(), stats=d.stats())
    d.close()
    return out


def test_texture_scales_the_throughput_exactly(pg):
    rng = np.random.default_rng(4)
    rho = rng.choice(np.array([1.0, 0.5, 0.25, 0.125], np.float32), (4, 4, 3))
    sc = lit_quad(pg)
    cfg = dict(max_depth=2, aovs=1)
    white = render(pg, sc, 4, **cfg)
    tex = [pg.scenes.make_texture("bitmap", rho, filter="nearest", wrap="clamp")]
    col = render(pg, sc, 4, textures=(tex, [(0, 0)], sc.texcoords), **cfg)
    fw, fc = white["film"][0], col["film"][0]
    np.testing.assert_array_equal(fw[..., 3], 4.0)
    np.testing.assert_array_equal(fc[..., 3], fw[..., 3])  # the counts
    assert fw[..., :3].min() > 0
    # pixels whose square, widened by one pixel, lies inside one texel (16 pixels wide): px % 16 in [1, 14]
    p = np.arange(W)
    inside = ((p - 1) // 16 == (p + 1) // 16)
    mask = inside[:, None] & inside[None, :]
    assert mask.mean() >= 0.6
    r = rho[(p // 16)[:, None], (p // 16)[None, :]]  # [py, px] -> texel (px // 16, py // 16) = rho[y, x]
    want = r * fw[..., :3]
    print("pixels compared: %.1f %%; mismatching: %d" % (100 * mask.mean(), (fc[..., :3][mask] != want[mask]).any(-1).sum()))
    np.testing.assert_array_equal(fc[..., :3][mask], want[mask])
    np.testing.assert_array_equal(col["film"][1][..., :3][mask], (r * r * white["film"][1][..., :3])[mask])
    alb = col["aov"][0]
    np.testing.assert_array_equal(alb[..., 3], 4.0)
    np.testing.assert_array_equal(alb[..., :3][mask], (r * np.float32(4.0))[mask])
    np.testing.assert_array_equal(white["aov"][0][..., :3], 4.0)
    for k in COUNTED:
        assert col["stats"][k] == white["stats"][k], k


def test_bilinear_reaches_the_shader(pg):
    rgb = np.array([[[0.1, 0.9, 0.5], [0.8, 0.2, 0.5]], [[0.4, 0.6, 0.0], [1.0, 0.0, 1.0]]], np.float32)
    sc = lit_quad(pg)
    tex = [pg.scenes.make_texture("bitmap", rgb, filter="bilinear", wrap="clamp")]
    out = render(pg, sc, 1, textures=(tex, [(0, 0)], sc.texcoords), max_depth=2, aovs=1)
    alb = out["aov"][0]
    np.testing.assert_array_equal(alb[..., 3], 1.0)
    c = (np.arange(W, dtype=np.float32) + np.float32(0.5)) / np.float32(W)
    centre = np.stack(np.meshgrid(c, c), -1).reshape(-1, 2)  # [py, px] -> (u, v) = (x, y) film position
    ref = T.bitmap(rgb, centre, "bilinear", "clamp").reshape(W, W, 3)
    L = (rgb.reshape(-1, 3).max(0) - rgb.reshape(-1, 3).min(0)).max() * 2  # largest texel difference x max(W, H)
    d = np.sqrt(2.0) / W                                                     # a pixel diagonal in uv
    err = np.abs(alb[..., :3] - ref).max()
    print("bilinear albedo: max |albedo - ref(centre)| = %.4f, bound L d = %.4f" % (err, L * d))
    assert err <= L * d
    assert np.ptp(alb[..., 0]) > 0.5  # and it is not a constant


VARIANTS = {
    "norays": ({}, ("PG_NO_RAYS_FUSION",)),
    "notail": ({"tail_paths": -1}, ()),
    "chunks": ({"max_paths_in_flight": 4096}, ()),
}


@pytest.fixture(scope="module")
def variant_job(pg):
    sc = lit_quad(pg, (0.5, 0.5, 0.5))
    tex = [pg.scenes.make_texture("bitmap", texels(5, 4, 9), filter="bilinear", wrap="repeat", uscale=3.0, vscale=2.0)]
    textures = (tex, [(0, 0)], sc.texcoords)
    return sc, textures, render(pg, sc, 4, textures=textures, passes=2, guiding=1, s_tree_threshold=300.0)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_launch_variants_are_bit_identical(pg, monkeypatch, variant_job, variant):
    sc, textures, base = variant_job
    cfg, env = VARIANTS[variant]
    for name in env:
        monkeypatch.setenv(name, "1")
    out = render(pg, sc, 4, textures=textures, passes=2, guiding=1, s_tree_threshold=300.0, **cfg)
    assert np.array_equal(out["film"][0], base["film"][0]) and np.array_equal(out["film"][1], base["film"][1])
    assert np.array_equal(out["tree"], base["tree"])
    assert base["film"][0][..., :3].sum() > 0


def test_shard_union_is_bit_identical(pg, variant_job):
    sc, textures, base = variant_job
    parts = [make_dev(pg, sc, guiding=1, s_tree_threshold=300.0, rank=r, world_size=2, tile_size=16) for r in range(2)]
    full = make_dev(pg, sc, guiding=1, s_tree_threshold=300.0, tile_size=16)
    for d in parts + [full]:
        d.set_textures(*textures)
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
        assert np.array_equal(films[2][k], base["film"][k])  # per-pixel results do not depend on the tile size
    assert ((films[0][0][..., 3] > 0) ^ (films[1][0][..., 3] > 0)).all()
    for d in parts + [full]:
        d.close()


# ---- 10. errors -------------------------------------------------------------------------------------------------------
def test_errors(pg):
    from mitsuba_path_guiding_amd.integrator import PGError
    S, c = pg.scenes, pg.capi
    good = S.make_texture("bitmap", texels(2, 2))

    def fails(d, status, *args):
        with pytest.raises(PGError) as e:
            d.set_textures(*args)
        assert e.value.status == status, e.value
        assert len(d.lib.pg_last_error(d.h)) > 0

    d = make_dev(pg)
    fails(d, c.PG_ERR_STATE, [good], [(0, 0)], None)  # before pg_upload_scene
    sc = S.cornell(16, 16, short_material=S.material("conductor"))
    d.upload(sc)
    d.set_textures([good], [(0, 0)], None)            # fine, and again (replaces them)
    d.set_textures([good, S.make_texture("checkerboard")], [(0, 1), (1, 0)], None)
    zero = S.make_texture("bitmap", texels(2, 2))
    zero.width = 0
    fails(d, c.PG_ERR_INVALID, [zero], [(0, 0)], None)
    zero.width, zero.height = 2, 0
    fails(d, c.PG_ERR_INVALID, [zero], [(0, 0)], None)
    for bad in (np.nan, np.inf, -0.5):
        t = texels(2, 2)
        t[1, 0, 2] = bad
        fails(d, c.PG_ERR_INVALID, [S.make_texture("bitmap", t)], [(0, 0)], None)
    fails(d, c.PG_ERR_INVALID, [good], [(0, 1)], None)                    # texture index out of range
    fails(d, c.PG_ERR_INVALID, [good], [(len(sc.materials), 0)], None)    # material index out of range
    fails(d, c.PG_ERR_INVALID, [good], [(4, 0)], None)                    # a conductor has no diffuse slot
    fails(d, c.PG_ERR_INVALID, [good, good], [(0, 0), (0, 1)], None)      # a material bound twice
    d.render_pass(1, 0)  # the failed calls left the last good textures in place
    fails(d, c.PG_ERR_STATE, [good], [(0, 0)], None)                      # after the first render pass
    fails(d, c.PG_ERR_STATE, [], [], None)
    d.upload(sc)
    d.set_textures([good], [(0, 0)], None)                                # a new upload: allowed again
    d.close()
    v = make_dev(pg, integrator=c.PG_INTEGRATOR_VOLPATH)
    v.upload(S.smoke(8, 8, res=32))
    fails(v, c.PG_ERR_INVALID, [good], [(0, 0)], None)                    # a volpath context
    v.close()


# ---- 11. XML end to end ------------------------------------------------------------------------------------------------
def test_xml_end_to_end(pg, tmp_path):
    """The scene of test_textures.py loaded from XML renders what the same scene built through scenes.py renders"""
    import warnings
    from test_textures import xml_scene
    S = pg.scenes
    p, rgb = xml_scene(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = pg.mitsuba_xml.load(str(p)).scene
    b = S.Scene()
    m0 = b.add_material(S.material("diffuse", reflectance=(0.5, 0.5, 0.5), twosided=True))
    m1 = b.add_material(S.material("plastic", diffuse_reflectance=(0.5, 0.5, 0.5)))
    for k, sh in enumerate(a.shapes):  # the loader's geometry; materials, textures and texcoords built here
        v0 = int(a.indices[sh.tri_begin:sh.tri_begin + sh.tri_count].min())
        v1 = int(a.indices[sh.tri_begin:sh.tri_begin + sh.tri_count].max()) + 1
        F = a.indices[sh.tri_begin:sh.tri_begin + sh.tri_count] - v0
        uv = np.array([[0, 1], [1, 1], [1, 0.25], [0, 0.25]], np.float32) if k < 2 else None
        if k < 2:
            b.add_mesh(a.positions[v0:v1], F, a.normals[v0:v1], material=(m0, m1)[k], uv=uv)
        else:
            e = b.add_material(S.material("diffuse", reflectance=(0.0, 0.0, 0.0)))
            b.add_mesh(a.positions[v0:v1], F, a.normals[v0:v1], material=e, radiance=(5.0, 5.0, 5.0))
    b.bind_texture(m0, b.add_texture("bitmap", rgb, filter="bilinear", wrap="mirror", wrap_v="clamp", uscale=2.0, vscale=2.0,
                                     voffset=0.25))
    b.bind_texture(m1, b.add_texture("checkerboard", color0=(0.8, 0.1, 0.1), color1=(0.1, 0.1, 0.8), uscale=4.0, vscale=3.0))
    c = a.camera
    b.set_camera(list(c.origin), list(c.target), list(c.up), c.fov_x_deg, 32, 32, c.near_clip, c.far_clip)
    a.set_camera(list(c.origin), list(c.target), list(c.up), c.fov_x_deg, 32, 32, c.near_clip, c.far_clip)
    a.finalize()
    b.finalize()
    ja, jb = job(pg, a, 2, 4), job(pg, b, 2, 4)
    assert_same_job(ja, jb)
    a.texture_bindings = []  # and the textures were on: the same scene without them renders another image
    assert not np.array_equal(job(pg, a, 2, 4)["film"][0], ja["film"][0])
