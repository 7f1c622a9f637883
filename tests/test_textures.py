"""Textures on the host: the numpy restatement of the lookups (tests/texture_ref.py, the yardstick of
test_gpu_textures.py) against hand-computed values, and the scene builder's texture records."""
import ctypes as C

import numpy as np
import pytest

import texture_ref as T

# 2 x 2 texture, texel (x, y) = 1 + x + 2 y in every channel: T(0,0) = 1, T(1,0) = 2, T(0,1) = 3, T(1,1) = 4
RGB = np.repeat(np.array([[1, 2], [3, 4]], np.float32)[:, :, None], 3, axis=2)


@pytest.mark.parametrize("wrap,left_edge,right_edge", [
    # left edge uv = (0, 0.25): x = -0.5 -> 0.5 T(-1, 0) + 0.5 T(0, 0); right edge uv = (1, 0.75): 0.5 T(1, 1) + 0.5 T(2, 1)
    ("repeat", 0.5 * 2 + 0.5 * 1, 0.5 * 4 + 0.5 * 3),  # T(-1, 0) = T(1, 0), T(2, 1) = T(0, 1)
    ("clamp", 1.0, 4.0),                                # T(-1, 0) = T(0, 0), T(2, 1) = T(1, 1)
    ("mirror", 1.0, 4.0),                               # -1 mod 4 = 3 -> 4 - 3 - 1 = 0; 2 -> 4 - 2 - 1 = 1
    ("zero", 0.5, 2.0),
    ("one", 0.5 * 1 + 0.5 * 1, 0.5 * 4 + 0.5 * 1),
])
def test_bilinear_by_hand(wrap, left_edge, right_edge):
    uv = [(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75), (0.5, 0.5), (0.0, 0.25), (1.0, 0.75)]
    got = T.bitmap(RGB, uv, "bilinear", wrap)
    want = [1.0, 2.0, 3.0, 4.0, 2.5, left_edge, right_edge]  # texel centres, the middle, the two edges
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, np.repeat(np.array(want, np.float32)[:, None], 3, axis=1))


def test_nearest_and_wraps_by_hand():
    uv = [(0.1, 0.1), (0.6, 0.1), (0.1, 0.6), (0.999, 0.999), (-0.25, 0.25), (1.25, 0.75), (2.75, 0.25)]
    # floor(u W): 0, 1, 0, 1, -1, 2, 5
    want = {"repeat": [1, 2, 3, 4, 2, 3, 2], "clamp": [1, 2, 3, 4, 1, 4, 2], "mirror": [1, 2, 3, 4, 1, 4, 2],
            "zero": [1, 2, 3, 4, 0, 0, 0], "one": [1, 2, 3, 4, 1, 1, 1]}
    for wrap, w in want.items():
        np.testing.assert_array_equal(T.bitmap(RGB, uv, "nearest", wrap)[:, 0], np.array(w, np.float32), err_msg=wrap)
    # x is answered before y: x out of range with "one" wins over y out of range with "zero"
    np.testing.assert_array_equal(T.bitmap(RGB, [(1.5, 1.5)], "nearest", "one", "zero"), [[1, 1, 1]])
    np.testing.assert_array_equal(T.bitmap(RGB, [(1.5, 1.5)], "nearest", "zero", "one"), [[0, 0, 0]])
    # the uv transform, and non-finite uv
    np.testing.assert_array_equal(T.bitmap(RGB, [(0.05, 0.3)], "nearest", "clamp", uscale=2.0, vscale=0.5, uoffset=0.5,
                                           voffset=0.5)[:, 0], [4.0])  # (0.6, 0.65)
    bad = [(np.nan, 0.1), (0.1, np.inf), (-np.inf, 0.2)]
    assert not T.bitmap(RGB, bad, "bilinear").any() and not T.bitmap(RGB, bad, "nearest").any()


def test_checkerboard_by_hand():
    c0, c1 = (1.0, 0.5, 0.25), (0.0, 0.125, 0.5)
    uv = [(0.25, 0.25), (0.75, 0.25), (-0.25, 0.25), (1.25, 1.75)]
    # (int)(u 2), (int)(v 2): (0, 0) -> x = y = -1: color0; (1, 0): color1; (-0.5 -> 0 by truncation, 0): color0 (floor
    # would give -1 and color1); (2, 3) -> x = -1, y = 1: color1
    np.testing.assert_array_equal(T.checkerboard(c0, c1, uv), np.array([c0, c1, c0, c1], np.float32))
    np.testing.assert_array_equal(T.average(color0=c0, color1=c1), np.array([0.5, 0.3125, 0.375], np.float32))
    np.testing.assert_array_equal(T.average(RGB), [2.5, 2.5, 2.5])


def test_hit_uv_by_hand():
    # test_dgeom.cpp case 2: barycentrics (0.7, 0.1, 0.2) over (0.1, 0.1), (1.1, 0.1), (0.1, 0.9) -> (0.2, 0.26)
    uv = T.hit_uv((0.1, 0.1), (1.1, 0.1), (0.1, 0.9), [0.1], [0.2])
    assert uv.dtype == np.float32 and np.allclose(uv, [[0.2, 0.26]], atol=1e-6)
    np.testing.assert_array_equal(T.hit_uv((0, 0), (1, 0), (0, 1), [0.3], [0.6]), np.array([[0.3, 0.6]], np.float32))


def test_scene_builder_textures(pg):
    S = pg.scenes
    s = S.Scene()
    m0 = s.add_material(S.material("diffuse", reflectance=(0.5, 0.5, 0.5)))
    m1 = s.add_material(S.material("diffuse", reflectance=(0.2, 0.2, 0.2)))
    V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    F = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    s.add_mesh(V, F, material=m0, uv=uv)          # flat shading unshares the vertices: texcoords follow
    s.add_mesh(V + 2, F, material=m1)             # no texcoords: zeros
    assert s.texcoords.shape == (12, 2)
    np.testing.assert_array_equal(s.texcoords[:6], uv[F].reshape(-1, 2))
    assert not s.texcoords[6:].any()
    t = s.add_texture("bitmap", RGB, filter="nearest", wrap="mirror", wrap_v="one", uscale=2.0, voffset=0.25)
    k = s.add_texture("checkerboard", color0=(1, 0, 0), color1=(0, 0, 1), average=(0.5, 0.0, 0.5))
    s.bind_texture(m0, t)
    s.bind_texture(m1, k)
    a, b = s.textures
    c = pg.capi
    assert (a.type, a.width, a.height, a.filter, a.wrap_u, a.wrap_v) == (c.PG_TEXTURE_BITMAP, 2, 2, c.PG_TEXFILTER_NEAREST,
                                                                         c.PG_TEXWRAP_MIRROR, c.PG_TEXWRAP_ONE)
    assert (a.uscale, a.vscale, a.uoffset, a.voffset) == (2.0, 1.0, 0.0, 0.25) and a.average[0] < 0
    np.testing.assert_array_equal(np.ctypeslib.as_array(a.rgb, (12,)), RGB.reshape(-1))
    assert b.type == c.PG_TEXTURE_CHECKERBOARD and list(b.color1) == [0, 0, 1] and list(b.average) == [0.5, 0.0, 0.5]
    assert s.texture_bindings == [(m0, t), (m1, k)]
    assert C.sizeof(c.pg_texture) == 88 and C.sizeof(c.pg_texture_binding) == 8
    with pytest.raises(ValueError):
        s.add_texture("scale")
    assert S.Scene().texcoords is None


# ---- the XML layer (mitsuba_xml.load / save) ---------------------------------------------------------------------------
QUAD_OBJ = """v -1 -1 0
v 1 -1 0
v 1 1 0
v -1 1 0
vn 0 0 1
vt 0 0
vt 1 0
vt 1 0.75
vt 0 0.75
f 1/1/1 2/2/1 3/3/1
f 1/1/1 3/3/1 4/4/1
"""
SENSOR = ('<sensor type="perspective"><float name="fov" value="40"/><transform name="toWorld"><lookat origin="0, 0, 4" '
          'target="0, 0, 0" up="0, 1, 0"/></transform><film type="hdrfilm"><integer name="width" value="16"/>'
          '<integer name="height" value="16"/></film></sensor>')


def xml_scene(tmp_path, extra=""):
    """a bitmap (.npy, default filterType = ewa) through <ref> inside twosided, and a nested checkerboard on plastic"""
    rgb = np.random.default_rng(1).uniform(0, 1, (3, 5, 3)).astype(np.float32)
    np.save(tmp_path / "tex.npy", rgb)
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    xml = f"""<scene version="0.5.0">{SENSOR}
    <texture type="bitmap" id="wood"><string name="filename" value="tex.npy"/><string name="wrapModeU" value="mirror"/>
      <string name="wrapModeV" value="clamp"/><float name="uvscale" value="2"/><float name="voffset" value="0.25"/></texture>
    <bsdf type="twosided" id="front"><bsdf type="diffuse"><ref id="wood" name="reflectance"/></bsdf></bsdf>
    <shape type="obj"><string name="filename" value="quad.obj"/><ref id="front"/></shape>
    <shape type="obj"><string name="filename" value="quad.obj"/>
      <transform name="toWorld"><translate x="2.5"/></transform>
      <bsdf type="plastic"><texture type="checkerboard" name="diffuseReflectance"><rgb name="color0" value="0.8, 0.1, 0.1"/>
        <rgb name="color1" value="0.1, 0.1, 0.8"/><float name="uscale" value="4"/><float name="vscale" value="3"/></texture>
        {extra}</bsdf></shape>
    <shape type="rectangle"><transform name="toWorld"><rotate y="1" angle="180"/><translate y="2.5" z="3"/></transform>
      <emitter type="area"><rgb name="radiance" value="5, 5, 5"/></emitter></shape>
    </scene>"""
    p = tmp_path / "scene.xml"
    p.write_text(xml)
    return p, rgb


def test_xml_textures(pg, tmp_path):
    X, c = pg.mitsuba_xml, pg.capi
    p, rgb = xml_scene(tmp_path)
    with pytest.warns(UserWarning, match="ewa"):
        sc = X.load(str(p)).scene
    assert len(sc.textures) == 2 and sc.texture_bindings == [(0, 0), (1, 1)]
    a, b = sc.textures
    assert (a.type, a.width, a.height, a.filter, a.wrap_u, a.wrap_v) == (c.PG_TEXTURE_BITMAP, 5, 3, c.PG_TEXFILTER_BILINEAR,
                                                                         c.PG_TEXWRAP_MIRROR, c.PG_TEXWRAP_CLAMP)
    assert (a.uscale, a.vscale, a.uoffset, a.voffset) == (2.0, 2.0, 0.0, 0.25)
    np.testing.assert_array_equal(a._rgb, rgb)
    assert b.type == c.PG_TEXTURE_CHECKERBOARD and (b.uscale, b.vscale) == (4.0, 3.0)
    np.testing.assert_array_equal(list(b.color0) + list(b.color1), np.array([0.8, 0.1, 0.1, 0.1, 0.1, 0.8], np.float32))
    m0, m1 = sc.materials[0], sc.materials[1]
    assert m0.type == c.PG_BSDF_DIFFUSE and (m0.flags & c.PG_MAT_TWOSIDED) and m1.type == c.PG_BSDF_PLASTIC
    np.testing.assert_allclose(list(m0.diffuse_reflectance)[:3], rgb.reshape(-1, 3).mean(0), rtol=1e-6)  # getAverage
    # texcoords: vt with v flipped (obj.cpp flipTexCoords), per vertex of both quads; none on the rectangle
    uv = sc.texcoords
    assert uv.shape == (len(sc.positions), 2)
    want = np.array([[0, 1], [1, 1], [1, 0.25], [0, 0.25]], np.float32)
    np.testing.assert_array_equal(uv[:4], want)
    np.testing.assert_array_equal(uv[4:8], want)
    assert not uv[8:].any()
    # any other textured parameter still raises
    bad, _ = xml_scene(tmp_path, '<texture type="checkerboard" name="specularReflectance"/>')
    with pytest.raises(NotImplementedError, match="specularReflectance"):
        X.load(str(bad))
    with pytest.raises(NotImplementedError):
        X.load('<scene version="0.5.0"><bsdf type="diffuse"><texture type="scale" name="reflectance"/></bsdf></scene>')


def test_xml_texture_round_trip(pg, tmp_path):
    import warnings
    X = pg.mitsuba_xml
    p, _ = xml_scene(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = X.load(str(p)).scene
    out = tmp_path / "saved"
    out.mkdir()
    b = X.load(X.save(a, str(out / "again.xml"))).scene  # explicit filterType: no warning needed
    np.testing.assert_array_equal(a.positions, b.positions)
    np.testing.assert_array_equal(a.indices, b.indices)
    np.testing.assert_array_equal(a.texcoords, b.texcoords)
    assert len(b.texture_bindings) == len(a.texture_bindings) == 2
    for (ma, ta), (mb, tb) in zip(a.texture_bindings, b.texture_bindings):
        x, y = a.textures[ta], b.textures[tb]
        assert a.materials[ma].type == b.materials[mb].type and a.materials[ma].flags == b.materials[mb].flags
        for f in ("type", "width", "height", "filter", "wrap_u", "wrap_v", "uscale", "vscale", "uoffset", "voffset"):
            assert getattr(x, f) == getattr(y, f), f
        assert list(x.color0) == list(y.color0) and list(x.color1) == list(y.color1)
        if x.type == pg.capi.PG_TEXTURE_BITMAP:
            np.testing.assert_array_equal(x._rgb, y._rgb)


def test_texture_images(pg, tmp_path):
    """8-bit PNG through PIL: the sRGB curve, or value^gamma; float formats stay linear; anything else raises"""
    from PIL import Image
    X = pg.mitsuba_xml
    px = np.array([[[0, 128, 255], [64, 64, 64]]], np.uint8)
    Image.fromarray(px).save(tmp_path / "t.png")
    lin = X.read_texture_image(str(tmp_path / "t.png"))
    v = px / 255.0
    srgb = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    np.testing.assert_allclose(lin, srgb, atol=1e-6)
    np.testing.assert_allclose(X.read_texture_image(str(tmp_path / "t.png"), 2.2), v ** 2.2, atol=1e-6)
    np.save(tmp_path / "t.npy", v.astype(np.float32))
    np.testing.assert_array_equal(X.read_texture_image(str(tmp_path / "t.npy")), v.astype(np.float32))
    with pytest.raises(NotImplementedError):
        X.read_texture_image(str(tmp_path / "t.tga"))
