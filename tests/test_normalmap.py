"""Normal maps without a GPU: the numpy restatement's known answers (normalmap_ref.py), the XML loader's normalmap
branch and the Scene methods."""
import numpy as np
import pytest

import normalmap_ref as R
from test_textures import QUAD_OBJ, SENSOR

F = np.float32
P = [np.array(p, F) for p in ((0.25, -1.0, 2.0), (1.5, 0.5, 2.25), (-0.75, 1.0, 3.0))]
TC = [np.array(t, F) for t in ((0.125, 0.75), (0.9, -0.3), (0.4, 1.6))]


def frame_of(c, tc=TC):
    d1, d2 = P[1] - P[0], P[2] - P[0]
    n = R.normalize(R.cross(d1, d2))
    dpdu = R.tangent(*P, *(tc if tc is not None else (None, None, None)))
    return n, dpdu, R.perturbed_frame(n, dpdu, np.array(c, F))


# ---- reference KATs -----------------------------------------------------------------------------------------------------
def test_flat_map_returns_the_base_frame():
    n, dpdu, (s, t, n2) = frame_of((0.5, 0.5, 1.0))
    bs, bt, bn = R.shading_frame(n, dpdu)
    # toWorld((0, 0, 1)) = n and |n| = 1 within one rounding: the renormalised normal moves by an ulp at most
    np.testing.assert_allclose(n2, bn, atol=2e-7)
    np.testing.assert_allclose(s, bs, atol=1e-6)
    np.testing.assert_allclose(t, bt, atol=1e-6)
    # an axis-aligned normal renormalises exactly: the base frame bit for bit
    s, t, n2 = R.perturbed_frame(np.array([0, 1, 0], F), np.array([2, 0.5, -1], F), np.array([0.5, 0.5, 1.0], F))
    bs, bt, bn = R.shading_frame(np.array([0, 1, 0], F), np.array([2, 0.5, -1], F))
    for a, b in ((s, bs), (t, bt), (n2, bn)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("c", [(0.5, 0.5, 1.0), (0.9, 0.3, 0.8), (0.1, 0.7, 0.6), (0.75, 0.5, 0.933)])
def test_frame_is_orthonormal(c):
    _, _, (s, t, n) = frame_of(c)
    assert s.dtype == F and t.dtype == F and n.dtype == F
    G = np.array([[R.dot(a, b) for b in (s, t, n)] for a in (s, t, n)], np.float64)
    np.testing.assert_allclose(G, np.eye(3), atol=1e-6)
    np.testing.assert_allclose(R.cross(s, t), n, atol=1e-6)  # right-handed


def test_perturbed_normal_is_the_tilted_one():
    # nl = (sin 30, 0, cos 30) in the base frame: n' = s sin + n cos
    a = np.radians(30.0)
    c = (np.array([np.sin(a), 0.0, np.cos(a)]) + 1) / 2
    n, dpdu, (s2, t2, n2) = frame_of(c)
    bs, bt, bn = R.shading_frame(n, dpdu)
    np.testing.assert_allclose(n2, bs * F(np.sin(a)) + bn * F(np.cos(a)), atol=1e-6)
    np.testing.assert_allclose(t2, bt, atol=1e-6)  # a tilt about t leaves t


def test_degenerate_uv_tangent_is_orthogonal_to_the_face_normal():
    for tc in ([TC[0], TC[0], TC[2]], [TC[0], TC[1], TC[0] + F(2) * (TC[1] - TC[0])], [TC[1]] * 3):
        dpdu = R.tangent(*P, *tc)
        fn = R.normalize(R.cross(P[1] - P[0], P[2] - P[0]))
        assert abs(float(R.dot(dpdu, fn))) < 1e-6
        np.testing.assert_allclose(np.sqrt(R.dot(dpdu, dpdu)), 1.0, atol=1e-6)
    # both branches of coordinateSystem
    for q in ([(0, 0, 0), (0, 1, 0), (0, 0, 1)], [(0, 0, 0), (1, 0, 0), (0, 0, 1)]):
        dpdu = R.tangent(*q, TC[0], TC[0], TC[0])
        fn = R.normalize(R.cross(np.array(q[1], F), np.array(q[2], F)))
        assert float(R.dot(dpdu, fn)) == 0.0
    # a zero-area triangle keeps p1 - p0
    np.testing.assert_array_equal(R.tangent(P[0], P[1], P[0] + F(2) * (P[1] - P[0]), *TC).view(np.uint32),
                                  (P[1] - P[0]).view(np.uint32))


def test_no_texcoord_tangent_is_p1_minus_p0_bitwise():
    rng = np.random.default_rng(0)
    for _ in range(64):
        p = rng.normal(size=(3, 3)).astype(F)
        p[rng.integers(3), rng.integers(3)] = rng.choice([0.0, -0.0])
        np.testing.assert_array_equal(R.tangent(*p).view(np.uint32), (p[1] - p[0]).view(np.uint32))


def test_uv_tangent_is_dp_du():
    # texcoords affine in the position, u along a and v along b: dpdu = a / |a|^2 scaled so that u grows by 1
    a, b = np.array([2.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.5])
    q = [np.array(x, F) for x in ((0, 1, 0), (1, 1, 0), (0.25, 1, 1))]
    tc = [np.array([np.dot(x, a) / np.dot(a, a), np.dot(x, b) / np.dot(b, b)], F) for x in q]
    np.testing.assert_allclose(R.tangent(*q, *tc), a, atol=1e-6)


def test_hemisphere_rule():
    shN = np.array([0, 0, 1], F)
    assert R.wrong_side(np.array([0.1, 0, 0.2], F), shN, F(-0.3))
    assert R.wrong_side(np.array([0.1, 0, -0.2], F), shN, F(0.3))
    assert R.wrong_side(np.array([1, 0, 0], F), shN, F(0.3))  # grazing: zero counts as wrong
    assert not R.wrong_side(np.array([0.1, 0, 0.2], F), shN, F(0.3))
    assert not R.wrong_side(np.array([0.1, 0, -0.2], F), shN, F(-0.3))


# ---- XML ---------------------------------------------------------------------------------------------------------------
def nmap_xml(tmp_path, bsdf, gamma='<float name="gamma" value="1"/>'):
    rgb = np.random.default_rng(2).uniform(0.3, 0.7, (4, 4, 3)).astype(F)
    rgb[..., 2] = 0.9
    np.save(tmp_path / "nmap.npy", rgb)
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    tex = (f'<texture type="bitmap"><string name="filename" value="nmap.npy"/><string name="filterType" value="nearest"/>'
           f'<float name="uscale" value="3"/>{gamma}</texture>')
    xml = f"""<scene version="0.5.0">{SENSOR}
    <shape type="obj"><string name="filename" value="quad.obj"/>{bsdf.replace("TEX", tex)}</shape>
    <shape type="rectangle"><transform name="toWorld"><rotate y="1" angle="180"/><translate y="2.5" z="3"/></transform>
      <emitter type="area"><rgb name="radiance" value="5, 5, 5"/></emitter></shape>
    </scene>"""
    p = tmp_path / "scene.xml"
    p.write_text(xml)
    return p, rgb


GOOD = ('<bsdf type="normalmap">TEX<bsdf type="twosided"><bsdf type="roughconductor"><string name="material" value="Al"/>'
        '<float name="alpha" value="0.2"/></bsdf></bsdf></bsdf>')


def test_xml_normalmap_loads_and_round_trips(pg, tmp_path):
    X, c = pg.mitsuba_xml, pg.capi
    p, rgb = nmap_xml(tmp_path, GOOD)
    sc = X.load(str(p)).scene
    assert len(sc.normal_maps) == 1 and sc.normal_map_bindings == [(0, 0)] and sc.texture_bindings == []
    t = sc.normal_maps[0]
    assert (t.type, t.width, t.height, t.filter, t.uscale) == (c.PG_TEXTURE_BITMAP, 4, 4, c.PG_TEXFILTER_NEAREST, 3.0)
    np.testing.assert_array_equal(t._rgb, rgb)
    m = sc.materials[0]
    assert m.type == c.PG_BSDF_ROUGHCONDUCTOR and (m.flags & c.PG_MAT_TWOSIDED)
    q = tmp_path / "out" / "saved.xml"
    X.save(sc, str(q))
    assert '<bsdf type="normalmap">' in q.read_text()
    sc2 = X.load(str(q)).scene
    assert sc2.normal_map_bindings == [(0, 0)]
    t2 = sc2.normal_maps[0]
    np.testing.assert_array_equal(t2._rgb, rgb)
    assert (t2.filter, t2.wrap_u, t2.wrap_v, t2.uscale, t2.vscale) == (t.filter, t.wrap_u, t.wrap_v, t.uscale, t.vscale)
    assert bytes(sc2.materials[0]) == bytes(m)
    np.testing.assert_array_equal(sc2.texcoords, sc.texcoords)


def test_xml_normalmap_with_a_textured_nested_bsdf(pg, tmp_path):
    bsdf = ('<bsdf type="normalmap">TEX<bsdf type="diffuse"><texture type="checkerboard" name="reflectance"/></bsdf></bsdf>')
    p, _ = nmap_xml(tmp_path, bsdf)
    sc = pg.mitsuba_xml.load(str(p)).scene
    assert sc.normal_map_bindings == [(0, 0)] and sc.texture_bindings == [(0, 0)]


def test_xml_normalmap_needs_an_explicit_gamma(pg, tmp_path):
    p, _ = nmap_xml(tmp_path, GOOD, gamma="")
    with pytest.raises(ValueError, match="gamma"):
        pg.mitsuba_xml.load(str(p))


def test_xml_twosided_normalmap_is_out_of_scope(pg, tmp_path):
    p, _ = nmap_xml(tmp_path, '<bsdf type="twosided"><bsdf type="normalmap">TEX<bsdf type="diffuse"/></bsdf></bsdf>')
    with pytest.raises(NotImplementedError, match="perturbed frame"):
        pg.mitsuba_xml.load(str(p))


@pytest.mark.parametrize("nested", ["dielectric", "roughdielectric", "null"])
def test_xml_normalmap_rejects_transmissive_nested_bsdfs(pg, tmp_path, nested):
    p, _ = nmap_xml(tmp_path, f'<bsdf type="normalmap">TEX<bsdf type="{nested}"/></bsdf>')
    with pytest.raises(NotImplementedError, match="dielectric"):
        pg.mitsuba_xml.load(str(p))


def test_xml_normalmap_accepts_only_a_bitmap(pg, tmp_path):
    p, _ = nmap_xml(tmp_path, '<bsdf type="normalmap"><texture type="checkerboard"/><bsdf type="diffuse"/></bsdf>')
    with pytest.raises(NotImplementedError, match="bitmap"):
        pg.mitsuba_xml.load(str(p))


# ---- Scene methods -----------------------------------------------------------------------------------------------------
def test_scene_methods(pg):
    S = pg.scenes
    s = S.Scene()
    d = s.add_material(S.material("diffuse"))
    g = s.add_material(S.material("dielectric"))
    flat = np.tile(np.array([0.5, 0.5, 1.0], F), (2, 2, 1))
    k = s.add_normal_map(flat, filter="nearest")
    assert k == 0 and s.normal_maps[0].type == pg.capi.PG_TEXTURE_BITMAP
    s.bind_normal_map(d, k)
    assert s.normal_map_bindings == [(d, k)]
    with pytest.raises(ValueError, match="twice"):
        s.bind_normal_map(d, k)
    with pytest.raises(ValueError, match="dielectric"):
        s.bind_normal_map(g, k)
    with pytest.raises(ValueError, match="range"):
        s.bind_normal_map(d, 5)
    assert s.normal_map_bindings == [(d, k)]
