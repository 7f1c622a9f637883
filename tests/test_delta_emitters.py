"""Point, spot and directional emitters without a GPU: the ctypes mirror against the header, the Mitsuba XML subset
(mitsuba_xml.load / save) and the numpy restatement (tests/emitter_ref.py) against hand values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emitter_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENE = """<scene version="0.5.0">
<sensor type="perspective">
  <float name="fov" value="40"/>
  <transform name="toWorld"><lookat origin="0.5, 1, -3" target="0.5, 1, 0" up="0, 1, 0"/></transform>
  <film type="hdrfilm"><integer name="width" value="32"/><integer name="height" value="24"/></film>
</sensor>
<shape type="rectangle"><bsdf type="diffuse"/></shape>
{emitters}
</scene>"""
POINT = '<emitter type="point"><point name="position" x="0.25" y="2" z="-1.5"/><rgb name="intensity" value="3, 2, 1"/></emitter>'
SPOT = ('<emitter type="spot"><rgb name="intensity" value="10, 10, 8"/><float name="cutoffAngle" value="25"/>'
        '<float name="beamWidth" value="10"/><transform name="toWorld"><lookat origin="1, 3, -2" target="0, 0, 0" '
        'up="0, 1, 0"/></transform></emitter>')
DIRECTIONAL = ('<emitter type="directional"><vector name="direction" x="0.5" y="-1" z="0.25"/>'
               '<rgb name="irradiance" value="1.5, 1.25, 1"/></emitter>')


def fields(e):
    return (e.type, tuple(e.position), tuple(e.direction), tuple(e.intensity), e.cutoff_angle, e.beam_width)


def test_struct_matches_the_header(pg):
    """size and field offsets of capi.pg_delta_emitter against include/pg_capi.h, read as text"""
    text = open(os.path.join(ROOT, "include", "pg_capi.h")).read()
    body = re.search(r"typedef struct pg_delta_emitter \{(.*?)\} pg_delta_emitter;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        assert typ in ("int32_t", "float")  # 4-byte fields only: no padding
        for name in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            n = int(m.group(2) or 1)
            want.append((m.group(1), off, 4 * n))
            off += 4 * n
    T = pg.capi.pg_delta_emitter
    got = [(name, getattr(T, name).offset, getattr(T, name).size) for name, _ in T._fields_]
    assert got == want
    assert C.sizeof(T) == off == 48
    enum = re.search(r"typedef enum \{(.*?)\} pg_delta_type;", text, re.S).group(1)
    assert [x.replace(" ", "") for x in enum.split(",")] == ["PG_EMITTER_POINT=0", "PG_EMITTER_SPOT=1", "PG_EMITTER_DIRECTIONAL=2"]
    assert (pg.capi.PG_EMITTER_POINT, pg.capi.PG_EMITTER_SPOT, pg.capi.PG_EMITTER_DIRECTIONAL) == (0, 1, 2)
    names = [s[0] for s in pg.capi.SIGNATURES]
    assert "pg_set_delta_emitters" in names and "pg_emitter_query" in names


def test_xml_round_trip(pg, tmp_path):
    X = pg.mitsuba_xml
    sc = X.load(SCENE.format(emitters=POINT + SPOT + DIRECTIONAL)).scene
    p, s, d = sc.delta_emitters
    assert fields(p)[:2] == (0, (0.25, 2.0, -1.5)) and tuple(p.intensity) == (3.0, 2.0, 1.0)
    assert s.type == 1 and tuple(s.position) == (1.0, 3.0, -2.0) and tuple(s.intensity) == (10.0, 10.0, 8.0)
    axis = np.array([-1.0, -3.0, 2.0]) / np.sqrt(14.0)
    assert np.abs(np.array(tuple(s.direction)) - axis).max() < 1e-6
    assert s.cutoff_angle == np.float32(np.deg2rad(25.0)) and s.beam_width == np.float32(np.deg2rad(10.0))
    assert d.type == 2 and tuple(d.direction) == (0.5, -1.0, 0.25) and tuple(d.intensity) == (1.5, 1.25, 1.0)
    path = X.save(sc, str(tmp_path / "lights.xml"), spp=4)
    text = open(path).read()
    assert all(f'<emitter type="{t}">' in text for t in ("point", "spot", "directional"))
    back = X.load(path).scene
    assert [fields(e) for e in back.delta_emitters] == [fields(e) for e in sc.delta_emitters]
    again = X.load(X.save(back, str(tmp_path / "lights2.xml"), spp=4)).scene  # the saved file is a fixed point
    assert [fields(e) for e in again.delta_emitters] == [fields(e) for e in sc.delta_emitters]
    assert X.load(SCENE.format(emitters="")).scene.delta_emitters == []


def test_xml_defaults_and_transforms(pg):
    X = pg.mitsuba_xml
    spot = '<emitter type="spot"><rgb name="intensity" value="1"/></emitter>'
    s, = X.load(SCENE.format(emitters=spot)).scene.delta_emitters
    assert tuple(s.direction) == (0.0, 0.0, 1.0) and tuple(s.position) == (0.0, 0.0, 0.0)
    assert s.cutoff_angle == np.float32(np.deg2rad(20.0)) and s.beam_width == np.float32(np.deg2rad(15.0))  # spot.cpp:70-71
    point = ('<emitter type="point"><rgb name="intensity" value="2"/><transform name="toWorld">'
             '<translate x="1" y="2" z="3"/></transform></emitter>')
    p, = X.load(SCENE.format(emitters=point)).scene.delta_emitters
    assert tuple(p.position) == (1.0, 2.0, 3.0) and tuple(p.intensity) == (2.0, 2.0, 2.0)
    direc = ('<emitter type="directional"><rgb name="irradiance" value="1"/><transform name="toWorld">'
             '<rotate x="1" angle="90"/></transform></emitter>')
    d, = X.load(SCENE.format(emitters=direc)).scene.delta_emitters
    assert np.abs(np.array(tuple(d.direction)) - [0, -1, 0]).max() < 1e-6  # toWorld * +z
    both = ('<emitter type="directional"><rgb name="irradiance" value="1"/><vector name="direction" x="0" y="-1" z="0"/>'
            '<transform name="toWorld"><rotate x="1" angle="90"/></transform></emitter>')
    with pytest.raises(ValueError, match="direction"):
        X.load(SCENE.format(emitters=both))


@pytest.mark.parametrize("xml, name", [
    ('<emitter type="spot"><rgb name="intensity" value="1"/><texture type="checkerboard" name="texture"/></emitter>', "texture"),
    ('<emitter type="point"><rgb name="intensity" value="1"/><float name="samplingWeight" value="2"/></emitter>', "samplingWeight"),
    ('<emitter type="point"/>', "intensity"),
    ('<emitter type="spot"/>', "intensity"),
    ('<emitter type="directional"/>', "irradiance"),
])
def test_xml_rejects_what_is_not_restated(pg, xml, name):
    with pytest.raises(NotImplementedError, match=name):
        pg.mitsuba_xml.load(SCENE.format(emitters=xml))


def test_scene_helpers(pg):
    S = pg.scenes
    s = S.Scene()
    assert s.add_point_light((1, 2, 3), 4.0) == 0
    assert s.add_spot_light((0, 5, 0), (0, 0, 0), (1, 2, 3)) == 1
    assert s.add_directional_light((0, -2, 0), 1.0) == 2
    p, sp, d = s.delta_emitters
    assert tuple(p.intensity) == (4.0, 4.0, 4.0)
    assert tuple(sp.direction) == (0.0, -5.0, 0.0)  # normalised on upload
    assert sp.cutoff_angle == np.float32(np.deg2rad(20)) and sp.beam_width == np.float32(np.deg2rad(15))
    assert tuple(d.direction) == (0.0, -2.0, 0.0)
    for bad in (lambda: s.add_spot_light((0, 0, 0), (0, 0, 1), 1.0, cutoff_angle=20, beam_width=20),
                lambda: s.add_spot_light((0, 0, 0), (0, 0, 0), 1.0), lambda: s.add_point_light((0, 0, 0), -1.0),
                lambda: s.add_directional_light((0, 0, 0), 1.0)):
        with pytest.raises(ValueError):
            bad()
    assert len(s.delta_emitters) == 3


def test_adapter_passes_the_delta_emitters():
    """the Mitsuba adapter, textually (it is not compiled here): it flattens the three emitter classes and sets them
    after the upload"""
    src = open(os.path.join(ROOT, "mitsuba_plugin", "guided_gpu.h")).read()
    pre = src[src.index("bool preprocess("):src.index("bool render(") if "bool render(" in src else len(src)]
    assert pre.index("pg_upload_scene(") < pre.index("pg_set_delta_emitters(")
    flat = src[src.index("inline void GuidedGPUIntegrator::flattenDeltaEmitters"):]
    flat = flat[:flat.index("\n}\n")]
    for cls, typ in (("PointEmitter", "PG_EMITTER_POINT"), ("SpotEmitter", "PG_EMITTER_SPOT"),
                     ("DirectionalEmitter", "PG_EMITTER_DIRECTIONAL")):
        assert f'cls == "{cls}"' in flat and typ in flat
    assert "getSamplingWeight() != 1" in flat and 'hasProperty("texture")' in flat and "isOnSurface()" in flat
    assert "flattenDeltaEmitters(scene, f);" in src


def test_shadow_cases_are_usable(pg):
    """the GPU shadow tests' scenes, from the restatement alone: at most 5 % of the pixels have a sample within 1e-3
    of the shadow's edge, there is an umbra to check, and in the "wide" case the quad blocks more than 60 % of the
    shadow rays (the blocker list needs half of them on its triangles)"""
    import test_gpu_delta_emitters as G
    for case in G.SHADOWS:
        want, keep, umbra, near_edge, blocked = G.shadow_reference(G.shadow_scene(pg, case), case)
        assert near_edge.mean() <= 0.05 and umbra.sum() > 20 and keep.mean() > 0.8, (case, near_edge.mean())
        assert not want[umbra].any() and want[keep].max() > 0.1
        assert (~umbra & keep).mean() > 0.1  # lit pixels too
        if case == "wide":
            assert blocked > 0.6, blocked


def test_closed_form_cases_are_usable(pg):
    """every camera ray of the plane scenes hits the plane; the spot's cone and beam edges both cross the image"""
    import test_gpu_delta_emitters as G
    for name, light in G.LIGHTS.items():
        want, _ = G.closed_form(G.plane_scene(pg, light))
        assert want.max() > 0.05 and np.isfinite(want).all()
        if name == "spot":
            point = G.closed_form(G.plane_scene(pg, lambda s: s.add_point_light((0.0, 3.0, 0.5), (40.0, 40.0, 30.0))))[0]
            dark, full = (want.max(2) == 0), np.isclose(want, point, rtol=1e-12).all(2) & (want.max(2) > 0)
            assert dark.mean() > 0.1 and full.mean() > 0.02 and (~dark & ~full).mean() > 0.02


# ---- the restatement against hand values ----------------------------------------------------------------------------
BOX = np.float32([[-1, -1, -1], [1, 1, 1]])  # a box with half diagonal sqrt(3): the sphere's radius is 1.1 sqrt(3)


def rec(pg, e):
    return ER.records([e], BOX)[0]


def test_point_at_distance_two_is_a_quarter(pg):
    r = rec(pg, pg.scenes.point_light((0, 2, 0), (4, 2, 1)))
    d, dist, value, ok = ER.sample_delta(r, [[0, 0, 0]])
    assert ok[0] and dist[0] == 2.0 and tuple(d[0]) == (0, 1, 0) and tuple(value[0]) == (1.0, 0.5, 0.25)


def test_spot_falloff(pg):
    S = pg.scenes
    spot = rec(pg, S.spot_light((0, 2, 0), (0, 0, 0), 8.0, cutoff_angle=20, beam_width=10))
    point = rec(pg, S.point_light((0, 2, 0), 8.0))
    at = lambda deg: [[2 * np.tan(np.deg2rad(deg)), 0, 0]]  # the point of the plane y = 0 at `deg` from the axis
    for deg in (0.0, 5.0, 9.9):  # inside the beam: the point light
        assert np.array_equal(ER.sample_delta(spot, at(deg))[2], ER.sample_delta(point, at(deg))[2])
    half = ER.sample_delta(spot, at(15.0))[2] / ER.sample_delta(point, at(15.0))[2]
    assert np.abs(half - 0.5).max() < 1e-6  # halfway through the ramp (float32 angles: 1e-7)
    for deg in (20.001, 25.0, 80.0):  # at or beyond the cutoff: nothing, and the sample counts as failed
        d, dist, value, ok = ER.sample_delta(spot, at(deg))
        assert not ok[0] and not value.any()
    edge = dict(spot, cos_cutoff=float(np.cos(np.deg2rad(20.0))))
    x = np.float64(2 * np.tan(np.deg2rad(20.0)))
    cos_theta = 2 / np.hypot(2, x)
    edge["cos_cutoff"] = cos_theta  # exactly on the cone: cosTheta <= cosCutoff
    assert not ER.sample_delta(edge, [[x, 0, 0]])[3][0]


def test_directional(pg):
    r = rec(pg, pg.scenes.directional_light((0, -3, 0), (2, 1, 0.5)))
    radius = np.float32(np.sqrt(np.float32(3))) * np.float32(1.1)
    assert np.allclose(r["pos"], [0, radius, 0], atol=0, rtol=1e-7)
    d, dist, value, ok = ER.sample_delta(r, [[0.3, 0.5, -0.2], [5, float(radius) + 1, 0]])
    assert ok[0] and tuple(d[0]) == (0, 1, 0) and abs(dist[0] - (float(radius) - 0.5)) < 1e-12
    assert tuple(value[0]) == (2.0, 1.0, 0.5)  # the irradiance, whatever the distance
    assert not ok[1] and not value[1].any()  # behind the disk


def test_pick_order_and_measure(pg):
    """area emitters first, then the delta emitters in their order; value / pdf has 1 / ne divided out"""
    S = pg.scenes
    sc = S.cornell(8, 8)
    sc.add_point_light((2.78, 2.0, 2.8), 5.0)
    deltas = ER.records(sc.delta_emitters, sc.positions)
    area = [ER.area_emitter(sc, 0)]
    ref = np.float32([[1, 1, 1], [1, 1, 1]])
    ei, out = ER.sample_emitter(area, deltas, ref, np.float32([[0.25, 0.5], [0.75, 0.5]]))
    assert tuple(ei) == (0, 1) and tuple(out[:, 7]) == (1.0, 2.0)
    dist = np.linalg.norm(np.float64([2.78, 2.0, 2.8]) - 1)
    assert np.allclose(out[1, 4:7], 2 * 5.0 / dist ** 2, rtol=1e-6)
    p = 1 + out[0, :3] * out[0, 3]  # the sampled point lies on the ceiling panel
    assert abs(p[1] - 5.487) < 1e-5 and 2.13 <= p[0] <= 3.43 and 2.27 <= p[2] <= 3.32
