"""The homogeneous medium without a GPU: the ctypes mirror against the header, the numpy restatement
(tests/medium_ref.py) against closed forms, and the Mitsuba XML subset (mitsuba_xml.load / save)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import medium_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pg_capi.h")

SCENE = """<scene version="0.5.0">
<sensor type="perspective">
  <float name="fov" value="40"/>
  <transform name="toWorld"><lookat origin="0, 0, -4" target="0, 0, 0" up="0, 1, 0"/></transform>
  <film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/></film>
</sensor>
{medium}
<shape type="cube"><ref name="interior" id="fog"/></shape>
<shape type="rectangle"><transform name="toWorld"><translate z="3"/></transform>
  <emitter type="area"><rgb name="radiance" value="1"/></emitter></shape>
</scene>"""
CHROMATIC = ('<medium type="homogeneous" id="fog"><rgb name="sigmaA" value="0.25, 0.5, 1"/>'
             '<rgb name="sigmaS" value="1, 2, 4"/><float name="scale" value="2"/>{extra}'
             '<phase type="hg"><float name="g" value="0.25"/></phase></medium>')
GREY = ('<medium type="homogeneous" id="fog"><rgb name="sigmaT" value="2, 2, 2"/><rgb name="albedo" value="0.5, 0.25, 0.75"/>'
        '{extra}</medium>')


def record(h):
    return (h.medium, tuple(h.sigma_a), tuple(h.sigma_s), h.g, h.medium_sampling_weight)


def test_struct_matches_the_header(pg):
    """sizeof / offsetof of pg_homogeneous_medium from a gcc probe against the ctypes mirror"""
    T = pg.capi.pg_homogeneous_medium
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(pg_homogeneous_medium));']
    for f, _ in T._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(pg_homogeneous_medium, {f}));')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-o", exe, src])
        got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(T) == 40
    for f, _ in T._fields_:
        assert int(got[f]) == getattr(T, f).offset, f
    names = [s[0] for s in pg.capi.SIGNATURES]
    assert "pg_set_homogeneous_media" in names and "pg_homogeneous_query" in names


@pytest.mark.parametrize("weight", [0.5, 1.0, -1.0])
@pytest.mark.parametrize("dist", [0.1, 1.0, 10.0])
def test_reference_pdfs_integrate_to_one(weight, dist):
    """the quadrature of pdfSuccess over [0, dist] plus pdfFailure(dist) is 1"""
    st = np.array([0.5, 2.0, 6.0])
    w = MR.sampling_weight(0.1 * st, 0.9 * st, weight)
    x, gw = np.polynomial.legendre.leggauss(64)
    total = 0.0
    edges = np.linspace(0.0, dist, 17)  # composite Gauss-Legendre: exp(-60) .. 1 over the longest interval
    for a, b in zip(edges[:-1], edges[1:]):
        s = 0.5 * (b - a) * x + 0.5 * (a + b)
        total += 0.5 * (b - a) * (gw * MR.pdfs(st, w, s)[0]).sum()
    total += MR.pdfs(st, w, np.array(dist))[1]
    assert abs(total - 1) < 1e-6, total


def test_reference_default_weight():
    st = np.array([0.5, 2.0, 6.0], np.float32)
    assert MR.sampling_weight(st, 0 * st) == 0  # a pure absorber never scatters
    assert MR.sampling_weight(np.float32(0.7) * st, np.float32(0.3) * st) == np.float32(0.5)
    assert abs(MR.sampling_weight(np.float32(0.1) * st, np.float32(0.9) * st) - 0.9) < 1e-6
    assert MR.sampling_weight(st, st, 0.25) == np.float32(0.25)  # a given weight is kept
    # a channel with sigma_t = 0 takes no part in the maximum
    assert abs(MR.sampling_weight([0, 0.2, 0], [0, 0.8, 0]) - 0.8) < 1e-6


def test_reference_sample_distance_by_hand():
    """one ray by hand: weight 1, the channel and the distance from the two draws"""
    st = np.array([0.5, 2.0, 6.0], np.float32)
    keys = np.array([[12345, 7]], np.uint32)
    rays = np.array([[0, 0, 0, 0.25, 0, 0, 1, 100.0]], np.float32)
    u0, u1 = float(MR.next1(keys, 1)[0]), float(MR.next1(keys, 2)[0])
    out = MR.sample_distance(st, 1.0, rays, keys)[0]
    ch = min(int(u1 * 3), 2)
    s = -np.log(1 - u0) / st[ch]
    assert out[0] == 1 and out[7] == 2 and abs(out[1] - (s + 0.25)) < 1e-5 * (s + 0.25)
    e = np.exp(-st.astype(np.float64) * s)
    assert np.allclose(out[2:5], e, rtol=1e-5)
    assert np.allclose(out[5:7], [(st * e).mean(), e.mean()], rtol=1e-5)
    # weight 0: no medium interaction, one draw, the whole segment's transmittance, pdfFailure 1
    rays[0, 7] = 1.25
    out = MR.sample_distance(st, 0.0, rays, keys)[0]
    assert out[0] == 0 and out[7] == 1 and out[1] == 1.25 and out[6] == 1 and out[5] == 0
    assert np.allclose(out[2:5], np.exp(-st), rtol=1e-6)
    assert np.array_equal(MR.eval_transmittance([0.0, 2.0, 6.0], rays)[0, 0], np.float32(1.0))


def test_xml_chromatic_medium(pg):
    X = pg.mitsuba_xml
    sc = X.load(SCENE.format(medium=CHROMATIC.format(extra=""))).scene
    h, = sc.homogeneous_media
    # scale applies to both coefficients; no `g` property on the medium, so sigma_s is not reduced
    assert record(h) == (0, (0.5, 1.0, 2.0), (2.0, 4.0, 8.0), 0.25, -1.0)
    assert len(sc.media) == 1 and tuple(sc.media[0].res) == (2, 2, 2)  # the placeholder entry
    assert sc.shapes[0].interior_medium == 0
    w = SCENE.format(medium=CHROMATIC.format(extra='<float name="mediumSamplingWeight" value="0.75"/>'))
    assert X.load(w).scene.homogeneous_media[0].medium_sampling_weight == 0.75
    with pytest.raises(NotImplementedError, match="single"):
        X.load(SCENE.format(medium=CHROMATIC.format(extra='<string name="strategy" value="single"/>')))
    X.load(SCENE.format(medium=CHROMATIC.format(extra='<string name="strategy" value="balance"/>')))


def test_xml_grey_medium_keeps_the_grid_by_default(pg):
    X = pg.mitsuba_xml
    text = SCENE.format(medium=GREY.format(extra=""))
    sc = X.load(text).scene
    assert sc.homogeneous_media == [] and len(sc.media) == 1
    m = sc.media[0]
    assert tuple(m.res) == (2, 2, 2) and m.scale == 2.0 and tuple(m.albedo) == (0.5, 0.25, 0.75)
    sc = X.load(text, analytic_media=True).scene
    h, = sc.homogeneous_media
    assert record(h) == (0, (1.0, 1.5, 0.5), (1.0, 0.5, 1.5), 0.0, -1.0)
    assert len(sc.media) == 1 and sc.shapes[0].interior_medium == 0


def test_xml_round_trip(pg, tmp_path):
    X = pg.mitsuba_xml
    extra = '<float name="mediumSamplingWeight" value="0.625"/>'
    sc = X.load(SCENE.format(medium=CHROMATIC.format(extra=extra))).scene
    path = X.save(sc, str(tmp_path / "fog.xml"), spp=4, integrator="volpath")
    text = open(path).read()
    assert '<medium type="homogeneous"' in text and '<phase type="hg">' in text
    back = X.load(path).scene
    assert [record(h) for h in back.homogeneous_media] == [record(h) for h in sc.homogeneous_media]
    assert [(s.interior_medium, s.exterior_medium) for s in back.shapes] == \
           [(s.interior_medium, s.exterior_medium) for s in sc.shapes]
    assert np.array_equal(back.positions[back.indices], sc.positions[sc.indices])  # the same triangles
    again = X.load(X.save(back, str(tmp_path / "fog2.xml"), spp=4, integrator="volpath")).scene
    assert [record(h) for h in again.homogeneous_media] == [record(h) for h in sc.homogeneous_media]


def test_scene_builder_rules(pg):
    S = pg.scenes
    s = S.Scene()
    a = s.add_homogeneous_medium(sigma_t=(1.0, 2.0, 4.0), albedo=(0.5, 0.5, 0.25), g=0.3)
    b = s.add_homogeneous_medium(sigma_a=0.5, sigma_s=(1.0, 2.0, 3.0), medium_sampling_weight=0.75)
    assert (a, b) == (0, 1) and len(s.media) == 2
    assert record(s.homogeneous_media[0]) == (0, (0.5, 1.0, 3.0), (0.5, 1.0, 1.0), np.float32(0.3), -1.0)
    assert record(s.homogeneous_media[1]) == (1, (0.5, 0.5, 0.5), (1.0, 2.0, 3.0), 0.0, 0.75)
    with pytest.raises(ValueError):  # either pair, never a mix (materials.h:104-106)
        s.add_homogeneous_medium(sigma_a=1.0, albedo=0.5)
    with pytest.raises(ValueError):
        s.add_homogeneous_medium()
