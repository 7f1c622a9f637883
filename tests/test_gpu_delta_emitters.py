"""Point, spot and directional emitters (pg_set_delta_emitters / pg_emitter_query) on the GPU.

The oracle does not know these emitters, so the yardsticks are the numpy float64 restatement (tests/emitter_ref.py)
and closed forms: the direct light of one delta emitter on a diffuse plane is rho / pi * cos(theta) * value(x) at
every camera sample's plane point, and the camera rays are bit-exact already (camera_ref.pinhole_rays)."""
import ctypes as C

import numpy as np
import pytest

import camera_ref as CR
import emitter_ref as ER

pytestmark = pytest.mark.gpu

SEED = 1337  # pg_config_default
W, H, SPP = 64, 48, 16
RHO = np.float64([0.5, 0.6, 0.7])
UNFUSED = ("PG_NO_RAYS_FUSION", "PG_NO_SHADE_FUSION")


def make_dev(pg, scene, **cfg):
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(**cfg))
    d.upload(scene)
    return d


def render(pg, scene, spp=SPP, **cfg):
    d = make_dev(pg, scene, **cfg)
    d.render_pass(spp, 0)
    rgbw, sq = d.read_film()
    st = d.stats()
    d.close()
    return rgbw, sq, st


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1: unit parity -------------------------------------------------------------------------------------------------
def cornell_lights(pg, area=True, w=W, h=H):
    """the Cornell box with one light of each delta kind: a point light under the ceiling, the issue's spot (cutoff
    20, beam 15 degrees) over the short block and a directional light tilted 10 degrees off straight down"""
    sc = pg.scenes.cornell(w, h, area_light=area)
    sc.add_point_light((1.2, 4.6, 2.0), (30.0, 24.0, 18.0))
    sc.add_spot_light((4.2, 5.2, 1.0), (1.9, 0.0, 1.7), (90.0, 90.0, 70.0), cutoff_angle=20, beam_width=15)
    sc.add_directional_light((np.sin(np.deg2rad(10.0)), -np.cos(np.deg2rad(10.0)), 0.05), (2.0, 1.8, 1.5))
    return sc


def test_emitter_query_matches_the_restatement(pg):
    """4096 points in the Cornell box against tests/emitter_ref.py.  Bounds (issue): d 2^-20, dist 2^-20 relative,
    value 1e-5 I / dist^2 (delta; the irradiance for the directional light).  The area branch, the code every scene
    has run so far, is held to 1e-5 relative, derived as the spot's bound is: value = radiance |cos| / (inv_area
    dist^2), a dozen float32 operations (1e-6 relative), plus the cancellation in cos = dot(d, n), whose absolute error
    of about 2e-7 (three products of components <= 1, two sums) is divided by cos itself; the reference points keep
    0.02 of the box's extent from its walls, 0.11 below the panel, so over the box's 5.6 the cosine stays above 0.02:
    1e-5 relative, and the reused triangle sample (sy - cdf) / 0.5 moves the point by 2.4e-7 of an edge at most.
    Measured on an MI355X (profiles/r14_delta_emitters/README.md): d within 1.8e-7, dist 2.0e-7 relative; value:
    point 2.8e-7, spot 6.2e-6, directional 0 (of I / dist^2), area 5.9e-7 relative."""
    sc = cornell_lights(pg)
    rng = np.random.default_rng(7)
    lo, hi = sc.bounds()
    ref = (lo + (hi - lo) * (0.02 + 0.96 * rng.random((4096, 3)))).astype(np.float32)
    smp = rng.random((4096, 2)).astype(np.float32)
    d = make_dev(pg, sc)
    got = d.emitter_query(ref, smp).astype(np.float64)
    assert same_bits(d.emitter_query(ref, smp), got.astype(np.float32))
    d.close()
    deltas = ER.records(sc.delta_emitters, sc.positions)
    ei, want = ER.sample_emitter([ER.area_emitter(sc, 0)], deltas, ref, smp)
    assert set(ei.tolist()) == {0, 1, 2, 3}
    assert np.array_equal(got[:, 7], want[:, 7]), np.argwhere(got[:, 7] != want[:, 7])[:8]
    for e in range(4):
        m = (ei == e) & (want[:, 7] != 0)
        assert m.sum() > 100
        ed = np.abs(got[m, :3] - want[m, :3]).max()
        edist = np.abs(got[m, 3] / want[m, 3] - 1).max()
        if e == 0:
            ev = np.abs(got[m, 4:7] / np.maximum(want[m, 4:7], 1e-300) - 1).max()
            bound_v = 1e-5
        else:
            r = deltas[e - 1]
            scale = r["intensity"].max() * (1.0 if r["type"] == ER.DIRECTIONAL else 1 / want[m, 3] ** 2)
            ev = (np.abs(got[m, 4:7] - want[m, 4:7]).max(1) / 4 / scale).max()  # value / pdf = 4 value: ne = 4
            bound_v = 1e-5
        print(f"emitter {e}: {m.sum()} samples, |dd|inf {ed:.3e} dist rel {edist:.3e} (bound {2.0 ** -20:.3e}), "
              f"value {ev:.3e} (bound {bound_v:.0e})")
        assert ed <= 2.0 ** -20 and edist <= 2.0 ** -20 and ev <= bound_v
    failed = want[:, 7] == 0
    assert failed.sum() > 100 and not got[failed, :7].any()  # outside the spot's cone, behind the area light


# ---- 2: closed-form direct light ------------------------------------------------------------------------------------
def plane_scene(pg, light):
    """a 100 x 100 diffuse plane y = 0 facing +y, seen from (0, 3, -4); `light(scene)` adds the one emitter"""
    S = pg.scenes
    s = S.Scene()
    V, F = S.quad((-50, 0, -50), (-50, 0, 50), (50, 0, 50), (50, 0, -50), facing=(0, 1, 0))
    s.add_mesh(V, F, material=s.add_material(S.material("diffuse", reflectance=tuple(RHO))))
    s.set_camera((0, 3, -4), (0, 0, 0.5), (0, 1, 0), 50.0, W, H)
    light(s)
    return s.finalize()


LIGHTS = {
    "point": lambda s: s.add_point_light((0.5, 2.0, 0.5), (8.0, 6.0, 4.0)),
    # the cone (40 degrees: radius 2.5 on the plane) and the beam (25 degrees: 1.4) both cross the image
    "spot": lambda s: s.add_spot_light((0.0, 3.0, 0.5), (0.3, 0.0, 0.8), (40.0, 40.0, 30.0), cutoff_angle=40, beam_width=25),
    "directional": lambda s: s.add_directional_light((np.sin(np.deg2rad(30.0)), -np.cos(np.deg2rad(30.0)), 0.0), (2.0, 1.5, 1.0)),
    # the scene's only emitter, off to the side: no emitter triangles, an empty CDF, no doom box
    "only": lambda s: s.add_point_light((-1.5, 0.75, 1.5), (3.0, 3.0, 3.0)),
}


def closed_form(sc, occluder=None, spp=SPP, attenuation=None):
    """per pixel, the mean over the spp samples of rho / pi * cos(theta) * value(x) at the pinhole ray's plane point;
    occluder(x, light position) -> True where the segment is blocked (n); attenuation(camera origins, x, light
    position) -> a factor per sample (n); also returns the plane points"""
    SPP = spp
    pix = np.repeat(np.arange(W * H, dtype=np.uint32), SPP)
    smp = np.tile(np.arange(SPP, dtype=np.uint32), W * H)
    ro, rd = CR.pinhole_rays(sc.camera, pix, smp, SEED)
    o, dr = ro[:, :3].astype(np.float64), rd[:, :3].astype(np.float64)
    t = -o[:, 1] / dr[:, 1]
    assert (dr[:, 1] < 0).all()  # every camera ray hits the plane
    x = o + dr * t[:, None]
    assert np.abs(x[:, [0, 2]]).max() < 50
    rec, = ER.records(sc.delta_emitters, sc.positions)
    d, dist, value, ok = ER.sample_delta(rec, x)
    L = RHO[None, :] / np.pi * np.maximum(d[:, 1], 0)[:, None] * value
    if occluder is not None:
        L = np.where(occluder(x, rec["pos"])[:, None], 0.0, L)
    if attenuation is not None:
        L = L * attenuation(o, x, rec["pos"])[:, None]
    return L.reshape(H, W, SPP, 3).mean(2), x.reshape(H, W, SPP, 3)


@pytest.fixture(scope="module", params=list(LIGHTS))
def plane(request, pg):
    sc = plane_scene(pg, LIGHTS[request.param])
    want, _ = closed_form(sc)
    want.setflags(write=False)
    return request.param, sc, want


def check_image(name, rgbw, want):
    assert (rgbw[..., 3] == SPP).all()
    got = rgbw[..., :3].astype(np.float64) / SPP
    err = np.abs(got - want).max() / want.max()
    print(f"{name}: max |pixel - closed form| / image max = {err:.3e} (bound 1e-3), image max {want.max():.4f}")
    assert want.max() > 0.05 and err <= 1e-3
    return err


def test_direct_light_surface_tracer(pg, plane, monkeypatch):
    """The wavefront, k_tail and the unfused launches give one film, bit for bit.  Measured on an MI355X
    (profiles/r14_delta_emitters/README.md), max error / image max against the bound 1e-3: point 1.3e-6, spot 3.1e-6,
    directional 1.9e-7, point as the only emitter 2.9e-6; the volumetric tracer the same."""
    name, sc, want = plane
    wave, _, st = render(pg, sc, max_depth=2, tail_paths=-1)
    tail, _, st_tail = render(pg, sc, max_depth=2, tail_paths=1 << 30)
    for k in UNFUSED:
        monkeypatch.setenv(k, "1")
    unfused, _, _ = render(pg, sc, max_depth=2, tail_paths=-1)
    for k in UNFUSED:
        monkeypatch.delenv(k)
    check_image(f"{name} wavefront", wave, want)
    assert st["tail_launches"] == 0 and st_tail["tail_launches"] > 0
    assert same_bits(wave, tail) and same_bits(wave, unfused)
    assert st["shadow_rays"] > 0
    if name == "spot":  # both edges are in the image: dark pixels outside the cone, the point light's value inside
        assert (want.max(2) == 0).mean() > 0.1
    if name == "only":  # no emitter box: every doomed ray is probed
        assert st["probes"] > 0


def test_direct_light_volumetric_tracer(pg, plane):
    name, sc, want = plane
    vol, _, _ = render(pg, sc, max_depth=2, integrator=pg.capi.PG_INTEGRATOR_VOLPATH)
    check_image(f"{name} volpath", vol, want)


# ---- 3: shadow ------------------------------------------------------------------------------------------------------
# (light position, the occluding quad's height and its x0, x1, z0, z1).  "half": the quad halfway between the light and
# the plane.  "wide": a quad high above the camera's view whose shadow covers most of the image, so that more than half
# of the shadow rays end on its two triangles and the recording passes list them as shadow blockers.
SHADOWS = {"half": ((0.5, 2.0, 0.5), 1.0, (-0.1, 0.9, 0.1, 1.1)),
           "wide": ((0.5, 6.0, 0.5), 4.0, (-1.5, 1.0, -0.5, 1.5))}


def shadow_scene(pg, case="half"):
    S = pg.scenes
    lp, qy, (x0, x1, z0, z1) = SHADOWS[case]

    def light(s):
        V, F = S.quad((x0, qy, z0), (x0, qy, z1), (x1, qy, z1), (x1, qy, z0), facing=(0, 1, 0))
        s.add_mesh(V, F, material=s.add_material(S.material("diffuse", reflectance=(0, 0, 0))))
        s.add_point_light(lp, tuple(v * (lp[1] / 2.0) ** 2 for v in (8.0, 6.0, 4.0)))
    return plane_scene(pg, light)


def shadow_reference(sc, case="half"):
    """closed form with the quad's occlusion; the pixels to compare (no sample within 1e-3 of the shadow's edge and
    no camera ray through the quad itself), the umbra pixels, the pixels near the edge and the share of the samples
    whose shadow ray the quad blocks"""
    lp, qy, (x0, x1, z0, z1) = SHADOWS[case]

    def margin(x, to):  # > 0: the segment from the plane point x to `to` crosses y = qy inside the quad
        s = (qy - x[:, 1]) / (to[1] - x[:, 1])
        q = x + (to - x) * s[:, None]
        m = np.minimum(np.minimum(q[:, 0] - x0, x1 - q[:, 0]), np.minimum(q[:, 2] - z0, z1 - q[:, 2]))
        return np.where((s > 0) & (s < 1), m, -np.inf)  # the quad is not between the two points

    want, x = closed_form(sc, lambda x, lp: margin(x, lp) > 0)
    rec, = ER.records(sc.delta_emitters, sc.positions)
    m = margin(x.reshape(-1, 3), rec["pos"]).reshape(H, W, SPP)
    # a plane point that moves by 1e-3 moves its segment's crossing of the quad's plane by (1 - qy / light height) of it
    eps = 1e-3 * (1 - qy / lp[1])
    near_edge = (np.abs(m) < eps).any(2)
    cam = np.float64(list(sc.camera.origin))
    sees_quad = (margin(x.reshape(-1, 3), cam).reshape(H, W, SPP) > -1e-3).any(2)
    umbra = (m > eps).all(2) & ~sees_quad
    return want, ~near_edge & ~sees_quad, umbra, near_edge, float((m > 0).mean())


def check_shadow(name, rgbw, ref):
    want, keep, umbra = ref[:3]
    got = rgbw[..., :3].astype(np.float64) / SPP
    err = np.abs(got - want)[keep].max() / want.max()
    print(f"shadow {name}: {keep.mean():.3f} of the pixels compared, max error / image max {err:.3e} (bound 1e-3)")
    assert err <= 1e-3
    assert not got[umbra].any()


def test_point_light_shadow(pg):
    """Measured on an MI355X (profiles/r14_delta_emitters/README.md): 1.5e-6 of the image maximum over the 96.3 % of
    the pixels away from the shadow's edge, on all three variants."""
    sc = shadow_scene(pg)
    ref = shadow_reference(sc)
    for name, cfg in (("wavefront", dict(tail_paths=-1)), ("tail", dict(tail_paths=1 << 30)),
                      ("volpath", dict(integrator=pg.capi.PG_INTEGRATOR_VOLPATH))):
        rgbw, _, _ = render(pg, sc, max_depth=2, **cfg)
        check_shadow(name, rgbw, ref)


@pytest.mark.parametrize("tail", [-1, 1 << 30], ids=["wavefront", "tail"])
def test_point_light_shadow_with_a_live_blocker_list(pg, monkeypatch, tail):
    """After two recording passes the occluding quad's triangles are the shadow-blocker list; the shaders then
    resolve a delta emitter's shadow rays against it (pg_stats), and the film is the closed form's and, bit for bit,
    the one rendered with PG_NO_SHADOW_CULL=1.  Measured on an MI355X: 36182 of 49152 shadow rays resolved, 5.4e-7
    of the image maximum from the closed form."""
    sc = shadow_scene(pg, "wide")
    ref = shadow_reference(sc, "wide")
    d = make_dev(pg, sc, max_depth=2, guiding=1, tail_paths=tail)
    for k in range(2):
        d.render_pass(SPP, SPP * k, record=True)
    ids, orig = d.blockers()
    quad_tris = {2, 3}  # the scene's triangles: the plane's two, then the quad's two
    assert set(orig.tolist()) == quad_tris, (ids, orig)
    d.reset_film()
    before = d.stats()["shadow_culled"]
    d.render_pass(SPP, 0)
    live, _ = d.read_film()
    culled = d.stats()["shadow_culled"] - before
    print(f"blocker list {orig.tolist()}: {culled} of {W * H * SPP} shadow rays resolved in the shader")
    assert culled > 0.4 * W * H * SPP  # the restatement has > 60 % of them blocked; the margins leave out a few
    monkeypatch.setenv("PG_NO_SHADOW_CULL", "1")
    d.reset_film()
    before = d.stats()["shadow_culled"]
    d.render_pass(SPP, 0)
    plain, _ = d.read_film()
    assert d.stats()["shadow_culled"] == before
    monkeypatch.delenv("PG_NO_SHADOW_CULL")
    d.close()
    assert same_bits(live, plain)
    check_shadow(f"live blocker list ({'tail' if tail > 0 else 'wavefront'})", live, ref)


# ---- 4: emitter pick and MIS are linear -----------------------------------------------------------------------------
def z_scores(films, sign):
    """per pixel and channel z of sum_k sign_k mean_k from the films' sums and sums of squares"""
    total, var = 0.0, 0.0
    for (rgbw, sq), s in zip(films, sign):
        n = rgbw[..., 3:4].astype(np.float64)
        mean = rgbw[..., :3] / n
        total = total + s * mean
        var = var + np.maximum(sq[..., :3] / n - mean * mean, 0) / n
    ok = var > 0
    assert (np.abs(total[~ok]) < 1e-6).all()
    return total, var, ok


def check_linear(name, films):
    total, var, ok = z_scores(films, (1, -1, -1))
    z = np.abs(total[ok]) / np.sqrt(var[ok])
    zmean = abs(total.mean()) / np.sqrt(var.sum()) * total.size
    print(f"{name}: |z| < 5 for {(z < 5).mean():.5f} of {z.size} values, max {z.max():.2f}; z of the image mean {zmean:.2f}")
    assert (z < 5).mean() >= 0.999 and zmean < 4.5


def test_area_plus_point_is_their_sum(pg):
    S = pg.scenes
    light = lambda s: s.add_point_light((1.2, 4.6, 2.0), (30.0, 24.0, 18.0))
    a = S.cornell(W, H)
    b = S.cornell(W, H, area_light=False)
    light(b)
    c = S.cornell(W, H)
    light(c)
    films = [render(pg, sc, max_depth=4, seed=seed)[:2] for sc, seed in ((c, 11), (a, 12), (b, 13))]
    check_linear("area + point", films)
    assert films[2][0][..., :3].max() > 0  # the point light alone lights the box


def test_area_plus_point_plus_envmap_is_their_sum(pg):
    S = pg.scenes
    env = np.full((8, 16, 3), 0.4, np.float32)
    light = lambda s: s.add_point_light((1.2, 4.6, 2.0), (30.0, 24.0, 18.0))
    a = S.cornell(W, H)
    a.set_envmap(env)
    a.finalize()
    b = S.cornell(W, H, area_light=False)
    light(b)
    c = S.cornell(W, H)
    c.set_envmap(env)
    c.finalize()
    light(c)
    films = [render(pg, sc, max_depth=4, seed=seed)[:2] for sc, seed in ((c, 21), (a, 22), (b, 23))]
    check_linear("area + envmap + point", films)


# ---- 5: guided ------------------------------------------------------------------------------------------------------
def spot_cornell(pg):
    sc = pg.scenes.cornell(W, H, area_light=False)
    sc.add_spot_light((2.78, 5.3, 2.8), (2.78, 0.0, 2.8), (200.0, 200.0, 160.0), cutoff_angle=50, beam_width=35)
    return sc


def test_guided_spot_light(pg):
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer, ProgressivePathTracer
    sc = spot_cornell(pg)
    props = {"maxDepth": 4, "trainingIterations": 4}
    recs, films = [], []
    for tail in (-1, 1 << 30):
        g = GuidedPathTracer(dict(props, tailPaths=tail))
        g.preprocess(sc)
        offset = 0
        for it in range(4):  # GuidedPathTracer.train, with the records of the last iteration kept
            g.dev.render_pass(2 ** it, offset, record=True)
            offset += 2 ** it
            if it == 3:
                r = np.asarray(g.dev.get_records()).view(np.uint32).reshape(-1, 8)
                recs.append((g.dev.record_count(), r[np.lexsort(r.T)].tobytes()))  # the append order is not fixed
            g.dev.splat_local()
            g.dev.refit(it)
        g.dev.reset_film()
        g.dev.render_pass(SPP, offset)
        films.append(g.dev.read_film())
        g.postprocess()
    assert recs[0][0] > 0 and recs[0] == recs[1]  # the records do not depend on the launch variant
    assert same_bits(films[0][0], films[1][0])
    u = ProgressivePathTracer({"maxDepth": 4})
    u.preprocess(sc)
    u.dev.render_pass(SPP, 5000)
    plain = u.dev.read_film()
    u.postprocess()
    total, var, ok = z_scores([films[0], plain], (1, -1))
    z = np.abs(total[ok]) / np.sqrt(var[ok])
    zmean = abs(total.mean()) / np.sqrt(var.sum()) * total.size
    print(f"guided - unguided: |z| < 5 for {(z < 5).mean():.5f}, max {z.max():.2f}; z of the image mean {zmean:.2f}")
    assert (z < 5).mean() >= 0.999 and zmean < 4.5


# ---- 6: volumetric medium -------------------------------------------------------------------------------------------
# a null-BSDF box between the point light (y = 2) and the plane, filled by a constant-density 8^3 grid (the grid's box
# is a little larger than the shape, so the density is 1 throughout it), albedo 0: pure absorption.  sigma_t = 0.4
# keeps exp(-sigma_t l) above 0.4 on the longest chord (0.5 / sin(14 degrees) = 2.1 for the flattest camera ray),
# so with 64 samples no pixel's estimate is all zeros and the sums of squares give a usable variance.
MED_LO, MED_HI, SIGMA_T, MSPP = (-1.5, 0.6, -1.0), (2.0, 1.1, 2.5), 0.4, 64


def medium_scene(pg):
    S = pg.scenes

    def light(s):
        med = s.add_medium(np.ones((8, 8, 8), np.float32), tuple(v - 0.25 for v in MED_LO),
                           tuple(v + 0.25 for v in MED_HI), SIGMA_T, albedo=(0.0, 0.0, 0.0), g=0.0)
        V, F = S.box(MED_LO, MED_HI)
        s.add_mesh(V, F, material=s.add_material(S.material("null")), interior=med)
        LIGHTS["point"](s)
    return plane_scene(pg, light)


def chord(a, b):
    """length of the part of the segments a -> b (n, 3) inside the box (MED_LO, MED_HI): a numpy slab test"""
    d = b - a
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (np.float64(MED_LO) - a) / d
        t1 = (np.float64(MED_HI) - a) / d
    tn = np.nanmax(np.minimum(t0, t1), axis=1).clip(0, 1)
    tf = np.nanmin(np.maximum(t0, t1), axis=1).clip(0, 1)
    return np.maximum(tf - tn, 0) * np.linalg.norm(d, axis=1)


def medium_reference(sc):
    att = lambda o, x, lp: np.exp(-SIGMA_T * (chord(x, np.broadcast_to(lp, x.shape)) + chord(o, x)))
    want, _ = closed_form(sc, spp=MSPP, attenuation=att)
    clear, _ = closed_form(sc, spp=MSPP)
    return want, clear


def check_medium(name, rgbw, sq, want, clear):
    n = float(MSPP)
    assert (rgbw[..., 3] == n).all()
    mean = rgbw[..., :3].astype(np.float64) / n
    var = np.maximum(sq[..., :3].astype(np.float64) / n - mean * mean, 0) / n
    # a pixel whose samples all agree (neither leg of any of them crosses the box) is deterministic: test 2's bound
    # (a per-sample deviation below 3e-3 of the value: float32 sums of equal samples leave up to 3e-4, sqrt(2^-23))
    flat = var * n <= (3e-3 * want) ** 2
    assert np.abs(mean - want)[flat].max(initial=0) <= 1e-3 * want.max()
    assert (mean[~flat] > 0).all()
    z = np.abs(mean - want)[~flat] / np.sqrt(var[~flat])
    zmean = abs((mean - want).sum()) / np.sqrt(var.sum())
    print(f"medium {name}: {(~flat).mean():.3f} of the values stochastic, |z| < 5 for {(z < 5).mean():.5f}, max "
          f"{z.max():.2f}; z of the image mean {zmean:.2f}; mean attenuation {want.sum() / clear.sum():.3f}")
    assert (~flat).mean() > 0.5 and want.sum() < 0.8 * clear.sum()
    assert (z < 5).mean() >= 0.999 and zmean < 4.5


def test_point_light_through_an_absorbing_medium(pg, monkeypatch):
    """The closed form of test 2 times exp(-sigma_t (l_light + l_camera)).  maxDepth is 8, not 2: the reference counts
    every crossing of an index-matched surface as a bounce (progressive_volpath.cpp:322-333), so the plane behind the
    box is a path's third vertex, and the shadow walk may cross maxDepth - depth - 1 such surfaces; with albedo 0 and
    nothing else to light the plane, the deeper paths add exactly nothing to the closed form.
    The wavefront, the wavefront with the k_vnee stage (bit-identical films) and the megakernel.  Measured on an
    MI355X: |z| < 5 for 99.967 % of the values (max 8.16), z of the image mean 1.42, both variants."""
    sc = medium_scene(pg)
    want, clear = medium_reference(sc)
    cfg = dict(max_depth=8, integrator=pg.capi.PG_INTEGRATOR_VOLPATH)
    wave, wave_sq, _ = render(pg, sc, spp=MSPP, **cfg)
    monkeypatch.setenv("PG_VOL_NEE_STAGE", "1")
    stage, stage_sq, st = render(pg, sc, spp=MSPP, **cfg)
    monkeypatch.delenv("PG_VOL_NEE_STAGE")
    monkeypatch.setenv("PG_VOL_WAVEFRONT", "0")
    mega, mega_sq, _ = render(pg, sc, spp=MSPP, **cfg)
    monkeypatch.delenv("PG_VOL_WAVEFRONT")
    assert st["vol_nee_walks"] > 0
    assert same_bits(wave, stage) and same_bits(wave_sq, stage_sq)
    check_medium("wavefront", wave, wave_sq, want, clear)
    check_medium("megakernel", mega, mega_sq, want, clear)


# ---- 7: off is off, errors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol", [False, True], ids=["path", "volpath"])
def test_removed_lights_leave_no_trace(pg, vol):
    S = pg.scenes
    cfg = dict(max_depth=4, integrator=pg.capi.PG_INTEGRATOR_VOLPATH if vol else pg.capi.PG_INTEGRATOR_PATH)
    for sc in (S.cornell(W, H), S.smoke(width=32, height=32, res=32)) if vol else (S.cornell(W, H),):
        fresh, fresh_sq, _ = render(pg, sc, spp=4, **cfg)
        d = make_dev(pg, sc, **cfg)
        d.set_delta_emitters([S.point_light((1, 1, 1), 5.0), S.directional_light((0, -1, 0), 1.0)])
        d.set_delta_emitters([])
        d.render_pass(4, 0)
        rgbw, sq = d.read_film()
        d.close()
        assert same_bits(rgbw, fresh) and same_bits(sq, fresh_sq)
        # and a light does change the picture
        d = make_dev(pg, sc, **cfg)
        d.set_delta_emitters([S.point_light((2.78, 2.7, 2.8), 5.0)])
        d.render_pass(4, 0)
        assert not same_bits(d.read_film()[0], fresh)
        d.close()


def test_invalid_emitters_are_rejected(pg):
    S, capi = pg.scenes, pg.capi
    from mitsuba_path_guiding_amd.integrator import PGError
    sc = S.cornell(16, 16)
    d = make_dev(pg, sc)
    ref, smp = np.float32([[1, 1, 1]] * 64), np.random.default_rng(1).random((64, 2)).astype(np.float32)
    good = [S.point_light((1, 4, 1), 5.0)]
    d.set_delta_emitters(good)
    before = d.emitter_query(ref, smp)

    def variant(base, **kw):
        e = capi.pg_delta_emitter.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(e, k, v if np.isscalar(v) else (C.c_float * 3)(*v))
        return e

    spot = S.spot_light((1, 4, 1), (1, 0, 1), 5.0)
    bad = [variant(good[0], type=3), variant(good[0], type=-1),
           variant(good[0], position=(np.nan, 0, 0)), variant(good[0], intensity=(1, np.inf, 1)),
           variant(good[0], intensity=(1, -0.5, 1)), variant(spot, direction=(0, 0, 0)),
           variant(S.directional_light((0, -1, 0), 1.0), direction=(0, 0, 0)),
           variant(spot, beam_width=spot.cutoff_angle), variant(spot, beam_width=-0.1),
           variant(spot, cutoff_angle=3.2), variant(spot, cutoff_angle=np.nan)]
    for e in bad:
        with pytest.raises(PGError) as err:
            d.set_delta_emitters([good[0], e])
        assert err.value.status == capi.PG_ERR_INVALID
        assert same_bits(d.emitter_query(ref, smp), before)  # the state is untouched
    with pytest.raises(PGError) as err:
        d.set_delta_emitters(good * 65534)  # plus the area light
    assert err.value.status == capi.PG_ERR_INVALID
    d.set_delta_emitters(good * 65533)
    d.set_delta_emitters(good)
    # a re-upload clears them
    d.upload(sc)
    assert not (d.emitter_query(ref, smp)[:, 7] == 2).any()
    d.set_delta_emitters(good)
    assert (d.emitter_query(ref, smp)[:, 7] == 2).any()
    # not after a pass
    d.render_pass(1, 0)
    for ems in (good, []):
        with pytest.raises(PGError) as err:
            d.set_delta_emitters(ems)
        assert err.value.status == capi.PG_ERR_STATE
    d.close()
