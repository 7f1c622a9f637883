"""The thin-lens sensor (pg_set_lens / pg_get_lens / pg_camera_rays) on the GPU.

The camera rays are pinned against the numpy restatement (tests/camera_ref.py) and against properties that do not
depend on it; the images against closed forms: a half-plane emitter seen through the lens is blurred by the disk's
marginal distribution, and a plane in focus is as sharp as the pinhole's.  Lens off must be bit for bit the context
that never heard of a lens, and lens on must leave every later random dimension where it was."""
import numpy as np
import pytest

import camera_ref as CR

pytestmark = pytest.mark.gpu

SEED = 1337  # pg_config_default
LENSES = [(0.05, 3.0), (0.5, 0.7)]
UNFUSED = ("PG_NO_RAYS_FUSION", "PG_NO_SHADE_FUSION")


def make_dev(pg, scene, lens=None, rfilter=None, **cfg):
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(**cfg))
    d.upload(scene)
    if rfilter is not None:
        d.set_rfilter(rfilter)
    if lens is not None:
        d.set_lens(*lens)
    return d


# ---- 1, 2: the rays -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rays(pg):
    """cornell 16 x 12 (camera at (2.78, 2.73, -8)), samples 0..7 of every pixel: the pairs, and per lens the GPU's
    rays and the restatement's"""
    sc = pg.scenes.cornell(width=16, height=12)
    pix = np.repeat(np.arange(16 * 12, dtype=np.uint32), 8)
    smp = np.tile(np.arange(8, dtype=np.uint32), 16 * 12)
    d = make_dev(pg, sc)
    out = {None: d.camera_rays(pix, smp)}
    for lens in LENSES:
        d.set_lens(*lens)
        assert d.get_lens() == tuple(np.float32(v) for v in lens)
        out[lens] = d.camera_rays(pix, smp)
        again = d.camera_rays(pix, smp)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(out[lens], again))
    d.close()
    for pair in out.values():
        for a in pair:
            a.setflags(write=False)
    return sc, pix, smp, out


def bound(cam, radius):
    return 2.0 ** -20 * max(1.0, float(np.abs(np.array(list(cam.origin))).max()), radius)


@pytest.mark.parametrize("lens", LENSES, ids=lambda l: f"R{l[0]}-f{l[1]}")
def test_rays_match_the_restatement(rays, lens):
    """Measured on an MI355X (16 x 12 x 8 rays, camera |o|inf = 8; profiles/r13_thinlens/README.md): origin within
    1.8e-7, direction 1.1e-7 (bound 7.6e-6), tmin / tmax 1.8e-7 relative (bound 9.5e-7)."""
    sc, pix, smp, out = rays
    o, d = out[lens]
    ro, rd = CR.thinlens_rays(sc.camera, pix, smp, SEED, *lens)
    eo, ed = np.abs(o[:, :3] - ro[:, :3]).max(), np.abs(d[:, :3] - rd[:, :3]).max()
    etmin = np.abs(o[:, 3] / ro[:, 3] - 1).max()
    etmax = np.abs(d[:, 3] / rd[:, 3] - 1).max()
    b = bound(sc.camera, lens[0])
    print(f"lens {lens}: |do|inf {eo:.3e} |dd|inf {ed:.3e} (bound {b:.3e}); tmin rel {etmin:.3e} tmax rel {etmax:.3e} "
          f"(bound {2.0 ** -20:.3e})")
    assert eo <= b and ed <= b
    assert etmin <= 2.0 ** -20 and etmax <= 2.0 ** -20
    # the lens moved the origins: no pinhole passes this
    assert np.abs(o[:, :3] - out[None][0][:, :3]).max() > 0.5 * lens[0]


def test_lens_off_is_the_float32_pinhole(rays):
    sc, pix, smp, out = rays
    o, d = out[None]
    ro, rd = CR.pinhole_rays(sc.camera, pix, smp, SEED)
    assert np.array_equal(o.view(np.uint32), ro.view(np.uint32)), np.argwhere(o != ro)[:8]
    assert np.array_equal(d.view(np.uint32), rd.view(np.uint32)), np.argwhere(d != rd)[:8]


@pytest.mark.parametrize("lens", LENSES, ids=lambda l: f"R{l[0]}-f{l[1]}")
def test_ray_invariants(rays, lens):
    sc, pix, smp, out = rays
    R, focus = lens
    o, d = (a.astype(np.float64) for a in out[lens])
    cam_o, left, up, fwd, _, _ = (np.asarray(v, np.float64) for v in CR.frame(sc.camera))
    b = bound(sc.camera, R)
    rel = o[:, :3] - cam_o
    assert np.abs(rel @ fwd).max() <= b  # in the plane through cam_o perpendicular to dir
    assert np.sqrt((rel * rel).sum(1)).max() <= R + b  # on the aperture
    assert np.sqrt((rel * rel).sum(1)).max() > 0.9 * R
    assert np.abs(np.sqrt((d[:, :3] ** 2).sum(1)) - 1).max() <= b
    # every ray of a sample passes through the pinhole ray's point on the focal plane
    po, pd = (a.astype(np.float64) for a in out[None])
    hit = o[:, :3] + d[:, :3] * (focus / (d[:, :3] @ fwd))[:, None]
    want = cam_o + pd[:, :3] * (focus / (pd[:, :3] @ fwd))[:, None]
    print(f"lens {lens}: focal-plane miss {np.abs(hit - want).max():.3e} (bound {b:.3e})")
    assert np.abs(hit - want).max() <= b


# ---- 3: closed-form blur --------------------------------------------------------------------------------------------
BW, BH, BSPP, BR, BFOCUS = 96, 32, 256, 0.1, 4.0


def half_plane(pg, z, textured=False):
    """camera at the origin looking down +z; one rectangle at depth z over the camera-space half-plane x < 0 (the
    restated frame has left = +x, up = +y, so camera space is world space), facing the camera"""
    S = pg.scenes
    s = S.Scene()
    V, F = S.quad((-50, -50, z), (-50, 50, z), (0, 50, z), (0, -50, z), facing=(0, 0, -1))
    if not textured:
        s.add_mesh(V, F, material=s.add_material(S.material("diffuse", reflectance=(0, 0, 0))), radiance=(1, 1, 1))
    else:
        m = s.add_material(S.material("diffuse"))
        s.add_mesh(V, F, N=np.tile(np.float32([0, 0, -1]), (4, 1)), material=m, uv=V[:, :2])  # uv = world (x, y)
        s.bind_texture(m, s.add_texture("checkerboard", color0=(0.8, 0.1, 0.1), color1=(0.1, 0.2, 0.9)))
        V, F = S.quad((-1, -1, -5), (1, -1, -5), (1, 1, -5), (-1, 1, -5), facing=(0, 0, 1))  # a light behind the camera
        s.add_mesh(V, F, material=s.add_material(S.material("diffuse", reflectance=(0, 0, 0))), radiance=(1, 1, 1))
    s.set_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 40.0, BW, BH)
    return s.finalize()


@pytest.fixture(scope="module")
def blur_samples(pg):
    """the local near-plane x of every sample of the 96 x 32 x 256 job, from the restatement alone"""
    cam = half_plane(pg, 2.0).camera
    o, left, up, fwd, _, _ = CR.frame(cam)
    assert np.array_equal(left, [1, 0, 0]) and np.array_equal(up, [0, 1, 0]) and np.array_equal(fwd, [0, 0, 1])
    pix = np.repeat(np.arange(BW * BH), BSPP)
    smp = np.tile(np.arange(BSPP), BW * BH)
    nx, ny = CR.near_plane64(cam, pix, smp, SEED)
    nx, ny = nx.reshape(-1, BSPP), ny.reshape(-1, BSPP)
    nx.setflags(write=False)
    ny.setflags(write=False)
    return nx, ny


def film_mean(pg, scene, lens, **cfg):
    d = make_dev(pg, scene, lens, max_depth=1, **cfg)
    d.render_pass(BSPP, 0)
    rgbw = d.read_film()[0]
    d.close()
    assert np.array_equal(rgbw[..., 3], np.full((BH, BW), BSPP, np.float32))
    assert np.array_equal(rgbw[..., 0], rgbw[..., 1]) and np.array_equal(rgbw[..., 0], rgbw[..., 2])
    return (rgbw[..., 0].astype(np.float64) / BSPP).reshape(-1)


def blur_prediction(nx, z):
    """A sample with local near-plane x = nx meets depth z at x = ax (1 - z / focus) + nx z, ax the aperture
    point's x: uniform on the disk of radius R.  It hits x < 0 with probability F(-nx z / (R |1 - z / focus|))
    (for z > focus the inequality flips, and F(-s) = 1 - F(s))."""
    Fi = CR.disk_cdf(-nx * z / (BR * abs(1 - z / BFOCUS)))
    return Fi.mean(1), np.sqrt((Fi * (1 - Fi)).sum(1)) / BSPP


def test_blur_has_something_to_show(blur_samples):
    """From the restatement alone: 100 pixels or more with 0.05 < mean F < 0.95 over the two depths (192 at z = 2,
    64 at z = 8: the blur is two pixel columns wide there, so the bar of 100 is set on their sum), and the edge
    blurred in every one of the 32 rows at either depth."""
    nx, _ = blur_samples
    counts = []
    for z in (2.0, 8.0):
        mean, _ = blur_prediction(nx, z)
        counts.append(int(((mean > 0.05) & (mean < 0.95)).sum()))
    print("partially covered pixels at z = 2, 8:", counts)
    assert sum(counts) >= 100 and min(counts) >= BH


@pytest.mark.parametrize("z,vol", [(2.0, False), (8.0, False), (2.0, True)], ids=["z2", "z8", "z2-volpath"])
def test_blur_closed_form(pg, blur_samples, z, vol):
    nx, _ = blur_samples
    cfg = dict(integrator=pg.capi.PG_INTEGRATOR_VOLPATH) if vol else {}
    got = film_mean(pg, half_plane(pg, z), (BR, BFOCUS), **cfg)
    mean, sigma = blur_prediction(nx, z)
    dev = np.abs(got - mean) - (5 * sigma + 1e-6)
    part = (mean > 0.05) & (mean < 0.95)
    print(f"z = {z}{' volpath' if vol else ''}: worst excess over 5 sigma + 1e-6: {dev.max():.3e}; worst |got - mean| / "
          f"sigma among the {part.sum()} partially covered pixels: {(np.abs(got - mean)[part] / sigma[part]).max():.2f}")
    assert (dev <= 0).all(), np.argwhere(dev > 0)[:8]


def test_in_focus_is_sharp(pg, blur_samples):
    nx, _ = blur_samples
    sc = half_plane(pg, BFOCUS)
    got = film_mean(pg, sc, (BR, BFOCUS))
    pin = film_mean(pg, sc, None)
    clear = (np.abs(nx * BFOCUS) > 1e-4).all(1)
    assert clear.mean() > 0.98
    assert np.isin(got[clear], (0.0, 1.0)).all()
    assert np.array_equal(got[clear], pin[clear])
    assert (got[clear] == 1).any() and (got[clear] == 0).any()


# ---- 4: off is off --------------------------------------------------------------------------------------------------
def guided_job(pg, scene, prepare, lens=None, passes=3, final_spp=0, rfilter=None, world=None, **cfg):
    """a guided job: `passes` training iterations (and a final render); everything a context can be asked for"""
    d = make_dev(pg, scene, lens, rfilter, guiding=1, s_tree_threshold=300.0, **cfg)
    prepare(d)
    off, recs = 0, []
    for it in range(passes):
        d.render_pass(2 ** it, off, True)
        rec = d.get_records().reshape(-1, 32)  # in commit order, which no run fixes: compare them sorted
        recs.append(rec[np.lexsort(rec.T[::-1])])
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    if final_spp:
        d.reset_film()
        d.render_pass(final_spp, off)
    stats = {k: v for k, v in d.stats().items() if not k.endswith("_ms")}  # every counter of pg_stats, no clocks
    out = dict(film=d.read_film(), tree=d.get_sdtree(), recs=recs, stats=stats)
    if rfilter is not None:
        out["raw"] = d.read_film_filtered(raw=True)
    d.close()
    return out


def same_job(a, b, stats=True):
    assert np.array_equal(a["film"][0], b["film"][0]) and np.array_equal(a["film"][1], b["film"][1])
    assert np.array_equal(a["tree"], b["tree"])
    assert len(a["recs"]) == len(b["recs"]) and all(len(x) > 0 and np.array_equal(x, y)
                                                     for x, y in zip(a["recs"], b["recs"]))
    if stats:
        assert a["stats"] == b["stats"]
    if "raw" in a:
        assert np.array_equal(a["raw"], b["raw"])


@pytest.fixture(scope="module")
def cornell_job(pg):
    sc = pg.scenes.cornell(width=64, height=48)
    return sc, guided_job(pg, sc, lambda d: None)


def _off_by_zero(d):
    d.set_lens(0.0, 12345.0)


def _set_and_unset(d):
    d.set_lens(0.3, 5.0)
    d.set_lens(0.0, 0.0)


def _set_then_upload(d):
    d.set_lens(0.3, 5.0)
    d.lib.pg_upload_scene(d.h, __import__("ctypes").byref(d.scene.desc()))  # the bare call: no lens re-applied
    assert d.get_lens() == (0.0, 0.0)


@pytest.mark.parametrize("prepare", [_off_by_zero, _set_and_unset, _set_then_upload], ids=lambda f: f.__name__.strip("_"))
def test_off_is_off(pg, cornell_job, prepare):
    sc, base = cornell_job
    same_job(guided_job(pg, sc, prepare), base)
    assert base["film"][0][..., :3].sum() > 0 and base["stats"]["records"] > 0


# ---- 5: later dimensions untouched ----------------------------------------------------------------------------------
LENS5 = (0.3, 8.0)


@pytest.fixture(scope="module")
def lens_job(pg, cornell_job):
    import rfilter_ref as RF
    sc = cornell_job[0]
    t = RF.table("gaussian", 0.5)
    return sc, t, guided_job(pg, sc, lambda d: None, LENS5, final_spp=4, rfilter=t)


def test_lens_changes_the_job(pg, cornell_job, lens_job):
    sc, t, on = lens_job
    off = guided_job(pg, sc, lambda d: None, None, final_spp=4, rfilter=t)
    assert not np.array_equal(on["film"][0], off["film"][0])
    assert on["stats"] != off["stats"]
    assert on["stats"]["paths"] == off["stats"]["paths"]


@pytest.mark.parametrize("cfg,env", [(dict(max_paths_in_flight=1024), ()), (dict(max_paths_in_flight=64 * 48), ()),
                                     (dict(path_lanes=1), ()), (dict(path_lanes=3), ()), ({}, UNFUSED),
                                     (dict(tail_paths=-1), ()), (dict(tail_paths=1 << 20), ())],
                         ids=["chunk1024", "chunk-one-layer", "lanes1", "lanes3", "unfused", "no-tail", "all-tail"])
def test_lens_on_is_deterministic(pg, lens_job, monkeypatch, cfg, env):
    sc, t, on = lens_job
    for name in env:
        monkeypatch.setenv(name, "1")
    # launch counts and the tail's share of the segments differ by design; paths, records, film, trees do not
    got = guided_job(pg, sc, lambda d: None, LENS5, final_spp=4, rfilter=t, **cfg)
    same_job(got, on, stats=False)
    for k in ("paths", "records"):
        assert got["stats"][k] == on["stats"][k]


def test_lens_on_shard_union(pg, lens_job):
    """unguided (a shard trains on its own records): box film, sums of squares and filtered sums of 4 shards"""
    sc, t, _ = lens_job
    whole = make_dev(pg, sc, LENS5, t)
    whole.render_pass(4, 0)
    want = whole.read_film() + (whole.read_film_filtered(raw=True),)
    whole.close()
    total = [np.zeros_like(a) for a in want]
    for r in range(4):
        d = make_dev(pg, sc, LENS5, t, rank=r, world_size=4)
        d.render_pass(4, 0)
        for acc, part in zip(total, d.read_film() + (d.read_film_filtered(raw=True),)):
            acc += part
        d.close()
    for a, b in zip(total, want):
        assert a.any() and np.array_equal(a, b)


@pytest.mark.parametrize("wavefront", ["1", "0"])
def test_lens_on_volpath_variants_agree(pg, monkeypatch, wavefront):
    """k_vcam and the k_volpath megakernel call the same function: the same film, guided, with a medium"""
    sc = pg.scenes.smoke(width=24, height=24, res=16)
    monkeypatch.setenv("PG_VOL_WAVEFRONT", "1")
    cfg = dict(integrator=pg.capi.PG_INTEGRATOR_VOLPATH)
    base = guided_job(pg, sc, lambda d: None, (0.2, 5.0), final_spp=2, **cfg)
    pin = guided_job(pg, sc, lambda d: None, None, final_spp=2, **cfg)
    assert not np.array_equal(base["film"][0], pin["film"][0])
    monkeypatch.setenv("PG_VOL_WAVEFRONT", wavefront)
    same_job(guided_job(pg, sc, lambda d: None, (0.2, 5.0), final_spp=2, max_paths_in_flight=4096, **cfg), base,
             stats=False)


# ---- 6: AOVs --------------------------------------------------------------------------------------------------------
def test_aovs_in_focus(pg):
    """the in-focus plane, diffuse with a checkerboard (checks of 0.5 in world x and y): first-hit albedo and normal
    of the pixels whose samples all stay 1e-3 clear of a check's edge and of the plane's edge equal the pinhole's"""
    sc = half_plane(pg, BFOCUS, textured=True)
    spp = 8
    out = []
    for lens in (None, (BR, BFOCUS)):
        d = make_dev(pg, sc, lens, aovs=1, max_depth=2)
        d.render_pass(spp, 0)
        out.append(d.read_aovs())
        d.close()
    pix = np.repeat(np.arange(BW * BH), spp)
    smp = np.tile(np.arange(spp), BW * BH)
    nx, ny = CR.near_plane64(sc.camera, pix, smp, SEED)
    x, y = nx * BFOCUS, ny * BFOCUS
    edge = lambda v: np.abs(v * 2 - np.rint(v * 2)) / 2
    interior = ((edge(x) > 1e-3) & (edge(y) > 1e-3)).reshape(-1, spp).all(1).reshape(BH, BW)
    assert interior.mean() > 0.5
    (a0, n0), (a1, n1) = out
    assert np.array_equal(a0[interior], a1[interior]) and np.array_equal(n0[interior], n1[interior])
    hit = interior & (x.reshape(-1, spp).max(1) < 0).reshape(BH, BW)
    assert np.array_equal(n1[hit][:, :3], np.tile(np.float32([0, 0, -spp]), (hit.sum(), 1)))
    reds = np.unique(a1[hit][:, 0])
    assert len(reds) > 2  # both colours, and pixels that mix them


# ---- 7: validation --------------------------------------------------------------------------------------------------
def test_validation(pg, cornell_job):
    from mitsuba_path_guiding_amd.integrator import PGError
    d = make_dev(pg, cornell_job[0])
    assert d.get_lens() == (0.0, 0.0)
    d.set_lens(0.25, 3.5)
    nan, inf = float("nan"), float("inf")
    for bad in ((-0.1, 1.0), (nan, 1.0), (inf, 1.0), (-inf, 1.0), (0.1, nan), (0.1, inf), (0.0, nan), (0.1, 0.0),
                (0.1, -1.0)):
        with pytest.raises(PGError) as e:
            d.set_lens(*bad)
        assert e.value.status == pg.capi.PG_ERR_INVALID and "pg_set_lens" in str(e.value)
        assert d.get_lens() == (0.25, 3.5)
    d.set_lens(0.0, -7.0)  # radius 0: off, the focus distance is ignored
    assert d.get_lens() == (0.0, 0.0)
    with pytest.raises(PGError) as e:
        d.camera_rays([64 * 48], [0])
    assert e.value.status == pg.capi.PG_ERR_INVALID
    d.close()


def test_scene_and_integrator_carry_the_lens(pg, rays):
    """Scene.set_lens is applied after every upload; the tracers' apertureRadius / focusDistance override it"""
    from mitsuba_path_guiding_amd.integrator import ProgressivePathTracer
    sc, pix, smp, out = rays
    lens = LENSES[0]
    sc2 = pg.scenes.cornell(width=16, height=12)
    sc2.set_lens(*lens)
    d = make_dev(pg, sc2)
    assert d.get_lens() == tuple(np.float32(v) for v in lens)
    assert np.array_equal(d.camera_rays(pix, smp)[0], out[lens][0])
    d.upload(sc2)
    assert d.get_lens() == tuple(np.float32(v) for v in lens)
    d.close()
    t = ProgressivePathTracer({"apertureRadius": LENSES[1][0], "focusDistance": LENSES[1][1]})
    t.preprocess(sc2)
    o, dd = t.camera_rays(pix, smp)
    assert np.array_equal(o, out[LENSES[1]][0]) and np.array_equal(dd, out[LENSES[1]][1])
    t.postprocess()
    t = ProgressivePathTracer({"apertureRadius": 0})
    t.preprocess(sc2)
    assert np.array_equal(t.camera_rays(pix, smp)[0], out[None][0])
    t.postprocess()
