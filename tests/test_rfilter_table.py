"""Host side of the filtered film (no GPU): pg_rfilter_table against the reference's filters in closed form, the
numpy restatement of the camera jitter against the oracle's first ray, the numpy splat's footprint, and the
<rfilter> element in mitsuba_xml.load."""
import numpy as np
import pytest

import rfilter_ref as R


@pytest.mark.parametrize("name,stddev,radius", [("box", 0.5, 0.5), ("tent", 0.5, 1.0), ("gaussian", 0.5, 2.0),
                                                ("gaussian", 1.0, 4.0)])
def test_table_matches_closed_form(pg, name, stddev, radius):
    from mitsuba_path_guiding_amd.integrator import rfilter_table
    r, v = rfilter_table(name, stddev)
    r2, v2 = R.table(name, stddev)
    assert r == radius == r2
    assert v.dtype == np.float32 and v.shape == (32,)
    assert v[31] == 0
    np.testing.assert_allclose(v, v2, rtol=1e-6, atol=0)
    assert abs(float(v.astype(np.float64).sum()) * 2 * r / 31 - 1) < 1e-6
    if name == "box":
        assert (v[:31] == 1).all()
    else:
        assert (np.diff(v[:31]) < 0).all() and v[30] >= 0


def test_table_errors(pg):
    from mitsuba_path_guiding_amd.integrator import PGError, rfilter_table, library
    import ctypes as C
    with pytest.raises(ValueError):
        rfilter_table("lanczos")
    with pytest.raises(PGError):
        rfilter_table("gaussian", -1.0)
    out = np.zeros(32, np.float32)
    r = C.c_float()
    assert library().pg_rfilter_table(7, 0.0, C.byref(r), C.c_void_p(out.ctypes.data)) == pg.capi.PG_ERR_INVALID
    # stddev 0 = the default
    assert np.array_equal(rfilter_table("gaussian", 0.0)[1], rfilter_table("gaussian", 0.5)[1])


def test_jitter_gives_the_oracles_camera_ray(pg, O):
    sc = pg.scenes.cornell(48, 40)
    cfg = pg.capi.default_config()
    osc = O.OracleScene(pg.capi, sc)
    rng = np.random.default_rng(5)
    pairs = [(0, 0), (47, 1), (48 * 39, 2), (48 * 40 - 1, 1000003)]
    pairs += [(int(p), int(s)) for p, s in zip(rng.integers(0, 48 * 40, 12), rng.integers(0, 1 << 20, 12))]
    for pixel, sample in pairs:
        rays = osc.path_rays(cfg, None, pixel, sample, max_rays=8)[0]
        assert rays[0, 0] == 0  # the camera ray: a closest-hit query
        d = R.camera_direction(sc.camera, pixel, sample, cfg.seed)
        assert np.abs(d - rays[0, 5:8]).max() < 1e-6, (pixel, sample, d, rays[0, 5:8])
    jx, jy = R.jitter(np.arange(4096), 3, cfg.seed)
    assert jx.dtype == np.float32 and (jx >= 0).all() and (jx < 1).all() and (jy >= 0).all() and (jy < 1).all()
    assert 0.45 < jx.mean() < 0.55 and 0.45 < jy.mean() < 0.55


def _one(W, H, radius, values, pixel, jx, jy, L=(1.0, 0.5, 0.25)):
    acc = np.zeros((H, W, 4), np.int64)
    R.splat(acc, W, H, radius, values, pixel, np.float32(jx), np.float32(jy), np.array(L, np.float32))
    return acc


def test_numpy_splat_footprint():
    W, H = 9, 7
    rb, box = R.table("box")
    rg, gau = R.table("gaussian")
    centre = 3 * W + 4
    a = _one(W, H, rb, box, centre, 0.5, 0.5)
    assert np.count_nonzero(a[..., 3]) == 1 and a[3, 4, 3] == 1 << 28
    assert list(a[3, 4, :3]) == [1 << 28, 1 << 27, 1 << 26]
    # gaussian 0.5 (radius 2) at a pixel centre: columns ceil(4 - 2) .. floor(4 + 2) are in range, the outermost at
    # distance 2 hit table entry 31 (zero): a 3 x 3 footprint at the exact centre, 4 x 4 just off it
    a = _one(W, H, rg, gau, centre, 0.5, 0.5)
    assert np.count_nonzero(a[..., 3]) == 9
    a = _one(W, H, rg, gau, centre, 0.75, 0.75)
    nz = np.argwhere(a[..., 3])
    assert len(nz) == 16 and nz[:, 0].min() == 2 and nz[:, 0].max() == 5 and nz[:, 1].min() == 3 and nz[:, 1].max() == 6
    # the taps are separable products of table entries
    w = a[..., 3].astype(np.float64) / 2 ** 28
    assert abs(w.sum() - 1) < 0.05  # the table integrates to one
    # corner pixel: clipped to the image, no renormalisation
    a = _one(W, H, rg, gau, 0, 0.25, 0.25)
    nz = np.argwhere(a[..., 3])
    assert len(nz) == 4 and nz.max() == 1
    assert a[..., 3].sum() < 0.9 * (1 << 28)
    a = _one(W, H, rg, gau, W * H - 1, 0.75, 0.75)
    nz = np.argwhere(a[..., 3])
    assert len(nz) == 4 and nz[:, 0].min() == H - 2 and nz[:, 1].min() == W - 2
    # a negative lobe gives negative sums
    neg = np.array([1.0] * 16 + [-0.25] * 15 + [0.0], np.float32)
    a = _one(W, H, 2.0, neg, centre, 0.75, 0.75)
    assert (a[..., 3] < 0).any() and (a[..., 3] > 0).any()
    # a dropped sample adds nothing
    acc = np.zeros((H, W, 4), np.int64)
    R.splat(acc, W, H, rg, gau, [centre], [0.5], [0.5], np.ones((1, 3), np.float32), np.array([False]))
    assert not acc.any()


XML = """<scene version="0.5.0">
  <integrator type="path"/>
  <sensor type="perspective">
    <float name="fov" value="40"/>
    <transform name="toWorld"><lookat origin="0,0,-4" target="0,0,0" up="0,1,0"/></transform>
    <sampler type="independent"><integer name="sampleCount" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="32"/><integer name="height" value="24"/>%s</film>
  </sensor>
  <shape type="rectangle"><bsdf type="diffuse"/></shape>
  <shape type="rectangle">
    <transform name="toWorld"><translate y="2"/></transform>
    <emitter type="area"><rgb name="radiance" value="5"/></emitter>
  </shape>
</scene>"""


def _load(pg, rf):
    return pg.mitsuba_xml.load(XML % rf)


def test_xml_rfilter(pg):
    assert _load(pg, "").scene.rfilter == ("gaussian", 0.5)  # Film::Film's default (film.cpp:93)
    assert _load(pg, '<rfilter type="box"/>').scene.rfilter == ("box", 0.5)
    assert _load(pg, '<rfilter type="tent"/>').scene.rfilter[0] == "tent"
    name, s = _load(pg, '<rfilter type="gaussian"><float name="stddev" value="0.7"/></rfilter>').scene.rfilter
    assert name == "gaussian" and abs(s - 0.7) < 1e-12
    with pytest.raises(NotImplementedError, match="lanczos"):
        _load(pg, '<rfilter type="lanczos"/>')
    assert (_load(pg, "").scene.width, _load(pg, "").scene.height) == (32, 24)
