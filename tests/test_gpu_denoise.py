"""The film denoiser (pg_denoise / pg_denoise_arrays, include/pg_capi.h "denoiser") on the GPU, against its float64
restatement tests/denoise_ref.py (checked on the host by test_denoise_ref.py) and against the properties the
definition promises.  Shapes are tiny on purpose: 37 x 23 is no multiple of the 32 x 8 block and smaller than the
32-pixel reach of level 5, so every level meets every border."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D

pytestmark = pytest.mark.gpu

F = np.float32
# Parity bar, relative, on valid pixels whose reference exceeds 1e-3 (absolute bar * 1e-3 below that).  expf and
# float32 accumulation against float64 are expected to give ~1e-6 per level, ~1e-5 after six.  The first GPU run
# measured a worst deviation of 2.117e-6 (levels 5 and 6; 1.900e-6 at 1, 1.668e-6 at 3) on this input
# (profiles/r22_denoise/README.md); the bar is ten times that, and would never be looser than 1e-4.
PARITY_BAR = 2.117e-5


@pytest.fixture(scope="module")
def dev(pg):
    """a context without a scene: all pg_denoise_arrays needs"""
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config())
    yield d
    d.close()


def f32(*arrays):
    out = [np.ascontiguousarray(a, F) for a in arrays]
    for a in out:
        a.setflags(write=False)
    return out


def parity_input():
    """37 x 23, three albedo / normal regions behind two diagonal edges with a little per-pixel feature jitter,
    random colours and variances, counts from {0, 1, 2, 9} with at most 15 % of the pixels invalid"""
    rng = np.random.default_rng(22)
    H, W = 23, 37
    y, x = np.mgrid[0:H, 0:W]
    region = (x + 2 * y >= 30).astype(int) + (x + 2 * y >= 58)
    base_alb = np.array([[0.2, 0.3, 0.6], [0.8, 0.7, 0.2], [0.45, 0.5, 0.55]])[region]
    base_nrm = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])[region]
    colour = np.array([[0.9, 0.5, 0.2], [0.1, 0.6, 1.4], [2.0, 2.0, 1.5]])[region] * rng.uniform(0.5, 1.5, (H, W, 1))
    n = rng.choice([0, 1, 2, 9], size=(H, W), p=[0.12, 0.2, 0.3, 0.38])
    extra = np.flatnonzero(n == 0)[int(0.15 * H * W):]  # the cap: later invalid pixels get one sample
    n.flat[extra] = 1
    assert 0 < (n == 0).mean() <= 0.15
    k = np.arange(9)[None, None, :, None] < n[..., None, None]  # sample k of a pixel exists
    L = np.clip(colour[:, :, None, :] * (1 + 0.6 * rng.standard_normal((H, W, 9, 3))), 0, None) * k
    a = np.clip(base_alb[:, :, None, :] + 0.01 * rng.standard_normal((H, W, 9, 3)), 0, 1) * k
    N = base_nrm[:, :, None, :] + 0.03 * rng.standard_normal((H, W, 9, 3))
    N = N / np.linalg.norm(N, axis=-1, keepdims=True) * k
    cnt = n[..., None].astype(float)
    return f32(np.concatenate([L.sum(2), cnt], -1), np.concatenate([(L * L).sum(2), 0 * cnt], -1),
               np.concatenate([a.sum(2), cnt], -1), np.concatenate([N.sum(2), 0 * cnt], -1))


@pytest.fixture(scope="module")
def parity():
    return parity_input()


@pytest.mark.parametrize("levels", [1, 3, 5, 6])
def test_parity_with_restatement(dev, parity, levels):
    ref = D.denoise(*parity, levels=levels)
    out = dev.denoise_arrays(*parity, params={"levels": levels})
    valid = parity[0][..., 3] > 0
    assert np.isfinite(out).all()
    assert (out[~valid] == 0).all()
    big = valid[..., None] & (np.abs(ref) > 1e-3)
    rel = (np.abs(out - ref) / np.where(big, np.abs(ref), 1.0))[big].max()
    small = np.abs(out - ref)[valid[..., None] & ~big]
    absd = small.max() if small.size else 0.0
    print(f"levels {levels}: worst relative deviation {rel:.3e} over {big.sum()} values, "
          f"worst absolute below 1e-3 {absd:.3e} over {small.size}")
    assert rel <= PARITY_BAR
    assert absd <= PARITY_BAR * 1e-3
    assert np.abs(out[..., :3] - parity[0][..., :3] / np.maximum(parity[0][..., 3:], 1))[valid].max() > 1e-2  # it filters


def test_tiled_and_gathered_levels_agree(dev, parity, monkeypatch):
    """steps 1 and 2 read their taps from an LDS tile by default; PG_DENOISE_TILED=0 gathers them: same bits"""
    monkeypatch.setenv("PG_DENOISE_TILED", "0")
    gathered = [dev.denoise_arrays(*parity, params={"levels": k}) for k in (1, 2, 5)]
    monkeypatch.setenv("PG_DENOISE_TILED", "1")
    tiled = [dev.denoise_arrays(*parity, params={"levels": k}) for k in (1, 2, 5)]
    for a, b in zip(gathered, tiled):
        assert np.array_equal(a, b)


def edge_input(seed, H=20, W=24):
    """flat 4-spp noise across an albedo edge 0.2 | 0.8 at the middle column: d_a = 108 > 80"""
    rng = np.random.default_rng(seed)
    L = np.array([0.5, 0.4, 0.3]) + 0.2 * rng.standard_normal((H, W, 4, 3))
    rgbw, sumsq = D.film_from_samples(L)
    albedo = np.where(np.arange(W)[None, :, None] < W // 2, 0.2, 0.8) * np.ones((H, W, 3))
    alb, nrm = D.features(H, W, albedo=albedo, n=4.0)
    return rgbw, sumsq, alb, nrm


def test_edge_is_impermeable(dev):
    rgbw, sumsq, alb, nrm = edge_input(5)
    W = rgbw.shape[1]
    a = dev.denoise_arrays(rgbw, sumsq, alb, nrm)
    rgbw2, sumsq2 = rgbw.copy(), sumsq.copy()
    rgbw2[:, W // 2:, :3] *= 7.0   # brighter and far noisier on the right only
    sumsq2[:, W // 2:, :3] *= 90.0
    b = dev.denoise_arrays(rgbw2, sumsq2, alb, nrm)
    # colour and variance of the left half, bit for bit: the hard cut and the feature-aware variance prefilter
    assert np.array_equal(a[:, :W // 2], b[:, :W // 2])
    assert not np.array_equal(a[:, W // 2:], b[:, W // 2:])
    assert np.abs(a[:, :W // 2, :3] - (rgbw[:, :W // 2, :3] / 4).astype(F)).max() > 1e-3  # the left half is filtered


def test_invalid_pixels_do_not_influence(dev):
    rgbw, sumsq, alb, nrm = edge_input(7)
    rng = np.random.default_rng(8)
    hole = rng.random(rgbw.shape[:2]) < 0.1
    hole[:, :3] = True  # an empty tile column, as on a rank of a sharded job
    outs = []
    for junk in (0.0, 1e6, np.nan):
        arrs = [a.copy() for a in (rgbw, sumsq, alb, nrm)]
        for a in arrs:
            a[hole] = junk
        arrs[0][hole, 3] = 0
        outs.append(dev.denoise_arrays(*arrs))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert (outs[0][hole] == 0).all()
    assert np.isfinite(outs[0]).all() and (outs[0][~hole][:, :3] != 0).all()


@pytest.mark.parametrize("n", [1.0, 4.0])
def test_constant_image(dev, n):
    H, W = 23, 37
    c = np.array([0.7, 0.2, 1.3], F)
    rgbw = np.concatenate([np.broadcast_to(c * F(n), (H, W, 3)), np.full((H, W, 1), n)], -1).astype(F)
    sumsq = np.concatenate([np.broadcast_to(c * c * F(n), (H, W, 3)), np.zeros((H, W, 1))], -1).astype(F)
    alb, nrm = D.features(H, W, albedo=(0.3, 0.5, 0.7), n=n)
    mean = rgbw[..., :3] / rgbw[..., 3:]  # float32
    for levels in (1, 5, 6):
        out = dev.denoise_arrays(rgbw, sumsq, alb, nrm, params={"levels": levels})
        ulps = np.abs(out[..., :3].astype(np.float64) - mean) / np.spacing(mean)
        print(f"n {n} levels {levels}: worst {ulps.max():.2f} ulp")
        assert ulps.max() <= 2 * levels


SPP = 16


@pytest.fixture(scope="module")
def cornell(pg):
    """cornell 64 x 64 with feature buffers at 16 spp: the context, its film and features, and a 2048-spp film of
    the same context from other samples as the truth"""
    from mitsuba_path_guiding_amd.integrator import Device
    sc = pg.scenes.cornell(64, 64)
    d = Device(pg.capi.default_config(aovs=1))
    d.upload(sc)
    d.render_pass(2048, SPP)
    t = d.read_film()[0]
    truth = t[..., :3] / t[..., 3:]
    d.reset_film()
    d.render_pass(SPP, 0)
    film, aovs = d.read_film(), d.read_aovs()
    for a in (truth,) + film + aovs:
        a.setflags(write=False)
    yield d, film, aovs, truth
    d.close()


def test_determinism_and_both_paths(cornell, dev):
    d, film, aovs, _ = cornell
    a = d.denoise()
    b = d.denoise()
    assert np.array_equal(a, b)
    assert np.isfinite(a).all() and (a[..., :3] >= 0).all() and a[..., :3].max() > 0
    assert np.array_equal(a, dev.denoise_arrays(*film, *aovs))  # another context, host arrays
    assert np.array_equal(a, d.denoise_arrays(*film, *aovs))
    for before, after in zip(film + aovs, d.read_film() + d.read_aovs()):
        assert np.array_equal(before, after)
    assert d.denoise_ms() > 0


def test_it_denoises(cornell):
    d, film, _, truth = cornell
    den = d.denoise()[..., :3]
    noisy = film[0][..., :3] / film[0][..., 3:]

    def relmse(img):
        return float((((img - truth) ** 2) / (truth ** 2 + 1e-2)).mean())

    print(f"cornell 64 x 64 at {SPP} spp: relMSE noisy {relmse(noisy):.5f} denoised {relmse(den):.5f} "
          f"ratio {relmse(noisy) / relmse(den):.2f}")
    assert relmse(den) < relmse(noisy)


def test_off_is_off(pg):
    from mitsuba_path_guiding_amd.integrator import Device
    sc = pg.scenes.cornell(48, 40)
    outs = []
    for use in (False, True):
        d = Device(pg.capi.default_config(aovs=1))
        d.upload(sc)
        d.render_pass(4, 0)
        if use:
            d.denoise()
        d.render_pass(4, 4)
        outs.append(d.read_film() + d.read_aovs())
        d.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_errors(pg, dev, parity):
    from mitsuba_path_guiding_amd.integrator import Device, PGError
    lib, capi = dev.lib, pg.capi
    p = capi.pg_denoise_params()
    assert lib.pg_denoise_default_params(C.byref(p)) == capi.PG_OK
    assert (p.levels, p.sigma_l, p.sigma_n, p.sigma_a) == (5, 4.0, F(0.1), F(0.1))
    assert lib.pg_denoise_default_params(None) == capi.PG_ERR_INVALID
    out = np.zeros(parity[0].shape, F)
    ptr = [C.c_void_p(a.ctypes.data) for a in parity] + [C.c_void_p(out.ctypes.data)]
    assert lib.pg_denoise(dev.h, None, ptr[4]) == capi.PG_ERR_STATE  # no scene
    sc = pg.scenes.cornell(16, 16)
    d = Device(capi.default_config())  # aovs = 0
    d.upload(sc)
    d.render_pass(1, 0)
    with pytest.raises(PGError) as e:
        d.denoise()
    assert e.value.status == capi.PG_ERR_STATE
    d.denoise_arrays(*parity)  # needs no feature buffers of the context
    d.close()
    for bad in ({"levels": 0}, {"levels": 7}, {"sigma_l": 0.0}, {"sigma_l": -1.0}, {"sigma_n": float("nan")},
                {"sigma_a": float("inf")}, {"sigma_a": 0.0}):
        with pytest.raises(PGError) as e:
            dev.denoise_arrays(*parity, params=bad)
        assert e.value.status == capi.PG_ERR_INVALID, bad
    H, W = parity[0].shape[:2]
    for k in range(5):
        args = list(ptr)
        args[k] = None
        assert lib.pg_denoise_arrays(dev.h, None, W, H, *args) == capi.PG_ERR_INVALID
    assert lib.pg_denoise_arrays(dev.h, None, 0, H, *ptr) == capi.PG_ERR_INVALID
    assert lib.pg_denoise_arrays(dev.h, None, W, 0, *ptr) == capi.PG_ERR_INVALID
    assert lib.pg_denoise_arrays(None, None, W, H, *ptr) == capi.PG_ERR_INVALID
    one = dev.denoise_arrays(*(a[:1, :1] for a in parity))  # 1 x 1
    assert one.shape == (1, 1, 4)


def test_denoise_property(pg):
    from mitsuba_path_guiding_amd import integrator as I
    for cls in (I.ProgressiveVolumetricPathTracer, I.GuidedVolumetricPathTracer):
        with pytest.raises(ValueError):
            cls({"denoise": True})
    with pytest.raises(ValueError):
        I.GuidedPathTracer({"denoise": True, "sampleCombination": "inversevar"})
    assert I.ProgressivePathTracer({}).cfg.aovs == 0 and I.ProgressivePathTracer({"denoise": True}).cfg.aovs == 1
    images = []
    for mirror in (False, True):
        sc = pg.scenes.cornell(32, 24)
        sc.mirror_x = mirror  # the read-out flip of a mirrored sensor
        t = I.ProgressivePathTracer({"denoise": True, "denoiseLevels": 3, "denoiseSigmaL": 3.0})
        t.preprocess(sc)
        rgbw, _ = t.render(4)
        assert t.denoised.shape == (24, 32, 3) and t.denoised_variance.shape == (24, 32)
        assert t.denoised.dtype == F and np.isfinite(t.denoised).all()
        d = t.dev.denoise({"levels": 3, "sigma_l": 3.0})
        t.postprocess()
        images.append((rgbw, t.denoised, t.denoised_variance, d))
    (f0, d0, v0, raw0), (f1, d1, v1, _) = images
    assert np.array_equal(raw0[..., :3], d0) and np.array_equal(raw0[..., 3], v0)  # the properties reach the filter
    assert np.array_equal(f1, f0[:, ::-1]) and np.array_equal(d1, d0[:, ::-1]) and np.array_equal(v1, v0[:, ::-1])
    assert not np.array_equal(d0, d0[:, ::-1])
    g = I.GuidedPathTracer({"denoise": True, "trainingIterations": 2, "sTreeThreshold": 200.0})
    g.preprocess(pg.scenes.cornell(32, 24))
    g.render(4)
    g.postprocess()
    assert g.denoised.shape == (24, 32, 3) and g.denoised_variance.shape == (24, 32)
    plain = I.ProgressivePathTracer({})
    assert plain.denoised is None and plain.denoised_variance is None
