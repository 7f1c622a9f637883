"""The float64 restatement of the film denoiser (tests/denoise_ref.py) checked against the properties the
definition promises (include/pg_capi.h "denoiser"): it is the yardstick of tests/test_gpu_denoise.py."""
import numpy as np
import pytest

import denoise_ref as D


def flat(H, W, rng, spp=4, truth=(0.5, 0.4, 0.3), sigma=0.2):
    L = np.asarray(truth) + sigma * rng.standard_normal((H, W, spp, 3))
    return D.film_from_samples(L)


def edge_case(rng, H=20, W=24):
    """albedo 0.2 | 0.8 across the middle column: d_a = 3 * 0.36 / 0.01 = 108 > 80"""
    rgbw, sumsq = flat(H, W, rng)
    albedo = np.where(np.arange(W)[None, :, None] < W // 2, 0.2, 0.8) * np.ones((H, W, 3))
    alb, nrm = D.features(H, W, albedo=albedo, n=4.0)
    return rgbw, sumsq, alb, nrm


def test_constant_image_unchanged():
    H, W = 19, 23
    c = np.array([0.7, 0.2, 1.3])
    for n in (1.0, 4.0):
        rgbw = np.concatenate([np.broadcast_to(c * n, (H, W, 3)), np.full((H, W, 1), n)], -1)
        sumsq = np.concatenate([np.broadcast_to(c * c * n, (H, W, 3)), np.zeros((H, W, 1))], -1)
        alb, nrm = D.features(H, W, albedo=(0.3, 0.5, 0.7), n=n)
        for levels in (1, 5, 6):
            out = D.denoise(rgbw, sumsq, alb, nrm, levels=levels)
            assert np.abs(out[..., :3] - c).max() <= 1e-12


def test_weights_partition_of_unity():
    rng = np.random.default_rng(3)
    rgbw, sumsq, alb, nrm = edge_case(rng)
    rgbw[3, 5] = sumsq[3, 5] = alb[3, 5] = nrm[3, 5] = 0  # an invalid pixel
    e, V, N, abar, mod, valid = D.prepare(rgbw, sumsq, alb, nrm)
    for step in (1, 2, 8, 32):
        w = D.tap_weights(e, V, N, abar, valid, step, 4.0, 0.1, 0.1)
        assert (w >= 0).all()
        assert np.array_equal(w[12][valid], np.full(valid.sum(), D.H5[2] ** 2))  # the centre, unconditionally
        assert (w[:, ~valid] == 0).all()
        wn = w[:, valid] / w[:, valid].sum(0)
        assert np.abs(wn.sum(0) - 1).max() <= 1e-14
        # a constant is reproduced by every level whatever the weights are
        const = np.where(valid[..., None], 2.5, 0.0) * np.ones(3)
        e1, _ = D.atrous_level(const, V, N, abar, valid, step, 4.0, 0.1, 0.1)
        assert np.abs(e1[valid] - 2.5).max() <= 1e-14


def test_albedo_edge_is_impermeable():
    rng = np.random.default_rng(5)
    rgbw, sumsq, alb, nrm = edge_case(rng)
    W = rgbw.shape[1]
    a = D.denoise(rgbw, sumsq, alb, nrm)
    rgbw2, sumsq2 = rgbw.copy(), sumsq.copy()
    rgbw2[:, W // 2:, :3] *= 7.0   # brighter and far noisier on the right only
    sumsq2[:, W // 2:, :3] *= 90.0
    b = D.denoise(rgbw2, sumsq2, alb, nrm)
    assert np.array_equal(a[:, :W // 2], b[:, :W // 2])  # colour and variance, bit for bit
    assert not np.array_equal(a[:, W // 2:], b[:, W // 2:])
    # the left half is still filtered
    assert np.abs(a[:, :W // 2, :3] - rgbw[:, :W // 2, :3] / 4).max() > 1e-3


def test_invalid_pixels_do_not_influence_neighbours():
    rng = np.random.default_rng(7)
    H, W = 20, 24
    rgbw, sumsq = flat(H, W, rng)
    alb, nrm = D.features(H, W, n=4.0)
    hole = rng.random((H, W)) < 0.1
    hole[:, :3] = True  # an empty tile column, as on a rank of a sharded job
    outs = []
    for junk in (0.0, 1e6):
        r, s, a, n = rgbw.copy(), sumsq.copy(), alb.copy(), nrm.copy()
        r[hole], s[hole], a[hole], n[hole] = junk, junk, junk, junk
        r[hole, 3] = 0
        outs.append(D.denoise(r, s, a, n))
    assert np.array_equal(outs[0], outs[1])
    assert (outs[0][hole] == 0).all()
    assert (outs[0][~hole][:, :3] != 0).all()


def noise_reduction(levels):
    rng = np.random.default_rng(1)
    truth = np.array([0.5, 0.4, 0.3])
    H, W = 40, 48
    rgbw, sumsq = flat(H, W, rng, spp=4, truth=truth, sigma=0.2)
    alb, nrm = D.features(H, W, albedo=0.5, n=4.0)
    noisy = rgbw[..., :3] / 4
    den = D.denoise(rgbw, sumsq, alb, nrm, levels=levels)[..., :3]
    return ((noisy - truth) ** 2).mean() / ((den - truth) ** 2).mean()


@pytest.mark.parametrize("levels,floor", [(5, 100.0), (1, 8.0)])
def test_noise_reduction(levels, floor):
    """MSE ratio noisy / denoised on a flat 40 x 48 region at 4 spp, sigma 0.2.  Level 0 alone with unit edge
    weights would give 1 / (70 / 256)^2 = 13.4; the prototype of the definition gave 636 (5 levels), 134 (3) and
    10.08 (1)."""
    ratio = noise_reduction(levels)
    print(f"levels {levels}: MSE ratio {ratio:.2f}")
    assert ratio >= floor
