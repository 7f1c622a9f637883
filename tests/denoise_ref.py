"""Host restatement of the film denoiser (include/pg_capi.h "denoiser") for the tests: the
variance-guided edge-avoiding a-trous wavelet over the film and the feature buffers, in float64 numpy,
vectorised over the image and looping over the taps, step by step as the header spells it out."""
import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])   # B3 spline
H3 = np.array([1 / 4, 1 / 2, 1 / 4])
CUT = 80.0
MOD_EPS = 0.01
DEFAULTS = dict(levels=5, sigma_l=4.0, sigma_n=0.1, sigma_a=0.1)


def shift(a, ox, oy):
    """(b, inside): b[y, x] = a[y + oy, x + ox] where that pixel lies inside the image (0 elsewhere)"""
    H, W = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((H, W), bool)
    if abs(ox) < W and abs(oy) < H:
        dst = (slice(max(0, -oy), min(H, H - oy)), slice(max(0, -ox), min(W, W - ox)))
        src = (slice(max(0, oy), min(H, H + oy)), slice(max(0, ox), min(W, W + ox)))
        b[dst] = a[src]
        inside[dst] = True
    return b, inside


def prepare(rgbw, sumsq, albedo, normal):
    """step 1: (e, V, N, abar, mod, valid) from the film sums and the feature sums"""
    rgbw, sumsq, albedo, normal = (np.asarray(a, np.float64) for a in (rgbw, sumsq, albedo, normal))
    n = rgbw[..., 3]
    valid = n > 0
    ns = np.where(valid, n, 1.0)[..., None]
    c = rgbw[..., :3] / ns
    abar = albedo[..., :3] / ns
    N = normal[..., :3] / ns
    ln = np.sqrt((N * N).sum(-1, keepdims=True))
    N = np.where(ln > 0, N / np.where(ln > 0, ln, 1.0), 0.0)
    mod = abar + MOD_EPS
    e = c / mod
    var = np.where(n[..., None] >= 2, np.maximum(sumsq[..., :3] / ns - c * c, 0.0) / ns, c * c)
    V = (var / (mod * mod)) @ LUM
    m = valid[..., None]
    return e * m, V * valid, N * m, abar * m, mod, valid


def feature_distance(N, abar, Nq, aq, sigma_n, sigma_a):
    d_n = np.maximum(0.0, 1.0 - (N * Nq).sum(-1)) / sigma_n
    d_a = ((abar - aq) ** 2).sum(-1) / sigma_a ** 2
    return d_n + d_a


def prefilter_variance(V, N, abar, valid, sigma_n, sigma_a):
    """step 2a: the feature-aware 3 x 3 average of V at step 1, normalised by the weights used"""
    vs = np.zeros_like(V)
    ws = np.zeros_like(V)
    for iy, oy in enumerate((-1, 0, 1)):
        for ix, ox in enumerate((-1, 0, 1)):
            k = H3[ix] * H3[iy]
            if ox == 0 and oy == 0:
                use = np.ones_like(valid)
                Vq = V
            else:
                Vq, inside = shift(V, ox, oy)
                Nq, _ = shift(N, ox, oy)
                aq, _ = shift(abar, ox, oy)
                vq, _ = shift(valid, ox, oy)
                use = inside & vq & (feature_distance(N, abar, Nq, aq, sigma_n, sigma_a) <= CUT)
            vs += np.where(use, k * Vq, 0.0)
            ws += np.where(use, k, 0.0)
    return vs / ws


def tap_weights(e, V, N, abar, valid, step, sigma_l, sigma_n, sigma_a):
    """step 2b: the 25 unnormalised tap weights of every pixel, (25, H, W), in (dy, dx) order; 0 for invalid
    centres"""
    Vt = prefilter_variance(V, N, abar, valid, sigma_n, sigma_a)
    tol = sigma_l * np.sqrt(Vt) + 1e-6
    lum = e @ LUM
    w = np.zeros((25,) + V.shape)
    for iy in range(5):
        for ix in range(5):
            ox, oy = step * (ix - 2), step * (iy - 2)
            k = H5[ix] * H5[iy]
            if ox == 0 and oy == 0:
                w[iy * 5 + ix] = k
                continue
            eq, inside = shift(e, ox, oy)
            Nq, _ = shift(N, ox, oy)
            aq, _ = shift(abar, ox, oy)
            vq, _ = shift(valid, ox, oy)
            d = feature_distance(N, abar, Nq, aq, sigma_n, sigma_a) + np.abs(lum - eq @ LUM) / tol
            use = inside & vq & ~(d > CUT)
            w[iy * 5 + ix] = np.where(use, k * np.exp(-np.where(use, d, 0.0)), 0.0)
    return w * valid


def atrous_level(e, V, N, abar, valid, step, sigma_l, sigma_n, sigma_a):
    """one level: (e', V')"""
    w = tap_weights(e, V, N, abar, valid, step, sigma_l, sigma_n, sigma_a)
    se = np.zeros_like(e)
    sv = np.zeros_like(V)
    for iy in range(5):
        for ix in range(5):
            eq, _ = shift(e, step * (ix - 2), step * (iy - 2))
            Vq, _ = shift(V, step * (ix - 2), step * (iy - 2))
            wk = w[iy * 5 + ix]
            se += wk[..., None] * eq
            sv += wk * wk * Vq
    sw = w.sum(0)
    sws = np.where(valid, sw, 1.0)
    return se / sws[..., None] * valid[..., None], sv / (sws * sws) * valid


def denoise(rgbw, sumsq, albedo, normal, levels=5, sigma_l=4.0, sigma_n=0.1, sigma_a=0.1):
    """the whole filter: (H, W, 4) float64, rgb and the filtered variance of the demodulated luminance"""
    e, V, N, abar, mod, valid = prepare(rgbw, sumsq, albedo, normal)
    for i in range(levels):
        e, V = atrous_level(e, V, N, abar, valid, 1 << i, sigma_l, sigma_n, sigma_a)
    return np.concatenate([e * mod * valid[..., None], (V * valid)[..., None]], -1)


def film_from_samples(L):
    """film sums of per-sample radiance L (H, W, n, 3): (rgbw, sumsq) as the library lays them out"""
    n = L.shape[2]
    rgbw = np.concatenate([L.sum(2), np.full(L.shape[:2] + (1,), float(n))], -1)
    sumsq = np.concatenate([(L * L).sum(2), np.zeros(L.shape[:2] + (1,))], -1)
    return rgbw, sumsq


def features(H, W, albedo=0.5, normal=(0.0, 0.0, 1.0), n=1.0):
    """feature sums of a flat region: (albedo rgb * n + count, normal * n + 0)"""
    cnt = np.broadcast_to(np.asarray(n, np.float64), (H, W))[..., None]
    alb = np.concatenate([np.broadcast_to(np.asarray(albedo, np.float64), (H, W, 3)) * cnt, cnt], -1)
    nrm = np.concatenate([np.broadcast_to(np.asarray(normal, np.float64), (H, W, 3)) * cnt, 0 * cnt], -1)
    return alb, nrm
