"""Host restatement of the homogeneous medium (include/pg_capi.h "homogeneous media") for the tests, in the role
rfilter_ref.py has for the filtered film: HomogeneousMedium with strategy = balance, step by step as the header
spells it out.  The float32 steps (rand / weight, 1 - rand, the division by sigma_t, the sums and products of the
pdfs) are done in float32; log and exp are evaluated in float64 and rounded to float32, which is what the
reference's math::fastlog / math::fastexp do.  The draws are dimensions 1, 2, ... of the Philox stream of
rfilter_ref.py, keyed by (rng key, sample)."""
import numpy as np

from rfilter_ref import philox, u2f

F = np.float32


def next1(keys, dim):
    """next1D number `dim` (an int or an array) of the streams keys (n, 2) = (rng key, sample)."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2)
    o0, _ = philox(keys[:, 1], dim, keys[:, 0])
    return u2f(o0)


def _exp(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, F).astype(np.float64)).astype(F)


def _log(x):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, F).astype(np.float64)).astype(F)


def sampling_weight(sigma_a, sigma_s, weight=-1.0):
    """The medium sampling weight: the given one, or with -1 the largest channel albedo over the channels with
    sigma_t != 0, raised to 0.5 when it is > 0."""
    if F(weight) != F(-1.0):
        return F(weight)
    sa, ss = np.asarray(sigma_a, F), np.asarray(sigma_s, F)
    st = sa + ss
    w = F(0)
    for c in range(3):
        if st[c] != 0:
            w = max(w, F(ss[c] / st[c]))
    return max(w, F(0.5)) if w > 0 else w


def sample_distance(sigma_t, weight, rays, keys):
    """sampleDistance on rays (n, 8) = (o, mint, d, maxt) -> (n, 8): success, t, transmittance rgb, pdfSuccess,
    pdfFailure, draws used.  t is mint + the sampled distance, and maxt where the sampled distance is not below
    maxt - mint."""
    st = np.asarray(sigma_t, F)
    weight = F(weight)
    rays = np.asarray(rays, F).reshape(-1, 8)
    o, mint, d, maxt = rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7]
    n = len(rays)
    rand = next1(keys, 1)
    scatter = rand < weight
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rand = np.where(scatter, rand / weight, rand).astype(F)
        channel = np.minimum((next1(keys, 2) * F(3)).astype(np.int32), 2)
        sampled = np.where(scatter, -_log(F(1) - rand) / st[channel], F(np.inf)).astype(F)
        dist = (maxt - mint).astype(F)
        inside = sampled < dist
        t = np.where(inside, sampled + mint, maxt).astype(F)
        p = (o + d * t[:, None]).astype(F)
        success = inside & ~np.all(p == o, axis=1)
        sampled = np.where(inside, sampled, dist).astype(F)
        e = _exp(-st[None, :] * sampled[:, None])
        pdf_f = ((e[:, 0] + e[:, 1]) + e[:, 2]) / F(3)
        pdf_s = ((st[0] * e[:, 0] + st[1] * e[:, 1]) + st[2] * e[:, 2]) / F(3)
        pdf_s = (pdf_s * weight).astype(F)
        pdf_f = (weight * pdf_f + (F(1) - weight)).astype(F)
    tr = np.where((e.max(axis=1) < F(1e-20))[:, None], F(0), e).astype(F)
    out = np.zeros((n, 8), F)
    out[:, 0] = success
    out[:, 1] = t
    out[:, 2:5] = tr
    out[:, 5] = pdf_s
    out[:, 6] = pdf_f
    out[:, 7] = np.where(scatter, 2, 1)
    return out


def eval_transmittance(sigma_t, rays):
    """evalTransmittance on rays (n, 8) -> (n, 3): exp(sigma_t (mint - maxt)), 1 where sigma_t = 0."""
    st = np.asarray(sigma_t, F)
    rays = np.asarray(rays, F).reshape(-1, 8)
    neg = (rays[:, 3] - rays[:, 7]).astype(F)
    with np.errstate(invalid="ignore"):
        e = _exp(st[None, :] * neg[:, None])
    return np.where(st[None, :] != 0, e, F(1)).astype(F)


def pdfs(sigma_t, weight, s):
    """(pdfSuccess, pdfFailure) of the balance strategy at distance s (float64: for the reference's own checks)."""
    st = np.asarray(sigma_t, np.float64)
    s = np.asarray(s, np.float64)
    e = np.exp(-st * s[..., None])
    w = float(weight)
    return w * (st * e).mean(-1), w * e.mean(-1) + (1 - w)
