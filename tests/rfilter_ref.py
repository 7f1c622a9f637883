"""Host restatement of the filtered film (include/pg_capi.h "filtered film") for the tests: the counter RNG's
camera jitter (Philox-2x32-10, rngKey, u2f: csrc/pg_device.h), the reference's filter tables in
closed form, and the fixed-point splat in float32 / float64 numpy, step by step as the header spells it out."""
import numpy as np

F = np.float32
FIX = 2.0 ** 28


def philox(c0, c1, key):
    """Philox-2x32-10 on uint32 arrays (held in uint64 so that the 32 x 32 product is exact)."""
    c0, c1, key = (np.asarray(a, np.uint64) & np.uint64(0xFFFFFFFF) for a in np.broadcast_arrays(c0, c1, key))
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        prod = np.uint64(0xD256D193) * c0
        c0, c1 = (prod >> np.uint64(32)) ^ key ^ c1, prod & m32
        key = (key + np.uint64(0x9E3779B9)) & m32
    return c0.astype(np.uint32), c1.astype(np.uint32)


def u2f(v):
    return (np.asarray(v, np.uint32) >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def rng_key(pixel, seed):
    return (np.asarray(pixel, np.uint64) ^ np.uint64((seed * 0x85EBCA6B) & 0xFFFFFFFF)).astype(np.uint32)


def jitter(pixel, sample, seed):
    """(jx, jy) of camera sample `sample` of global pixel `pixel`: dimension 0 of the path's stream."""
    o0, o1 = philox(sample, 0, rng_key(pixel, seed))
    return u2f(o0), u2f(o1)


def camera_direction(cam, pixel, sample, seed):
    """World direction of the camera ray k_camera builds from the jitter (float32 throughout)."""
    W, H = cam.width, cam.height
    o, t, up = (np.array(list(v), F) for v in (cam.origin, cam.target, cam.up))
    d = t - o
    d = d / np.sqrt((d * d).sum(dtype=F))
    left = np.cross(up, d).astype(F)
    left = left / np.sqrt((left * left).sum(dtype=F))
    nup = np.cross(d, left).astype(F)
    tan_half = F(np.tan(F(cam.fov_x_deg) * F(3.14159265358979323846) / F(360.0)))
    aspect = F(W) / F(H)
    jx, jy = jitter(pixel, sample, seed)
    px, py = F(pixel % W) + jx, F(pixel // W) + jy
    sx, sy = px / F(W), py / F(H)
    n = np.array([(F(1) - F(2) * sx) * tan_half, (F(1) - F(2) * sy) / aspect * tan_half, F(1)], F)
    n = n / np.sqrt((n * n).sum(dtype=F))
    return left * n[0] + nup * n[1] + d * n[2]


def table(name, stddev=0.5):
    """(radius, values[32]) of ReconstructionFilter::configure for box / tent / gaussian in closed form."""
    if name == "box":
        r = F(0.5)
        ev = lambda x: F(1.0) if abs(x) <= r else F(0.0)
    elif name == "tent":
        r = F(1.0)
        ev = lambda x: max(F(0.0), F(1.0) - abs(x / r))
    else:
        s = F(stddev)
        r = F(4) * s
        alpha = F(-1.0) / (F(2.0) * s * s)
        fastexp = lambda x: F(np.exp(np.float64(x)))
        ev = lambda x: max(F(0.0), fastexp(alpha * x * x) - fastexp(alpha * r * r))
    v = np.zeros(32, F)
    total = F(0)
    for i in range(31):
        v[i] = ev((r * F(i)) / F(31))
        total = F(total + v[i])
    total = F(total * (F(2) * r / F(31)))
    v[:31] *= F(1.0) / total
    return float(r), v


def splat(acc, W, H, radius, values, pixel, jx, jy, L, valid=None):
    """The taps of samples (arrays: global pixel, jitter, L (n, 3) float32, valid mask) into acc (H, W, 4) int64.
    Vectorised over the samples, one tap offset at a time; every step in the precision the header states."""
    pixel = np.atleast_1d(np.asarray(pixel, np.int64))
    jx, jy = np.atleast_1d(np.asarray(jx, F)), np.atleast_1d(np.asarray(jy, F))
    L = np.asarray(L, F).reshape(-1, 3)
    valid = np.ones(len(pixel), bool) if valid is None else np.atleast_1d(valid)
    values = np.asarray(values, F)
    r = F(radius)
    scale = F(31.0) / r
    bx, by = pixel % W, pixel // W
    posx = (bx.astype(F) + jx) - F(0.5)
    posy = (by.astype(F) + jy) - F(0.5)
    xa, xb = np.maximum(np.ceil(posx - r).astype(np.int64), 0), np.minimum(np.floor(posx + r).astype(np.int64), W - 1)
    ya, yb = np.maximum(np.ceil(posy - r).astype(np.int64), 0), np.minimum(np.floor(posy + r).astype(np.int64), H - 1)
    flat = acc.reshape(-1, 4)
    L64 = L.astype(np.float64)
    K = int(np.ceil(r)) + 2
    for dy in range(-K, K + 1):
        y = by + dy
        wy = values[np.minimum(np.abs((y.astype(F) - posy) * scale).astype(np.int64), 31)]
        for dx in range(-K, K + 1):
            x = bx + dx
            m = valid & (y >= ya) & (y <= yb) & (x >= xa) & (x <= xb)
            if not m.any():
                continue
            wx = values[np.minimum(np.abs((x.astype(F) - posx) * scale).astype(np.int64), 31)]
            w = (wx * wy).astype(F).astype(np.float64)
            v = np.empty((len(pixel), 4), np.int64)
            v[:, :3] = np.rint(w[:, None] * L64 * FIX).astype(np.int64)
            v[:, 3] = np.rint(w * FIX).astype(np.int64)
            np.add.at(flat, (y * W + x)[m], v[m])


def reference_film(W, H, radius, values, seed, samples):
    """samples: iterable of (sample index, box film rgbw (H, W, 4) of that one sample: rgb = L, w = 1 or 0
    where the sample was dropped).  Returns the int64 accumulators (H, W, 4)."""
    acc = np.zeros((H, W, 4), np.int64)
    pix = np.arange(W * H)
    for s, film in samples:
        jx, jy = jitter(pix, s, seed)
        f = film.reshape(-1, 4)
        splat(acc, W, H, radius, values, pix, jx, jy, f[:, :3], f[:, 3] > 0)
    return acc
