"""numpy float32 restatement of the texture lookups (include/pg_capi.h "textures"): the yardstick of
test_textures.py (hand-computed values) and test_gpu_textures.py (bit for bit against the device).

Every operation is one float32 operation in the order the header states: numpy rounds each of them, so there is no
contraction.  Texel arrays are (height, width, 3) float32, texel (x, y) at rgb[y, x]."""
import numpy as np

F = np.float32
WRAPS = ("repeat", "clamp", "mirror", "zero", "one")


def hit_uv(t0, t1, t2, u, v):
    """Intersection::uv: t0 * b.x + t1 * b.y + t2 * b.z with b = (1 - u - v, u, v); u, v float32 arrays."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    b0 = F(1) - u - v
    t0, t1, t2 = (np.asarray(t, F) for t in (t0, t1, t2))
    return np.stack([t0[k] * b0 + t1[k] * u + t2[k] * v for k in range(2)], axis=-1)


def transform(uv, uscale=1.0, vscale=1.0, uoffset=0.0, voffset=0.0):
    uv = np.asarray(uv, F).reshape(-1, 2)
    return uv[:, 0] * F(uscale) + F(uoffset), uv[:, 1] * F(vscale) + F(voffset)


def _wrap(x, n, mode):
    """index into [0, n), and where the axis answers with a constant instead (zero / one): (idx, mask, value)"""
    oob = (x < 0) | (x >= n)
    if mode == "repeat":
        return np.where(oob, np.mod(x, n), x), np.zeros_like(oob), 0.0
    if mode == "clamp":
        return np.clip(x, 0, n - 1), np.zeros_like(oob), 0.0
    if mode == "mirror":
        m = np.mod(x, 2 * n)
        m = np.where(m >= n, 2 * n - m - 1, m)
        return np.where(oob, m, x), np.zeros_like(oob), 0.0
    if mode in ("zero", "one"):
        return np.clip(x, 0, n - 1), oob, 1.0 if mode == "one" else 0.0
    raise ValueError(mode)


def texel(rgb, x, y, wrap_u, wrap_v):
    """evalTexel: x is wrapped (or answered) first, then y"""
    H, W = rgb.shape[:2]
    xi, cx, vx = _wrap(np.asarray(x, np.int64), W, wrap_u)
    yi, cy, vy = _wrap(np.asarray(y, np.int64), H, wrap_v)
    out = rgb[yi, xi].astype(F)
    out = np.where(cy[:, None], F(vy), out)
    return np.where(cx[:, None], F(vx), out).astype(F)


def bitmap(rgb, uv, filter="bilinear", wrap_u="repeat", wrap_v=None, uscale=1.0, vscale=1.0, uoffset=0.0, voffset=0.0):
    rgb = np.asarray(rgb, F)
    wrap_v = wrap_u if wrap_v is None else wrap_v
    H, W = rgb.shape[:2]
    u, v = transform(uv, uscale, vscale, uoffset, voffset)
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, F(0)), np.where(ok, v, F(0))
    if filter == "nearest":
        out = texel(rgb, np.floor(u * F(W)), np.floor(v * F(H)), wrap_u, wrap_v)
    else:
        x, y = u * F(W) - F(0.5), v * F(H) - F(0.5)
        xp, yp = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
        dx1, dy1 = x - xp.astype(F), y - yp.astype(F)
        dx2, dy2 = F(1) - dx1, F(1) - dy1
        t = lambda a, b: texel(rgb, a, b, wrap_u, wrap_v)
        c = lambda a: a[:, None]
        out = (t(xp, yp) * c(dx2) * c(dy2) + t(xp, yp + 1) * c(dx2) * c(dy1) + t(xp + 1, yp) * c(dx1) * c(dy2)
               + t(xp + 1, yp + 1) * c(dx1) * c(dy1))
    assert out.dtype == F
    return np.where(ok[:, None], out, F(0))


def checkerboard(color0, color1, uv, uscale=1.0, vscale=1.0, uoffset=0.0, voffset=0.0):
    u, v = transform(uv, uscale, vscale, uoffset, voffset)
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, F(0)), np.where(ok, v, F(0))
    x = 2 * np.mod(np.trunc(u * F(2)).astype(np.int64), 2) - 1  # (int) truncates toward zero
    y = 2 * np.mod(np.trunc(v * F(2)).astype(np.int64), 2) - 1
    out = np.where((x * y == 1)[:, None], np.asarray(color0, F)[None], np.asarray(color1, F)[None])
    return np.where(ok[:, None], out, F(0)).astype(F)


def average(rgb=None, color0=None, color1=None):
    """Texture::getAverage: the mean of the level-0 texels, or (color0 + color1) / 2"""
    if rgb is not None:
        return np.asarray(rgb, np.float64).reshape(-1, 3).mean(0).astype(F)
    return ((np.asarray(color0, F) + np.asarray(color1, F)) * F(0.5)).astype(F)
