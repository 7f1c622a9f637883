"""Host restatement of the camera rays (DESIGN.md §4 "Camera rays and the thin lens", include/pg_capi.h pg_set_lens)
for the tests: the pinhole of PerspectiveCamera::sampleRay in float32, step by step as the device function computes
it, and the thin lens of ThinLens::sampleRay in float64 from the same float32 Philox outputs.  The Philox draws come
from rfilter_ref.py."""
import ctypes
import ctypes.util

import numpy as np

import rfilter_ref as R

F = np.float32
PG_DIM_APERTURE = 0x40000000


def tanf(x):
    """The C library's float tangent, which pg_upload_scene calls (numpy's float32 tan rounds some arguments the
    other way: 1 ulp at fov 39.3077)."""
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    m.tanf.restype, m.tanf.argtypes = ctypes.c_float, [ctypes.c_float]
    return F(m.tanf(float(F(x))))


def frame(cam):
    """(origin, left, up, dir, tan_half, aspect) as pg_upload_scene derives them (Transform::lookAt), float32."""
    o, t, up = (np.array(list(v), F) for v in (cam.origin, cam.target, cam.up))
    d = t - o
    d = d / np.sqrt((d * d).sum(dtype=F))
    left = np.cross(up, d).astype(F)
    left = left / np.sqrt((left * left).sum(dtype=F))
    nup = np.cross(d, left).astype(F)
    tan_half = tanf(F(cam.fov_x_deg) * F(3.14159265358979323846) / F(360.0))
    return o, left, nup, d, tan_half, F(cam.width) / F(cam.height)


def near_plane(cam, pixel, sample, seed):
    """The local near-plane point (x, y; z = 1) of the samples, float32."""
    W, H = cam.width, cam.height
    _, _, _, _, tan_half, aspect = frame(cam)
    pixel = np.asarray(pixel, np.int64)
    jx, jy = R.jitter(pixel, sample, seed)
    px, py = (pixel % W).astype(F) + jx, (pixel // W).astype(F) + jy
    sx, sy = px / F(W), py / F(H)
    return (F(1) - F(2) * sx) * tan_half, (F(1) - F(2) * sy) / aspect * tan_half


def pinhole_rays(cam, pixel, sample, seed):
    """(o, tmin), (d, tmax) of the pinhole in float32, (n, 4) each: what the lens-off kernels store, bit for bit."""
    o, left, up, d, _, _ = frame(cam)
    nx, ny = near_plane(cam, pixel, sample, seed)
    ln = np.sqrt((nx * nx + ny * ny) + F(1))
    dx, dy, dz = nx / ln, ny / ln, F(1) / ln
    invz = F(1) / dz
    wd = (left[None, :] * dx[:, None] + up[None, :] * dy[:, None]) + d[None, :] * dz[:, None]
    ro = np.concatenate([np.broadcast_to(o, (len(nx), 3)), (F(cam.near_clip) * invz)[:, None]], 1).astype(F)
    rd = np.concatenate([wd, (F(cam.far_clip) * invz)[:, None]], 1).astype(F)
    return ro, rd


def aperture_sample(pixel, sample, seed):
    """(a0, a1): dimension PG_DIM_APERTURE of the pixel's counter stream, float32."""
    o0, o1 = R.philox(sample, PG_DIM_APERTURE, R.rng_key(pixel, seed))
    return R.u2f(o0), R.u2f(o1)


def concentric_disk(a0, a1):
    """squareToUniformDiskConcentric on float32 samples: the branch by the float32 comparison the device makes
    (r1, r2 are exact in float32), the point in float64."""
    a0, a1 = np.asarray(a0, F), np.asarray(a1, F)
    r1f, r2f = F(2) * a0 - F(1), F(2) * a1 - F(1)
    first = (r1f * r1f) > (r2f * r2f)
    zero = (r1f == 0) & (r2f == 0)
    r1, r2 = r1f.astype(np.float64), r2f.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(first, (np.pi / 4) * (r2 / r1), (np.pi / 2) - (r1 / r2) * (np.pi / 4))
    r = np.where(first, r1, r2)
    phi = np.where(zero, 0.0, phi)
    r = np.where(zero, 0.0, r)
    return r * np.cos(phi), r * np.sin(phi)


def thinlens_rays(cam, pixel, sample, seed, radius, focus):
    """(o, tmin), (d, tmax) of the thin lens in float64, (n, 4) each, from the float32 jitter and aperture draws
    and the float32 camera constants the device holds."""
    o, left, up, d, _, _ = (np.asarray(v, np.float64) for v in frame(cam))
    nx, ny = (np.asarray(v, np.float64) for v in near_plane64(cam, pixel, sample, seed))
    a0, a1 = aperture_sample(pixel, sample, seed)
    ax, ay = concentric_disk(a0, a1)
    ax, ay = ax * float(F(radius)), ay * float(F(radius))
    f = float(F(focus))
    vx, vy, vz = nx * f - ax, ny * f - ay, np.full_like(nx, f)
    ln = np.sqrt(vx * vx + vy * vy + vz * vz)
    dx, dy, dz = vx / ln, vy / ln, vz / ln
    invz = 1.0 / dz
    org = o[None, :] + left[None, :] * ax[:, None] + up[None, :] * ay[:, None]
    wd = left[None, :] * dx[:, None] + up[None, :] * dy[:, None] + d[None, :] * dz[:, None]
    ro = np.concatenate([org, (float(F(cam.near_clip)) * invz)[:, None]], 1)
    rd = np.concatenate([wd, (float(F(cam.far_clip)) * invz)[:, None]], 1)
    return ro, rd


def near_plane64(cam, pixel, sample, seed):
    """near_plane in float64 from the float32 jitter and the float32 tan_half / aspect."""
    W, H = cam.width, cam.height
    _, _, _, _, tan_half, aspect = frame(cam)
    pixel = np.asarray(pixel, np.int64)
    jx, jy = (np.asarray(v, np.float64) for v in R.jitter(pixel, sample, seed))
    sx, sy = ((pixel % W) + jx) / W, ((pixel // W) + jy) / H
    return (1 - 2 * sx) * float(tan_half), (1 - 2 * sy) / float(aspect) * float(tan_half)


def disk_cdf(s):
    """P(x < s) of a point uniform on the unit disk: 1/2 + (s sqrt(1 - s^2) + asin s) / pi, clamped."""
    s = np.clip(np.asarray(s, np.float64), -1.0, 1.0)
    return 0.5 + (s * np.sqrt(1 - s * s) + np.arcsin(s)) / np.pi
