"""numpy float32 restatement of the normal-map semantics (include/pg_capi.h "normal maps"): the yardstick of
test_normalmap.py and test_gpu_normalmap.py.  Built on texture_ref.py for the lookup.

Every operation is one float32 operation in the order the header states (numpy rounds each: no contraction)."""
import numpy as np

import texture_ref as T

F = np.float32


def _f3(a):
    return np.asarray(a, F).reshape(3)


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize(a):
    return a / np.sqrt(dot(a, a))[..., None]


def tangent(p0, p1, p2, t0=None, t1=None, t2=None):
    """dpdu of TriMesh::computeUVTangents; without texcoords (t0 is None) p1 - p0."""
    p0, p1, p2 = _f3(p0), _f3(p1), _f3(p2)
    d1, d2 = p1 - p0, p2 - p0
    if t0 is None:
        return d1
    n = cross(d1, d2)
    length = np.sqrt(dot(n, n))
    if length == 0:
        return d1
    t0, t1, t2 = (np.asarray(t, F).reshape(2) for t in (t0, t1, t2))
    u1, u2 = t1 - t0, t2 - t0
    det = u1[0] * u2[1] - u1[1] * u2[0]
    if det == 0:  # coordinateSystem(n / length): dpdu = cross(c, a)
        a = n / length
        if abs(a[0]) > abs(a[1]):
            inv = F(1) / np.sqrt(a[0] * a[0] + a[2] * a[2])
            c = np.array([a[2] * inv, F(0), -a[0] * inv], F)
        else:
            inv = F(1) / np.sqrt(a[1] * a[1] + a[2] * a[2])
            c = np.array([F(0), a[2] * inv, -a[1] * inv], F)
        return cross(c, a)
    inv = F(1) / det
    return ((u2[1] * d1 - u1[1] * d2) * inv).astype(F)


def shading_frame(n, dpdu):
    """computeShadingFrame: (s, t, n); n (..., 3), dpdu (..., 3)"""
    n, dpdu = np.asarray(n, F), np.asarray(dpdu, F)
    s = normalize(dpdu - n * dot(n, dpdu)[..., None])
    return s, cross(n, s), n


def to_world(frame, v):
    s, t, n = frame
    return s * v[..., 0:1] + t * v[..., 1:2] + n * v[..., 2:3]


def to_local(frame, v):
    s, t, n = frame
    return np.stack([dot(v, s), dot(v, t), dot(v, n)], -1)


def perturbed_frame(shN, dpdu, c):
    """NormalMap::getFrame: (s', t', n') from the unperturbed shading normal, the tangent and the looked-up texel c."""
    shN, dpdu, c = np.asarray(shN, F), np.asarray(dpdu, F), np.asarray(c, F)
    base = shading_frame(shN, dpdu)
    nl = F(2) * c - F(1)
    n2 = normalize(to_world(base, nl))
    return shading_frame(n2, dpdu)


def lookup(rgb, uv, **kw):
    """the map's value at the hits' uv: texture_ref.bitmap"""
    return T.bitmap(rgb, uv, **kw)


def wrong_side(wo_world, shN, wo_local_z):
    """the hemisphere rule: True where the direction evaluates to zero / a sample is rejected"""
    return dot(np.asarray(wo_world, F), np.asarray(shN, F)) * np.asarray(wo_local_z, F) <= 0
