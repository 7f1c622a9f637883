"""numpy restatement of the device's emitter sampling ("Delta emitters"; pg_capi.h
pg_set_delta_emitters), in the role camera_ref.py has for the cameras.

What pg_set_delta_emitters precomputes on the host in float32 (the normalised direction, the bounding sphere of the
uploaded triangles' box, a directional light's disk centre, a spot's cosines and 1 / (cutoff - beam)) is restated in
float32, in the same order; everything the device computes per sample is restated in float64, so the comparison
measures the device's float32 error.  Tests only."""
import numpy as np

F = np.float32
POINT, SPOT, DIRECTIONAL = 0, 1, 2


def bounding_sphere(positions):
    """centre and 1.1 x half diagonal of the box over `positions` (n, 3) float32, as pgh::boxSphere (float32)"""
    p = np.asarray(positions, F).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    c = (lo + hi) * F(0.5)
    d = hi - c
    r2 = F(0)
    for a in range(3):
        r2 = F(r2 + F(d[a] * d[a]))
    return c, F(np.sqrt(r2) * F(1.1))


def records(delta_emitters, positions):
    """the device records of pg_delta_emitter structs, as dicts of float64 values holding the host's float32 results"""
    centre, radius = bounding_sphere(positions)
    out = []
    for e in delta_emitters:
        r = dict(type=int(e.type), intensity=np.array(list(e.intensity), F).astype(np.float64))
        d = np.array(list(e.direction), F)
        if r["type"] != POINT:
            l = F(np.sqrt(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))))
            d = (d / l).astype(F)
        r["dir"] = d.astype(np.float64)
        if r["type"] == DIRECTIONAL:
            r["pos"] = (centre - (d * radius).astype(F)).astype(F).astype(np.float64)
        else:
            r["pos"] = np.array(list(e.position), F).astype(np.float64)
        if r["type"] == SPOT:
            cutoff, beam = F(e.cutoff_angle), F(e.beam_width)
            r["cutoff"] = float(cutoff)
            r["cos_cutoff"] = float(F(np.cos(np.float64(cutoff))))
            r["cos_beam"] = float(F(np.cos(np.float64(beam))))
            r["inv_transition"] = float(F(1) / F(cutoff - beam))
        out.append(r)
    return out


def sample_delta(rec, ref):
    """one delta emitter at reference points ref (n, 3): d (n, 3), dist (n), value (n, 3) -- the emitter-pick
    probability not divided out -- and ok (n): False where the sample fails (its value is then 0)"""
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    n = len(ref)
    I = rec["intensity"]
    if rec["type"] == DIRECTIONAL:
        dist = (ref - rec["pos"]) @ rec["dir"]
        ok = dist >= 0
        d = np.broadcast_to(-rec["dir"], (n, 3)).copy()
        value = np.broadcast_to(I, (n, 3)).copy()
    else:
        v = rec["pos"] - ref
        dist = np.sqrt((v * v).sum(1))
        d = v / dist[:, None]
        value = I[None, :] / (dist * dist)[:, None]
        ok = np.ones(n, bool)
        if rec["type"] == SPOT:
            cos_theta = -(d @ rec["dir"])
            ramp = (rec["cutoff"] - np.arccos(np.clip(cos_theta, -1, 1))) * rec["inv_transition"]
            factor = np.where(cos_theta <= rec["cos_cutoff"], 0.0, np.where(cos_theta >= rec["cos_beam"], 1.0, ramp))
            value = value * factor[:, None]
    ok = ok & (value.max(1) > 0)
    value = np.where(ok[:, None], value, 0.0)
    return np.where(ok[:, None], d, 0.0), np.where(ok, dist, 0.0), value, ok


def area_emitter(scene, emitter):
    """the triangles (k, 3, 3), area CDF (float32, as pg_upload_scene builds it), 1 / area and radiance of area
    emitter `emitter` of a finalized scenes.Scene with flat-shaded emitter meshes"""
    e = scene.emitters[emitter]
    sh = scene.shapes[e.shape]
    tri = scene.positions[scene.indices[sh.tri_begin:sh.tri_begin + sh.tri_count]].astype(F)
    u, v = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    x = np.stack([F(u[:, 1] * v[:, 2]) - F(u[:, 2] * v[:, 1]), F(u[:, 2] * v[:, 0]) - F(u[:, 0] * v[:, 2]),
                  F(u[:, 0] * v[:, 1]) - F(u[:, 1] * v[:, 0])], 1).astype(F)
    area = (F(0.5) * np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(F) + x[:, 2] * x[:, 2]).astype(F)).astype(F)
    cum = np.concatenate([[0.0], np.cumsum(area.astype(np.float64))])
    cdf = (cum / cum[-1]).astype(F)
    cdf[-1] = F(1)
    return dict(tri=tri.astype(np.float64), cdf=cdf.astype(np.float64), inv_area=float(F(1) / F(cum[-1])),
                radiance=np.array(list(e.radiance)[:3], np.float64))


def sample_area(em, ref, sx, sy):
    """sampleEmitter's area branch with a zero reference normal (area.cpp:158-171, triangle.cpp:24-45): d, dist,
    value = radiance / pdf (solid angle), ok"""
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    cdf, k = em["cdf"], len(em["tri"])
    idx = np.clip(np.searchsorted(cdf, sy, side="left") - 1, 0, k - 1)
    sy = (sy - cdf[idx]) / (cdf[idx + 1] - cdf[idx])
    t = em["tri"][idx]
    a = np.sqrt(np.maximum(1 - sx, 0))
    p = t[:, 0] + (t[:, 1] - t[:, 0]) * (1 - a)[:, None] + (t[:, 2] - t[:, 0]) * (a * sy)[:, None]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    v = p - ref
    dist = np.sqrt((v * v).sum(1))
    d = v / dist[:, None]
    cos = (d * nrm).sum(1)
    ok = cos < 0
    pdf = em["inv_area"] * dist * dist / np.maximum(np.abs(cos), 1e-300)
    value = np.where(ok[:, None], em["radiance"][None, :] / pdf[:, None], 0.0)
    return np.where(ok[:, None], d, 0.0), np.where(ok, dist, 0.0), value, ok


def sample_emitter(area, deltas, ref, samples):
    """Scene::sampleEmitterDirect over area emitters (area_emitter records) then delta emitters (records): the pick
    ei = min((uint32)(sx ne), ne - 1) in float32, then the emitter's sample.  Returns the picked emitter (n) and
    (n, 8): d, dist, value / pdf with the pick probability divided out, measure (0 failed, 1 solid angle, 2 discrete)"""
    ref = np.asarray(ref, F).reshape(-1, 3)
    s = np.asarray(samples, F).reshape(-1, 2)
    ne = len(area) + len(deltas)
    scaled = (s[:, 0] * F(ne)).astype(F)
    ei = np.minimum(scaled.astype(np.uint32), ne - 1)
    sx = (scaled - ei.astype(F)).astype(F).astype(np.float64)
    out = np.zeros((len(ref), 8))
    for e in range(ne):
        m = ei == e
        if not m.any():
            continue
        if e < len(area):
            d, dist, value, ok = sample_area(area[e], ref[m], sx[m], s[m, 1].astype(np.float64))
            flag = 1.0
        else:
            d, dist, value, ok = sample_delta(deltas[e - len(area)], ref[m])
            flag = 2.0
        out[m, :3], out[m, 3], out[m, 4:7], out[m, 7] = d, dist, value * ne, np.where(ok, flag, 0.0)
    return ei, out
