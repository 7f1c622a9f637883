"""Cost of the thin lens on the flagship scene: C3 (ajar door, 1280 x 720, guided) with the lens off and with a lens
of radius 1 % of the scene's diagonal focused on the door.  Prints Mpaths/s of the final render and, with
kernel_timing, the split pg_stats keeps (trace_ms = the camera rays' k_trace, rays_ms = k_rays, shade_ms =
k_shade_all).  k_camera has no timer in pg_stats: its cost shows only in the Mpaths/s."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pgload

pg = pgload.load()
from mitsuba_path_guiding_amd.integrator import Device

SPP = int(sys.argv[1]) if len(sys.argv) > 1 else 64
DOOR = np.array([5.0, 1.1, 2.5])  # the doorway's centre (scenes.ajar_door)


def run(lens, timing):
    sc = pg.scenes.ajar_door(1280, 720)
    lo, hi = sc.bounds()
    o, t = np.array(list(sc.camera.origin)), np.array(list(sc.camera.target))
    fwd = (t - o) / np.linalg.norm(t - o)
    radius, focus = 0.01 * float(np.linalg.norm(hi - lo)), float(np.dot(DOOR - o, fwd))
    d = Device(pg.capi.default_config(guiding=1, kernel_timing=timing))
    d.upload(sc)
    if lens:
        d.set_lens(radius, focus)
    off = 0
    for it in range(5):
        d.render_pass(2 ** it, off, True)
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    d.reset_film()
    s0 = d.stats()
    t0 = time.perf_counter()
    d.render_pass(SPP, off)
    dt = time.perf_counter() - t0
    s1 = d.stats()
    d.close()
    out = {"lens": [round(radius, 4), round(focus, 4)] if lens else None, "kernel_timing": timing, "spp": SPP,
           "Mpaths_per_s": round(1280 * 720 * SPP / dt / 1e6, 1), "segments": s1["segments"] - s0["segments"]}
    if timing:
        out.update({k: round(s1[k] - s0[k], 1) for k in ("trace_ms", "rays_ms", "shade_ms")})
    return out


for timing in (0, 1):
    for lens in (False, True):
        print(json.dumps(run(lens, timing)), flush=True)
