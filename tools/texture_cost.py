"""Cost of textures on the flagship scene: C3 (ajar door, 1280 x 720, guided) with its wall, floor and door materials
bound to 256 x 256 bilinear bitmaps against the same scene with constant reflectances equal to the bitmaps' averages.
Prints Mpaths/s of the final render and the kernel_timing split (shade_ms = k_shade_all, rays_ms = k_rays)."""
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


def run(textured, timing):
    sc = pg.scenes.ajar_door(1280, 720)
    rng = np.random.default_rng(1)
    tc = rng.uniform(0, 8, (sc.desc().num_vertices, 2)).astype(np.float32)
    for m in (0, 1, 2):  # walls, floor, door
        c = np.array(list(sc.materials[m].diffuse_reflectance)[:3], np.float32)
        rgb = (c * rng.uniform(0.5, 1.5, (256, 256, 1))).astype(np.float32)
        if textured:
            sc.bind_texture(m, sc.add_texture("bitmap", rgb, filter="bilinear", wrap="repeat"))
        else:
            sc.materials[m].diffuse_reflectance = pg.scenes._f4(rgb.reshape(-1, 3).mean(0, dtype=np.float64).tolist() + [0.0])
    sc.finalize()
    d = Device(pg.capi.default_config(guiding=1, kernel_timing=timing))
    d.upload(sc)
    if textured:
        d.set_textures(sc.textures, sc.texture_bindings, tc)
    off = 0
    for it in range(5):
        d.render_pass(2 ** it, off, True)
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    d.reset_film()
    s0 = d.stats()
    t = time.perf_counter()
    d.render_pass(SPP, off)
    dt = time.perf_counter() - t
    s1 = d.stats()
    d.close()
    out = {"textured": textured, "kernel_timing": timing, "spp": SPP, "Mpaths_per_s": round(1280 * 720 * SPP / dt / 1e6, 1)}
    if timing:
        out.update({k: round(s1[k] - s0[k], 1) for k in ("shade_ms", "rays_ms", "trace_ms")})
    return out


for timing in (0, 1):
    for textured in (False, True):
        print(json.dumps(run(textured, timing)), flush=True)
