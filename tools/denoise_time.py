"""One pg_denoise of a 1280 x 720 C3 (ajar door) film: device time from events around the launches, three runs each,
gather and LDS-tiled variants alternating (PG_DENOISE_TILED is read per call), and the two variants' bits compared."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgload

pg = pgload.load()
from mitsuba_path_guiding_amd.integrator import Device

sc = pg.scenes.ajar_door(1280, 720)
d = Device(pg.capi.default_config(aovs=1))
d.upload(sc)
d.render_pass(16, 0)
outs = {}
for tiled in ("0", "1"):  # warm-up of both
    os.environ["PG_DENOISE_TILED"] = tiled
    outs[tiled] = d.denoise()
for run in range(3):
    for tiled in ("0", "1"):
        os.environ["PG_DENOISE_TILED"] = tiled
        for levels in (5,):
            o = d.denoise({"levels": levels})
            print(f"run {run} tiled {tiled} levels {levels}: {d.denoise_ms():.3f} ms", flush=True)
            assert np.array_equal(o, outs[tiled])
print("variants bit-equal:", np.array_equal(outs["0"], outs["1"]))
for levels in (1, 2, 3):
    for tiled in ("0", "1"):
        os.environ["PG_DENOISE_TILED"] = tiled
        d.denoise({"levels": levels})
        print(f"tiled {tiled} levels {levels}: {d.denoise_ms():.3f} ms", flush=True)
film = d.read_film()[0]
print("valid pixels", int((film[..., 3] > 0).sum()), "of", film.shape[0] * film.shape[1])
d.close()
