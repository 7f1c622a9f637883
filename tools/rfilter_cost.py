#!/usr/bin/env python3
"""Cost of the filtered film on the flagship job's final render (C3: guided ajar door, 1280 x 720, 1024 spp).

Each run is a fresh context: train (5 iterations), then time one final-render pass.  Variants alternate within a
round: no filter, the gaussian through the LDS tile (k_film_filtered<true>), the gaussian through the direct
variant (PG_FILM_FILTER_DIRECT=1).  Prints one JSON line.  Kernel times per chunk come from running this under
a kernel trace with --rounds 1.

    python tools/rfilter_cost.py [--rounds 3] [--spp 1024] [--width 1280 --height 720]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--train", type=int, default=5)
    a = ap.parse_args()
    import pgload
    pg = pgload.load()
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer
    sc = pg.scenes.ajar_door(a.width, a.height)
    variants = [("none", None, None), ("lds", "gaussian", "0"), ("direct", "gaussian", "1")]
    out = {v[0]: [] for v in variants}
    for _ in range(a.rounds):
        for name, rf, direct in variants:
            if direct is None:
                os.environ.pop("PG_FILM_FILTER_DIRECT", None)
            else:
                os.environ["PG_FILM_FILTER_DIRECT"] = direct
            props = {"trainingIterations": a.train}
            if rf:
                props["rfilter"] = rf
            t = GuidedPathTracer(props)
            t.preprocess(sc)
            t.train()
            t.dev.reset_film()
            t0 = time.perf_counter()
            t.dev.render_pass(a.spp, t.sample_offset)
            dt = time.perf_counter() - t0
            if rf:
                w = t.dev.read_film_filtered()[..., 3]
                assert abs(float(w.mean()) / a.spp - 1) < 0.05, w.mean()
            t.postprocess()
            out[name].append(round(a.width * a.height * a.spp / dt / 1e6, 2))
    print(json.dumps({"job": f"ajar_door {a.width}x{a.height} final render {a.spp} spp", "mpaths_per_s": out}))


if __name__ == "__main__":
    main()
