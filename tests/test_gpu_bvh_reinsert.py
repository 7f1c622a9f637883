"""Results on the GPU do not depend on the tree: the builder's reinsertion pass on (the default) against
PG_BVH_REINSERT=0, each in a child process of its own (the switch is read when the scene is uploaded).

Cornell box and ajar door at 64 x 36, guided, one training iteration (1 spp, recorded, splatted, refitted) and an
8 spp pass, with the tail kernel off, at its default and forced: films and sums of squares equal element for element,
SD-trees byte-equal, the counters equal and the training records equal after sorting.  On the ajar door 20 000 rays
through pg_trace_rays, closest hit and any hit: equal between the two trees (t, original triangle id, u, v), and
agreeing with the oracle on every consistent ray."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAILS = {"off": -1, "default": 0, "forced": 1 << 30}
COUNTERS = ("segments", "escaped", "shadow_rays", "records", "culled")


def make_scene(pg, name):
    return pg.scenes.cornell(64, 36) if name == "cornell" else pg.scenes.ajar_door(64, 36)


def unit_rays(scene, n=20000, seed=5):
    rng = np.random.default_rng(seed)
    lo, hi = scene.bounds()
    d = rng.normal(size=(n, 3))
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 7] = lo + (hi - lo) * rng.random((n, 3)), 1e-5, np.inf  # not 1e-4: the oracle scales that one by max |o|
    r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return r


def worker(name, tail, out):
    sys.path[:0] = [ROOT]
    import pgload
    pg = pgload.load()
    from mitsuba_path_guiding_amd.integrator import Device
    sc = make_scene(pg, name)
    dev = Device(pg.capi.default_config(guiding=1, tail_paths=TAILS[tail]))
    dev.upload(sc)
    dev.render_pass(1, 0, record=True)
    recs = np.array(dev.get_records()).reshape(-1, 32)
    dev.splat_local()
    dev.refit(0)
    dev.reset_film()
    dev.render_pass(8, 1)
    rgbw, sq = dev.read_film()
    st = dev.stats()
    res = dict(rgbw=rgbw, sq=sq, tree=np.frombuffer(bytes(dev.get_sdtree()), np.uint8),
               recs=recs[np.lexsort(recs.T[::-1])], counters=np.array([st[k] for k in COUNTERS], np.uint64))
    if name == "ajar" and tail == "default":
        rays = unit_rays(sc)
        res["closest"] = dev.trace_rays(rays)
        res["any"] = dev.trace_rays(rays, any_hit=True)
    dev.close()
    np.savez(out, **res)


def run(tmp_path, name, tail, mode):
    out = str(tmp_path / f"{name}_{tail}_{mode}.npz")
    env = dict(os.environ, PG_BVH_REINSERT=str(mode))
    subprocess.run([sys.executable, os.path.abspath(__file__), name, tail, out], check=True, env=env, timeout=120)
    return dict(np.load(out))


@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("name", ["cornell", "ajar"])
def test_results_do_not_depend_on_the_tree(pg, tmp_path, name, tail):
    on, off = run(tmp_path, name, tail, 1), run(tmp_path, name, tail, 0)
    print(name, tail, dict(zip(COUNTERS, on["counters"])), "records", len(on["recs"]))
    assert on["rgbw"][..., 3].sum() == 64 * 36 * 8 and len(on["recs"]) > 1000
    for k in ("rgbw", "sq", "tree", "counters", "recs"):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    if "closest" in on:
        np.testing.assert_array_equal(on["closest"].view(np.uint32), off["closest"].view(np.uint32))
        np.testing.assert_array_equal(on["any"], off["any"])


def test_ajar_unit_rays_agree_with_oracle(pg, O, tmp_path):
    """pg_trace_rays on the optimised tree, closest hit and any hit, against the oracle with the rule of
    test_gpu_parity.test_trace_matches_bruteforce: every ray whose hit lies inside its triangle's own box
    (test_bvh4_build.consistent_hits, for the oracle's hit and for the device's) agrees -- the triangle, and t / u / v
    bit for bit; the excluded share stays under test_bvh8_build's cap."""
    import test_bvh4_build as T
    import test_bvh8_build as W
    on = run(tmp_path, "ajar", "default", 1)
    sc = make_scene(pg, "ajar")
    V, F = sc.positions.reshape(-1, 3), sc.indices.reshape(-1, 3)
    rays = unit_rays(sc)
    osc = O.OracleScene(pg.capi, sc)
    c, oc = osc.trace(rays), osc.trace(rays, any_hit=True)
    g = on["closest"]
    gp, cp = g[:, 1].view(np.uint32), c[:, 1].view(np.uint32)
    ok = T.consistent_hits(V, F, rays, cp, c[:, 0]) & T.consistent_hits(V, F, rays, gp, g[:, 0])
    occ, oocc = on["any"][:, 0] > 0.5, oc[:, 0] > 0.5
    print(f"closest: {int((gp != cp).sum())} of {len(rays)} triangles differ from the oracle's ({int((gp != cp)[ok].sum())} "
          f"on consistent rays), {int((gp != 0xFFFFFFFF).sum())} hit, {int((~ok).sum())} rays excluded; any hit: "
          f"{int((occ != oocc).sum())} differ ({int((occ != oocc)[ok].sum())} on consistent rays)")
    assert (gp != 0xFFFFFFFF).mean() > 0.5
    assert (~ok).mean() < W.EXCLUDED_CAP
    np.testing.assert_array_equal(gp[ok], cp[ok])
    hit = (gp == cp) & (gp != 0xFFFFFFFF)
    np.testing.assert_array_equal(g[hit][:, [0, 2, 3]], c[hit][:, [0, 2, 3]])
    np.testing.assert_array_equal(occ[ok], oocc[ok])


if __name__ == "__main__":
    worker(*sys.argv[1:4])
