"""The doom probe (pg_layout.h "Doom probe"): a doomed extension ray -- its next vertex has already lost its roulette
or its depth test -- matters only if its closest hit is an emitter triangle.  The shader slab-tests it against padded
boxes over the emitter triangles; a ray that misses them all is not traced but probed: an any-hit walk of the same
4-wide nodes that only decides `culled` against `escaped`.  A probed ray could not have reached an emitter and the
any-hit walk agrees with the closest-hit walk on whether anything is hit, so films, sums of squares, SD-trees and
the path statistics are bit-identical with PG_NO_DOOM_PROBE=1, which sends every doomed ray through the closest-hit
walk as before.  Scenes: the Cornell box (open front: probes escape; the light is on the ceiling: some doomed rays
pass its box and are traced), the ajar door (emitter out of sight: nearly every doomed ray is probed), a Cornell box
with a second emitter mesh (two boxes).  Every probing run must probe something and every switched-off run nothing,
so the comparison cannot pass on an idle switch.  With an environment emitter the shortcut stays off: an escaping
doomed ray picks up environment radiance there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTED = ("segments", "escaped", "shadow_rays", "records", "culled")

VARIANTS = {
    "default": ({}, ()),
    "rr1": ({"rrDepth": 1}, ()),
    "maxdepth2": ({"maxDepth": 2}, ()),
    "maxdepth4": ({"maxDepth": 4}, ()),
    "notail": ({"tailPaths": -1}, ()),
    "alltail": ({"tailPaths": 1 << 30}, ()),
    "norays": ({}, ("PG_NO_RAYS_FUSION",)),
    "noshade": ({}, ("PG_NO_SHADE_FUSION",)),
}


def _scene(S, name):
    if name == "cornell":
        return S.cornell(96, 96)
    if name == "ajar":
        return S.ajar_door(160, 90)
    # a second emitter mesh: a small panel on the back wall, facing the camera
    sc = S.cornell(96, 96)
    V, F = S.quad((1.0, 1.0, 5.58), (1.6, 1.0, 5.58), (1.6, 1.5, 5.58), (1.0, 1.5, 5.58), facing=(0, 0, -1))
    sc.add_mesh(V, F, material=3, radiance=(4.0, 6.0, 9.0))
    return sc.finalize()


def _guided(pg, sc, props):
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer
    t = GuidedPathTracer(dict({"trainingIterations": 4, "sTreeThreshold": 400.0}, **props))
    t.preprocess(sc)
    rgbw, sq = t.render(16)
    tree = t.dev.get_sdtree()
    st = t.postprocess()
    return rgbw, sq, tree, st


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("scene", ["cornell", "ajar", "cornell2"])
def test_probe_is_bit_identical(pg, monkeypatch, scene, variant):
    sc = _scene(pg.scenes, scene)
    props, env = VARIANTS[variant]
    for name in env:
        monkeypatch.setenv(name, "1")
    monkeypatch.delenv("PG_NO_PATH_CULL", raising=False)
    monkeypatch.delenv("PG_NO_DOOM_PROBE", raising=False)
    on = _guided(pg, sc, props)
    monkeypatch.setenv("PG_NO_DOOM_PROBE", "1")
    off = _guided(pg, sc, props)
    print(scene, variant, "probes", on[3]["probes"], "culled", on[3]["culled"], "escaped", on[3]["escaped"], "of",
          on[3]["segments"], "segments")
    assert on[3]["probes"] > 0
    assert off[3]["probes"] == 0
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(on[2], off[2])
    for k in COUNTED:
        assert on[3][k] == off[3][k], k


def test_no_probe_without_path_cull(pg, monkeypatch):
    """PG_NO_PATH_CULL=1 implies PG_NO_DOOM_PROBE=1: without doomed rays there is nothing to probe."""
    monkeypatch.delenv("PG_NO_DOOM_PROBE", raising=False)
    monkeypatch.setenv("PG_NO_PATH_CULL", "1")
    st = _guided(pg, pg.scenes.cornell(96, 96), {})[3]
    assert st["probes"] == 0 and st["culled"] == 0


def test_no_probe_with_environment_emitter(pg, monkeypatch):
    monkeypatch.delenv("PG_NO_PATH_CULL", raising=False)
    monkeypatch.delenv("PG_NO_DOOM_PROBE", raising=False)
    S = pg.scenes
    st = _guided(pg, S.sky_courtyard(64, 48, env=S.sky_envmap(128, 64, sun_radiance=20.0)), {})[3]
    assert st["culled"] > 0  # doomed rays exist, and all of them are traced
    assert st["probes"] == 0
