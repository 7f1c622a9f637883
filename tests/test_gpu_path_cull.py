"""The path cull (pg_layout.h PF_DOOMED): the shader that writes an extension ray already decides whether the
next vertex can do anything -- it makes that vertex's Russian-roulette draw and depth tests -- and the
closest-hit kernels drop a doomed ray that hits a non-emitter instead of queueing it for shading.  A culled
vertex would have added nothing, so films, sums of squares, SD-trees and the path statistics are
bit-identical with PG_NO_PATH_CULL=1, which sends every vertex through the shader as before: default
integrator, roulette from the second vertex on (culls in every launch), a last vertex doomed by maxDepth,
the per-bounce launches and the k_tail loop, and the unfused launches.  Every culled run must cull
something and every switched-off run nothing, so the comparison cannot pass on an idle switch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTED = ("segments", "escaped", "shadow_rays", "records")

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


def _guided(pg, sc, props):
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer
    t = GuidedPathTracer(dict({"trainingIterations": 4, "sTreeThreshold": 400.0}, **props))
    t.preprocess(sc)
    rgbw, sq = t.render(16)
    tree = t.dev.get_sdtree()
    st = t.postprocess()
    return rgbw, sq, tree, st


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("scene", ["cornell", "envmap"])
def test_cull_is_bit_identical(pg, monkeypatch, scene, variant):
    S = pg.scenes
    sc = S.cornell(96, 96) if scene == "cornell" else S.sky_courtyard(64, 48, env=S.sky_envmap(128, 64, sun_radiance=20.0))
    props, env = VARIANTS[variant]
    for name in env:
        monkeypatch.setenv(name, "1")
    monkeypatch.delenv("PG_NO_PATH_CULL", raising=False)
    on = _guided(pg, sc, props)
    monkeypatch.setenv("PG_NO_PATH_CULL", "1")
    off = _guided(pg, sc, props)
    print(scene, variant, "culled", on[3]["culled"], "of", on[3]["segments"] - on[3]["escaped"], "hits")
    assert on[3]["culled"] > 0
    assert off[3]["culled"] == 0
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(on[2], off[2])
    for k in COUNTED:
        assert on[3][k] == off[3][k], k
