"""The paired path-state records (pg_layout.h "Path state"): a slot's ray origin and direction rows are the halves of
one 32-B record of PathDev::ray, and its info and throughput rows the halves of one of PathDev::vst.

What an interleaved layout can get wrong that the other files' sizes do not reach:

  - a stride or end-of-buffer mistake at the last slot of a chunk: the Cornell box at 37 x 29 pixels, 1073 slots per
    sample layer, no multiple of 64 or of the 128- and 256-thread blocks;
  - chunk and lane reuse: the same job with maxPathsInFlight = 2048 on three lanes and on one (several chunks per
    lane, so a camera row is written next to the throughput half a previous chunk left in the record) and as one
    chunk per pass;
  - every launch variant at that size, and a scene under an environment emitter at 45 x 35 (envEscapeRadiance reads
    the vst record from the tracer; shading runs per class).

Films, sums of squares, SD-trees and counters must be equal element for element among all runs that share integrator
properties.  So that equal-but-wrong cannot pass, the default variant is held against the oracle on the same streams:
its final render with the GPU-trained tree (bars of tests/test_gpu_parity.py test_guided_training_parity: |z| < 5 on
more than 99.5 % of the values, image means within 1 %) and one recording pass (tests/record_parity.py with the bars
of tests/test_gpu_records.py: counts within 0.1 %, >= 99 % matched, >= 99 % of the pairs in every field bar).  No
Cornell case can pass idle: segments > 3 x paths and shadow_rays > 0."""
import numpy as np
import pytest

import record_parity as R

pytestmark = pytest.mark.gpu

THREADS = 16
COUNTED = ("segments", "escaped", "shadow_rays", "records", "culled")
MATCH_BAR = IN_BAR = 0.99  # tests/test_gpu_records.py
SPP = 5
ITERATIONS = 3  # training passes of 1, 2 and 4 spp

# (integrator properties, environment switches)
VARIANTS = {
    "default": ({}, ()),
    "norays": ({}, ("PG_NO_RAYS_FUSION",)),
    "noshade": ({}, ("PG_NO_SHADE_FUSION",)),
    "notail": ({"tailPaths": -1}, ()),
    "alltail": ({"tailPaths": 1 << 30}, ()),
    "noprobe": ({}, ("PG_NO_DOOM_PROBE",)),
    "nocull": ({}, ("PG_NO_PATH_CULL",)),
}
SWITCHES = ("PG_NO_RAYS_FUSION", "PG_NO_SHADE_FUSION", "PG_NO_DOOM_PROBE", "PG_NO_PATH_CULL")
# the same job cut three ways (one lane and the default chunk size: every pass is one chunk)
CHUNKINGS = {
    "one": {"pathLanes": 1},
    "small3": {"maxPathsInFlight": 2048, "pathLanes": 3},
    "small1": {"maxPathsInFlight": 2048, "pathLanes": 1},
}

_scenes, _runs = {}, {}


def scene(pg, name):
    if name not in _scenes:
        S = pg.scenes
        if name == "sky":
            _scenes[name] = S.sky_courtyard(45, 35, env=S.sky_envmap(128, 64, sun_radiance=20.0))
        else:
            _scenes[name] = S.cornell(37, 29)
    return _scenes[name]


def _guided(pg, sc, props):
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer
    t = GuidedPathTracer(dict({"trainingIterations": ITERATIONS, "sTreeThreshold": 400.0}, **props))
    t.preprocess(sc)
    rgbw, sq = t.render(SPP)
    tree = t.dev.get_sdtree()
    off = t.sample_offset - SPP
    cfg = t.cfg
    st = t.postprocess()
    return rgbw, sq, tree, st, off, cfg


def run(pg, monkeypatch, name, props, env=()):
    """One guided job of a scene (3 training iterations, a 5-spp render), computed once per setting."""
    key = (name, tuple(sorted(props.items())), tuple(env))
    if key not in _runs:
        for s in SWITCHES:
            monkeypatch.delenv(s, raising=False)
        for s in env:
            monkeypatch.setenv(s, "1")
        _runs[key] = _guided(pg, scene(pg, name), props)
    return _runs[key]


def assert_equal_runs(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])
    for k in COUNTED:
        assert a[3][k] == b[3][k], k


def assert_not_idle(st):
    assert st["segments"] > 3 * st["paths"] and st["shadow_rays"] > 0, st


def test_awkward_slot_count_runs(pg, monkeypatch):
    sc = scene(pg, "cornell")
    assert sc.width * sc.height == 1073 and 1073 % 64 and 1073 % 128
    st = run(pg, monkeypatch, "cornell", {}, ())[3]
    print({k: st[k] for k in COUNTED}, "paths", st["paths"])
    assert st["paths"] == 1073 * (1 + 2 + 4 + SPP)
    assert st["records"] > 0
    assert_not_idle(st)


@pytest.mark.parametrize("chunking", ["small3", "small1"])
def test_chunk_and_lane_reuse(pg, monkeypatch, chunking):
    one = run(pg, monkeypatch, "cornell", CHUNKINGS["one"], ())
    got = run(pg, monkeypatch, "cornell", CHUNKINGS[chunking], ())
    # a chunk ends with at most one k_tail launch, so the launches count chunks from below; the one-chunk setting
    # has one per pass (the render is a pass per sample layer here)
    print(chunking, "k_tail launches", got[3]["tail_launches"], "one chunk per pass:", one[3]["tail_launches"])
    assert 1 <= one[3]["tail_launches"] <= ITERATIONS + SPP
    assert got[3]["tail_launches"] - one[3]["tail_launches"] > 3
    assert_not_idle(got[3])
    assert_equal_runs(got, one)
    assert_equal_runs(got, run(pg, monkeypatch, "cornell", {}, ()))  # the default: one chunk per lane


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants_agree(pg, monkeypatch, variant):
    props, env = VARIANTS[variant]
    got = run(pg, monkeypatch, "cornell", props, env)
    st = got[3]
    print(variant, {k: st[k] for k in COUNTED}, "tail launches", st["tail_launches"])
    assert_not_idle(st)
    if variant == "notail":
        assert st["tail_launches"] == 0
    if variant == "alltail":
        assert st["tail_launches"] > 0
    ref = run(pg, monkeypatch, "cornell", {}, ())
    if variant == "nocull":
        # without PF_DOOMED no hit is culled in the tracer; everything a path computes is the same
        assert st["culled"] == 0 and ref[3]["culled"] > 0
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        for k in ("segments", "escaped", "shadow_rays", "records"):
            assert st[k] == ref[3][k], k
        return
    assert_equal_runs(got, ref)


@pytest.mark.parametrize("variant", ["norays", "noshade", "alltail"])
def test_environment_emitter_variants_agree(pg, monkeypatch, variant):
    props, env = VARIANTS[variant]
    got = run(pg, monkeypatch, "sky", props, env)
    st = got[3]
    print("sky", variant, {k: st[k] for k in COUNTED})
    assert st["segments"] > st["paths"] and st["escaped"] > 0 and st["records"] > 0
    assert_equal_runs(got, run(pg, monkeypatch, "sky", {}, ()))


def _zstats(g, c):  # tests/test_gpu_parity.py
    n1 = np.maximum(g[0][..., 3:4], 1)
    n2 = np.maximum(c[0][..., 3:4], 1)
    m1, m2 = g[0][..., :3] / n1, c[0][..., :3] / n2
    v1 = np.maximum(g[1][..., :3] / n1 - m1 ** 2, 0) / n1
    v2 = np.maximum(c[1][..., :3] / n2 - m2 ** 2, 0) / n2
    z = (m1 - m2) / np.sqrt(v1 + v2 + 1e-12)
    return m1, m2, z


def test_final_render_matches_oracle_with_the_same_tree(pg, O, monkeypatch):
    rgbw, sq, blob, st, off, cfg = run(pg, monkeypatch, "cornell", {}, ())
    osc = O.OracleScene(pg.capi, scene(pg, "cornell"))
    tree = O.OracleSDTree(osc)
    tree.deserialize(blob)
    c = O.render(osc, cfg, SPP, sample_offset=off, sdtree=tree, nthreads=THREADS)[:2]
    assert np.array_equal(rgbw[..., 3], c[0][..., 3])  # same accepted-sample counts
    m1, m2, z = _zstats((rgbw, sq), c)
    print("|z| < 5:", (np.abs(z) < 5).mean(), "means", m1.mean(), m2.mean())
    assert (np.abs(z) < 5).mean() > 0.995
    assert abs(m1.mean() - m2.mean()) / m2.mean() < 0.01


def test_records_match_oracle(pg, O):
    from mitsuba_path_guiding_amd.integrator import Device
    sc = scene(pg, "cornell")
    lo, hi = (np.asarray(b, np.float64) for b in sc.bounds())
    extent = float((hi - lo).max())
    osc = O.OracleScene(pg.capi, sc)
    cfg = pg.capi.default_config(guiding=1, s_tree_threshold=400.0)
    tree, off = R.train_oracle_tree(O, osc, cfg, nthreads=THREADS)
    blob = tree.serialize()
    ref = R.oracle_records(pg.capi, O, osc, cfg, tree, off, nthreads=THREADS)
    assert len(ref) >= 2000
    dev = Device(pg.capi.default_config(guiding=1, s_tree_threshold=400.0))
    dev.upload(sc)
    dev.put_sdtree(blob)
    dev.render_pass(R.PASS_SPP, off, record=True)
    got = R.as_records(dev.get_records())
    dev.close()
    c = R.compare(ref, got, extent)
    print(c.summary("records cornell 37 x 29"))
    assert c.count_ok, (len(got), len(ref))
    assert c.matched_share >= MATCH_BAR, c.matched_share
    assert c.in_bar_share >= IN_BAR, (c.in_bar_share, c.fail)
