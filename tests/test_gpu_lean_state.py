"""The lean per-bounce path state (pg_layout.h "Path state"): the `prev` array is gone -- a bounce ray keeps woPdf in
ray_d.w, where the tracers used to load a stored +inf as tmax, and PF_PREV_FRONT replaces the stored reference normal
-- and the shader loads L only where it uses it.

Every consumer of the moved fields is reached: bounce rays that land on the ceiling light after a diffuse, a delta
(PF_PREV_DELTA) and a rough-dielectric (refN = 0) vertex; an emitter quad standing free inside the box, reached from
its front and from its back (the two outcomes of PF_PREV_FRONT and of dot(rd, shN) < 0); and a scene under an
environment emitter (envEscapeRadiance, the per-class shading launches).  Each scene runs under the launch variants
that read the new rows separately -- fused k_rays, the unfused launches with k_probe, k_shade_all and the
per-class launches, the per-bounce launches alone, k_tail from the first bounce, doomed rays traced instead of probed
-- and all variants that share integrator properties must give equal films, sums of squares, SD-trees and counters.

The default variant is also held against the oracle on the same streams: its final render, with the tree the GPU
trained, against the oracle rendering the same pixels and samples with that tree (the z-score comparison and bars of
tests/test_gpu_parity.py test_guided_training_parity: |z| < 5 on more than 99.5 % of the values, image means within
1 %), and a recording pass against the oracle's records (tests/record_parity.py with the bars of
tests/test_gpu_records.py: counts within 0.1 %, >= 99 % matched, >= 99 % of the pairs in every field bar).

No case can pass idle: the oracle's own paths for the first two samples of every pixel (path_rays, no GPU involved)
must hold bounce rays that end on an emitter right after a vertex on one of the blocks (which carry the case's
material), and in the quad scene bounce rays that reach the quad from either side."""
import numpy as np
import pytest

import record_parity as R

pytestmark = pytest.mark.gpu

THREADS = 16
COUNTED = ("segments", "escaped", "shadow_rays", "records")
MATCH_BAR = IN_BAR = 0.99  # tests/test_gpu_records.py

# (integrator properties, environment switches)
VARIANTS = {
    "default": ({}, ()),
    "norays": ({}, ("PG_NO_RAYS_FUSION",)),
    "noshade": ({}, ("PG_NO_SHADE_FUSION",)),
    "notail": ({"tailPaths": -1}, ()),
    "alltail": ({"tailPaths": 1 << 30}, ()),
    "rr1": ({"rrDepth": 1}, ()),
    "maxdepth3": ({"maxDepth": 3}, ()),
    "noprobe": ({}, ("PG_NO_DOOM_PROBE",)),
}
SWITCHES = ("PG_NO_RAYS_FUSION", "PG_NO_SHADE_FUSION", "PG_NO_DOOM_PROBE", "PG_NO_PATH_CULL")
SCENES = ("diffuse", "mirror", "roughglass", "quad", "sky")
# the free-standing emitter quad: upright in the middle of the box, facing the camera (-z)
QUAD = ((1.6, 1.8, 3.0), (3.9, 1.8, 3.0), (3.9, 3.6, 3.0), (1.6, 3.6, 3.0))

_scenes, _runs = {}, {}


def scene(pg, name):
    if name not in _scenes:
        S = pg.scenes
        if name == "sky":
            sc = S.sky_courtyard(64, 48, env=S.sky_envmap(128, 64, sun_radiance=20.0))
        elif name == "mirror":
            m = S.material("conductor")
            sc = S.cornell(96, 96, short_material=m, tall_material=m)
        elif name == "roughglass":
            m = S.material("roughdielectric", alpha=0.3)
            sc = S.cornell(96, 96, short_material=m, tall_material=m)
        else:
            sc = S.cornell(96, 96)
            if name == "quad":
                V, F = S.quad(*QUAD, facing=(0, 0, -1))
                sc.add_mesh(V, F, material=3, radiance=(3.0, 3.0, 3.0))
                sc = sc.finalize()
        _scenes[name] = sc
    return _scenes[name]


def _guided(pg, sc, props):
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer
    t = GuidedPathTracer(dict({"trainingIterations": 4, "sTreeThreshold": 400.0}, **props))
    t.preprocess(sc)
    rgbw, sq = t.render(16)
    tree = t.dev.get_sdtree()
    off = t.sample_offset - 16
    cfg = t.cfg
    st = t.postprocess()
    return rgbw, sq, tree, st, off, cfg


def run(pg, monkeypatch, name, props, env=()):
    """One guided job of a scene (4 training iterations, a 16-spp render), computed once per setting."""
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


def oracle_emitter_arrivals(pg, O, name):
    """From the oracle's own paths (samples 0 and 1 of every pixel, BSDF sampling): the bounce rays that end on an
    emitter triangle, as (count after a vertex on a block, count from the quad's front, count from its back)."""
    sc = scene(pg, name)
    osc = O.OracleScene(pg.capi, sc)
    cfg = pg.capi.default_config()
    tri_em = np.zeros(len(sc.indices), bool)
    for sh in sc.shapes:
        tri_em[sh.tri_begin:sh.tri_begin + sh.tri_count] = sh.emitter >= 0
    # the two blocks are the last two meshes cornell() adds (the quad comes after them)
    blocks = sc.shapes[-3:-1] if name == "quad" else sc.shapes[-2:]
    tri_block = np.zeros(len(sc.indices), bool)
    for sh in blocks:
        tri_block[sh.tri_begin:sh.tri_begin + sh.tri_count] = True
    quad_tris = np.zeros(len(sc.indices), bool)
    if name == "quad":
        sh = sc.shapes[-1]
        quad_tris[sh.tri_begin:sh.tri_begin + sh.tri_count] = True
    after_block = front = back = total = 0
    for pixel in range(sc.width * sc.height):
        for sample in (0, 1):
            rays = osc.path_rays(cfg, None, pixel, sample, max_rays=512)[0]
            closest = rays[rays[:, 0] == 0]
            prim = closest[:, 10].copy().view(np.uint32)
            hit = prim != 0xFFFFFFFF
            for k in range(1, len(closest)):  # bounce rays
                if not hit[k] or not tri_em[prim[k]]:
                    continue
                total += 1
                if hit[k - 1] and tri_block[prim[k - 1]]:
                    after_block += 1
                if quad_tris[prim[k]]:
                    if closest[k, 7] > 0:  # the quad faces -z: a ray travelling +z meets its front
                        front += 1
                    else:
                        back += 1
    return total, after_block, front, back


@pytest.mark.parametrize("name", [s for s in SCENES if s != "sky"])
def test_oracle_paths_reach_the_emitters(pg, O, name):
    """The anti-idle guard, on the CPU alone."""
    total, after_block, front, back = oracle_emitter_arrivals(pg, O, name)
    print(name, "emitter arrivals of bounce rays:", total, "after a block vertex:", after_block, "quad front / back:",
          front, back)
    assert total > 0
    if name == "quad":
        assert front > 0 and back > 0
    else:
        assert after_block > 0


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", SCENES)
def test_variants_agree(pg, monkeypatch, name, variant):
    props, env = VARIANTS[variant]
    got = run(pg, monkeypatch, name, props, env)
    st = got[3]
    print(name, variant, {k: st[k] for k in COUNTED}, "culled", st.get("culled"), "tail launches", st.get("tail_launches"))
    assert st["segments"] > st["paths"] and st["records"] > 0  # bounce rays were traced, vertices recorded
    if props and "tailPaths" not in props:
        # integrator properties of its own: the per-bounce launches against k_tail from the first bounce
        a = run(pg, monkeypatch, name, dict(props, tailPaths=-1), env)
        b = run(pg, monkeypatch, name, dict(props, tailPaths=1 << 30), env)
        assert a[3]["tail_launches"] == 0 and b[3]["tail_launches"] > 0
        assert_equal_runs(got, a)
        assert_equal_runs(got, b)
        return
    assert_equal_runs(got, run(pg, monkeypatch, name, {}, ()))


def _zstats(g, c):  # tests/test_gpu_parity.py
    n1 = np.maximum(g[0][..., 3:4], 1)
    n2 = np.maximum(c[0][..., 3:4], 1)
    m1, m2 = g[0][..., :3] / n1, c[0][..., :3] / n2
    v1 = np.maximum(g[1][..., :3] / n1 - m1 ** 2, 0) / n1
    v2 = np.maximum(c[1][..., :3] / n2 - m2 ** 2, 0) / n2
    z = (m1 - m2) / np.sqrt(v1 + v2 + 1e-12)
    return m1, m2, z


@pytest.mark.parametrize("name", SCENES)
def test_final_render_matches_oracle_with_the_same_tree(pg, O, monkeypatch, name):
    rgbw, sq, blob, st, off, cfg = run(pg, monkeypatch, name, {}, ())
    osc = O.OracleScene(pg.capi, scene(pg, name))
    tree = O.OracleSDTree(osc)
    tree.deserialize(blob)
    c = O.render(osc, cfg, 16, sample_offset=off, sdtree=tree, nthreads=THREADS)[:2]
    assert np.array_equal(rgbw[..., 3], c[0][..., 3])  # same accepted-sample counts
    m1, m2, z = _zstats((rgbw, sq), c)
    print(name, "|z| < 5:", (np.abs(z) < 5).mean(), "means", m1.mean(), m2.mean())
    assert (np.abs(z) < 5).mean() > 0.995
    assert abs(m1.mean() - m2.mean()) / m2.mean() < 0.01


@pytest.mark.parametrize("tail", [0, -1], ids=["tail", "wavefront"])
@pytest.mark.parametrize("name", SCENES)
def test_records_match_oracle(pg, O, name, tail):
    from mitsuba_path_guiding_amd.integrator import Device
    sc = scene(pg, name)
    lo, hi = (np.asarray(b, np.float64) for b in sc.bounds())
    extent = float((hi - lo).max())
    key = ("oracle records", name)
    if key not in _runs:
        osc = O.OracleScene(pg.capi, sc)
        cfg = pg.capi.default_config(guiding=1, s_tree_threshold=400.0)
        tree, off = R.train_oracle_tree(O, osc, cfg, nthreads=THREADS)
        blob = tree.serialize()
        _runs[key] = (R.oracle_records(pg.capi, O, osc, cfg, tree, off, nthreads=THREADS), blob, off)
    ref, blob, off = _runs[key]
    assert len(ref) >= 2000
    dev = Device(pg.capi.default_config(guiding=1, s_tree_threshold=400.0, tail_paths=tail))
    dev.upload(sc)
    dev.put_sdtree(blob)
    dev.render_pass(R.PASS_SPP, off, record=True)
    got = R.as_records(dev.get_records())
    launches = dev.stats()["tail_launches"]
    dev.close()
    assert (launches > 0) == (tail == 0)
    c = R.compare(ref, got, extent)
    print(c.summary(f"records {name} tail_paths={tail}"))
    assert c.count_ok, (len(got), len(ref))
    assert c.matched_share >= MATCH_BAR, c.matched_share
    assert c.in_bar_share >= IN_BAR, (c.in_bar_share, c.fail)
