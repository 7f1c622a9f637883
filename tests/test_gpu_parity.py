"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same inputs.

Tolerances: integer/index work bit-exact (hit triangle ids, SD-tree topology and
fixed-point sums, shard union); fp32 per-query results within 1e-3 relative (different libm /
FMA contraction on the device); images per pixel within a Monte-Carlo z-test (|z| < 5 for
>= 99.9 % of pixels) and image-mean relative difference < 0.5 %.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(pg):
    return {"cornell": pg.scenes.cornell(64, 64), "ajar": pg.scenes.ajar_door(96, 54)}


def make_dev(pg, scene, **cfg):
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(**cfg))
    d.upload(scene)
    return d


def random_rays(scene, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = scene.bounds()
    o = lo + (hi - lo) * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = o
    r[:, 3] = 1e-4
    r[:, 4:7] = d
    r[:, 7] = np.inf
    return r


@pytest.mark.parametrize("name", ["cornell", "ajar"])
def test_trace_parity(pg, O, scenes, name):
    sc = scenes[name]
    dev = make_dev(pg, sc)
    osc = O.OracleScene(pg.capi, sc)
    rays = random_rays(sc, 200_000, 1)
    g = dev.trace_rays(rays)
    c = osc.trace(rays)
    gp = g[:, 1].view(np.uint32)
    cp = c[:, 1].view(np.uint32)
    ghit, chit = gp != 0xFFFFFFFF, cp != 0xFFFFFFFF
    assert (ghit == chit).mean() > 0.999
    both = ghit & chit
    same = both & (gp == cp)
    assert same.sum() / both.sum() > 0.999
    rel = np.abs(g[same, 0] - c[same, 0]) / np.maximum(np.abs(c[same, 0]), 1e-3)
    assert np.quantile(rel, 0.999) < 1e-3
    assert np.quantile(np.abs(g[same, 2:4] - c[same, 2:4]), 0.999) < 1e-3
    # any-hit agrees with closest-hit existence (same tmax)
    occ = dev.trace_rays(rays, any_hit=True)[:, 0] > 0.5
    assert (occ == ghit).mean() > 0.9999
    dev.close()


@pytest.mark.parametrize("n", [1, 257, 4097])
def test_trace_rays_ragged_bunny(pg, O, n):
    """pg_trace_rays at ragged ray counts on the deep bunny BVH (data/tests/bunny.ply): the overflow
    ring is sized from the launched threads (pg_trace_rays_threads), not a hard-coded block size."""
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "bunny.npz"))
    V, F = z["positions"], z["faces"]
    s = pg.scenes.Scene()
    s.add_mesh(V, F, material=s.add_material(pg.scenes.material("diffuse")))
    c = V.mean(0)
    s.set_camera(tuple(c + np.array([0, 0, 1.0])), tuple(c), (0, 1, 0), 40, 8, 8)
    s.finalize()
    rng = np.random.default_rng(n)
    lo, hi = V.min(0), V.max(0)
    ctr, rad = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    a, b = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    a = ctr + rad * a / np.linalg.norm(a, axis=1, keepdims=True)
    b = ctr + rad * 0.2 * b / np.linalg.norm(b, axis=1, keepdims=True)  # chords through the body
    d = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = a, 0.0, d, np.inf
    dev = make_dev(pg, s)
    g = dev.trace_rays(rays)
    occ = dev.trace_rays(rays, any_hit=True)[:, 0] > 0.5
    dev.close()
    cpu = O.OracleScene(pg.capi, s).trace(rays)
    gp, cp = g[:, 1].view(np.uint32), cpu[:, 1].view(np.uint32)
    assert (gp == cp).mean() >= (0.99 if n > 100 else 1.0)
    assert (occ == (gp != 0xFFFFFFFF)).mean() >= (0.999 if n > 100 else 1.0)


@pytest.mark.parametrize("name", ["strip", "bunny"])
def test_trace_matches_bruteforce(pg, O, tmp_path_factory, name):
    """GPU closest hits (pg_trace_rays, the 4-wide walk) against brute force over the library's own
    triangle records on the CPU (tests/csrc/bvh_shim.cpp) and against the oracle.  The records and the
    device test are the reference's TriAccel with contraction off (pg_layout.h PG_TRIACCEL), so the walk
    must return the brute force's triangle for every ray, and the oracle's t and barycentrics bit for
    bit.  The strip of triangles spanning 1 to 1.6e5 is the geometry on which the unpadded slab test let
    0.55 % of the rays through a box edge past their triangle (pg_trace.h slabRay)."""
    import test_bvh4_build as T
    shim = T.build_shim(tmp_path_factory)
    V, F = T.geometry(pg, name)
    rays = T.rays_through(V, F, 4000, 7)
    s = pg.scenes.Scene()
    s.add_mesh(V, F, material=s.add_material(pg.scenes.material("diffuse")))
    c = V.mean(0)
    s.set_camera(tuple(c + np.array([0, 0, 1.0])), tuple(c), (0, 1, 0), 40, 8, 8)
    s.finalize()
    dev = make_dev(pg, s)
    g = dev.trace_rays(rays)
    dev.close()
    gp = g[:, 1].view(np.uint32)
    bf, bt = T.brute_force_hits(shim, V, F, rays, with_t=True)
    assert (bf != 0xFFFFFFFF).mean() > 0.2
    # hits whose t lies in their triangle's box (test_bvh4_build.consistent_hits: a grazing ray at 1e5
    # can get a TriAccel t ~100 ulps off, outside the box no walk can be required to open)
    ok = T.consistent_hits(V, F, rays, bf, bt)
    assert ok.mean() > 0.97
    np.testing.assert_array_equal(gp[ok], bf[ok])
    # the oracle (its own BVH, TriAccel, ties to the lower original index): same triangles, and the
    # same t / u / v bit for bit where the triangle is the same
    osc = O.OracleScene(pg.capi, s)
    cpu = osc.trace(rays)
    cp = cpu[:, 1].view(np.uint32)
    same = gp == cp
    # ties go to the lower original triangle index on both sides (pg_trace.h acceptHit): every ray agrees
    np.testing.assert_array_equal(gp[ok], cp[ok])
    hit = same & (gp != 0xFFFFFFFF)
    np.testing.assert_array_equal(g[hit][:, [0, 2, 3]], cpu[hit][:, [0, 2, 3]])


@pytest.mark.parametrize("name", ["strip", "bunny", "dups"])
def test_any_hit_matches_bruteforce(pg, O, tmp_path_factory, name):
    """GPU shadow rays (pg_trace_rays(any_hit = 1), the 8-wide walk traverseWide<true>) against brute force over the
    library's own triangle records on the CPU (tests/csrc/bvh_shim.cpp shim_trace_any) and against the oracle, on the
    ray families of test_bvh8_build: rays through the scene with tmax = inf, the same with a finite tmax,
    surface-to-surface segments with the shadow rays' epsilons, and axis-parallel rays (zero direction components
    of both signs).  Exact both ways: where the walk says occluded, brute force accepts a triangle; where brute force
    accepts a triangle at a t inside that triangle's own box, the walk says occluded.  The strip's 100 000 rays per
    family are what it takes to see the 2-in-10 000 misses of the unpadded slab test (pg_trace.h wideRay)."""
    import test_bvh4_build as T
    import test_bvh8_build as W
    shim = T.build_shim(tmp_path_factory)
    V, F, fams = W.references(pg, shim, name, 100_000 if name == "strip" else 4000)
    s = pg.scenes.Scene()
    s.add_mesh(V, F, material=s.add_material(pg.scenes.material("diffuse")))
    c = V.mean(0)
    s.set_camera(tuple(c + np.array([0, 0, 1.0])), tuple(c), (0, 1, 0), 40, 8, 8)
    s.finalize()
    dev = make_dev(pg, s)
    occ = {fam: dev.trace_rays(rays, any_hit=True)[:, 0] > 0.5 for fam, (rays, _, _) in fams.items()}
    dev.close()
    osc = O.OracleScene(pg.capi, s)
    failed = []
    for fam, (rays, walk, brute) in fams.items():
        hit, consistent = brute[:, 0] > 0, brute[:, 1] == 1
        try:  # the device returns 0 / 1 only: a false positive is an "occluded" where brute force accepts nothing
            W.check_family(f"gpu {name}/{fam}", occ[fam], brute, hit)
        except AssertionError as e:  # every family's figures are printed before the test fails
            failed.append(str(e))
        # the walk's CPU restatement is the device's arithmetic: the same answers, excluded rays included
        same = int((occ[fam] == (walk != 0xFFFFFFFF)).sum())
        print(f"gpu {name}/{fam}: {same} of {len(walk)} answers equal the CPU restatement's")
        if same != len(walk):
            failed.append(f"gpu {name}/{fam}: {len(walk) - same} answers differ from the CPU restatement's")
        # the oracle (its own BVH and slab test) on every ray that is not excluded
        keep = ~(hit & ~consistent)
        oc = osc.trace(rays, any_hit=True)[:, 0] > 0.5
        diff = int((occ[fam] != oc)[keep].sum())
        if diff:
            failed.append(f"gpu {name}/{fam}: {diff} answers differ from the oracle's")
    assert not failed, failed


def test_dgeom_kat_gpu(pg, O):
    """src/tests/test_dgeom.cpp:35-177 through the GPU traversal and the shading kernels' hit record
    (pg_hit_records: fetchHit's position, geometric and shading normals, shading frame and local wi), and
    that record equal to the oracle's bit for bit."""
    import json, os
    from test_oracle_kat import check_dgeom_case, dgeom_scene
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dgeom_kat.json")))
    for case in kat["cases"]:
        s = dgeom_scene(pg, case)
        dev = make_dev(pg, s)
        r = np.array([[*case["ray_o"], 1e-4, *case["ray_d"], np.inf]], np.float32)
        h = dev.trace_rays(r)[0]
        rec = dev.hit_records(r)[0]
        dev.close()
        assert h[1].view(np.uint32) == 0
        check_dgeom_case(case, rec, h[2:4])
        orec = O.OracleScene(pg.capi, s).hit_records(r)[0]
        np.testing.assert_array_equal(rec, orec)


def test_hit_records_match_oracle(pg, O, scenes):
    """The hit record of random rays (smooth-shaded spheres of the ajar door included): every field the
    shading kernels use, GPU against the oracle."""
    sc = scenes["ajar"]
    rays = random_rays(sc, 100_000, 9)
    dev = make_dev(pg, sc)
    g = dev.hit_records(rays)
    dev.close()
    c = O.OracleScene(pg.capi, sc).hit_records(rays)
    hit = (c[:, 3] > 0) & (g[:, 3] > 0)
    assert hit.mean() > 0.5
    same_t = hit & (g[:, 3] == c[:, 3])
    assert same_t.sum() / hit.sum() > 0.999
    bit = np.all(g[same_t] == c[same_t], axis=1)
    print(f"hit records: {same_t.sum()} rays with equal t, bit-equal records {bit.mean():.6f}, max |diff| "
          f"{np.abs(g[same_t] - c[same_t]).max():.3g}")
    assert np.quantile(np.abs(g[same_t] - c[same_t]).max(1), 0.999) < 1e-5


def _probe_scene(pg):
    S = pg.scenes
    mats = [
        S.material("diffuse", reflectance=(0.5, 0.4, 0.3)),
        S.material("diffuse", reflectance=(0.5, 0.4, 0.3), twosided=True),
        S.material("conductor", conductor="Cu"),
        S.material("roughconductor", conductor="Au", alpha=0.3, distribution="beckmann"),
        S.material("roughconductor", conductor="Al", alpha_u=0.1, alpha_v=0.3, distribution="ggx"),
        S.material("roughconductor", conductor="Cu", alpha=0.3, distribution="ggx", sample_visible=False),
        S.material("dielectric", int_ior=1.333, ext_ior=1.000277),
        S.material("roughdielectric", int_ior=1.5, ext_ior=1.0, alpha=0.3, distribution="beckmann"),
        S.material("roughdielectric", int_ior=1.5, ext_ior=1.0, alpha=0.3, distribution="ggx"),
        S.material("roughdielectric", int_ior=1.5, ext_ior=1.0, alpha=0.3, distribution="ggx", sample_visible=False),
        S.material("plastic", diffuse_reflectance=(0.5, 0.5, 0.5)),
        S.material("plastic", diffuse_reflectance=(0.5, 0.3, 0.2), nonlinear=True),
        S.material("roughplastic", alpha=0.7),
        S.material("roughplastic", alpha=0.2, distribution="ggx", diffuse_reflectance=(0.5, 0.3, 0.2), nonlinear=True),
    ]
    s = S.Scene()
    for i, m in enumerate(mats):
        k = s.add_material(m)
        V, F = S.quad((i, 0, 0), (i + 1, 0, 0), (i + 1, 1, 0), (i, 1, 0), facing=(0, 0, -1))
        s.add_mesh(V, F, material=k)
    s.set_camera((6, 0.5, -10), (6, 0.5, 0), (0, 1, 0), 80, 16, 16)
    return s.finalize(), mats


def test_bsdf_parity(pg, O):
    sc, mats = _probe_scene(pg)
    dev = make_dev(pg, sc)
    rng = np.random.default_rng(3)
    n = 50_000
    for mi, m in enumerate(mats):
        wi = rng.normal(size=(n, 3))
        wi /= np.linalg.norm(wi, axis=1, keepdims=True)
        wi[: n // 2, 2] = np.abs(wi[: n // 2, 2])  # mostly front-facing, some back-facing
        u = rng.random((n, 3)).astype(np.float32)
        wg = rng.normal(size=(n, 3))
        wg /= np.linalg.norm(wg, axis=1, keepdims=True)
        g = dev.bsdf_query(mi, wi, u, wg)
        c = O.bsdf_query(pg.capi, m, wi, u, wg)
        same_type = g[:, 7] == c[:, 7]
        ok = same_type & (c[:, 7] != 0)
        qv = []
        for col in (3, 4, 5, 6, 8, 9, 10, 11):
            sel = (ok if col < 8 else np.ones(n, bool)) & (np.abs(c[:, col]) > 1e-6)
            if sel.sum():
                qv.append(np.quantile(np.abs(g[sel, col] - c[sel, col]) / np.abs(c[sel, col]), 0.999))
        print(f"bsdf {mi}: same lobe {same_type.mean():.5f}, bit-equal rows {np.all(g == c, axis=1).mean():.5f}, "
              f"direction q999 {np.quantile(np.abs(g[ok, 0:3] - c[ok, 0:3]).max(1), 0.999):.3g}, "
              f"value columns q999 rel {max(qv):.3g}")
        # round 5 (profiles/r05x_fastlog/r05ab/bsdf.log): every model but roughplastic within 2.7e-5 of the
        # oracle (directions 1.7e-6) at the 99.9th percentile, 34-100 % of rows bit for bit.  roughplastic
        # (8.0e-3 then: two quadratures of its rough-transmittance tables) now shares the library's tables
        # bit for bit (tests/test_rtrans.py)
        assert same_type.mean() > 0.9995, (mi, same_type.mean())
        tol_dir, tol_val = 2e-5, 2e-4
        assert np.quantile(np.abs(g[ok, 0:3] - c[ok, 0:3]).max(1), 0.999) < tol_dir, mi
        for col in (3, 4, 5, 6, 8, 9, 10, 11):
            a, b = g[:, col], c[:, col]
            sel = (ok if col < 8 else np.ones(n, bool)) & (np.abs(b) > 1e-6)
            rel = np.abs(a[sel] - b[sel]) / np.abs(b[sel])
            if sel.sum():
                assert np.quantile(rel, 0.999) < tol_val, (mi, col, np.quantile(rel, 0.999))
    dev.close()


def _zstats(g, c):
    n1 = np.maximum(g[0][..., 3:4], 1)
    n2 = np.maximum(c[0][..., 3:4], 1)
    m1, m2 = g[0][..., :3] / n1, c[0][..., :3] / n2
    v1 = np.maximum(g[1][..., :3] / n1 - m1 ** 2, 0) / n1
    v2 = np.maximum(c[1][..., :3] / n2 - m2 ** 2, 0) / n2
    z = (m1 - m2) / np.sqrt(v1 + v2 + 1e-12)
    return m1, m2, z


def test_image_parity_cornell_unguided(pg, O, scenes):
    sc = scenes["cornell"]
    spp = 256
    dev = make_dev(pg, sc)
    dev.render_pass(spp, 0)
    g = dev.read_film()
    cfg = pg.capi.default_config()
    c = O.render(O.OracleScene(pg.capi, sc), cfg, spp)[:2]
    assert np.array_equal(g[0][..., 3], c[0][..., 3])  # same accepted-sample counts
    m1, m2, z = _zstats(g, c)
    assert (np.abs(z) < 5).mean() > 0.999
    rel = abs(m1.mean() - m2.mean()) / m2.mean()
    assert rel < 5e-3
    st = dev.stats()
    assert st["paths"] == 64 * 64 * spp
    dev.close()


def test_image_parity_ajar_unguided(pg, O, scenes):
    sc = scenes["ajar"]
    spp = 64
    dev = make_dev(pg, sc)
    dev.render_pass(spp, 0)
    g = dev.read_film()
    c = O.render(O.OracleScene(pg.capi, sc), pg.capi.default_config(), spp)[:2]
    m1, m2, z = _zstats(g, c)
    assert (np.abs(z) < 5).mean() > 0.999
    rel = abs(m1.mean() - m2.mean()) / max(m2.mean(), 1e-8)
    assert rel < 0.02
    dev.close()


def test_shard_union_bitexact(pg, scenes):
    """Tile shards of 2 ranks add up to the single-rank film bit for bit (RNG keyed by pixel)."""
    sc = scenes["ajar"]
    full = make_dev(pg, sc)
    full.render_pass(8, 0)
    f = full.read_film()[0]
    parts = []
    for r in range(2):
        d = make_dev(pg, sc, rank=r, world_size=2)
        d.render_pass(8, 0)
        parts.append(d.read_film()[0])
        assert d.local_pixel_count() < sc.width * sc.height
        d.close()
    assert np.array_equal(parts[0] + parts[1], f)
    assert ((parts[0][..., 3] > 0) ^ (parts[1][..., 3] > 0)).all()
    full.close()


def test_sdtree_splat_refit_bitexact(pg, O, scenes):
    """Identical records -> identical SD-trees (topology, fixed-point sums, fp32 sums) on GPU and
    oracle; identical trees -> identical pdfs / samples."""
    sc = scenes["cornell"]
    cfg = pg.capi.default_config(guiding=1, s_tree_threshold=400.0)
    osc = O.OracleScene(pg.capi, sc)
    otree = O.OracleSDTree(osc)
    dev = make_dev(pg, sc, guiding=1, s_tree_threshold=400.0)
    assert np.array_equal(dev.get_sdtree(), otree.serialize())
    for it in range(3):
        O.render(osc, cfg, 2 ** it, sample_offset=2 ** it - 1, record=True, sdtree=otree)
        recs = otree.take_records(pg.capi)
        assert len(recs) > 1000
        dev.splat_records(recs)
        otree.splat_bytes(recs)
        assert np.array_equal(dev.get_sdtree(), otree.serialize()), it
        dev.refit(it)
        otree.refit(it, cfg)
        assert np.array_equal(dev.get_sdtree(), otree.serialize()), it
    rng = np.random.default_rng(5)
    lo, hi = sc.bounds()
    n = 100_000
    pos = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gp, cp = dev.sdtree_pdf(pos, d), otree.pdf(pos, d)
    assert (np.abs(gp - cp) <= 1e-5 * np.abs(cp)).mean() > 0.999
    u = rng.random((n, 2)).astype(np.float32)
    gd, gpdf = dev.sdtree_sample(pos, u)
    cd, cpdf = otree.sample(pos, u)
    assert np.array_equal(gpdf, cpdf) or (np.abs(gpdf - cpdf) <= 1e-5 * cpdf).mean() > 0.9999
    assert np.quantile(np.abs(gd - cd).max(1), 0.999) < 1e-4
    dev.close()


def test_sdtree_deep_lookup_matches_oracle(pg, O, scenes):
    """An S-tree far deeper than the 64^3 jump grid resolves (records concentrated in a tiny cube, a low
    split threshold): lookups there take the grid's node entry and descend the rest of the way
    (pg_device.h sdLookup / sdDescend; most cells of trained trees hold a leaf's D-tree id), and must
    match the oracle's plain descent."""
    sc = scenes["cornell"]
    cfg = pg.capi.default_config(guiding=1, s_tree_threshold=50.0)
    osc = O.OracleScene(pg.capi, sc)
    otree = O.OracleSDTree(osc)
    dev = make_dev(pg, sc, guiding=1, s_tree_threshold=50.0)
    lo, hi = (np.asarray(b, np.float64) for b in sc.bounds())
    centre = lo + 0.3 * (hi - lo)
    rng = np.random.default_rng(11)
    rec_t = np.dtype([("pos", "<f4", 3), ("dir", "<u4"), ("radiance", "<f4"), ("wo_pdf", "<f4"),
                      ("product", "<f4"), ("weight", "<f4")])
    assert rec_t.itemsize == 32
    for it in range(3):
        n = 200_000
        r = np.zeros(n, rec_t)
        r["pos"] = centre + (hi - lo) * 1e-5 * (rng.random((n, 3)) - 0.5)
        r["dir"] = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
        r["radiance"] = rng.random(n).astype(np.float32) + 0.1
        r["wo_pdf"] = 0.25
        r["weight"] = -1.0
        recs = r.view(np.uint8)
        dev.splat_records(recs)
        otree.splat_bytes(recs)
        dev.refit(it)
        otree.refit(it, cfg)
        assert np.array_equal(dev.get_sdtree(), otree.serialize()), it
    blob = otree.serialize().tobytes()  # header 16 + box 32 + counts 16, then the S-tree node pairs
    ns = int(np.frombuffer(blob, np.uint32, 1, 48)[0])
    sn = np.frombuffer(blob, np.uint32, 2 * ns, 64).reshape(-1, 2)
    depth, stack, deepest = {0: 0}, [0], 0
    while stack:
        k = stack.pop()
        deepest = max(deepest, depth[k])
        if sn[k, 0] != 0xFFFFFFFF:
            for c in sn[k]:
                depth[int(c)] = depth[k] + 1
                stack.append(int(c))
    assert deepest > 3 * 6, deepest  # deeper than the 2^6-per-axis jump grid resolves (measured 35)
    m = 50_000
    pos = np.concatenate([centre + (hi - lo) * 2e-5 * (rng.random((m, 3)) - 0.5),
                          lo + (hi - lo) * rng.random((m, 3))]).astype(np.float32)
    d = rng.normal(size=(2 * m, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gp, cp = dev.sdtree_pdf(pos, d), otree.pdf(pos, d)
    assert (np.abs(gp - cp) <= 1e-5 * np.abs(cp)).mean() > 0.999
    dev.close()


def test_guided_training_parity(pg, O, scenes):
    """Guided training on GPU vs oracle: every iteration writes as many records as an oracle pass with the same
    tree and streams (within 0.1 %, measured 12863 / 12863, 13311 / 13311, 43008 / 43005, 84920 / 84920; what
    is in the records: tests/test_gpu_records.py), and the guided image agrees with the unguided oracle image
    (guiding is unbiased)."""
    sc = scenes["cornell"]
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer
    integ = GuidedPathTracer({"trainingIterations": 4, "sTreeThreshold": 400.0})
    integ.preprocess(sc)
    osc = O.OracleScene(pg.capi, sc)
    otree = O.OracleSDTree(osc)
    counts = []
    splat_and_refit = integ.postprogression_train

    def count_then_train(it):  # after iteration it's pass, before its records are splatted
        spp = 2 ** it
        otree.deserialize(integ.dev.get_sdtree())  # the tree the pass just sampled
        n_cpu = int(O.render(osc, integ.cfg, spp, sample_offset=integ.sample_offset - spp, record=True, sdtree=otree,
                             nthreads=16)[2][3])
        otree.take_records(pg.capi)
        counts.append((integ.dev.record_count(), n_cpu))
        splat_and_refit(it)

    integ.postprogression_train = count_then_train
    rgbw, sq = integ.render(128)
    st = integ.postprocess()
    print("records per training iteration (gpu, oracle):", counts)
    assert len(counts) == 4
    for n_gpu, n_cpu in counts:
        assert n_cpu > 1000 and abs(n_gpu - n_cpu) <= 0.001 * n_cpu, counts
    assert st["records"] == sum(n for n, _ in counts)
    assert st["records"] > 0 and st["stree_nodes"] > 1
    cfgu = pg.capi.default_config()
    c = O.render(O.OracleScene(pg.capi, sc), cfgu, 512)[:2]
    m1, m2, z = _zstats((rgbw, sq), c)
    assert (np.abs(z) < 5).mean() > 0.995
    assert abs(m1.mean() - m2.mean()) / m2.mean() < 0.01


def test_image_parity_kitchen_unguided(pg, O):
    """C4 kitchen class (~1 M triangles, 5 area emitters, plastic / rough conductor / glass
    clutter) at a small resolution: per-pixel z-test and image mean against the oracle."""
    sc = pg.scenes.kitchen(96, 54)
    spp = 64
    dev = make_dev(pg, sc)
    dev.render_pass(spp, 0)
    g = dev.read_film()
    dev.close()
    c = O.render(O.OracleScene(pg.capi, sc), pg.capi.default_config(), spp)[:2]
    m1, m2, z = _zstats(g, c)
    assert (np.abs(z) < 5).mean() > 0.999
    assert abs(m1.mean() - m2.mean()) / m2.mean() < 5e-3


def test_image_parity_roughplastic(pg, O):
    """roughplastic blocks (GGX and Beckmann) in the Cornell box: unguided GPU vs oracle per-pixel
    z-test, then the guided GPU image against the same unguided oracle (guiding is unbiased).  Both sides
    integrate the rough-transmittance tables with the same quadrature (since round 5, tests/test_rtrans.py);
    the two renders here use different random streams, so this is a statistical comparison (the same-stream
    comparisons are test_bsdf_parity and tests/test_gpu_params.py)."""
    S = pg.scenes
    sc = S.cornell(64, 64, short_material=S.material("roughplastic", alpha=0.2, distribution="ggx",
                                                        diffuse_reflectance=(0.6, 0.3, 0.2)),
                   tall_material=S.material("roughplastic", alpha=0.5, diffuse_reflectance=(0.3, 0.4, 0.6)))
    spp = 256
    dev = make_dev(pg, sc)
    dev.render_pass(spp, 0)
    g = dev.read_film()
    dev.close()
    c = O.render(O.OracleScene(pg.capi, sc), pg.capi.default_config(), spp)[:2]
    m1, m2, z = _zstats(g, c)
    assert (np.abs(z) < 5).mean() > 0.999
    assert abs(m1.mean() - m2.mean()) / m2.mean() < 5e-3
    from mitsuba_path_guiding_amd.integrator import GuidedPathTracer
    integ = GuidedPathTracer({"trainingIterations": 4, "sTreeThreshold": 400.0})
    integ.preprocess(sc)
    rgbw, sq = integ.render(spp)
    integ.postprocess()
    m1, m2, z = _zstats((rgbw, sq), c)
    assert (np.abs(z) < 5).mean() > 0.995
    assert abs(m1.mean() - m2.mean()) / m2.mean() < 0.01


def test_tree_stats_allreduce_equals_single_rank(pg, scenes):
    """The all-reduce exchange through the C-ABI (pg_get/put_tree_stats), emulated with two shard
    contexts on one GPU: summed building statistics give the single-rank tree bit for bit."""
    sc = scenes["cornell"]
    cfg = dict(guiding=1, s_tree_threshold=300.0)
    full = make_dev(pg, sc, **cfg)
    parts = [make_dev(pg, sc, rank=r, world_size=2, **cfg) for r in range(2)]
    off = 0
    for it in range(3):
        full.render_pass(2 ** it, off, True)
        full.splat_local()
        full.refit(it)
        for d in parts:
            d.render_pass(2 ** it, off, True)
            d.splat_local()
        stats = [d.get_tree_stats() for d in parts]
        assert len(stats[0]) == parts[0].tree_stats_words()
        total = stats[0] + stats[1]
        for d in parts:
            d.put_tree_stats(total)
            d.refit(it)
        off += 2 ** it
    t = full.get_sdtree()
    assert all(np.array_equal(d.get_sdtree(), t) for d in parts)
    for d in parts + [full]:
        d.close()


def test_cancel_and_errors(pg, scenes):
    from mitsuba_path_guiding_amd.integrator import Device, PGError
    d = Device(pg.capi.default_config())
    with pytest.raises(PGError):
        d.render_pass(1, 0)  # no scene yet -> PG_ERR_STATE
    d.upload(scenes["cornell"])
    d.cancel()
    with pytest.raises(PGError) as e:
        d.render_pass(1, 0)
    assert e.value.status == pg.capi.PG_ERR_CANCELLED
    d.close()
