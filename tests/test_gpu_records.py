"""The training records the GPU writes (pg_get_records after a recording pass) against the oracle's, record by
record: the per-vertex snapshots of k_shade / k_shade_all / k_tail, the path cull of k_trace / k_rays, and
k_commit's (L_final - L_snapshot) / T with its guards, truncation, env_hits correction and allocation.

Setup, the same on both sides: the oracle trains an SD-tree for 3 iterations (1, 2, 4 spp, s-tree threshold
400) under the case's configuration, the tree goes into the device (put_sdtree; the device's blob must equal
it), and one 4 spp pass with record=True at the next sample offset runs on both.  Each case takes one knob off
its default and runs twice on the GPU: tail_paths at its default (passes this small sit under the tail
threshold, so k_tail takes every path right after the camera rays) and tail_paths = -1 (every bounce through
k_shade_all / the per-class k_shade launches and k_rays).  Which record path a case reaches:

    every case             tail (k_tail) and wavefront (k_shade*, k_rays), k_commit
    sky-*                  k_commit's env_hits branch, the unfused shading launches
    *-rr1, *-maxdepth3     the cull decides the last vertex of almost every path (rr1) / of the deepest (maxdepth3)
    *-rmv0/1/2             record_max_vertices truncation in the snapshot writes and k_commit
    *-unbuilt              iteration 0: no guided vertex (weight -1, product 0)
    spheres-*              rough conductor / roughplastic vertices, glass (delta: no record), strictNormals

Bars (tests/record_parity.py; set by the issue from the project's loosest same-stream divergence bar, C4 in
test_gpu_configs, not from these measurements): counts within 0.1 %, >= 99 % of the oracle's records matched,
>= 99 % of the matched pairs inside every field bar.  The exact conditions on the GPU's records carry no
tolerance.

Measured on an MI355X (the two tail settings give the same figures, their records being bit-identical):
record counts equal to the oracle's in all 22 cases; matched share / in-bar share

    cornell   default, rr1, maxdepth3, rmv1, rmv2   1.00000 / 1.00000
              learned, unbuilt                      0.99992 / 0.99992
    spheres   default 0.99990 / 0.99990   rr1 0.99992 / 0.99984   maxdepth3 1.00000 / 1.00000
              glossy  0.99908 / 0.99985   strict 0.99989 / 0.99984   learned 0.99896 / 0.99992
              rmv2    1.00000 / 0.99982
    sky       default, rr1, maxdepth3, nonee, rmv1  1.00000 / 1.00000
              learned 1.00000 / 0.99977   unbuilt 0.99966 / 0.99977

Worst: matched 0.99896 (spheres-learned), in-bar 0.99977 (sky-learned, sky-unbuilt).  The pairs outside a bar
are one or two paths per scene whose later vertices took another branch in fp32 (the same two positions in
every spheres case).
"""
import numpy as np
import pytest

import record_parity as R

pytestmark = pytest.mark.gpu

THREADS = 16  # the GPU box's CPU share
MATCH_BAR = IN_BAR = 0.99

# one knob off its default per case
KNOBS = {
    "default": {},
    "rr1": dict(rr_depth=1),
    "maxdepth3": dict(max_depth=3),
    "nonee": dict(use_nee=0),
    "glossy": dict(glossy_prior=1),
    "learned": dict(bsdf_fraction_bound=3),  # PG_FRACTION_LEARNED (asserted below)
    "strict": dict(strict_normals=1),
    "unbuilt": {},  # guiding on, the tree of iteration 0
    "rmv0": dict(record_max_vertices=0),
    "rmv1": dict(record_max_vertices=1),
    "rmv2": dict(record_max_vertices=2),
}
# use_nee = 0 only under the sky: in the two boxes a path without NEE sees light only by hitting the small lamp,
# and 6 % of the oracle's records have positive radiance (15 % at 128 x 128), short of the 20 % precondition
CASES = [("cornell", k) for k in ("default", "rr1", "maxdepth3", "learned", "unbuilt", "rmv0", "rmv1", "rmv2")] + \
        [("spheres", k) for k in ("default", "rr1", "maxdepth3", "glossy", "strict", "learned", "rmv2")] + \
        [("sky", k) for k in ("default", "rr1", "maxdepth3", "nonee", "learned", "unbuilt", "rmv1")]
TAILS = {"tail": 0, "wavefront": -1}

_scenes, _oracle, _gpu = {}, {}, {}


def scene(pg, name):
    if name not in _scenes:
        S = pg.scenes
        if name == "cornell":
            sc = S.cornell(32, 32)
        elif name == "spheres":
            from test_gpu_params import smooth_spheres
            sc = smooth_spheres(pg)
        else:
            sc = S.sky_courtyard(48, 36, env=S.sky_envmap(64, 32, sun_radiance=20.0))
        lo, hi = (np.asarray(b, np.float64) for b in sc.bounds())
        _scenes[name] = (sc, lo, hi, float((hi - lo).max()))
    return _scenes[name]


def config(pg, knob, **more):
    assert pg.capi.PG_FRACTION_LEARNED == 3
    return pg.capi.default_config(guiding=1, s_tree_threshold=400.0, **dict(KNOBS[knob], **more))


def oracle_side(pg, O, scene_name, knob):
    """(oracle records, tree blob, sample offset) of a case.  The tree is trained with the case's knob, except
    record_max_vertices: the truncated cases share the default case's tree, so that their records are subsets
    of the default's."""
    key = (scene_name, knob)
    if key not in _oracle:
        sc = scene(pg, scene_name)[0]
        osc = O.OracleScene(pg.capi, sc)
        tkey = (scene_name, "default" if knob.startswith("rmv") else knob)
        if ("tree",) + tkey not in _oracle:
            tree, off = R.train_oracle_tree(O, osc, config(pg, tkey[1]), nthreads=THREADS,
                                            iterations=0 if knob == "unbuilt" else len(R.TRAIN_SPP))
            _oracle[("tree",) + tkey] = (tree.serialize(), off)
        blob, off = _oracle[("tree",) + tkey]
        tree = O.OracleSDTree(osc)
        tree.deserialize(blob)
        recs = R.oracle_records(pg.capi, O, osc, config(pg, knob), tree, off, nthreads=THREADS)
        _oracle[key] = (recs, blob, off)
    return _oracle[key]


def check_preconditions(recs, knob):
    """Oracle side: the case has something to compare."""
    if knob == "rmv0":
        assert len(recs) == 0
        return
    assert len(recs) >= 2000, len(recs)
    assert (recs["radiance"] > 0).mean() >= 0.2, (recs["radiance"] > 0).mean()
    if knob == "unbuilt":
        assert (recs["weight"] == -1).all() and (recs["product"] == 0).all()
    else:
        assert (recs["weight"] >= 0).mean() >= 0.5, (recs["weight"] >= 0).mean()


def gpu_side(pg, scene_name, knob, tail, blob, off):
    """The GPU's records of a case (one fresh device per run), with its three record counts checked equal."""
    key = (scene_name, knob, tail)
    if key not in _gpu:
        from mitsuba_path_guiding_amd.integrator import Device
        sc = scene(pg, scene_name)[0]
        dev = Device(config(pg, knob, tail_paths=TAILS[tail]))
        dev.upload(sc)
        dev.put_sdtree(blob)
        assert np.array_equal(dev.get_sdtree(), blob)
        before = dev.stats()
        assert dev.record_count() == 0
        dev.render_pass(R.PASS_SPP, off, record=True)
        n = dev.record_count()
        st = dev.stats()
        recs = R.as_records(dev.get_records())
        dev.close()
        assert st["paths"] - before["paths"] == sc.width * sc.height * R.PASS_SPP
        assert n == st["records"] - before["records"] == len(recs)
        if knob != "rmv0":
            assert (st["tail_launches"] > before["tail_launches"]) == (tail == "tail")
        _gpu[key] = recs
    return _gpu[key]


def check_exact(recs, lo, hi, extent):
    """Conditions on the GPU's records alone; no tolerance."""
    for f in ("pos", "radiance", "wo_pdf", "product", "weight"):
        assert np.isfinite(recs[f]).all(), f
    assert (recs["wo_pdf"] > 0).all()
    assert ((recs["weight"] == -1) | (recs["weight"] >= 0)).all()
    assert (recs["product"][recs["weight"] < 0] == 0).all()
    pad = 1e-3 * extent
    assert (recs["pos"] >= lo - pad).all() and (recs["pos"] <= hi + pad).all()


@pytest.mark.parametrize("scene_name,knob", CASES, ids=[f"{s}-{k}" for s, k in CASES])
def test_records_match_oracle(pg, O, scene_name, knob):
    sc, lo, hi, extent = scene(pg, scene_name)
    ref, blob, off = oracle_side(pg, O, scene_name, knob)
    check_preconditions(ref, knob)
    got = {}
    for tail in TAILS:
        g = got[tail] = gpu_side(pg, scene_name, knob, tail, blob, off)
        check_exact(g, lo, hi, extent)
        if knob == "rmv0":
            assert len(g) == 0
            continue
        c = R.compare(ref, g, extent)
        print(c.summary(f"records {scene_name} {knob} {tail}"))
        assert c.count_ok, (len(g), len(ref))
        assert c.matched_share >= MATCH_BAR, c.matched_share
        assert c.in_bar_share >= IN_BAR, (c.in_bar_share, c.fail)
        if knob == "unbuilt":
            assert (g["weight"] == -1).all() and (g["product"] == 0).all()
    # the tail kernel and the per-bounce launches write the same records bit for bit
    assert np.array_equal(R.sorted_rows(got["tail"]), R.sorted_rows(got["wavefront"]))


@pytest.mark.parametrize("scene_name,maxv", [("cornell", 1), ("cornell", 2), ("spheres", 2), ("sky", 1)])
@pytest.mark.parametrize("tail", list(TAILS))
def test_truncated_records_are_subset_of_default(pg, O, scene_name, maxv, tail):
    """record_max_vertices = 1, 2: the first training vertices of every path, bit-identical to the same
    records of the default (32) pass, and no more than paths x record_max_vertices of them."""
    sc = scene(pg, scene_name)[0]
    _, blob, off = oracle_side(pg, O, scene_name, "default")
    full = gpu_side(pg, scene_name, "default", tail, blob, off)
    part = gpu_side(pg, scene_name, f"rmv{maxv}", tail, blob, off)
    assert 0 < len(part) <= sc.width * sc.height * R.PASS_SPP * maxv
    assert len(part) < len(full)
    assert R.is_row_subset(part, full)
