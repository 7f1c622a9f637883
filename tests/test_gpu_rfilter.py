"""The reconstruction-filtered film (pg_set_rfilter / pg_read_film_filtered) on the GPU.

The reference is built from pieces that exist without the feature: a 1-spp box render at sample_offset s (film
reset in between) gives every sample's exact L (and n = 0 where ImageBlock::put drops it); the jitter comes
from the numpy Philox restatement and the splat from numpy in float32 / float64 (tests/rfilter_ref.py,
checked on the host by test_rfilter_table.py).  The sums are integers, so the GPU's raw accumulators must equal
the reference's int64 array element for element: there is no tolerance anywhere in the exact tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rfilter_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_LOBE = (3.0, np.array([1.0, 0.97, 0.9, 0.8, 0.68, 0.55, 0.42, 0.3, 0.19, 0.1, 0.03, -0.02, -0.06, -0.085, -0.1,
                           -0.105, -0.1, -0.09, -0.078, -0.064, -0.05, -0.038, -0.027, -0.018, -0.011, -0.006,
                           -0.003, -0.001, 0.0, 0.0005, 0.0002, 0.0], np.float32))
SPP = 4


def tables():
    return {"gaussian": R.table("gaussian", 0.5), "tent": R.table("tent"), "box": R.table("box"), "neg": NEG_LOBE}


def make_dev(pg, scene, table=None, **cfg):
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(**cfg))
    d.upload(scene)
    if table is not None:
        d.set_rfilter(table)
    return d


def per_sample_films(pg, scene, spp, off=0, **cfg):
    """[(sample index, box film rgbw of that one sample)]: the exact L of every sample, n = 0 where dropped"""
    d = make_dev(pg, scene, **cfg)
    out = []
    for s in range(off, off + spp):
        d.reset_film()
        d.render_pass(1, s)
        out.append((s, d.read_film()[0]))
    d.close()
    return out


def gpu_raw(pg, scene, table, spp, off=0, **cfg):
    d = make_dev(pg, scene, table, **cfg)
    d.render_pass(spp, off)
    raw = d.read_film_filtered(raw=True)
    d.close()
    return raw


def reference(scene, table, samples, seed=1337):
    return R.reference_film(scene.width, scene.height, table[0], table[1], seed, samples)


@pytest.fixture(scope="module")
def cornell(pg):
    """cornell 48 x 40: four tiles at tile_size 32, three of them partial, image edges on every side, borders that
    cross the tile seams; its per-sample films; the default configuration's gaussian raw film"""
    sc = pg.scenes.cornell(width=48, height=40)
    samples = per_sample_films(pg, sc, SPP)
    assert all((f[..., 3] == 1).mean() > 0.99 for _, f in samples)
    raw = gpu_raw(pg, sc, tables()["gaussian"], SPP)
    for a in [raw] + [f for _, f in samples]:
        a.setflags(write=False)
    return sc, samples, raw


@pytest.mark.parametrize("name", ["gaussian", "tent", "neg"])
def test_exact_splat(pg, cornell, name):
    sc, samples, raw_g = cornell
    t = tables()[name]
    raw = raw_g if name == "gaussian" else gpu_raw(pg, sc, t, SPP)
    ref = reference(sc, t, samples)
    assert raw.dtype == np.int64 and raw.shape == (40, 48, 4)
    bad = np.argwhere(raw != ref)
    print(f"{name}: {len(bad)} of {raw.size} accumulators differ; sum w gpu {raw[..., 3].sum()} ref {ref[..., 3].sum()}")
    assert np.array_equal(raw, ref), bad[:8]
    assert np.count_nonzero(raw[..., :3]) > 1000
    if name == "neg":
        assert (raw < 0).any()


def test_developed_image(pg, cornell):
    from mitsuba_path_guiding_amd.integrator import ProgressivePathTracer, develop
    sc, samples, raw = cornell
    ref = reference(sc, tables()["gaussian"], samples).astype(np.float64)
    want = np.where(ref[..., 3:4] != 0, ref[..., :3] / np.where(ref[..., 3:4] != 0, ref[..., 3:4], 1), 0)
    t = ProgressivePathTracer({"rfilter": "gaussian", "samplesPerProgression": SPP})
    t.preprocess(sc)
    rgbw, _ = t.render(SPP)
    t.postprocess()
    assert t.filtered.dtype == np.float32 and t.developed.shape == (40, 48, 3)
    assert np.array_equal(t.filtered, (raw.astype(np.float64) * 2.0 ** -28).astype(np.float32))
    got = develop(t.filtered)
    assert np.array_equal(got, t.developed)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
    print(f"developed image: max relative error {err[want != 0].max():.3e}")
    assert (err[want != 0] < 1e-6).all() and (got[want == 0] == 0).all()
    assert want.max() > 0.1
    # without the property nothing is set
    t = ProgressivePathTracer({})
    t.preprocess(sc)
    t.render(1)
    assert t.filtered is None and t.developed is None
    t.postprocess()


def test_box_table_consistency(pg, cornell):
    """the box table (radius 0.5, every entry 1) weighs a sample 1 in its own pixel, unless its jitter lies on a
    pixel edge, where the neighbour's tap is in range too"""
    sc, samples, _ = cornell
    d = make_dev(pg, sc, tables()["box"])
    d.render_pass(SPP, 0)
    raw = d.read_film_filtered(raw=True)
    n = d.read_film()[0][..., 3]
    d.close()
    pix = np.arange(48 * 40)
    edge = np.zeros(48 * 40, bool)
    for s in range(SPP):
        jx, jy = R.jitter(pix, s, 1337)
        edge |= (np.minimum(jx, 1 - jx) < 1e-6) | (np.minimum(jy, 1 - jy) < 1e-6)
    near = edge.reshape(40, 48)
    for dy in (-1, 0, 1):  # a sample on an edge also reaches the neighbouring pixel
        for dx in (-1, 0, 1):
            near = near | np.roll(np.roll(edge.reshape(40, 48), dy, 0), dx, 1)
    w = raw[..., 3] / 2.0 ** 28
    assert (~near).mean() > 0.99
    assert np.array_equal(w[~near], n[~near].astype(np.float64))
    assert np.array_equal(raw, reference(sc, tables()["box"], samples))


@pytest.mark.parametrize("cfg", [dict(max_paths_in_flight=1024), dict(max_paths_in_flight=48 * 40), dict(path_lanes=1),
                                 dict(path_lanes=3), dict(tail_paths=-1), dict(tile_size=16), dict(tile_size=64)],
                         ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_determinism(pg, cornell, cfg):
    """pixel-range chunks that start mid-tile (1024), one layer per chunk, lanes, no tail kernel, another tile
    size, and a tile whose padded LDS tile exceeds 64 KiB (the direct variant): the same integers"""
    sc, _, raw = cornell
    assert np.array_equal(gpu_raw(pg, sc, tables()["gaussian"], SPP, **cfg), raw)


CHILD = """
import sys
sys.path.insert(0, {root!r})
import numpy as np, pgload
pg = pgload.load()
from mitsuba_path_guiding_amd.integrator import Device
sys.path.insert(0, {tests!r})
import rfilter_ref as R
d = Device(pg.capi.default_config())
d.upload(pg.scenes.cornell(width=48, height=40))
d.set_rfilter(R.table("gaussian", 0.5))
d.render_pass({spp}, 0)
np.save({out!r}, d.read_film_filtered(raw=True))
d.close()
"""


def test_direct_variant_in_a_fresh_process(pg, cornell, tmp_path):
    """PG_FILM_FILTER_DIRECT=1 (one thread per sample, global adds) against the LDS variant"""
    out = str(tmp_path / "direct.npy")
    env = dict(os.environ, PG_FILM_FILTER_DIRECT="1")
    subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), spp=SPP, out=out)],
                   env=env, check=True, timeout=120)
    assert np.array_equal(np.load(out), cornell[2])


def test_shard_union(pg, cornell):
    sc, _, raw = cornell
    t = tables()["gaussian"]
    border = int(np.ceil(t[0] - 0.5))
    total = np.zeros_like(raw)
    for r in range(4):
        d = make_dev(pg, sc, t, rank=r, world_size=4)
        d.render_pass(SPP, 0)
        part = d.read_film_filtered(raw=True)
        own = d.read_film()[0][..., 3] > 0
        d.close()
        total += part
        assert own.any() and not own.all()
        ys, xs = np.nonzero(own)
        reach = np.zeros_like(own)
        reach[max(ys.min() - border, 0):ys.max() + border + 1, max(xs.min() - border, 0):xs.max() + border + 1] = True
        touched = (part != 0).any(-1)
        assert not touched[~reach].any()
        assert touched[~own].any()  # the border does reach into the neighbours' tiles
    assert np.array_equal(total, raw)


def test_envmap_path_exact(pg):
    sc = pg.scenes.sky_courtyard(width=48, height=32)
    t = tables()["gaussian"]
    raw = gpu_raw(pg, sc, t, 2, off=5)
    ref = reference(sc, t, per_sample_films(pg, sc, 2, off=5))
    assert np.array_equal(raw, ref), np.argwhere(raw != ref)[:8]
    assert np.count_nonzero(raw[..., :3]) > 1000


@pytest.mark.parametrize("wavefront", ["1", "0"])
def test_volpath_exact(pg, monkeypatch, wavefront):
    """both volumetric film sites: the wavefront's lanes and the persistent kernel's chunks"""
    monkeypatch.setenv("PG_VOL_WAVEFRONT", wavefront)
    sc = pg.scenes.smoke(width=32, height=32, res=16)
    t = tables()["gaussian"]
    cfg = dict(integrator=pg.capi.PG_INTEGRATOR_VOLPATH)
    raw = gpu_raw(pg, sc, t, 2, **cfg)
    ref = reference(sc, t, per_sample_films(pg, sc, 2, **cfg))
    assert np.array_equal(raw, ref), np.argwhere(raw != ref)[:8]
    assert np.count_nonzero(raw[..., :3]) > 500


def test_guided_records_and_trees_unchanged(pg, cornell):
    sc = cornell[0]
    out = []
    for table in (None, tables()["gaussian"]):
        d = make_dev(pg, sc, table, guiding=1, s_tree_threshold=300.0)
        off, recs = 0, []
        for it in range(3):
            d.render_pass(2 ** it, off, True)
            rec = d.get_records().reshape(-1, 32)  # in commit order, which no run fixes: compare them sorted
            recs.append(rec[np.lexsort(rec.T[::-1])])
            d.splat_local()
            d.refit(it)
            off += 2 ** it
        out.append((recs, d.get_sdtree(), d.read_film()))
        if table is not None:
            assert d.read_film_filtered(raw=True)[..., 3].sum() > 0
        d.close()
    (r0, t0, f0), (r1, t1, f1) = out
    assert all(len(a) > 0 and np.array_equal(a, b) for a, b in zip(r0, r1))
    assert np.array_equal(t0, t1)
    assert np.array_equal(f0[0], f1[0]) and np.array_equal(f0[1], f1[1])


def test_box_film_sumsq_and_aovs_unchanged(pg, cornell):
    sc = cornell[0]
    out = []
    for table in (None, tables()["gaussian"]):
        d = make_dev(pg, sc, table, aovs=1)
        d.render_pass(SPP, 0)
        out.append(d.read_film() + d.read_aovs())
        d.close()
    for a, b in zip(*out):
        assert a.any() and np.array_equal(a, b)


def test_errors_and_reset(pg, cornell):
    from mitsuba_path_guiding_amd.integrator import PGError
    sc = cornell[0]
    t = tables()["gaussian"]
    d = make_dev(pg, sc)
    with pytest.raises(PGError) as e:
        d.read_film_filtered()
    assert e.value.status == pg.capi.PG_ERR_STATE
    for radius in (0.0, 5.0, -1.0, float("nan")):
        with pytest.raises(PGError) as e:
            d.set_rfilter((radius, t[1]))
        assert e.value.status == pg.capi.PG_ERR_INVALID
    d.set_rfilter(t)
    d.set_rfilter(None)  # off again
    with pytest.raises(PGError) as e:
        d.read_film_filtered()
    assert e.value.status == pg.capi.PG_ERR_STATE
    d.set_rfilter((4.0, t[1]))  # the largest radius
    d.set_rfilter(t)
    assert not d.read_film_filtered(raw=True).any()
    d.render_pass(1, 0)
    with pytest.raises(PGError) as e:
        d.set_rfilter(t)
    assert e.value.status == pg.capi.PG_ERR_STATE
    raw = d.read_film_filtered(raw=True)
    assert raw.any()
    assert np.array_equal(d.read_film_filtered(), (raw.astype(np.float64) * 2.0 ** -28).astype(np.float32))
    d.reset_film()
    assert not d.read_film_filtered(raw=True).any()
    d.render_pass(1, 0)
    assert np.array_equal(d.read_film_filtered(raw=True), raw)
    d.close()
    # set before the scene is uploaded
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config())
    d.set_rfilter(t)
    d.upload(sc)
    d.render_pass(1, 0)
    assert np.array_equal(d.read_film_filtered(raw=True), raw)
    d.close()


def test_banded_camera_map_is_refused(pg, cornell, monkeypatch):
    from mitsuba_path_guiding_amd.integrator import PGError
    monkeypatch.setenv("PG_CAMERA_BANDS", "16")
    d = make_dev(pg, cornell[0])
    with pytest.raises(PGError, match="PG_CAMERA_BANDS") as e:
        d.set_rfilter(tables()["gaussian"])
    assert e.value.status == pg.capi.PG_ERR_INVALID
    d.close()


def test_single_rank_reduce_leaves_the_filtered_film(pg, cornell):
    sc, _, raw4 = cornell
    d = make_dev(pg, sc, tables()["gaussian"])
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")  # single-host bootstrap
    d.comm_init(d.comm_unique_id())
    d.render_pass(SPP, 0)
    raw = d.read_film_filtered(raw=True)
    d.comm_reduce_film(0)
    assert np.array_equal(d.read_film_filtered(raw=True), raw)
    assert np.array_equal(raw, raw4)
    d.close()
