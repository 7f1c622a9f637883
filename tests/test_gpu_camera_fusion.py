"""Camera fusion (DESIGN.md section 5 "Camera fusion"): a chunk's first launch generates the camera rays it traces
(k_camera_trace) instead of reading back what k_camera stored.  It computes the slots of the interleaved camera queue in
closed form (pg_kernels.h pg_camera_slot) and stores neither the queue nor ray_o, so everything a job produces -- films,
sums of squares, SD-trees, training records (sorted: no run fixes the commit order), AOV buffers and every pg_stats
counter but the launch timers -- must equal, element for element, what the two launches give with
PG_NO_CAMERA_FUSION=1.

The configurations sit where the slot arithmetic can go wrong, not at workload size: chunks of 1, 63, 65, 4095, 4096
and 4097 paths (one lane short of and past a wave and a 64 x 64 block of the map), 851 pixels at 3 spp (a layer boundary
inside a wave), several chunks per pass on 1 and 3 lanes (whole layers, and pixel ranges with pix_begin != 0), rank 1 of
a 2-rank tile shard (a local_pixels subset), the thin lens, the environment-lit courtyard (the ENV instantiation, shaded
per class), AOVs, and a guided job with two recording passes.  Every case runs with the tail off (the bounce launches
follow the fused one) and with the default tail, which at these sizes takes the chunk over straight after the camera
rays and walks the camera queue (filled by k_camera_queue then).  PG_CAMERA_BANDS has no closed-form inverse and keeps
the two launches: it must still render the same film."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("PG_NO_CAMERA_FUSION", "PG_CAMERA_BANDS", "PG_NO_RAYS_FUSION", "PG_NO_SHADE_FUSION", "PG_NO_DOOM_PROBE",
            "PG_NO_PATH_CULL", "PG_NO_PROBE_LIST")
TAILS = (-1, 0)  # pg_config.tail_paths: off, the default (2^17 paths)


def _counters(d):
    return {k: v for k, v in d.stats().items() if not k.endswith("_ms")}


def _job(pg, sc, spp=1, lens=None, train=0, **cfg):
    """`train` recording passes (1, 2, ... spp) with their refits, then an spp-sample render; everything it produced"""
    from mitsuba_path_guiding_amd.integrator import Device
    d = Device(pg.capi.default_config(**cfg))
    d.upload(sc)
    if lens is not None:
        d.set_lens(*lens)
    out = {"recs": []}
    off = 0
    for it in range(train):
        d.render_pass(2 ** it, off, True)
        rec = d.get_records().reshape(-1, 32)
        out["recs"].append(rec[np.lexsort(rec.T[::-1])])
        d.splat_local()
        d.refit(it)
        off += 2 ** it
    if train:
        out["train_film"] = d.read_film()
        d.reset_film()
    d.render_pass(spp, off)
    out["film"] = d.read_film()
    if cfg.get("aovs"):
        out["aovs"] = d.read_aovs()
    if train:
        out["tree"] = d.get_sdtree()
    out["stats"] = _counters(d)
    d.close()
    return out


def _same(a, b):
    for k in ("film", "train_film", "aovs"):
        assert (k in a) == (k in b)
        if k in a:
            for x, y in zip(a[k], b[k]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
    if "tree" in a:
        assert np.array_equal(a["tree"], b["tree"])
    assert len(a["recs"]) == len(b["recs"])
    for x, y in zip(a["recs"], b["recs"]):
        assert len(x) > 0 and np.array_equal(x, y)
    assert a["stats"] == b["stats"]


def _both(pg, monkeypatch, sc, tails=TAILS, **kw):
    """the job fused and with PG_NO_CAMERA_FUSION=1, for each tail setting; the fused results"""
    outs = []
    for tail in tails:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        on = _job(pg, sc, tail_paths=tail, **kw)
        monkeypatch.setenv("PG_NO_CAMERA_FUSION", "1")
        off = _job(pg, sc, tail_paths=tail, **kw)
        monkeypatch.delenv("PG_NO_CAMERA_FUSION")
        _same(on, off)
        assert on["film"][0][..., 3].sum() > 0 and on["stats"]["segments"] >= on["stats"]["paths"] > 0
        outs.append(on)
    return outs


@pytest.mark.parametrize("width,height,spp", [(1, 1, 1), (9, 7, 1), (13, 5, 1), (65, 63, 1), (64, 64, 1), (17, 241, 1),
                                              (37, 23, 3)])
def test_paths_per_chunk(pg, monkeypatch, width, height, spp):
    sc = pg.scenes.cornell(width, height)
    for out in _both(pg, monkeypatch, sc, spp=spp):
        assert out["stats"]["paths"] == width * height * spp
        assert np.all(out["film"][0][..., 3] == spp)  # every pixel got every sample


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("cap", [1000, 500])  # 851 pixels: whole layers per chunk, pixel ranges (pix_begin != 0)
def test_several_chunks(pg, monkeypatch, lanes, cap):
    sc = pg.scenes.cornell(37, 23)
    for out in _both(pg, monkeypatch, sc, spp=5, max_paths_in_flight=cap, path_lanes=lanes):
        assert out["stats"]["paths"] == 37 * 23 * 5
        assert np.all(out["film"][0][..., 3] == 5)


def test_rank_shard(pg, monkeypatch):
    sc = pg.scenes.cornell(96, 64)  # six 32 x 32 tiles
    whole = _both(pg, monkeypatch, sc, spp=2, tails=(-1,))[0]["film"]
    parts = [_both(pg, monkeypatch, sc, spp=2, rank=r, world_size=2) for r in range(2)]
    for t in range(len(TAILS)):
        w0, w1 = parts[0][t]["film"][0][..., 3], parts[1][t]["film"][0][..., 3]
        assert w1.sum() > 0 and w0.sum() > 0 and np.all((w0 > 0) != (w1 > 0))  # disjoint, together every pixel
        for k in range(2):
            assert np.array_equal(parts[0][t]["film"][k] + parts[1][t]["film"][k], whole[k])


def test_thin_lens(pg, monkeypatch):
    sc = pg.scenes.cornell(37, 23)
    lens = _both(pg, monkeypatch, sc, spp=3, lens=(0.05, 3.0))
    pin = _both(pg, monkeypatch, sc, spp=3, tails=(-1,))
    assert not np.array_equal(lens[0]["film"][0], pin[0]["film"][0])  # the lens is really on


@pytest.mark.parametrize("aovs", [0, 1])
def test_environment_courtyard(pg, monkeypatch, aovs):
    sc = pg.scenes.sky_courtyard(37, 23, env=pg.scenes.sky_envmap(64, 32, sun_radiance=20.0))
    for out in _both(pg, monkeypatch, sc, spp=3, aovs=aovs):
        assert out["stats"]["escaped"] > 0
        if aovs:
            assert np.all(out["aovs"][0][..., 3] == 3)


def test_aovs(pg, monkeypatch):
    sc = pg.scenes.cornell(37, 23)
    for out in _both(pg, monkeypatch, sc, spp=3, aovs=1):
        alb, nrm = out["aovs"]
        assert np.all(alb[..., 3] == 3) and alb[..., :3].sum() > 0 and np.abs(nrm[..., :3]).sum() > 0


@pytest.mark.parametrize("cap", [0, 500])
def test_guided_job(pg, monkeypatch, cap):
    sc = pg.scenes.cornell(37, 23)
    for out in _both(pg, monkeypatch, sc, spp=4, train=2, guiding=1, s_tree_threshold=400.0, max_paths_in_flight=cap):
        assert len(out["recs"]) == 2 and out["stats"]["records"] > 0


def test_camera_bands_keep_the_two_launches(pg, monkeypatch):
    sc = pg.scenes.cornell(64, 64)  # 4096 pixels: the banded map engages
    for tail in TAILS:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        fused = _job(pg, sc, spp=2, tail_paths=tail)
        monkeypatch.setenv("PG_CAMERA_BANDS", "8")
        banded = _job(pg, sc, spp=2, tail_paths=tail)
        monkeypatch.setenv("PG_NO_CAMERA_FUSION", "1")
        banded_off = _job(pg, sc, spp=2, tail_paths=tail)
        _same(banded, banded_off)
        _same(fused, banded)  # paths are pure functions of (pixel, sample): the map changes no result
