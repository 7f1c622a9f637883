"""The record comparator (tests/record_parity.py) on oracle data alone, no GPU: the reference stays inside the
bars against itself (bit-equal across thread counts, and inside every bar when the positions are perturbed
by the fp32 noise the GPU's deeper vertices carry), and a subtly wrong record writer would be caught -- each
defective copy below fails the bars tests/test_gpu_records.py asserts (matched share >= 99 %, in-bar share
>= 99 %, counts within 0.1 %), for the reason it names.

Data: the Cornell box at 32 x 32, 4 spp with a tree the oracle trained for 3 iterations (1, 2, 4 spp): 8865
records, 63 % with positive radiance, all guided.
"""
import numpy as np
import pytest

import record_parity as R

MATCH_BAR = IN_BAR = 0.99  # the GPU test's bars


@pytest.fixture(scope="module")
def cornell(pg, O):
    sc = pg.scenes.cornell(32, 32)
    osc = O.OracleScene(pg.capi, sc)
    cfg = pg.capi.default_config(guiding=1, s_tree_threshold=400.0)
    tree, off = R.train_oracle_tree(O, osc, cfg, nthreads=4)
    recs = R.oracle_records(pg.capi, O, osc, cfg, tree, off, nthreads=4)
    lo, hi = (np.asarray(b, np.float64) for b in sc.bounds())
    return dict(sc=sc, osc=osc, tree=tree, off=off, recs=recs, extent=float((hi - lo).max()))


def test_reference_preconditions(cornell):
    r = cornell["recs"]
    assert len(r) >= 2000
    assert (r["radiance"] > 0).mean() >= 0.2
    assert (r["weight"] >= 0).mean() >= 0.5
    assert (r["product"] > 0).mean() >= 0.2


def test_oracle_against_itself_across_threads(pg, O, cornell):
    """nthreads 1 and 4 deliver the records in different orders: all matched, every row bit-equal."""
    cfg = pg.capi.default_config(guiding=1, s_tree_threshold=400.0)
    one = R.oracle_records(pg.capi, O, cornell["osc"], cfg, cornell["tree"], cornell["off"], nthreads=1)
    four = cornell["recs"]
    c = R.compare(four, one, cornell["extent"])
    print(c.summary("oracle 1 thread vs 4"))
    assert c.n_ref == c.n_got and c.matched == c.n_ref and c.in_bar == c.matched
    assert np.array_equal(R.rows(four)[c.ref_index], R.rows(one)[c.got_index])
    assert np.array_equal(R.sorted_rows(four), R.sorted_rows(one))


def _perturbed(recs, rel, extent, seed=1):
    out = recs.copy()
    rng = np.random.default_rng(seed)
    out["pos"] = (recs["pos"].astype(np.float64) + rel * extent * rng.uniform(-1, 1, size=(len(recs), 3)))
    return out[rng.permutation(len(out))]


def test_perturbed_positions_still_match(cornell):
    """Positions off by 2e-7 of the scene extent (the deeper vertices' fp32 noise), records shuffled."""
    ref = cornell["recs"]
    got = _perturbed(ref, 2e-7, cornell["extent"])
    assert (got["pos"] != ref["pos"]).any()
    c = R.compare(ref, got, cornell["extent"])
    print(c.summary("perturbed copy"))
    assert c.matched_share >= 0.999
    assert c.in_bar == c.matched and not c.failing_fields()
    assert c.count_ok


def test_far_positions_do_not_match(cornell):
    ref = cornell["recs"]
    got = ref.copy()
    got["pos"] += np.float32(1e-4 * cornell["extent"])  # ten times the position tolerance
    assert R.compare(ref, got, cornell["extent"]).matched == 0


def _some(n, share, seed):
    return np.random.default_rng(seed).random(n) < share


def _radiance_scaled(r):
    r["radiance"][_some(len(r), 0.05, 2)] *= np.float32(1.01)
    return {"radiance"}


def _product_is_radiance(r):
    g = r["weight"] >= 0
    r["product"][g] = r["radiance"][g]
    return {"product"}


def _dir_halves_swapped(r):
    r["dir"] = (r["dir"] >> 16) | (r["dir"] << 16)
    return {"dir"}


def _bsdf_only_pdf(r):
    r["wo_pdf"][_some(len(r), 0.05, 3)] *= np.float32(0.5)
    return {"wo_pdf"}


def _weight_class_lost(r):
    r["weight"][_some(len(r), 0.05, 4)] = -1.0
    return {"weight_class"}


@pytest.mark.parametrize("defect", [_radiance_scaled, _product_is_radiance, _dir_halves_swapped, _bsdf_only_pdf,
                                    _weight_class_lost], ids=lambda f: f.__name__.strip("_"))
def test_defective_copy_is_caught(cornell, defect):
    """A field wrong on a few percent of the records: everything still matches, the in-bar share falls below
    the GPU test's bar, and the field at fault is the one reported."""
    ref = cornell["recs"]
    got = _perturbed(ref, 2e-7, cornell["extent"])
    fields = defect(got)
    c = R.compare(ref, got, cornell["extent"])
    print(c.summary(defect.__name__))
    assert c.matched_share >= 0.999
    assert c.in_bar_share < IN_BAR
    assert c.failing_fields() == fields
    assert c.worst


def test_lost_records_are_caught(cornell):
    """The last vertex of 5 % of the paths lost (emulated by dropping 5 % of the records): the matched share
    and the count condition both fail, the records that are left stay inside the bars."""
    ref = cornell["recs"]
    got = _perturbed(ref, 2e-7, cornell["extent"])
    got = got[~_some(len(got), 0.05, 5)]
    c = R.compare(ref, got, cornell["extent"])
    print(c.summary("5 % dropped"))
    assert c.matched_share < MATCH_BAR
    assert not c.count_ok
    assert c.in_bar == c.matched


def test_truncated_records_are_a_subset(pg, O, cornell):
    """record_max_vertices = 2 keeps the first two training vertices of every path: a bit-identical subset
    of the default's (32) records, at most two per path; 0 writes none."""
    full = cornell["recs"]
    out = {}
    for maxv in (0, 1, 2):
        cfg = pg.capi.default_config(guiding=1, s_tree_threshold=400.0, record_max_vertices=maxv)
        out[maxv] = R.oracle_records(pg.capi, O, cornell["osc"], cfg, cornell["tree"], cornell["off"], nthreads=4)
    paths = 32 * 32 * R.PASS_SPP
    assert len(out[0]) == 0
    assert 0 < len(out[1]) <= paths and len(out[1]) < len(out[2]) <= 2 * paths and len(out[2]) < len(full)
    assert R.is_row_subset(out[1], out[2]) and R.is_row_subset(out[2], full)
    assert not R.is_row_subset(full, out[2])
    changed = out[2].copy()
    changed["radiance"][0] = np.nextafter(changed["radiance"][0], np.float32(np.inf))
    assert not R.is_row_subset(changed, full)
