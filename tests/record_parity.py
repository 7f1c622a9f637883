"""Comparator for training records (pg_record, 32 bytes: position, packed direction, radiance, wo_pdf,
product, weight): the records one side wrote against the records of a reference, used by
tests/test_record_parity.py (oracle against itself and against defective copies), tests/test_gpu_records.py
and tests/test_gpu_volume.py (GPU against the oracle).

Records come back in arbitrary order and carry no pixel id, and the positions of deeper vertices are not
bit-equal between the GPU and the oracle (sampled directions agree to ~1e-6, test_bsdf_parity), so the two
sets are matched geometrically: key = position . (a fixed unit vector) in float64; one side is sorted by key
and the other looked up in it with searchsorted.  A record within `POS_TOL` x scene extent (max-norm) has a
key within sqrt(3) x that distance, so the candidates of a reference record are the window of sorted
neighbours starting at the first key inside that range; the nearest candidate inside the position tolerance
is taken, each record of the other side at most once.

The bars on a matched pair (fixed by the project's fp32 per-query bar; not tuned to any
output):
    dir                both u16 halves within 1 quantum (the high half, phi, modulo 65536)
    wo_pdf, radiance,  within 1e-3 relative; radiance and product are differences L_final - L_snapshot that
    product, weight    lose precision to cancellation, so they also pass within an absolute floor of 1e-3 x
    (where >= 0)       the median positive reference value of that field
    classes            weight's sign class (-1 or >= 0) equal, radiance == 0 and product == 0 equal
"""
import collections

import numpy as np

RECORD = np.dtype([("pos", "<f4", 3), ("dir", "<u4"), ("radiance", "<f4"), ("wo_pdf", "<f4"), ("product", "<f4"),
                   ("weight", "<f4")])
assert RECORD.itemsize == 32

POS_TOL = 1e-5   # x scene extent, max-norm
REL_TOL = 1e-3   # fp32 per-query results
FLOOR = 1e-3     # x median positive reference value (radiance, product)
COUNT_TOL = 1e-3  # record counts (test_guided_volpath_same_tree_parity's bar)
ALL_FIELDS = ("dir", "wo_pdf", "radiance", "product", "weight", "weight_class", "radiance_zero", "product_zero")
# what oracle/orc_volpath.h writes: product is a constant 0 and weight a constant -1 there
VOLPATH_FIELDS = ("dir", "wo_pdf", "radiance", "weight_class", "radiance_zero")

_AXIS = np.array([0.36817957, 0.74199893, 0.56027486])
_AXIS /= np.linalg.norm(_AXIS)


TRAIN_SPP = (1, 2, 4)  # the oracle's training iterations before the compared pass
PASS_SPP = 4


def train_oracle_tree(O, osc, cfg, nthreads=0, iterations=len(TRAIN_SPP)):
    """An SD-tree trained by the oracle alone (TRAIN_SPP, its own records); returns (tree, next sample offset).
    iterations = 0 gives the unbuilt tree of training iteration 0 at the same sample offset."""
    tree = O.OracleSDTree(osc)
    off = 0
    for it, spp in enumerate(TRAIN_SPP):
        if it < iterations:
            O.render(osc, cfg, spp, sample_offset=off, record=True, sdtree=tree, nthreads=nthreads)
            tree.splat_pending()
            tree.refit(it, cfg)
        off += spp
    return tree, off


def oracle_records(capi, O, osc, cfg, tree, off, spp=PASS_SPP, nthreads=0):
    """The records of one oracle pass with `tree` at sample offset `off`."""
    st = O.render(osc, cfg, spp, sample_offset=off, record=True, sdtree=tree, nthreads=nthreads)[2]
    recs = as_records(tree.take_records(capi))
    assert len(recs) == int(st[3])
    return recs


def as_records(buf):
    """A byte buffer (Device.get_records / OracleSDTree.take_records) or record array as RECORD rows."""
    a = np.ascontiguousarray(buf)
    if a.dtype == RECORD:
        return a
    return np.frombuffer(a.tobytes(), RECORD)


def rows(recs):
    """n x 8 uint32 view of the records' bits."""
    return np.frombuffer(as_records(recs).tobytes(), np.uint32).reshape(-1, 8)


def sorted_rows(recs):
    """The records' bit patterns in lexicographic order: equal arrays <=> equal multisets of records."""
    r = rows(recs)
    return r[np.lexsort(r.T[::-1])]


def is_row_subset(part, whole):
    """Every record of `part` is in `whole` bit for bit, with at least the same multiplicity."""
    w = collections.Counter(x.tobytes() for x in rows(whole))
    p = collections.Counter(x.tobytes() for x in rows(part))
    return all(w[k] >= n for k, n in p.items())


def counts_agree(n_got, n_ref, tol=COUNT_TOL):
    return abs(int(n_got) - int(n_ref)) <= tol * int(n_ref)


def match_positions(ref_pos, got_pos, extent, tol=POS_TOL, max_window=64, chunk=32768):
    """For each reference position the index of its record on the other side, or -1.  A candidate must lie
    within tol x extent (max-norm); each index is given out once, to the nearest claimant."""
    ref = np.asarray(ref_pos, np.float64).reshape(-1, 3)
    got = np.asarray(got_pos, np.float64).reshape(-1, 3)
    out = np.full(len(ref), -1, np.int64)
    if len(ref) == 0 or len(got) == 0:
        return out
    eps = tol * float(extent)
    gk = got @ _AXIS
    order = np.argsort(gk, kind="stable")
    gk = gk[order]
    rk = ref @ _AXIS
    lo = np.searchsorted(gk, rk - np.sqrt(3.0) * eps, "left")
    hi = np.searchsorted(gk, rk + np.sqrt(3.0) * eps, "right")
    W = int(min(max(int((hi - lo).max()), 8), max_window))  # a few neighbours at the least
    cand = np.full((len(ref), W), -1, np.int64)
    dist = np.full((len(ref), W), np.inf)
    for b in range(0, len(ref), chunk):
        e = min(len(ref), b + chunk)
        # centre the window on the key range (it covers the range whenever the range holds <= W records)
        start = np.clip((lo[b:e] + hi[b:e] - W) // 2, 0, max(len(got) - W, 0))
        j = start[:, None] + np.arange(W)[None, :]
        ok = j < len(got)
        j = np.where(ok, j, 0)
        d = np.abs(got[order[j]] - ref[b:e, None, :]).max(-1)
        d = np.where(ok & (d <= eps), d, np.inf)
        cand[b:e] = np.where(np.isfinite(d), order[j], -1)
        dist[b:e] = d
    # nearest first per reference record; rounds of proposals, a contested record goes to the nearest
    s = np.argsort(dist, axis=1, kind="stable")
    cand = np.take_along_axis(cand, s, 1)
    dist = np.take_along_axis(dist, s, 1)
    taken = np.zeros(len(got), bool)
    nxt = np.zeros(len(ref), np.int64)  # next candidate column to try
    active = np.flatnonzero(np.isfinite(dist[:, 0]))
    while len(active):
        c = cand[active, nxt[active]]
        d = dist[active, nxt[active]]
        free = ~taken[c]
        # among the claimants of one free record the nearest wins
        o = np.lexsort((d, c))
        first = np.ones(len(o), bool)
        first[1:] = c[o][1:] != c[o][:-1]
        win = np.zeros(len(active), bool)
        win[o[first]] = True
        win &= free
        out[active[win]] = c[win]
        taken[c[win]] = True
        rest = active[~win]  # their candidate is taken now: on to the next nearest
        nxt[rest] += 1
        rest = rest[nxt[rest] < W]
        active = rest[np.isfinite(dist[rest, nxt[rest]])]
    return out


class Comparison:
    """Result of compare(): counts, shares, per-field failures and the worst pairs."""

    def __init__(self):
        self.n_ref = self.n_got = self.matched = self.in_bar = 0
        self.fail = {}
        self.worst = []
        self.ref_index = self.got_index = None

    @property
    def matched_share(self):  # of the reference's records
        return self.matched / self.n_ref if self.n_ref else 1.0

    @property
    def in_bar_share(self):  # of the matched pairs
        return self.in_bar / self.matched if self.matched else 0.0

    @property
    def count_ok(self):
        return counts_agree(self.n_got, self.n_ref)

    def failing_fields(self):
        return {k for k, n in self.fail.items() if n}

    def summary(self, tag=""):
        f = ", ".join(f"{k} {n}" for k, n in self.fail.items() if n) or "none"
        s = (f"{tag}: records {self.n_got} / {self.n_ref} (reference), matched {self.matched_share:.5f}, "
             f"in every bar {self.in_bar_share:.5f}, outside by field: {f}")
        for w in self.worst:
            s += f"\n    {w}"
        return s


def _rel_ok(g, c, floor=0.0):
    g = g.astype(np.float64)
    c = c.astype(np.float64)
    err = np.abs(g - c)
    with np.errstate(invalid="ignore"):
        ok = (err <= REL_TOL * np.abs(c)) | (err <= floor)
    return ok & np.isfinite(g), err / np.maximum(np.abs(c), 1e-30)


def _floor(values):
    pos = values[values > 0]
    return FLOOR * float(np.median(pos)) if len(pos) else 0.0


def compare(ref, got, extent, fields=ALL_FIELDS, n_worst=5):
    """Match `got` to the reference records `ref` by position and check every matched pair against the bars."""
    ref, got = as_records(ref), as_records(got)
    res = Comparison()
    res.n_ref, res.n_got = len(ref), len(got)
    idx = match_positions(ref["pos"], got["pos"], extent)
    m = idx >= 0
    res.matched = int(m.sum())
    res.ref_index, res.got_index = np.flatnonzero(m), idx[m]
    c, g = ref[m], got[idx[m]]
    ok = {}
    rel = {}
    if "dir" in fields:
        du = np.abs((g["dir"] & 0xFFFF).astype(np.int64) - (c["dir"] & 0xFFFF).astype(np.int64))
        dv = ((g["dir"] >> 16).astype(np.int64) - (c["dir"] >> 16).astype(np.int64)) % 65536
        dv = np.minimum(dv, 65536 - dv)
        ok["dir"] = (du <= 1) & (dv <= 1)
        rel["dir"] = np.maximum(du, dv).astype(np.float64)
    if "wo_pdf" in fields:
        ok["wo_pdf"], rel["wo_pdf"] = _rel_ok(g["wo_pdf"], c["wo_pdf"])
    for f in ("radiance", "product"):
        if f in fields:
            ok[f], rel[f] = _rel_ok(g[f], c[f], _floor(ref[f]))
    if "weight" in fields:
        both = (g["weight"] >= 0) & (c["weight"] >= 0)
        w_ok, w_rel = _rel_ok(g["weight"], c["weight"])
        ok["weight"], rel["weight"] = w_ok | ~both, np.where(both, w_rel, 0.0)
    if "weight_class" in fields:
        cls = lambda w: np.where(w >= 0, 1, np.where(w == -1, 0, 2))
        ok["weight_class"] = (cls(g["weight"]) == cls(c["weight"])) & (cls(g["weight"]) != 2)
    for f in ("radiance", "product"):
        if f + "_zero" in fields:
            ok[f + "_zero"] = (g[f] == 0) == (c[f] == 0)
    every = np.ones(res.matched, bool)
    for k in fields:
        res.fail[k] = int((~ok[k]).sum())
        every &= ok[k]
    res.in_bar = int(every.sum())
    bad = np.flatnonzero(~every)
    if len(bad):
        score = np.zeros(len(bad))
        for k, r in rel.items():
            score = np.maximum(score, np.where(ok[k][bad], 0.0, r[bad]))
        for i in bad[np.argsort(-score, kind="stable")[:n_worst]]:
            which = [k for k in fields if not ok[k][i]]
            res.worst.append(f"{which}: reference {c[i]} got {g[i]}")
    return res
