"""How a pass is cut into chunks (csrc/pg_chunks.h planChunks, which both schedulers of csrc/pg_pass.cpp consume), on
the CPU: every (pixel, sample layer) pair lies in exactly one chunk, no chunk exceeds the wanted size, a pixel's layers
ascend with the chunk index (films are summed in chunk order), each chunk's sample base is the pass's offset plus its
first layer, and the pixel ranges of one layer group ascend without gaps."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "chunk_shim.cpp")
OFFSET = 7

# (npix, spp, want)
TRIPLES = [
    # want >= npix * spp: one chunk
    (12, 5, 60), (12, 5, 61), (12, 5, 1000), (97, 97, 97 * 97), (1, 1, 1), (1, 1, 5), (5, 1, 5),
    # npix <= want < npix * spp, want a multiple of npix
    (12, 5, 12), (12, 5, 24), (12, 6, 24), (12, 6, 36), (10, 97, 30), (97, 8, 97), (97, 8, 388),
    # ... and not a multiple
    (12, 5, 13), (12, 5, 23), (12, 5, 35), (12, 5, 59), (10, 97, 39), (97, 8, 100), (97, 8, 193),
    # spp not a multiple of want / npix
    (12, 5, 24), (12, 7, 36), (8, 97, 32), (3, 10, 12), (97, 7, 200),
    # npix > want, npix divisible by want
    (12, 5, 6), (12, 5, 4), (12, 1, 3), (96, 3, 32), (64, 2, 8),
    # ... and not
    (12, 5, 5), (12, 5, 7), (12, 5, 11), (97, 3, 32), (97, 2, 96), (13, 97, 4),
    # want = 1, npix = 1, spp = 1
    (12, 5, 1), (1, 5, 1), (1, 97, 1), (1, 97, 10), (1, 97, 96), (97, 1, 1), (97, 1, 10), (97, 1, 96), (97, 1, 97),
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chunkshim") / "chunk_shim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    args = [str(v) for t in TRIPLES for v in t]
    lines = subprocess.check_output([exe, str(OFFSET)] + args, text=True).splitlines()
    out, i = [], 0
    while i < len(lines):
        head = lines[i].split()
        assert head[0] == "plan"
        n = int(head[4])
        out.append((tuple(int(v) for v in head[1:4]), [tuple(int(v) for v in l.split()) for l in lines[i + 1:i + 1 + n]]))
        i += 1 + n
    assert [t for t, _ in out] == TRIPLES
    return dict(out)


def test_the_cases_cover_every_branch():
    one = [t for t in TRIPLES if t[2] >= t[0] * t[1]]
    layers = [t for t in TRIPLES if t[0] <= t[2] < t[0] * t[1]]
    ranges = [t for t in TRIPLES if t[0] > t[2]]
    assert one and any(t[2] % t[0] == 0 for t in layers) and any(t[2] % t[0] for t in layers)
    assert any(t[1] % (t[2] // t[0]) for t in layers)
    assert any(t[0] % t[2] == 0 for t in ranges) and any(t[0] % t[2] for t in ranges)
    assert any(t[2] == 1 for t in TRIPLES) and any(t[0] == 1 for t in TRIPLES) and any(t[1] == 1 for t in TRIPLES)
    assert all(t[0] <= 97 and t[1] <= 97 for t in TRIPLES)


@pytest.mark.parametrize("triple", sorted(set(TRIPLES)))
def test_plan(plans, triple):
    npix, spp, want = triple
    plan = plans[triple]
    assert plan
    if want >= npix * spp:
        assert plan == [(0, npix, spp, OFFSET)]
    seen = {}
    for ci, (pb, np_, nl, base) in enumerate(plan):
        assert np_ >= 1 and nl >= 1 and np_ * nl <= want
        assert pb + np_ <= npix and OFFSET <= base and base - OFFSET + nl <= spp
        for p in range(pb, pb + np_):
            for layer in range(base - OFFSET, base - OFFSET + nl):
                assert (p, layer) not in seen  # covered once
                seen[(p, layer)] = ci
    assert len(seen) == npix * spp  # covered at all
    # a pixel's layers in ascending chunk order
    for p in range(npix):
        order = [seen[(p, layer)] for layer in range(spp)]
        assert order == sorted(order)
    # layer groups: consecutive chunks with the same sample base; pixel ranges ascending and contiguous, the
    # whole group on the same layers, and the groups' first layers ascending without gaps
    groups = []
    for ch in plan:
        if groups and groups[-1][-1][3] == ch[3]:
            groups[-1].append(ch)
        else:
            groups.append([ch])
    layer = 0
    for grp in groups:
        assert grp[0][3] == OFFSET + layer  # sample_base = sample_offset + first layer
        assert len({ch[2] for ch in grp}) == 1
        at = 0
        for pb, np_, _, _ in grp:
            assert pb == at
            at += np_
        assert at == npix
        layer += grp[0][2]
    assert layer == spp
