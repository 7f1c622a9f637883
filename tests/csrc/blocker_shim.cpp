// Test-only C entry point of the host build of pg_ray_hits_blockers (csrc/pg_layout.h), for tests/test_gpu_shadow_cull.py:
// the blocker test on given rays against triangles given by their vertices, so that the test can check its own
// inputs (each ray family must hold rays the test fires on) without the device.
#include <cstring>

#include "../../mitsuba-path-guiding_amd/csrc/pg_layout.h"
#include "triaccel_ref.h"


extern "C" {
// tris: k x 9 floats (three vertices each), k <= PG_MAX_BLOCKERS; rays: n x 8 (o, tmin, d, tmax); out[i] = 1 where
// the host helper answers "certainly occluded".  Returns the number of such rays, -1 on a degenerate triangle.
int blocker_shim_test(const float *tris, uint32_t k, float absmax, const float *rays, uint32_t n, uint32_t *out) {
    float blk[PG_MAX_BLOCKERS][12];
    if (k > PG_MAX_BLOCKERS) return -1;
    for (uint32_t b = 0; b < k; ++b) {
        float rows[12];
        const float *t = tris + 9 * b;
        if (!triAccelRows(t, t + 3, t + 6, rows)) return -1;
        pg_blocker_record(rows, t, t + 3, t + 6, b, blk[b]);
    }
    int fired = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float *r = rays + 8 * (size_t)i;
        out[i] = pg_ray_hits_blockers(blk, k, absmax, r, r + 4, r[3], r[7]) ? 1u : 0u;
        fired += (int)out[i];
    }
    return fired;
}
}
