// Test-only C entry points of the doom probe's host-side helpers (csrc/pg_layout.h): the padded boxes over a scene's
// emitter triangles and the slab test shadeOne runs against them (tests/test_emitter_boxes.py).
#include "../../mitsuba-path-guiding_amd/csrc/pg_layout.h"

extern "C" {
int embox_max(void) { return PG_EMBOX_MAX; }
// boxes: PG_EMBOX_MAX x 6 floats out; returns the number of boxes
uint32_t embox_build(const float *positions, const uint32_t *indices, const uint32_t *tri_emitter, uint32_t nt,
                     uint32_t num_emitters, float *boxes, float *absmax) {
    return pg_emitter_boxes(positions, indices, tri_emitter, nt, num_emitters, reinterpret_cast<float (*)[6]>(boxes), absmax);
}
// rays: n x 7 floats (o.xyz, d.xyz, tmin); out[i] = 1 when ray i misses every box
void embox_misses(const float *boxes, uint32_t nboxes, float absmax, const float *rays, uint32_t n, uint8_t *out) {
    for (uint32_t i = 0; i < n; ++i) {
        const float *r = rays + 7 * (size_t)i;
        out[i] = pg_ray_misses_boxes(reinterpret_cast<const float (*)[6]>(boxes), nboxes, absmax, r, r + 3, r[6]) ? 1 : 0;
    }
}
}
