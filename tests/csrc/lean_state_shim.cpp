// Test-only C entry points of the path-state helpers shared by the shader and the tracers (csrc/pg_layout.h):
// pg_ray_tmin and pg_prev_front, next to the literal expressions they replaced (tests/test_lean_state_helpers.py).
#include "../../mitsuba-path-guiding_amd/csrc/pg_layout.h"

extern "C" {
// p: n x 3; out_new / out_old: n floats
void lean_tmin(const float *p, uint32_t n, float *out_new, float *out_old) {
    const float kEpsilon = 1e-4f;
    for (uint32_t i = 0; i < n; ++i) {
        const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
        out_new[i] = pg_ray_tmin(x, y, z);
        // shadeOne's expression before the helper
        out_old[i] = kEpsilon * fmaxf(fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z)), kEpsilon);
    }
}
// wo, n: count x 3; out_new / out_old: count bytes
void lean_front(const float *wo, const float *nrm, uint32_t count, uint8_t *out_new, uint8_t *out_old) {
    for (uint32_t i = 0; i < count; ++i) {
        const float *a = wo + 3 * (size_t)i, *b = nrm + 3 * (size_t)i;
        out_new[i] = pg_prev_front(a[0], a[1], a[2], b[0], b[1], b[2]) ? 1 : 0;
        // the reading vertex's test before the flag: dot(rd, prevRefN) >= 0 with pg_device.h's dot
        const float d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
        out_old[i] = d >= 0 ? 1 : 0;
    }
}
uint32_t lean_flag_bits(void) { return PF_SCATTERED | PF_EMITTED_QUERY | PF_PREV_DELTA | PF_DOOMED | PF_PREV_FRONT; }
uint32_t lean_prev_front(void) { return PF_PREV_FRONT; }
}
