// Test-only: the TriAccel rows of a triangle exactly as the library stores them (pg_bvh.cpp triAccelRecord; pg_layout.h
// "Triangle records"), for the host checks of the probe-occluder helpers (probe_list_check.cpp, occluder_shim.cpp).
// triaccel_ref.h, which the shadow-blocker checks use, stores b_nu and b_nv (rows[6], rows[7]) the other way round, so
// its records put the barycentric u of pg_trace.h's triHitRow0 on the wrong edge; this header does not share its code.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

// rows: (n_u, n_v, n_d, bits(k)), (a_u, a_v, b_nu, b_nv), (c_nu, c_nv, 0, 0); b = C - A, c = B - A, N = cross(c, b),
// k = the axis of N's largest component, (u, v) = the next two axes.  False for a degenerate triangle.
static inline bool triAccelRowsLib(const float *A, const float *B, const float *C, float *rows) {
    float b[3], c[3], N[3];
    for (int a = 0; a < 3; ++a) {
        b[a] = C[a] - A[a];
        c[a] = B[a] - A[a];
    }
    N[0] = c[1] * b[2] - c[2] * b[1];
    N[1] = c[2] * b[0] - c[0] * b[2];
    N[2] = c[0] * b[1] - c[1] * b[0];
    uint32_t k = 0;
    for (uint32_t a = 0; a < 3; ++a)
        if (fabsf(N[a]) > fabsf(N[k])) k = a;
    const uint32_t u = (k + 1) % 3, v = (k + 2) % 3;
    const float denom = b[u] * c[v] - b[v] * c[u];
    if (N[k] == 0.0f || denom == 0.0f) return false;
    rows[0] = N[u] / N[k];
    rows[1] = N[v] / N[k];
    rows[2] = (A[0] * N[0] + A[1] * N[1] + A[2] * N[2]) / N[k];
    memcpy(rows + 3, &k, 4);
    rows[4] = A[u];
    rows[5] = A[v];
    rows[6] = b[u] / denom;   // b_nu
    rows[7] = -b[v] / denom;  // b_nv
    rows[8] = c[v] / denom;   // c_nu
    rows[9] = -c[u] / denom;  // c_nv
    rows[10] = rows[11] = 0.0f;
    return true;
}
