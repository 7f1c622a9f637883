// Test-only: the TriAccel rows of a triangle, shared by the host checks of the shadow-blocker helpers
// (blocker_check.cpp, blocker_shim.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

// TriAccel rows of triangle (A, B, C) (the reference's TriAccel::load, as pg_bvh.cpp builds them): (n_u, n_v, n_d,
// bits(k)), (a_u, a_v, b_nu, b_nv), (c_nu, c_nv, 0, 0).  False for a degenerate triangle.
static inline bool triAccelRows(const float *A, const float *B, const float *C, float *rows) {
    float b[3], c[3], N[3];
    for (int a = 0; a < 3; ++a) {
        b[a] = C[a] - A[a];
        c[a] = B[a] - A[a];
    }
    N[0] = c[1] * b[2] - c[2] * b[1];
    N[1] = c[2] * b[0] - c[0] * b[2];
    N[2] = c[0] * b[1] - c[1] * b[0];
    uint32_t k = 0;
    for (uint32_t a = 1; a < 3; ++a)
        if (fabsf(N[a]) > fabsf(N[k])) k = a;
    if (N[k] == 0.0f) return false;
    const uint32_t u = (k + 1) % 3, v = (k + 2) % 3;
    const float denom = b[u] * c[v] - b[v] * c[u];
    if (denom == 0.0f) return false;
    rows[0] = N[u] / N[k];
    rows[1] = N[v] / N[k];
    rows[2] = (A[0] * N[0] + A[1] * N[1] + A[2] * N[2]) / N[k];
    memcpy(rows + 3, &k, 4);
    rows[4] = A[u];
    rows[5] = A[v];
    rows[6] = -b[v] / denom;
    rows[7] = b[u] / denom;
    rows[8] = c[v] / denom;
    rows[9] = -c[u] / denom;
    rows[10] = rows[11] = 0.0f;
    return true;
}
