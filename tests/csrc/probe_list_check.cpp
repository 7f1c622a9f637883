// Stand-alone host check of the probe-occluder helpers (csrc/pg_layout.h "Probe occluders"; tests/test_probe_list.py
// runs it, and it is the program to build with -fsanitize=address,undefined): pg_ray_hits_occluders against the plain
// TriAccel test with tmax = +inf on random rays and records -- the margins may only ever remove answers --, the margin
// cases, agreement with pg_ray_hits_blockers where both are defined, and pg_select_listed's threshold, caps and tie
// rule.  Prints one line per check and returns the number of failed checks.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../mitsuba-path-guiding_amd/csrc/pg_layout.h"
#include "triaccel_rows.h"

// the probe walk's leaf test (pg_trace.h triHitRow0) on the host: t in [tmin, inf]
static bool triHit(const float *r, const float *o, const float *d, float tmin, float &tt, float &u, float &v) {
    uint32_t k;
    memcpy(&k, r + 3, 4);
    const float ou = o[(k + 1) % 3], ov = o[(k + 2) % 3], ok = o[k], du = d[(k + 1) % 3], dv = d[(k + 2) % 3], dk = d[k];
    tt = (r[2] - ou * r[0] - ov * r[1] - ok) / (du * r[0] + dv * r[1] + dk);
    if (!(tt >= tmin && tt <= __builtin_huge_valf())) return false;
    const float hu = ou + tt * du - r[4], hv = ov + tt * dv - r[5];
    u = hv * r[6] + hu * r[7];
    if (!(u >= 0.0f)) return false;
    v = hu * r[8] + hv * r[9];
    return v >= 0.0f && u + v <= 1.0f;
}

// the same question asked of the vertices, in double and without the records: does o + t d, t > 0, pass through
// triangle (A, B, C), its barycentric weights within `slack` of [0, 1]?  (Moeller-Trumbore)
static bool geomHit(const float *A, const float *B, const float *C, const float *o, const float *d, double slack) {
    double e1[3], e2[3], pv[3], tv[3], qv[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = (double)B[a] - A[a];
        e2[a] = (double)C[a] - A[a];
        tv[a] = (double)o[a] - A[a];
    }
    pv[0] = d[1] * e2[2] - d[2] * e2[1];
    pv[1] = d[2] * e2[0] - d[0] * e2[2];
    pv[2] = d[0] * e2[1] - d[1] * e2[0];
    const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (det == 0.0) return false;
    const double u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) / det;
    qv[0] = tv[1] * e1[2] - tv[2] * e1[1];
    qv[1] = tv[2] * e1[0] - tv[0] * e1[2];
    qv[2] = tv[0] * e1[1] - tv[1] * e1[0];
    const double v = ((double)d[0] * qv[0] + (double)d[1] * qv[1] + (double)d[2] * qv[2]) / det;
    const double t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) / det;
    return t > 0.0 && u >= -slack && v >= -slack && u + v <= 1.0 + slack;
}

static int check(bool ok, const char *what) {
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    return ok ? 0 : 1;
}

int main() {
    int failed = 0;
    std::mt19937 rng(20261020u);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f), U01(0.0f, 1.0f);
    // ---- the margins only ever remove answers
    const uint32_t N = 1000000;
    uint64_t accepted = 0, plain = 0, wrong = 0, tooNear = 0, offTriangle = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const float scale = i % 3 == 0 ? 1.0f : (i % 3 == 1 ? 40.0f : 0.05f);
        float A[3], B[3], C[3], prb[PG_PROBE_LIST_MAX][12], vtx[PG_PROBE_LIST_MAX][9];
        const uint32_t nb = 1 + i % PG_PROBE_LIST_MAX;
        float absmax = 0.0f;
        for (uint32_t b = 0; b < nb; ++b) {
            float rows[12];
            do {
                for (int a = 0; a < 3; ++a) {
                    A[a] = scale * U(rng);
                    B[a] = scale * U(rng);
                    C[a] = scale * U(rng);
                }
                if (i % 5 == 0) B[i % 3] = C[i % 3] = A[i % 3];  // axis-aligned: a flat box, as a wall's
            } while (!triAccelRowsLib(A, B, C, rows));
            pg_blocker_record(rows, A, B, C, b, prb[b]);
            memcpy(vtx[b], A, 12);
            memcpy(vtx[b] + 3, B, 12);
            memcpy(vtx[b] + 6, C, 12);
            for (int a = 0; a < 3; ++a) absmax = fmaxf(absmax, fmaxf(fabsf(A[a]), fmaxf(fabsf(B[a]), fabsf(C[a]))));
        }
        // a ray towards a point of the last triangle, often close to an edge or a vertex; every seventh starts
        // within a few margins of it
        float w0 = U01(rng), w1 = U01(rng);
        if (w0 + w1 > 1.0f) {
            w0 = 1.0f - w0;
            w1 = 1.0f - w1;
        }
        if (i % 4 == 1) w0 *= 1e-3f * U01(rng);
        if (i % 4 == 2) {
            w0 *= 2e-3f * U01(rng);
            w1 *= 2e-3f * U01(rng);
        }
        float o[3], d[3], P[3], len = 0.0f;
        for (int a = 0; a < 3; ++a) {
            P[a] = A[a] + w0 * (B[a] - A[a]) + w1 * (C[a] - A[a]);
            o[a] = scale * U(rng);
            d[a] = P[a] - o[a];
            len += d[a] * d[a];
        }
        len = sqrtf(len);
        for (int a = 0; a < 3; ++a) d[a] /= len;
        if (i % 7 == 0) {
            const float back = 1e-4f * scale * U01(rng);
            for (int a = 0; a < 3; ++a) o[a] = P[a] - back * d[a];
        }
        const float tmin = 1e-4f * fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
        const uint32_t hit = pg_ray_hits_occluders(prb, nb, absmax, o, d, tmin);
        float tt, u, v;
        bool any = false;
        for (uint32_t b = 0; b < nb; ++b) any |= triHit(prb[b], o, d, tmin, tt, u, v);
        plain += any;
        if (hit) {
            ++accepted;
            if (hit > nb || !triHit(prb[hit - 1], o, d, tmin, tt, u, v)) ++wrong;
            // ... and the ray really passes through that triangle: the 2^-10 margin leaves no room for fp32 rounding
            else if (!geomHit(vtx[hit - 1], vtx[hit - 1] + 3, vtx[hit - 1] + 6, o, d, 0.0)) ++offTriangle;
            // the distance margin: 2^-15 E / max|d| past tmin
            const float E = absmax + fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
            const float dmax = fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2]));
            if (!(tt >= tmin + PG_PROBE_TMIN_MARGIN * E / dmax)) ++tooNear;
        }
    }
    printf("%u rays: helper accepted %llu, plain test %llu\n", N, (unsigned long long)accepted, (unsigned long long)plain);
    failed += check(wrong == 0, "every accepted ray passes the plain TriAccel test of the triangle it names, tmax = inf");
    failed += check(offTriangle == 0, "every accepted ray passes through the named triangle's vertices (double precision, no records)");
    // every ray is aimed at a point of the last triangle; one in seven starts too close to it for tmin
    failed += check(plain > N / 10 * 8, "the records are the triangles': the plain test finds the triangle the ray is aimed at");
    failed += check(tooNear == 0, "every accepted hit is 2^-15 E / max|d| past tmin");
    failed += check(accepted > N / 10 && accepted < plain, "the helper fires, and on fewer rays than the plain test");
    {  // rays the margins must refuse
        float A[3] = {0, 0, 0}, B[3] = {4, 0, 0}, C[3] = {0, 4, 0}, rows[12], prb[2][12];
        triAccelRowsLib(A, B, C, rows);
        pg_blocker_record(rows, A, B, C, 7, prb[0]);
        float A2[3] = {0, 0, -3}, B2[3] = {4, 0, -3}, C2[3] = {0, 4, -3};
        triAccelRowsLib(A2, B2, C2, rows);
        pg_blocker_record(rows, A2, B2, C2, 9, prb[1]);
        const float o[3] = {1, 1, 2}, near[3] = {1, 1, 1e-4f}, behind[3] = {1, 1, -1};
        const float straight[3] = {0.01f, 0.02f, -1.0f}, zero[3] = {0.0f, 0.02f, -1.0f}, negzero[3] = {-0.0f, 0.02f, -1.0f};
        const float graze[3] = {1.0f, 0.1f, -0.05f}, away[3] = {0.01f, 0.02f, 1.0f};
        bool ok = pg_ray_hits_occluders(prb, 1, 4.0f, o, straight, 1e-4f) == 8;  // 1 + the triangle's id
        ok &= pg_ray_hits_occluders(prb, 1, 4.0f, o, zero, 1e-4f) == 0;
        ok &= pg_ray_hits_occluders(prb, 1, 4.0f, o, negzero, 1e-4f) == 0;
        ok &= pg_ray_hits_occluders(prb, 1, 4.0f, o, graze, 1e-4f) == 0;
        ok &= pg_ray_hits_occluders(prb, 1, 4.0f, o, away, 1e-4f) == 0;                 // the hit is behind the origin
        ok &= pg_ray_hits_occluders(prb, 1, 4.0f, near, straight, 1e-8f) == 0;          // within 2^-15 E of the origin
        ok &= pg_ray_hits_occluders(prb, 1, 4.0f, o, straight, 2.5f) == 0;              // tmin past the hit
        ok &= pg_ray_hits_occluders(prb, 1, 400.0f, o, straight, 1e-4f) == 0;           // too small for the scene
        ok &= pg_ray_hits_occluders(prb, 0, 4.0f, o, straight, 1e-4f) == 0;
        // any listed triangle anywhere along the ray: the first in list order that qualifies, however far
        ok &= pg_ray_hits_occluders(prb, 2, 4.0f, o, straight, 1e-4f) == 8;
        ok &= pg_ray_hits_occluders(prb, 2, 4.0f, behind, straight, 1e-4f) == 10;
        ok &= pg_ray_hits_occluders(prb + 1, 1, 4.0f, o, straight, 1e-4f) == 10;        // through the unlisted nearer one
        failed += check(ok, "margin cases: straight hits accepted at any distance; zero component, grazing, near origin, small refused");
    }
    {  // where a tmax is given as well, the blocker test never accepts a ray the occluder test refuses for its record
        float A[3] = {0, 0, 0}, B[3] = {4, 0, 0}, C[3] = {0, 4, 0}, rows[12], prb[1][12];
        triAccelRowsLib(A, B, C, rows);
        pg_blocker_record(rows, A, B, C, 3, prb[0]);
        uint64_t both = 0, onlyBlocker = 0;
        for (uint32_t i = 0; i < 200000; ++i) {
            float o[3] = {4 * U01(rng), 4 * U01(rng), 3 * U(rng)}, d[3] = {U(rng), U(rng), U(rng)};
            const float tmin = 1e-4f * fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
            const bool b = pg_ray_hits_blockers(prb, 1, 4.0f, o, d, tmin, 1e3f) != 0;
            const bool p = pg_ray_hits_occluders(prb, 1, 4.0f, o, d, tmin) != 0;
            both += b && p;
            onlyBlocker += b && !p;
        }
        printf("blocker test with tmax = 1e3 and occluder test: both %llu, blocker only %llu\n", (unsigned long long)both,
               (unsigned long long)onlyBlocker);
        failed += check(both > 1000 && onlyBlocker == 0, "a long shadow ray's certain hit is a probe's certain hit");
    }
    // ---- selection at the probe list's capacity
    {
        std::vector<uint32_t> c(1000, 0);
        uint32_t ids[PG_PROBE_LIST_MAX];
        failed += check(pg_select_listed(c.data(), 1000, 0, PG_PROBE_LIST_MAX, ids) == 0 &&
                            pg_select_listed(c.data(), 1000, 5000, PG_PROBE_LIST_MAX, ids) == 0 &&
                            pg_select_listed(c.data(), 0, 0, PG_PROBE_LIST_MAX, ids) == 0,
                        "empty counts, no hits, no triangles give an empty list");
        c[10] = 3000;
        c[500] = 3201;
        c[7] = 100;
        c[8] = 99;
        uint32_t n = pg_select_listed(c.data(), 1000, 6400, PG_PROBE_LIST_MAX, ids);
        failed += check(n == 3 && ids[0] == 500 && ids[1] == 10 && ids[2] == 7, "1/64 threshold: 100 of 6400 in, 99 out; descending order");
        failed += check(pg_select_listed(c.data(), 1000, 12402, PG_PROBE_LIST_MAX, ids) == 2 &&
                            pg_select_listed(c.data(), 1000, 12403, PG_PROBE_LIST_MAX, ids) == 0,
                        "a list that took less than half of all probes is dropped");
        // twenty equal counts: the sixteen lowest ids, in id order; with cap 8 the eight lowest
        c.assign(1000, 0);
        for (uint32_t t = 0; t < 20; ++t) c[950 - 50 * t] = 300;
        n = pg_select_listed(c.data(), 1000, 6000, PG_PROBE_LIST_MAX, ids);
        bool ok = n == PG_PROBE_LIST_MAX;
        for (uint32_t j = 0; j < n; ++j) ok &= ids[j] == 50 * j;
        uint32_t ids8[PG_MAX_BLOCKERS];
        // eight of them hold 2400 of 6000: less than half, so the shorter list is dropped; of 4800 it is kept
        ok &= pg_select_blockers(c.data(), 1000, 6000, ids8) == 0;
        const uint32_t n8 = pg_select_blockers(c.data(), 1000, 4800, ids8);
        ok &= n8 == PG_MAX_BLOCKERS;
        for (uint32_t j = 0; j < n8; ++j) ok &= ids8[j] == 50 * j;
        failed += check(ok, "cap at 16 (8 for the blockers); ties go to the lower triangle id");
        // a larger count arriving late displaces the last of a full list
        c[999] = 900;
        n = pg_select_listed(c.data(), 1000, 6900, PG_PROBE_LIST_MAX, ids);
        ok = n == PG_PROBE_LIST_MAX && ids[0] == 999 && ids[1] == 0 && ids[15] == 700;
        failed += check(ok, "a full list keeps the sixteen largest");
    }
    return failed;
}
