// Stand-alone host check of the shadow-blocker helpers (csrc/pg_layout.h "Shadow blockers";
// tests/test_shadow_blockers.py runs it): pg_ray_hits_blockers against the plain TriAccel test on random rays and
// records -- the margins may only ever remove answers -- and pg_select_blockers' threshold, cap and tie rule.
// Prints one line per check and returns the number of failed checks.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../mitsuba-path-guiding_amd/csrc/pg_layout.h"
#include "triaccel_ref.h"

// the walk's leaf test (pg_trace.h triHitRow0) on the host, unshrunk bounds
static bool triHit(const float *r, const float *o, const float *d, float tmin, float tmax, float &tt, float &u, float &v) {
    uint32_t k;
    memcpy(&k, r + 3, 4);
    const float ou = o[(k + 1) % 3], ov = o[(k + 2) % 3], ok = o[k], du = d[(k + 1) % 3], dv = d[(k + 2) % 3], dk = d[k];
    tt = (r[2] - ou * r[0] - ov * r[1] - ok) / (du * r[0] + dv * r[1] + dk);
    if (!(tt >= tmin && tt <= tmax)) return false;
    const float hu = ou + tt * du - r[4], hv = ov + tt * dv - r[5];
    u = hv * r[6] + hu * r[7];
    if (!(u >= 0.0f)) return false;
    v = hu * r[8] + hv * r[9];
    return v >= 0.0f && u + v <= 1.0f;
}

static int check(bool ok, const char *what) {
    printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    return ok ? 0 : 1;
}

int main() {
    int failed = 0;
    std::mt19937 rng(20261019u);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f), U01(0.0f, 1.0f);
    // ---- the margins only ever remove answers
    const uint32_t N = 1000000;
    uint64_t accepted = 0, plain = 0, wrong = 0, nearEdge = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const float scale = i % 3 == 0 ? 1.0f : (i % 3 == 1 ? 40.0f : 0.05f);
        float A[3], B[3], C[3], blk[PG_MAX_BLOCKERS][12];
        const uint32_t nb = 1 + i % PG_MAX_BLOCKERS;
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
            } while (!triAccelRows(A, B, C, rows));
            pg_blocker_record(rows, A, B, C, b, blk[b]);
            for (int a = 0; a < 3; ++a) absmax = fmaxf(absmax, fmaxf(fabsf(A[a]), fmaxf(fabsf(B[a]), fabsf(C[a]))));
        }
        // a ray towards a point of the last triangle, often close to an edge or a vertex, tmax on either side of it
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
        float o[3], d[3], len = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float P = A[a] + w0 * (B[a] - A[a]) + w1 * (C[a] - A[a]);
            o[a] = scale * U(rng);
            d[a] = P - o[a];
            len += d[a] * d[a];
        }
        len = sqrtf(len);
        for (int a = 0; a < 3; ++a) d[a] /= len;
        const float tmin = 1e-4f * fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
        const float tmax = len * (i % 7 == 0 ? 1.0f + 3e-3f * U(rng) : 1.0f + U01(rng));
        const uint32_t hit = pg_ray_hits_blockers(blk, nb, absmax, o, d, tmin, tmax);
        float tt, u, v;
        bool any = false;
        for (uint32_t b = 0; b < nb; ++b) any |= triHit(blk[b], o, d, tmin, tmax, tt, u, v);
        plain += any;
        if (w0 < 1e-3f || w1 < 1e-3f) ++nearEdge;
        if (hit) {
            ++accepted;
            if (hit > nb || !triHit(blk[hit - 1], o, d, tmin, tmax, tt, u, v)) ++wrong;
        }
    }
    printf("%u rays: helper accepted %llu, plain test %llu, near an edge %llu\n", N, (unsigned long long)accepted,
           (unsigned long long)plain, (unsigned long long)nearEdge);
    failed += check(wrong == 0, "every accepted ray passes the plain TriAccel test with t, u, v inside the unshrunk bounds");
    failed += check(accepted > N / 10 && accepted < plain, "the helper fires, and on fewer rays than the plain test");
    {  // rays the margins must refuse: grazing, a zero direction component, a short ray, past tmax
        float A[3] = {0, 0, 0}, B[3] = {4, 0, 0}, C[3] = {0, 4, 0}, rows[12], blk[1][12];
        triAccelRows(A, B, C, rows);
        pg_blocker_record(rows, A, B, C, 7, blk[0]);
        const float o[3] = {1, 1, 2};
        const float straight[3] = {0.01f, 0.02f, -1.0f}, zero[3] = {0.0f, 0.02f, -1.0f}, negzero[3] = {-0.0f, 0.02f, -1.0f};
        const float graze[3] = {1.0f, 0.1f, -0.05f};
        bool ok = pg_ray_hits_blockers(blk, 1, 4.0f, o, straight, 1e-4f, 3.0f) == 8;  // 1 + the triangle's id
        ok &= pg_ray_hits_blockers(blk, 1, 4.0f, o, zero, 1e-4f, 3.0f) == 0;
        ok &= pg_ray_hits_blockers(blk, 1, 4.0f, o, negzero, 1e-4f, 3.0f) == 0;
        ok &= pg_ray_hits_blockers(blk, 1, 4.0f, o, graze, 1e-4f, 100.0f) == 0;
        ok &= pg_ray_hits_blockers(blk, 1, 4.0f, o, straight, 1e-4f, 2.0005f * 1.0002f) == 0;  // ends within 2^-10 of it
        ok &= pg_ray_hits_blockers(blk, 1, 4.0f, o, straight, 1e-4f, 1.9f) == 0;
        ok &= pg_ray_hits_blockers(blk, 1, 400.0f, o, straight, 1e-4f, 3.0f) == 0;  // too small for the scene
        ok &= pg_ray_hits_blockers(blk, 0, 4.0f, o, straight, 1e-4f, 3.0f) == 0;
        uint32_t id;
        memcpy(&id, &blk[0][10], 4);
        ok &= id == 7 && blk[0][11] == 4.0f;
        failed += check(ok, "margin cases: straight hit accepted; zero component, grazing, tmax near the hit, small triangle refused");
    }
    // ---- selection
    {
        std::vector<uint32_t> c(1000, 0);
        uint32_t ids[PG_MAX_BLOCKERS];
        failed += check(pg_select_blockers(c.data(), 1000, 0, ids) == 0, "empty counts give an empty list");
        failed += check(pg_select_blockers(c.data(), 1000, 5000, ids) == 0, "no occluded ray gives an empty list");
        failed += check(pg_select_blockers(c.data(), 0, 0, ids) == 0, "no triangles give an empty list");
        // 6400 shadow rays: the threshold is 100
        c[10] = 3000;
        c[500] = 3201;
        c[7] = 100;
        c[8] = 99;
        uint32_t n = pg_select_blockers(c.data(), 1000, 6400, ids);
        failed += check(n == 3 && ids[0] == 500 && ids[1] == 10 && ids[2] == 7, "1/64 threshold: 100 of 6400 in, 99 out; descending order");
        // the same counts out of 12402 / 12403 shadow rays: the listed 6201 are half of them, or just less
        failed += check(pg_select_blockers(c.data(), 1000, 12402, ids) == 2 && pg_select_blockers(c.data(), 1000, 12403, ids) == 0,
                        "a list that blocked less than half of all shadow rays is dropped");
        // twelve equal counts: the eight lowest ids, in id order
        c.assign(1000, 0);
        for (uint32_t t = 0; t < 12; ++t) c[900 - 50 * t] = 500;
        n = pg_select_blockers(c.data(), 1000, 6000, ids);
        bool ok = n == PG_MAX_BLOCKERS;
        for (uint32_t j = 0; j < n; ++j) ok &= ids[j] == 350 + 50 * j;
        failed += check(ok, "cap at 8; ties go to the lower triangle id");
        // a larger count arriving late displaces the last of a full list
        c[999] = 900;
        c[0] = 500;
        n = pg_select_blockers(c.data(), 1000, 7400, ids);
        ok = n == PG_MAX_BLOCKERS && ids[0] == 999 && ids[1] == 0 && ids[2] == 350 && ids[7] == 600;
        failed += check(ok, "a full list keeps the eight largest");
    }
    return failed;
}
