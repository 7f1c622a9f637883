// Test-only shim (tests/test_bvh_reinsert.py, tools/bvh_reinsert_stats.py): everything bvh_shim.cpp exports, built
// over the same pg_bvh.cpp, plus what the reinsertion pass of the builder (PG_BVH_REINSERT) is judged by: the SAH
// cost of the binary tree, the built arrays for byte comparisons, and the node visits and triangle tests of the
// closest-hit walk (the counters of the PG_TRAV_STATS build: 4-wide nodes read, triangles of the leaves reached).
#include "bvh_shim.cpp"

namespace {
// shim_trace's restatement of traverse4 with the counters of PG_TRAV_STATS; returns the hit's BVH-order triangle
uint32_t countedWalk(const float *r, uint64_t &visits, uint64_t &tests) {
    const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]};
    const float eps = 1e-30f;
    float idir[3], ood[3];
    for (int a = 0; a < 3; ++a) {
        idir[a] = 1.0f / (std::fabs(d[a]) > eps ? d[a] : std::copysign(eps, d[a]));
        ood[a] = o[a] * idir[a];
    }
    const float tslack = 1e-6f * std::fmax(std::fmax(std::fabs(ood[0]), std::fabs(ood[1])), std::fabs(ood[2]));
    float addLo[3], addHi[3];
    for (int a = 0; a < 3; ++a) {
        const float se = std::copysign(4.76837158e-7f * std::fabs(ood[a]), idir[a]);
        addLo[a] = -ood[a] - se;
        addHi[a] = -ood[a] + se;
    }
    float tmax = r[7];
    uint32_t best = 0xFFFFFFFFu;
    int32_t st[256];
    int sp = 0;
    st[sp++] = 0;
    while (sp > 0) {
        const int32_t node = st[--sp];
        if (node < 0) {
            const uint32_t lr = ~(uint32_t)node, first = lr >> 4, cnt = lr & 15u;
            tests += cnt;
            for (uint32_t k = 0; k < cnt; ++k) {
                float tt;
                if (triHit(first + k, o, d, r[3], tmax, tt) && accept(tt, tmax, first + k, best)) {
                    tmax = tt;
                    best = first + k;
                }
            }
            continue;
        }
        ++visits;
        const float tcull = tmax * 1.000001f + tslack;
        const float *q = qnode(node);
        float key[4];
        int32_t ref[4];
        for (int s = 0; s < 4; ++s) {
            float cmin = r[3], cmax = tcull, blo[3], bhi[3];
            pg_qnode_box(q, s, blo, bhi);
            for (int a = 0; a < 3; ++a) {
                const float t0 = std::fma(blo[a], idir[a], addLo[a]);
                const float t1 = std::fma(bhi[a], idir[a], addHi[a]);
                cmin = std::fmax(cmin, std::fmin(t0, t1));
                cmax = std::fmin(cmax, std::fmax(t0, t1));
            }
            ref[s] = qref(node, s);
            key[s] = (cmin <= cmax * 1.000000477f && ref[s] != PG_QNODE_EMPTY) ? cmin : INFINITY;
        }
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b)
                if (key[b] > key[a]) {
                    std::swap(key[a], key[b]);
                    std::swap(ref[a], ref[b]);
                }
        for (int s = 0; s < 4; ++s)
            if (key[s] != INFINITY && sp < 256) st[sp++] = ref[s];
    }
    return best;
}
}  // namespace

extern "C" {

// SAH cost of the binary tree the arrays were collapsed from (BvhOut::sah_cost)
float shim_sah_cost() { return g_bvh.sah_cost; }

uint32_t shim_max_depth() { return g_bvh.max_depth; }

// sizes in bytes of nodes, wnodes, order, tris; then the arrays themselves
void shim_sizes(uint64_t *out) {
    out[0] = g_bvh.nodes.size() * 4;
    out[1] = g_bvh.wnodes.size() * 4;
    out[2] = g_bvh.order.size() * 4;
    out[3] = g_bvh.tris.size() * 4;
}
void shim_arrays(void *nodes, void *wnodes, void *order, void *tris) {
    if (!g_bvh.nodes.empty()) std::memcpy(nodes, g_bvh.nodes.data(), g_bvh.nodes.size() * 4);
    if (!g_bvh.wnodes.empty()) std::memcpy(wnodes, g_bvh.wnodes.data(), g_bvh.wnodes.size() * 4);
    if (!g_bvh.order.empty()) std::memcpy(order, g_bvh.order.data(), g_bvh.order.size() * 4);
    if (!g_bvh.tris.empty()) std::memcpy(tris, g_bvh.tris.data(), g_bvh.tris.size() * 4);
}

// rays as shim_trace; out[0] node visits, out[1] triangle tests, out[2] rays that hit, summed over the rays
void shim_visits(const float *rays, uint32_t n, uint64_t *out) {
    uint64_t visits = 0, tests = 0, hits = 0;
    for (uint32_t i = 0; i < n; ++i) hits += countedWalk(rays + 8 * (size_t)i, visits, tests) != 0xFFFFFFFFu;
    out[0] = visits;
    out[1] = tests;
    out[2] = hits;
}
}
