// Test-only shim (tests/test_bvh4_build.py): the library's BVH builder (pg_bvh.cpp) on the CPU.
// Checks the 4-wide closest-hit layout (pg_layout.h PG_QNODE_*) for structure -- every triangle in
// exactly one leaf, child boxes containing their subtrees, the stack bound -- and runs a scalar
// restatement of the device walk (traverse4: slabRay's padded slab test, widened culling distance, nearest-first
// order, tie rule on the lower original triangle id) against a brute-force loop over the same triangle records (TriAccel).
// The same for the 8-wide any-hit tree of the shadow rays (tests/test_bvh8_build.py): its structure (shim_check_wide)
// and a scalar restatement of traverseWide<true> against brute force (shim_trace_any).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../mitsuba-path-guiding_amd/csrc/pg_bvh.h"
#include "../../mitsuba-path-guiding_amd/csrc/pg_layout.h"

namespace {
pgh::BvhOut g_bvh;
std::vector<float> g_P;
std::vector<uint32_t> g_I;

bool triHit(uint32_t tr, const float *o, const float *d, float tmin, float tmax, float &tt) {
    // the record's three rows, wherever PG_TRI_ROW puts them
    float w[12];
    for (uint32_t r = 0; r < 3; ++r) std::memcpy(&w[4 * r], &g_bvh.tris[4 * (size_t)PG_TRI_ROW(tr, r)], 16);
    // TriAccel::rayIntersect (triaccel.h:96-157), the device triHit's arithmetic (no contraction)
    uint32_t k;
    std::memcpy(&k, &w[3], 4);
    const int iu = k == 0 ? 1 : (k == 1 ? 2 : 0), iv = k == 0 ? 2 : (k == 1 ? 0 : 1), ik = k == 0 ? 0 : (k == 1 ? 1 : 2);
    tt = (w[2] - o[iu] * w[0] - o[iv] * w[1] - o[ik]) / (d[iu] * w[0] + d[iv] * w[1] + d[ik]);
    if (!(tt >= tmin && tt <= tmax)) return false;
    const float hu = o[iu] + tt * d[iu] - w[4], hv = o[iv] + tt * d[iv] - w[5];
    const float u = hv * w[6] + hu * w[7];
    if (!(u >= 0.0f)) return false;
    const float v = hu * w[8] + hv * w[9];
    return v >= 0.0f && u + v <= 1.0f;
}

// the device walks' accept rule (pg_trace.h acceptHit): smaller t, or a tie on the lower original id
bool accept(float tt, float tmax, uint32_t tr, uint32_t best) {
    if (tt < tmax || best == 0xFFFFFFFFu) return true;
    uint32_t a, b;
    std::memcpy(&a, &g_bvh.tris[4 * (size_t)PG_TRI_ROW(tr, 2) + 2], 4);
    std::memcpy(&b, &g_bvh.tris[4 * (size_t)PG_TRI_ROW(best, 2) + 2], 4);
    return a < b;
}

const float *qnode(int32_t n) { return &g_bvh.nodes[(size_t)n * 4 * PG_QNODE_F4]; }
int32_t qref(int32_t n, int s) { return pg_qnode_ref(qnode(n), s); }

constexpr uint32_t kStackLimit = 48;  // pg_trace.h STACK_DEPTH, what the library passes to buildBvh

// 8-wide node (pg_layout.h "8-wide BVH node"): the words as the device walk reads them
struct WideNode {
    float p[3];
    uint32_t e, imask, childBase, triBase;
    uint8_t meta[8], q[6][8];  // q: lo.x lo.y lo.z hi.x hi.y hi.z, slot order
};
WideNode wideNode(uint32_t n) {
    const float *o = &g_bvh.wnodes[(size_t)n * 4 * PG_WIDE_NODE_F4];
    WideNode w;
    std::memcpy(w.p, o, 12);
    std::memcpy(&w.e, o + 3, 4);
    w.imask = w.e >> 24;
    std::memcpy(&w.childBase, o + 4, 4);
    std::memcpy(&w.triBase, o + 5, 4);
    std::memcpy(w.meta, o + 6, 8);
    std::memcpy(w.q, o + 8, 48);
    return w;
}
float wideScale(const WideNode &w, int a) {  // 2^(e_a - 127), the device's bit pattern
    const uint32_t b = ((w.e >> (8 * a)) & 0xFFu) << 23;
    float s;
    std::memcpy(&s, &b, 4);
    return s;
}
void wideBox(const WideNode &w, int s, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = w.p[a] + (float)w.q[a][s] * wideScale(w, a);
        hi[a] = w.p[a] + (float)w.q[3 + a][s] * wideScale(w, a);
    }
}

// pg_trace.h permuteXor8
uint32_t permuteXor8(uint32_t m, uint32_t x) {
    if (x & 1u) m = ((m & 0x55u) << 1) | ((m >> 1) & 0x55u);
    if (x & 2u) m = ((m & 0x33u) << 2) | ((m >> 2) & 0x33u);
    if (x & 4u) m = ((m & 0x0Fu) << 4) | ((m >> 4) & 0x0Fu);
    return m;
}

// traverseWide<true> (pg_trace.h) restated: the group stack, the octant order, the near / far byte planes picked by
// the direction's sign and the slab arithmetic with the device's fmafs; v_max3_f32 / v_min3_f32 as nested
// fmaxf / fminf (no operand is a NaN for the finite scenes and rays of the tests).  The triangle groups are tested
// one triangle at a time in bit order, which is the order the device's pairs keep.  Returns the accepted BVH-order
// triangle or ~0.
uint32_t wideAnyHit(const float *o, const float *d, float tmin, float tmax) {
    const float eps = 1e-30f, kWidePad = 4.76837158e-7f;  // 2^-21
    float idir[3], aN[3], aF[3];  // wideRay: near planes earlier, far planes later by 2^-21 |o_a idir_a|
    uint32_t octinv = 0;
    for (int a = 0; a < 3; ++a) {
        idir[a] = 1.0f / (std::fabs(d[a]) > eps ? d[a] : std::copysign(eps, d[a]));
        octinv |= (idir[a] < 0 ? 0u : 1u) << a;
        const float oa = o[a] * idir[a], sa = kWidePad * std::fabs(oa);
        aN[a] = -oa - sa;
        aF[a] = -oa + sa;
    }
    struct G2 { uint32_t x, y; };
    G2 G{0u, 0x80000000u}, T{0u, 0u};
    std::vector<G2> stk;
    for (;;) {
        if (G.y > 0x00FFFFFFu) {
            const int bit = 31 - __builtin_clz(G.y);
            const uint32_t slot = (uint32_t)(bit - 24) ^ octinv;
            const uint32_t ni = G.x + (uint32_t)__builtin_popcount(G.y & 0xFFu & ((1u << slot) - 1u));
            G.y &= ~(1u << bit);
            if (G.y > 0x00FFFFFFu) stk.push_back(G);
            const WideNode w = wideNode(ni);
            float A[3], Bn[3], Bf[3];  // the node's share of the pad: 2^-21 (|p idir| + 256 |2^e idir|)
            for (int a = 0; a < 3; ++a) {
                A[a] = wideScale(w, a) * idir[a];
                const float g = std::fma(256.0f, std::fabs(A[a]), std::fabs(w.p[a] * idir[a]));
                Bn[a] = std::fma(-kWidePad, g, std::fma(w.p[a], idir[a], aN[a]));
                Bf[a] = std::fma(kWidePad, g, std::fma(w.p[a], idir[a], aF[a]));
            }
            uint32_t hitSlots = 0;
            for (int s = 0; s < 8; ++s) {
                float tn[3], tf[3];
                for (int a = 0; a < 3; ++a) {
                    const bool pos = octinv >> a & 1u;  // the lo plane is the near one
                    tn[a] = std::fma((float)w.q[pos ? a : 3 + a][s], A[a], Bn[a]);
                    tf[a] = std::fma((float)w.q[pos ? 3 + a : a][s], A[a], Bf[a]);
                }
                const float cmin = std::fmax(std::fmax(tn[0], tn[1]), std::fmax(tn[2], tmin));
                const float cmax = std::fmin(std::fmin(tf[0], tf[1]), std::fmin(tf[2], tmax));
                hitSlots |= (cmin <= cmax ? 1u : 0u) << s;
            }
            const uint32_t nodeHits = permuteXor8(hitSlots & w.imask, octinv) << 24;
            uint32_t triHits = 0;
            for (uint32_t leaves = hitSlots & ~w.imask & 0xFFu; leaves; leaves &= leaves - 1u) {
                const uint32_t meta = w.meta[__builtin_ffs((int)leaves) - 1];
                triHits |= ((1u << (meta >> 5)) - 1u) << (meta & 31u);
            }
            G = G2{w.childBase, nodeHits | w.imask};
            T = G2{w.triBase, triHits};
        }
        while (T.y != 0) {
            const uint32_t tr = T.x + (uint32_t)(__builtin_ffs((int)T.y) - 1);
            T.y &= T.y - 1u;
            float tt;
            if (triHit(tr, o, d, tmin, tmax, tt)) return tr;
        }
        if (G.y <= 0x00FFFFFFu) {
            if (stk.empty()) break;
            G = stk.back();
            stk.pop_back();
        }
    }
    return 0xFFFFFFFFu;
}

// t inside the slab interval of triangle tr's own bounding box, widened by 2^-22 (max_a |o_a / d_a| + |t|): the
// rule of test_bvh4_build.consistent_hits, in double
bool boxConsistent(uint32_t tr, const float *o, const float *d, float tt) {
    const uint32_t orig = g_bvh.order[tr];
    double t0 = -INFINITY, t1 = INFINITY, m = 0.0;
    for (int a = 0; a < 3; ++a) {
        double lo = INFINITY, hi = -INFINITY;
        for (int j = 0; j < 3; ++j) {
            const double v = g_P[3 * (size_t)g_I[3 * (size_t)orig + j] + a];
            lo = std::min(lo, v);
            hi = std::max(hi, v);
        }
        const double da = std::fabs((double)d[a]) > 1e-30 ? (double)d[a] : 1e-30;
        const double ta = (lo - o[a]) / da, tb = (hi - o[a]) / da;
        t0 = std::max(t0, std::min(ta, tb));
        t1 = std::min(t1, std::max(ta, tb));
        m = std::max(m, std::fabs(o[a] / da));
    }
    const double pad = std::ldexp(1.0, -22) * (m + std::fabs((double)tt));
    return tt >= t0 - pad && tt <= t1 + pad;
}

// shim_trace_any's rays [lo, hi)
void traceAnyRange(const float *rays, uint32_t lo, uint32_t hi, uint32_t *walk, uint32_t *brute, uint32_t nt) {
    for (uint32_t i = lo; i < hi; ++i) {
        const float *r = rays + 8 * (size_t)i;
        const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]};
        uint32_t cnt = 0, consistent = 0;
        for (uint32_t tr = 0; tr < nt; ++tr) {
            float tt;
            if (!triHit(tr, o, d, r[3], r[7], tt)) continue;
            ++cnt;
            if (!consistent && boxConsistent(tr, o, d, tt)) consistent = 1;
        }
        const uint32_t w = wideAnyHit(o, d, r[3], r[7]);
        float tt;
        walk[i] = w;
        brute[3 * (size_t)i] = cnt;
        brute[3 * (size_t)i + 1] = consistent;
        brute[3 * (size_t)i + 2] = (w < nt && triHit(w, o, d, r[3], r[7], tt)) ? 1u : 0u;
    }
}
}  // namespace

extern "C" {

// 1: built; 0: the builder refused (stack bound)
int shim_build(const float *P, uint32_t nv, const uint32_t *I, uint32_t nt) {
    g_P.assign(P, P + 3 * (size_t)nv);
    g_I.assign(I, I + 3 * (size_t)nt);
    g_bvh = pgh::BvhOut();
    return pgh::buildBvh(g_P.data(), g_I.data(), nt, 48, g_bvh) ? 1 : 0;
}

// BVH-order triangle -> original triangle id
void shim_order(uint32_t *out) {
    for (size_t i = 0; i < g_bvh.order.size(); ++i) out[i] = g_bvh.order[i];
}

// structure of the 4-wide tree: out[0] nodes, out[1] max stack need, out[2] triangles reached
// exactly once (all: == nt), out[3] child boxes not containing their subtree's triangles, out[4] depth
void shim_check(uint32_t nt, uint32_t *out) {
    const uint32_t nn = (uint32_t)(g_bvh.nodes.size() / (4 * PG_QNODE_F4));
    std::vector<uint32_t> seen(nt, 0);
    uint32_t bad = 0, maxNeed = 0, maxDepth = 0;
    struct T { int32_t n; uint32_t need, depth; };
    std::vector<T> st{{0, 1, 1}};
    while (!st.empty()) {
        const T t = st.back();
        st.pop_back();
        maxDepth = std::max(maxDepth, t.depth);
        const float *o = qnode(t.n);
        int used = 0;
        for (int s = 0; s < 4; ++s) used += qref(t.n, s) != PG_QNODE_EMPTY;
        const uint32_t need = t.need + (used > 0 ? used - 1 : 0);
        maxNeed = std::max(maxNeed, need);
        for (int s = 0; s < 4; ++s) {
            const int32_t r = qref(t.n, s);
            if (r == PG_QNODE_EMPTY) continue;
            float lo[3], hi[3];
            pg_qnode_box(o, s, lo, hi);
            // triangles of the child's subtree
            std::vector<int32_t> sub{r};
            while (!sub.empty()) {
                const int32_t m = sub.back();
                sub.pop_back();
                if (m >= 0) {
                    for (int k = 0; k < 4; ++k)
                        if (qref(m, k) != PG_QNODE_EMPTY) sub.push_back(qref(m, k));
                    continue;
                }
                const uint32_t lr = ~(uint32_t)m, first = lr >> 4, cnt = lr & 15u;
                for (uint32_t k = 0; k < cnt; ++k) {
                    const uint32_t orig = g_bvh.order[first + k];
                    for (int j = 0; j < 3; ++j)
                        for (int a = 0; a < 3; ++a) {
                            const float v = g_P[3 * (size_t)g_I[3 * (size_t)orig + j] + a];
                            if (v < lo[a] || v > hi[a]) ++bad;
                        }
                }
            }
            if (r >= 0) {
                st.push_back({r, need, t.depth + 1});
            } else {
                const uint32_t lr = ~(uint32_t)r, first = lr >> 4, cnt = lr & 15u;
                for (uint32_t k = 0; k < cnt; ++k) seen[first + k]++;
            }
        }
    }
    uint32_t once = 0;
    for (uint32_t i = 0; i < nt; ++i) once += seen[i] == 1;
    out[0] = nn;
    out[1] = maxNeed;
    out[2] = once;
    out[3] = bad;
    out[4] = maxDepth;
}

// rays: 8 floats (o, tmin, d, tmax); hits: 2 words (bits(t), BVH-order triangle or ~0) per ray for the
// walk and for brute force
void shim_trace(const float *rays, uint32_t n, uint32_t *walk, uint32_t *brute, uint32_t nt) {
    for (uint32_t i = 0; i < n; ++i) {
        const float *r = rays + 8 * (size_t)i;
        const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]};
        // brute force, the same tie rule
        {
            float tmax = r[7];
            uint32_t best = 0xFFFFFFFFu;
            for (uint32_t tr = 0; tr < nt; ++tr) {
                float tt;
                if (triHit(tr, o, d, r[3], tmax, tt) && accept(tt, tmax, tr, best)) {
                    tmax = tt;
                    best = tr;
                }
            }
            std::memcpy(&brute[2 * i], &tmax, 4);
            brute[2 * i + 1] = best;
        }
        // traverse4
        const float eps = 1e-30f;
        float idir[3], ood[3];
        for (int a = 0; a < 3; ++a) {
            idir[a] = 1.0f / (std::fabs(d[a]) > eps ? d[a] : std::copysign(eps, d[a]));
            ood[a] = o[a] * idir[a];
        }
        const float tslack = 1e-6f * std::fmax(std::fmax(std::fabs(ood[0]), std::fabs(ood[1])), std::fabs(ood[2]));
        float addLo[3], addHi[3];  // slabRay: near planes earlier, far planes later by 2^-21 |o_a idir_a|
        for (int a = 0; a < 3; ++a) {
            const float se = std::copysign(4.76837158e-7f * std::fabs(ood[a]), idir[a]);
            addLo[a] = -ood[a] - se;
            addHi[a] = -ood[a] + se;
        }
        float tmax = r[7];
        uint32_t best = 0xFFFFFFFFu;
        std::vector<int32_t> st{0};
        while (!st.empty()) {
            const int32_t node = st.back();
            st.pop_back();
            if (node < 0) {
                const uint32_t lr = ~(uint32_t)node, first = lr >> 4, cnt = lr & 15u;
                for (uint32_t k = 0; k < cnt; ++k) {
                    float tt;
                    if (triHit(first + k, o, d, r[3], tmax, tt) && accept(tt, tmax, first + k, best)) {
                        tmax = tt;
                        best = first + k;
                    }
                }
                continue;
            }
            const float tcull = tmax * 1.000001f + tslack;
            const float *q = qnode(node);
            float key[4];
            int32_t ref[4];
            for (int s = 0; s < 4; ++s) {
                float cmin = r[3], cmax = tcull, blo[3], bhi[3];
                pg_qnode_box(q, s, blo, bhi);  // the decoded planes (quantised nodes: origin + q 2^e)
                for (int a = 0; a < 3; ++a) {
                    const float t0 = std::fma(blo[a], idir[a], addLo[a]);
                    const float t1 = std::fma(bhi[a], idir[a], addHi[a]);
                    cmin = std::fmax(cmin, std::fmin(t0, t1));
                    cmax = std::fmin(cmax, std::fmax(t0, t1));
                }
                ref[s] = qref(node, s);
                key[s] = (cmin <= cmax * 1.000000477f && ref[s] != PG_QNODE_EMPTY) ? cmin : INFINITY;
            }
            for (int a = 0; a < 4; ++a)  // far to near onto the stack
                for (int b = a + 1; b < 4; ++b)
                    if (key[b] > key[a]) {
                        std::swap(key[a], key[b]);
                        std::swap(ref[a], ref[b]);
                    }
            for (int s = 0; s < 4; ++s)
                if (key[s] != INFINITY) st.push_back(ref[s]);
        }
        std::memcpy(&walk[2 * i], &tmax, 4);
        walk[2 * i + 1] = best;
    }
}

// structure of the 8-wide tree (pg_bvh.cpp buildWide), walked from node 0:
//   out[0] nodes reached            out[1] triangles reached exactly once (all: == nt)
//   out[2] decoded child boxes (p + q 2^(e - 127)) that miss a vertex of their subtree (counted per coordinate)
//   out[3] leaf slots with offset + count > 24 (the width of the walk's triangle hit mask) or a count outside 1..3
//   out[4] slots both in imask and with meta != 0
//   out[5] inner children that are not the consecutive nodes child_base + (rank of the slot in imask) behind their
//          parent, or leaf triangles outside [0, nt)
//   out[6] maximum depth (the root: 1)      out[7] BvhOut::wide_depth      out[8] the stack limit given to buildBvh
void shim_check_wide(uint32_t nt, uint32_t *out) {
    const uint32_t nn = (uint32_t)(g_bvh.wnodes.size() / (4 * PG_WIDE_NODE_F4));
    std::vector<uint32_t> seen(nt, 0);
    uint32_t reached = 0, badBox = 0, badLeaf = 0, badBoth = 0, badRef = 0, maxDepth = 0;
    auto childOf = [](const WideNode &w, int s) {
        return w.childBase + (uint32_t)__builtin_popcount(w.imask & ((1u << s) - 1u));
    };
    auto validChild = [&](uint32_t parent, uint32_t c) { return c < nn && c > parent; };  // appended later: no cycles
    // vertices of the triangles under slot s of node n against that slot's decoded box
    auto checkBox = [&](uint32_t n, int s) {
        const WideNode top = wideNode(n);
        float lo[3], hi[3];
        wideBox(top, s, lo, hi);
        std::vector<std::pair<uint32_t, int>> st{{n, s}};
        while (!st.empty()) {
            const auto [m, sl] = st.back();
            st.pop_back();
            const WideNode w = wideNode(m);
            if (w.imask >> sl & 1u) {
                const uint32_t c = childOf(w, sl);
                if (!validChild(m, c)) continue;  // counted in out[5]
                const WideNode cw = wideNode(c);
                for (int k = 0; k < 8; ++k)
                    if ((cw.imask >> k & 1u) || cw.meta[k]) st.push_back({c, k});
                continue;
            }
            for (uint32_t k = 0; k < (uint32_t)(w.meta[sl] >> 5); ++k) {
                const uint32_t tr = w.triBase + (w.meta[sl] & 31u) + k;
                if (tr >= nt) continue;
                const uint32_t orig = g_bvh.order[tr];
                for (int j = 0; j < 3; ++j)
                    for (int a = 0; a < 3; ++a) {
                        const float v = g_P[3 * (size_t)g_I[3 * (size_t)orig + j] + a];
                        if (v < lo[a] || v > hi[a]) ++badBox;
                    }
            }
        }
    };
    struct T { uint32_t n, depth; };
    std::vector<T> st;
    if (nn > 0) st.push_back({0, 1});
    while (!st.empty()) {
        const T t = st.back();
        st.pop_back();
        ++reached;
        maxDepth = std::max(maxDepth, t.depth);
        const WideNode w = wideNode(t.n);
        uint32_t rank = 0;
        for (int s = 0; s < 8; ++s) {
            const bool inner = w.imask >> s & 1u;
            if (inner && w.meta[s]) ++badBoth;
            if (!inner && !w.meta[s]) continue;  // empty slot
            if (inner) {
                const uint32_t c = childOf(w, s);
                if (c != w.childBase + rank++ || !validChild(t.n, c)) {
                    ++badRef;
                    continue;
                }
                st.push_back({c, t.depth + 1});
            } else {
                const uint32_t off = w.meta[s] & 31u, cnt = w.meta[s] >> 5;
                if (off + cnt > 24 || cnt < 1 || cnt > 3) ++badLeaf;
                for (uint32_t k = 0; k < cnt; ++k) {
                    if (w.triBase + off + k < nt) seen[w.triBase + off + k]++;
                    else ++badRef;
                }
            }
            checkBox(t.n, s);
        }
    }
    uint32_t once = 0;
    for (uint32_t i = 0; i < nt; ++i) once += seen[i] == 1;
    out[0] = reached;
    out[1] = once;
    out[2] = badBox;
    out[3] = badLeaf;
    out[4] = badBoth;
    out[5] = badRef;
    out[6] = maxDepth;
    out[7] = g_bvh.wide_depth;
    out[8] = kStackLimit;
}

// Shadow rays.  rays: 8 floats (o, tmin, d, tmax), as shim_trace.  walk[i]: the BVH-order triangle the restated
// traverseWide<true> accepts, ~0: not occluded.  brute[3 i]: the number of triangle records whose test accepts the
// ray; brute[3 i + 1]: 1 if at least one of them is box-consistent (boxConsistent); brute[3 i + 2]: 1 if the record
// test accepts the walk's triangle (0 when the walk returned none).
void shim_trace_any(const float *rays, uint32_t n, uint32_t *walk, uint32_t *brute, uint32_t nt) {
    // the rays are independent and the tree is only read: large batches are split over a few threads
    const uint32_t nth = n < 4096 ? 1u : std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (uint32_t k = 0; k < nth; ++k)
        th.emplace_back(traceAnyRange, rays, (uint32_t)((uint64_t)n * k / nth), (uint32_t)((uint64_t)n * (k + 1) / nth),
                        walk, brute, nt);
    for (auto &t : th) t.join();
}
}
