// Host driver behind the C-ABI (include/pg_capi.h): device context (pg_ctx.h), scene flattening/upload,
// the query entry points, training-record management, the SD-tree refit hook (postprogression,
// src/librender/progressiveintegrator.cpp:314-317) and RCCL.  The pass drivers live in pg_pass.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pg_bvh.h"
#include "pg_ctx.h"
#include "pg_envmap.h"
#include "pg_rtrans.h"

namespace pgh __attribute__((visibility("hidden"))) {

constexpr uint32_t kStackDepth = 48;  // must match STACK_DEPTH in pg_kernels.hip
// the device's bounce cap (GParams::depth_cap): max_depth + 1 or gpu_depth_cap.  The surface path keeps
// one counter block per bounce, so its cap is at most kMaxBounces - 2 (pg_create rejects a larger
// max_depth and clamps gpu_depth_cap there), and the bounce-by-bounce loop (maxBounces = depth_cap + 2 <=
// kMaxBounces) and k_tail, which loops until shadeOne's depth_cap test ends the path, stop at the same
// bounce.  The volumetric path has no per-bounce buffer and honours max_depth exactly.
uint32_t deviceDepthCap(const pg_config &cfg) {
    const int64_t cap = cfg.max_depth > 0 ? (int64_t)cfg.max_depth + 1 : (int64_t)cfg.gpu_depth_cap;
    if (cfg.integrator == PG_INTEGRATOR_VOLPATH) return (uint32_t)std::min<int64_t>(cap, 0x7fffffff);
    return (uint32_t)std::min<int64_t>(cap, (int64_t)kMaxBounces - 2);
}

// shading-queue class of a BSDF model (one specialised k_shade per class)
int materialClass(uint32_t model) {
    switch (model) {
        case PG_BSDF_DIFFUSE: return PG_CLASS_DIFFUSE;
        case PG_BSDF_ROUGHCONDUCTOR: return PG_CLASS_ROUGHCONDUCTOR;
        case PG_BSDF_ROUGHDIELECTRIC: return PG_CLASS_ROUGHDIELECTRIC;
        case PG_BSDF_PLASTIC: return PG_CLASS_PLASTIC;
        case PG_BSDF_ROUGHPLASTIC: return PG_CLASS_ROUGHPLASTIC;
        default: return PG_CLASS_DELTA;
    }
}

#ifndef PG_PIXEL_BLOCK
#define PG_PIXEL_BLOCK 8  // local pixel order inside a tile: 8x8 blocks (0: row-major)
#endif

thread_local std::string g_tls_err;

pg_status fail(Ctx *c, pg_status code, const std::string &msg) {
    if (c) c->err = msg;
    else g_tls_err = msg;
    return code;
}

inline float luminance(const float *c) { return c[0] * 0.212671f + c[1] * 0.715160f + c[2] * 0.072169f; }

// fresnelDielectricExt (util.cpp:653-683), host copy for BSDF::configure()-time constants
float fresnelDielectricExtH(float cosThetaI_, float eta) {
    if (eta == 1) return 0.0f;
    float scale = (cosThetaI_ > 0) ? 1 / eta : eta;
    float cosThetaTSqr = 1 - (1 - cosThetaI_ * cosThetaI_) * (scale * scale);
    if (cosThetaTSqr <= 0.0f) return 1.0f;
    float cosThetaI = std::fabs(cosThetaI_);
    float cosThetaT = std::sqrt(cosThetaTSqr);
    float Rs = (cosThetaI - eta * cosThetaT) / (cosThetaI + eta * cosThetaT);
    float Rp = (eta * cosThetaI - cosThetaT) / (eta * cosThetaI + cosThetaT);
    return 0.5f * (Rs * Rs + Rp * Rp);
}
// fresnelDiffuseReflectance(eta, fast=false) (util.cpp:816-870): 2 * int_0^1 F(sqrt(xi)) dxi ... as
// the integral of F over the cosine-weighted hemisphere, by composite Simpson in double.
float fresnelDiffuseReflectanceH(float eta) {
    const int N = 2000;
    double h = 1.0 / N, acc = 0;
    for (int i = 0; i <= N; ++i) {
        double w = (i == 0 || i == N) ? 1 : ((i & 1) ? 4 : 2);
        acc += w * fresnelDielectricExtH((float)std::sqrt(i * h), eta);
    }
    return (float)(acc * h / 3.0);
}

// BSDF::configure(): type bits and derived constants of each plugin
GMat makeGMat(const pg_material &m) {
    GMat g{};
    g.model = m.type;
    g.dist = m.distribution;
    g.flags = m.flags;
    g.alpha_u = std::max(m.alpha_u, 1e-4f);  // MicrofacetDistribution clamps alpha (microfacet.h:70-72)
    g.alpha_v = std::max(m.alpha_v, 1e-4f);
    g.eta = m.int_ior / m.ext_ior;
    g.invEta = 1.0f / g.eta;
    g.invEta2 = 1.0f / (g.eta * g.eta);
    for (int i = 0; i < 4; ++i) {
        g.diff[i] = m.diffuse_reflectance[i];
        g.spec[i] = m.specular_reflectance[i];
        g.trans[i] = m.specular_transmittance[i];
        g.ceta[i] = m.eta[i];
        g.ck[i] = m.k[i];
    }
    uint32_t sides = 0x8000u;  // EFrontSide
    switch (m.type) {
        case PG_BSDF_DIFFUSE: g.type = 0x2; break;                       // EDiffuseReflection
        case PG_BSDF_CONDUCTOR: g.type = 0x20; break;                    // EDeltaReflection
        case PG_BSDF_ROUGHCONDUCTOR: g.type = 0x8; break;                // EGlossyReflection
        case PG_BSDF_DIELECTRIC: g.type = 0x20 | 0x40; sides |= 0x10000u; break;
        case PG_BSDF_ROUGHDIELECTRIC: g.type = 0x8 | 0x10; sides |= 0x10000u; break;
        case PG_BSDF_PLASTIC: {
            g.type = 0x20 | 0x2;
            g.fdrInt = fresnelDiffuseReflectanceH(1 / g.eta);
            float dAvg = luminance(m.diffuse_reflectance), sAvg = luminance(m.specular_reflectance);
            g.specWeight = sAvg / (dAvg + sAvg);
            break;
        }
        case PG_BSDF_NULL: g.type = 0x1; sides |= 0x10000u; break;  // ENull, both sides (null.cpp:40)
        case PG_BSDF_ROUGHPLASTIC: {  // roughplastic.cpp:258-307; table + fdrInt set by the caller
            g.type = 0x8 | 0x2;         // EGlossyReflection | EDiffuseReflection
            float dAvg = luminance(m.diffuse_reflectance), sAvg = luminance(m.specular_reflectance);
            g.specWeight = sAvg / (dAvg + sAvg);
            break;
        }
        default: g.type = 0;
    }
    if (m.flags & PG_MAT_TWOSIDED) sides |= 0x10000u;
    g.type |= sides;
    {  // BSDF::getAlbedo (as bsdfAlbedo in pg_kernels.hip), max channel: the guide-fraction bound
        float a[3];
        for (int i = 0; i < 3; ++i) {
            const float d = g.diff[i], s = g.spec[i], t = g.trans[i];
            switch (m.type) {
                case PG_BSDF_DIFFUSE: a[i] = d; break;
                case PG_BSDF_CONDUCTOR:
                case PG_BSDF_ROUGHCONDUCTOR: a[i] = s; break;
                case PG_BSDF_DIELECTRIC: a[i] = t * 0.5f + s * 0.5f; break;
                case PG_BSDF_ROUGHDIELECTRIC: a[i] = s * 0.5f + t * 0.5f; break;
                case PG_BSDF_PLASTIC: a[i] = d * 0.5f + s * 0.5f; break;
                case PG_BSDF_ROUGHPLASTIC: a[i] = s * 0.5f + d * 0.5f; break;
                default: a[i] = 0.0f;
            }
        }
        g.wbound = std::max(std::max(a[0], a[1]), a[2]);
    }
    return g;
}

// Shading record of triangle t (pg_layout.h PG_TRI_SHADE_F4)
void packShade(float *o, const float *P, const float *N, const uint32_t *I, uint32_t t, uint32_t bits, uint32_t orig) {
    const uint32_t i0 = I[3 * (size_t)t], i1 = I[3 * (size_t)t + 1], i2 = I[3 * (size_t)t + 2];
    const float *p0 = P + 3 * (size_t)i0, *p1 = P + 3 * (size_t)i1, *p2 = P + 3 * (size_t)i2;
    float n0[3], n1[3], n2[3];
    if (N) {
        for (int a = 0; a < 3; ++a) {
            n0[a] = N[3 * (size_t)i0 + a];
            n1[a] = N[3 * (size_t)i1 + a];
            n2[a] = N[3 * (size_t)i2 + a];
        }
    } else {  // face normal (TriMesh without vertex normals)
        float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        float l = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        for (int a = 0; a < 3; ++a) n0[a] = n1[a] = n2[a] = l > 0 ? c[a] / l : 0.0f;
    }
    float b, o2;
    std::memcpy(&b, &bits, 4);
    std::memcpy(&o2, &orig, 4);
    float rec[20] = {p0[0], p0[1], p0[2], b,     p1[0], p1[1], p1[2], n2[2], p2[0], p2[1],
                     p2[2], o2,    n0[0], n0[1], n0[2], n1[0], n1[1], n1[2], n2[0], n2[1]};
    std::memcpy(o, rec, sizeof rec);
}

template <class T>
pg_status upload(Ctx *c, DevBuf &b, const std::vector<T> &v) {
    size_t n = std::max<size_t>(v.size() * sizeof(T), 16);
    HIPC(c, b.alloc(n));
    if (!v.empty()) HIPC(c, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return PG_OK;
}

// the one reader of the occluder list's switch (read per call: the tests flip it between jobs of one process)
bool probeListEnabled(const Ctx *c) { return !c->has_env && !std::getenv("PG_NO_PROBE_LIST"); }
SceneDev sceneView(const Ctx *c) {
    SceneDev sc{c->nodes.as<float4>(), c->tris.as<float4>(), c->wnodes.as<float4>(), c->tris.as<float4>(),
                c->tshade.as<float4>(), c->tclass.as<uint8_t>(),
                c->mats.as<GMat>(),
                c->ems.as<GEmitter>(), c->emtri.as<float4>(), c->emcdf.as<float>(),
                c->has_env ? c->env.as<GEnv>() : nullptr, c->bvh_top_nodes};
    sc.num_em_boxes = c->num_em_boxes;
    sc.em_absmax = c->em_absmax;
    std::memcpy(sc.em_box, c->em_box, sizeof(sc.em_box));
    // the blocker list; PG_NO_SHADOW_CULL=1 (or an environment emitter) renders with an empty one (same results)
    sc.num_blockers = (c->has_env || std::getenv("PG_NO_SHADOW_CULL")) ? 0u : c->num_blockers;
    sc.absmax = c->absmax;
    sc.blk_counts = sc.blk_total = nullptr;  // set by the recording passes
    std::memcpy(sc.blk, c->blk, sizeof(sc.blk));
    // the occluder list; PG_NO_PROBE_LIST=1 (or an environment emitter: no probes) renders with an empty one
    sc.num_occluders = probeListEnabled(c) ? c->num_occluders : 0u;
    sc.prb_counts = sc.prb_total = nullptr;  // set by the recording passes
    std::memcpy(sc.prb, c->prb, sizeof(sc.prb));
    if (c->textured || c->nmapped) {  // syncTexRows: both calls share the uv records and mtex
        sc.tuv = c->tuv.as<float4>();
        sc.mtex = c->mtex.as<uint32_t>();
    }
    if (c->textured) sc.tex = c->tex.as<GTex>();
    if (c->nmapped) {
        sc.ntex = c->ntex.as<GTex>();
        sc.mnmap = c->mnmap.as<uint32_t>();
        sc.ttan = c->ttan.as<float4>();
    }
    if (c->num_delta) sc.delta = c->delta.as<GDelta>();
    return sc;
}

// a new job on the scene: no blockers, no probe occluders, no counts
pg_status resetBlockers(Ctx *c) {
    c->num_blockers = c->num_occluders = 0;
    c->blk_stopped = c->prb_stopped = false;
    if (c->blk_counts.p) HIPC(c, hipMemsetAsync(c->blk_counts.p, 0, 2 * ((size_t)c->num_tris + 1) * 4, c->stream));
    return PG_OK;
}
// lists the triangles `ids` (BVH order) in blk / blk_ids from the host copies of their TriAccel rows and shading
// records (no device round trip); triangles too small for the test's margins (pg_ray_hits_blockers) are left out.
// cap: the list's capacity (PG_MAX_BLOCKERS, or PG_PROBE_LIST_MAX for the probe occluders, whose records have the same form)
pg_status installBlockers(Ctx *c, const uint32_t *ids, uint32_t n, float (*blk)[12], uint32_t *blk_ids, uint32_t *orig,
                          uint32_t *count, uint32_t cap = PG_MAX_BLOCKERS) {
    *count = 0;
    uint32_t m = 0;
    for (uint32_t i = 0; i < n && m < cap; ++i) {
        if (ids[i] >= c->num_tris) return fail(c, PG_ERR_INVALID, "blocker triangle id out of range");
        float rows[12];
        for (int r = 0; r < 3; ++r) std::memcpy(rows + 4 * r, &c->host_tris[4 * (size_t)PG_TRI_ROW(ids[i], r)], 16);
        const float *sh = &c->host_shade[4 * (size_t)PG_TRI_SHADE_STRIDE * ids[i]];
        pg_blocker_record(rows, sh, sh + 4, sh + 8, ids[i], blk[m]);
        if (!(blk[m][11] * 32.0f >= c->absmax)) continue;
        if (orig) std::memcpy(&orig[m], &sh[11], 4);  // the original triangle id (pg_layout.h PG_TRI_SHADE_F4)
        blk_ids[m++] = ids[i];
    }
    *count = m;
    return PG_OK;
}
// after a recording pass: the cumulative counts to the host (pinned; the last word is the number of shadow rays the
// counts were taken from), the list chosen from them
// blockers / occluders: which of the two lists this pass counted for (the other keeps what it has)
pg_status learnBlockers(Ctx *c, bool blockers, bool occluders) {
    const size_t bytes = 2 * ((size_t)c->num_tris + 1) * 4;  // both halves in one copy
    HIPC(c, c->h_blk_counts.reserve(bytes));
    const uint32_t *counts = (const uint32_t *)c->h_blk_counts.p;
    HIPC(c, hipMemcpyAsync(c->h_blk_counts.p, c->blk_counts.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (occluders) {  // the same rule and the same stops on the probes' counts (pg_layout.h "Probe occluders")
        const uint32_t *pc = counts + c->num_tris + 1;
        uint32_t pids[PG_PROBE_LIST_MAX];
        const uint32_t ptotal = pc[c->num_tris];
        const uint32_t pn = pg_select_listed(pc, c->num_tris, ptotal, PG_PROBE_LIST_MAX, pids);
        if (ptotal >= PG_BLOCKER_COUNT_STOP || (pn == 0 && ptotal >= PG_BLOCKER_DECIDE)) c->prb_stopped = true;
        if (pg_status s = installBlockers(c, pids, pn, c->prb, c->prb_ids, c->prb_orig, &c->num_occluders, PG_PROBE_LIST_MAX))
            return s;
    }
    if (!blockers) return PG_OK;
    uint32_t ids[PG_MAX_BLOCKERS];
    const uint32_t total = counts[c->num_tris];
    const uint32_t n = pg_select_blockers(counts, c->num_tris, total, ids);
    if (total >= PG_BLOCKER_COUNT_STOP) c->blk_stopped = true;  // no count exceeds the total
    // no list from PG_BLOCKER_DECIDE counted rays or more: the light is mostly visible, or the blockers are many.  The
    // shares will not change, so the job's later recording passes neither count nor read back (the kitchen's training
    // paid 4-5 % for them)
    if (n == 0 && total >= PG_BLOCKER_DECIDE) c->blk_stopped = true;
    return installBlockers(c, ids, n, c->blk, c->blk_ids, c->blk_orig, &c->num_blockers);
}
SDDev sdView(const Ctx *c) {
    SDDev s{};
    s.snodes = reinterpret_cast<const uint2 *>(c->sdp.snodes);
    s.meta = reinterpret_cast<const uint4 *>(c->sdp.meta);
    s.qsum = reinterpret_cast<const float4 *>(c->sdp.qnode);
    s.qchild = reinterpret_cast<const uint4 *>(reinterpret_cast<const float4 *>(c->sdp.qnode) + 1);
    s.bchild = reinterpret_cast<const uint4 *>(c->sdp.bchild);
    s.bsum = reinterpret_cast<unsigned long long *>(c->sdp.bsum);
    s.count = reinterpret_cast<unsigned long long *>(c->sdp.count);
    s.jump = c->sdp.jump;
    s.frac = reinterpret_cast<unsigned long long *>(c->sdp.frac);
    s.jump_bits = c->sd_jump_bits;
    s.learned = c->cfg.bsdf_fraction_bound == PG_FRACTION_LEARNED ? 1 : 0;
    s.alpha0 = c->cfg.bsdf_sampling_fraction;
    for (int a = 0; a < 3; ++a) s.lo[a] = c->sd.lo[a];
    s.extent = c->sd.extent;
    s.built = c->sd.built ? 1 : 0;
    return s;
}
PathDev pathView(const Lane *c) {
    return PathDev{c->ray.as<float4>(),   c->hit.as<float4>(),   c->rad.as<float4>(), c->vst.as<uint4>(),
                   c->sh_d.as<float4>(),  c->sh_c.as<float4>(),  c->vtx.as<float4>(), c->stack_ovf.as<uint32_t>(),
                   c->P,                  c->vtxP,               c->aov.as<float4>()};
}

pg_status uploadSd(Ctx *c) {
    // the device layout (Ctx::sd_blob) is written straight into the pinned staging buffer at the same
    // offsets, then copied in one piece; the jump grid is derived on the device from the S-tree
    const pgh::SdTree &t = c->sd;
    const size_t R = (size_t)1 << pgh::SdTree::kJumpBits;
    const size_t nl = t.leaves.size(), ns = t.samplingNodes(), nb = t.buildingNodes();
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t oMeta = up(4 * t.snode.size()), oQ = oMeta + up(16 * nl), oB = oQ + up(32 * ns);
    const size_t oStats = oB + up(16 * nb), statBytes = 32 * nb + 8 * nl + 8 * pgh::kFracStats * nl;
    const size_t oJump = oStats + up(statBytes), total = oJump + 4 * R * R * R;
    HIPC(c, c->sd_stage.reserve(oJump));
    uint8_t *h = (uint8_t *)c->sd_stage.p;
    uint64_t *hs = (uint64_t *)(h + oStats);
    t.flattenInto(pgh::SdTree::Layout{(uint32_t *)h, (uint32_t *)(h + oMeta), (uint32_t *)(h + oQ),
                                      (uint32_t *)(h + oB), hs, hs + 4 * nb, nullptr, hs + 4 * nb + nl});
    HIPC(c, c->sd_blob.grow(total));
    uint8_t *d = (uint8_t *)c->sd_blob.p;
    c->sdp.snodes = (uint32_t *)d;
    c->sdp.meta = (uint32_t *)(d + oMeta);
    c->sdp.qnode = (uint32_t *)(d + oQ);
    c->sdp.bchild = (uint32_t *)(d + oB);
    c->sdp.bsum = (uint64_t *)(d + oStats);
    c->sdp.count = c->sdp.bsum + 4 * nb;
    c->sdp.frac = c->sdp.count + nl;
    c->sdp.jump = (uint32_t *)(d + oJump);
    HIPC(c, hipMemcpyAsync(d, h, oJump, hipMemcpyHostToDevice, c->stream));
    pg_launch_sd_jump(c->stream, c->sdp.snodes, pgh::SdTree::kJumpBits, c->sdp.jump);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    c->stats.stree_nodes = t.snode.size() / 2;
    c->stats.dtree_nodes = ns;
    c->sd_jump_bits = pgh::SdTree::kJumpBits;
    c->sd_dirty = false;
    return PG_OK;
}

// pull device-side building sums + counts (+ fraction statistics) into the host tree: one copy
pg_status downloadSd(Ctx *c) {
    const size_t nb = c->sd.buildingNodes(), nl = c->sd.leaves.size();
    const size_t bytes = 32 * nb + 8 * nl + 8 * pgh::kFracStats * nl;
    HIPC(c, c->sd_stage.reserve(bytes));
    uint64_t *bsum = (uint64_t *)c->sd_stage.p, *cnt = bsum + 4 * nb, *frac = cnt + nl;
    HIPC(c, hipMemcpyAsync(bsum, c->sdp.bsum, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> cnt32(nl);
    for (size_t i = 0; i < nl; ++i) cnt32[i] = (uint32_t)std::min<uint64_t>(cnt[i], 0xFFFFFFFFu);
    c->sd.absorb(bsum, cnt32.data(), frac);
    return PG_OK;
}

// training-vertex slots per path of a pass (only recording passes write training vertices)
int vertexSlots(const Ctx *c, bool rec) { return rec ? std::max(0, std::min(c->cfg.record_max_vertices, 64)) : 0; }

// release every lane's path state (streams, events and counters stay)
void releasePaths(Ctx *c) {
    for (int li = 0; li < c->nlanes; ++li) {
        Lane &l = c->lanes[li];
        for (DevBuf *b : {&l.ray, &l.hit, &l.rad, &l.vst, &l.sh_d, &l.sh_c,
                          &l.vtx, &l.q0, &l.q1, &l.qs, &l.qp, &l.class_q, &l.aov, &l.qkey, &l.qsorted})
            b->release();
        l.P = 0;
        l.vtx_slots = 0;
        l.vtxP = 0;
    }
}

// path-state capacity of every lane for chunks of up to `want` paths; recording passes also need
// vertex slots for `want` paths (a non-recording pass never allocates them: the 2^25-path chunks of
// a final render would need ~51 GB per lane)
pg_status ensurePaths(Ctx *c, uint32_t want, bool rec) {
    const int vslots = vertexSlots(c, rec);
    for (int li = 0; li < c->nlanes; ++li) {
        Lane &l = c->lanes[li];
        if (!l.stream) {
            HIPC(c, hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
            HIPC(c, hipEventCreateWithFlags(&l.ready, hipEventDisableTiming));
            HIPC(c, hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
            HIPC(c, hipHostMalloc((void **)&l.h_counts, kCounterWords * 4, hipHostMallocDefault));
            HIPC(c, hipHostMalloc((void **)&l.h_stats, kCounterWords * 4, hipHostMallocDefault));
            HIPC(c, l.counters.alloc(kCounterWords * 4));
            // k_rays: three launches' worth (closest hits, shadow rays, probes)
            HIPC(c, l.stack_ovf.alloc(3 * pg_stack_overflow_words(0) * 4));
            HIPC(c, l.tail_stats.alloc(kTailStats * 8));
            HIPC(c, hipHostMalloc((void **)&l.h_tail, kTailStats * 8, hipHostMallocDefault));
        }
        const bool aovMissing = c->cfg.aovs && !l.aov.p;
        if (vslots > 0 && (vslots > l.vtx_slots || want > l.vtxP)) {
            const int vs = std::max(vslots, l.vtx_slots);
            const uint32_t vp = std::max(want, l.vtxP);
            HIPC(c, l.vtx.alloc((size_t)vs * vp * 16 * PG_VTX_F4));
            l.vtx_slots = vs;
            l.vtxP = vp;
        }
        if (want <= l.P && !aovMissing) continue;
        const uint32_t P = std::max(want, l.P);
        size_t f4 = (size_t)P * 16;
        HIPC(c, l.ray.alloc(2 * f4));
        HIPC(c, l.hit.alloc(f4));
        HIPC(c, l.rad.alloc(f4));
        HIPC(c, l.vst.alloc(2 * f4));
        HIPC(c, l.sh_d.alloc(f4));
        HIPC(c, l.sh_c.alloc(f4));
        const size_t qbytes = (size_t)PG_QSHARDS * pg_queue_stride(P) * 4;
        HIPC(c, l.q0.alloc(qbytes));
        HIPC(c, l.q1.alloc(qbytes));
        HIPC(c, l.qs.alloc(qbytes));
        HIPC(c, l.qp.alloc(qbytes));
        HIPC(c, l.class_q.alloc((size_t)PG_NUM_CLASSES * qbytes));
        if (c->cfg.aovs) HIPC(c, l.aov.alloc((size_t)P * 16));
        if (raySortEnabled()) {
            HIPC(c, l.qkey.alloc(qbytes / 2));
            HIPC(c, l.qsorted.alloc(qbytes));
            HIPC(c, l.rsort_hist.alloc((size_t)PG_QSHARDS * PG_RAY_SORT_BINS * 4));
        }
        l.P = P;
    }
    return PG_OK;
}

pg_status ensureRecords(Ctx *c, uint64_t want) {
    if (want <= c->rec_capacity) return PG_OK;
    uint64_t cap = std::max<uint64_t>(want + want / 2, 1u << 20);
    DevBuf nb;
    HIPC(c, nb.alloc(cap * sizeof(pg_record)));
    if (c->rec_host_count)
        HIPC(c, hipMemcpyAsync(nb.p, c->records.p, c->rec_host_count * sizeof(pg_record), hipMemcpyDeviceToDevice,
                               c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    std::swap(c->records.p, nb.p);
    std::swap(c->records.bytes, nb.bytes);
    c->rec_capacity = cap;
    return PG_OK;
}

// the camera's XCD-banded shard map (pg_kernels.h pg_banded_shard_count) over PG_CAMERA_BANDS bands of the local
// pixels (0: the interleaved map): band g goes to XCD group g % 8, so with more than 8 bands each XCD takes
// every 8th band (the surface path's pixel order d_band_pixels groups them).  Paths are pure functions of
// (pixel, sample), so films and trees do not depend on it
uint32_t cameraBands() {
    const char *e = std::getenv("PG_CAMERA_BANDS");
    return e && *e ? (uint32_t)std::strtoul(e, nullptr, 10) : 0u;
}

// k_film_filtered for the chunk k_film has just been launched for (same stream, pixel order and path view)
void launchFilmFiltered(Ctx *c, hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p,
                        const uint32_t *pixels, uint32_t pb, uint32_t np, uint32_t nl, uint32_t sample_base) {
    if (!np || !nl) return;
    FilmFilter f{};
    f.radius = c->filter_radius;
    f.scale = 31.0f / c->filter_radius;
    f.border = (int32_t)std::ceil(c->filter_radius - 0.5f);
    f.tile = c->cfg.tile_size;
    f.values = c->filter_tab.as<float>();
    f.acc = c->film_acc.as<unsigned long long>();
    f.tile_first = c->tile_first.as<uint32_t>();
    f.tile_origin = c->tile_origin.as<uint2>();
    uint32_t tile0 = 0, ntiles = 0;
    if (!c->filter_direct) {  // the local tiles the chunk's pixel range [pb, pb + np) touches
        const std::vector<uint32_t> &tf = c->h_tile_first;
        tile0 = (uint32_t)(std::upper_bound(tf.begin(), tf.end(), pb) - tf.begin()) - 1;
        ntiles = (uint32_t)(std::upper_bound(tf.begin(), tf.end(), pb + np - 1) - tf.begin()) - tile0;
    }
    pg_launch_film_filtered(s, g, sc, p, f, pixels, pb, np, nl, sample_base, tile0, ntiles);
}

}  // namespace pgh

using namespace pgh;

extern "C" {

int32_t pg_abi_version(void) { return PG_ABI_VERSION; }

// HeterogeneousMedium / GridDataSource preconditions (heterogeneous.cpp:227-242: densities in
// [0, 1]; hg.cpp:47-50: |g| < 1).  The optical-depth bound keeps one Woodcock walk across the
// grid box below ~1e7 steps (the reference has no bound; a thicker medium is rejected).
pg_status validateMedium(Ctx *c, const pg_medium &pm, uint32_t m) {
    const std::string id = "pg_upload_scene: medium " + std::to_string(m) + ": ";
    if (pm.type != PG_MEDIUM_HETEROGENEOUS) return fail(c, PG_ERR_INVALID, id + "unknown type");
    if (!pm.density || pm.res[0] < 1 || pm.res[1] < 1 || pm.res[2] < 1 ||
        (uint64_t)pm.res[0] * pm.res[1] * pm.res[2] > (1ull << 30))
        return fail(c, PG_ERR_INVALID, id + "bad density grid");
    double diag2 = 0;
    for (int a = 0; a < 3; ++a) {
        if (!(pm.aabb_max[a] > pm.aabb_min[a]) || !std::isfinite(pm.aabb_min[a]) || !std::isfinite(pm.aabb_max[a]))
            return fail(c, PG_ERR_INVALID, id + "empty or non-finite AABB");
        diag2 += (double)(pm.aabb_max[a] - pm.aabb_min[a]) * (pm.aabb_max[a] - pm.aabb_min[a]);
        if (!(pm.albedo[a] >= 0) || !std::isfinite(pm.albedo[a])) return fail(c, PG_ERR_INVALID, id + "bad albedo");
    }
    if (!(pm.scale > 0) || !std::isfinite(pm.scale)) return fail(c, PG_ERR_INVALID, id + "scale must be finite and > 0");
    if (pm.scale * std::sqrt(diag2) > 1e7) return fail(c, PG_ERR_INVALID, id + "optical depth too large");
    if (!(pm.g > -1 && pm.g < 1)) return fail(c, PG_ERR_INVALID, id + "HG g must lie in (-1, 1)");
    const size_t n = (size_t)pm.res[0] * pm.res[1] * pm.res[2];
    for (size_t i = 0; i < n; ++i)
        if (!(pm.density[i] >= 0.0f && pm.density[i] <= 1.0f)) return fail(c, PG_ERR_INVALID, id + "density outside [0, 1]");
    return PG_OK;
}

// per-cell maxima of the density grid (cell c covers voxels [c * CELL - 1, (c + 1) * CELL + 1] per
// axis, clamped), times scale; appended to `out` in cell order (x fastest)
void buildMajorants(const pg_medium &pm, const GMedium &gm, std::vector<float> &out) {
    const int C = PG_MAJORANT_CELL;
    const int r[3] = {(int)pm.res[0], (int)pm.res[1], (int)pm.res[2]}, n[3] = {(int)gm.mx, (int)gm.my, (int)gm.mz};
    // separable running maxima: along x, then y, then z, each over the cell's voxel window
    auto win = [&](int a, int cidx, int &lo, int &hi) {
        lo = std::max(0, cidx * C - 1);
        hi = std::min(r[a] - 1, (cidx + 1) * C + 1);
    };
    std::vector<float> ax((size_t)n[0] * r[1] * r[2]), ay((size_t)n[0] * n[1] * r[2]);
    for (int z = 0; z < r[2]; ++z)
        for (int y = 0; y < r[1]; ++y) {
            const float *row = pm.density + ((size_t)z * r[1] + y) * r[0];
            for (int cx = 0; cx < n[0]; ++cx) {
                int lo, hi;
                win(0, cx, lo, hi);
                float m = 0;
                for (int x = lo; x <= hi; ++x) m = std::max(m, row[x]);
                ax[((size_t)z * r[1] + y) * n[0] + cx] = m;
            }
        }
    for (int z = 0; z < r[2]; ++z)
        for (int cy = 0; cy < n[1]; ++cy) {
            int lo, hi;
            win(1, cy, lo, hi);
            for (int cx = 0; cx < n[0]; ++cx) {
                float m = 0;
                for (int y = lo; y <= hi; ++y) m = std::max(m, ax[((size_t)z * r[1] + y) * n[0] + cx]);
                ay[((size_t)z * n[1] + cy) * n[0] + cx] = m;
            }
        }
    const size_t base = out.size();
    out.resize(base + (size_t)n[0] * n[1] * n[2]);
    for (int cz = 0; cz < n[2]; ++cz) {
        int lo, hi;
        win(2, cz, lo, hi);
        for (int cy = 0; cy < n[1]; ++cy)
            for (int cx = 0; cx < n[0]; ++cx) {
                float m = 0;
                for (int z = lo; z <= hi; ++z) m = std::max(m, ay[((size_t)z * n[1] + cy) * n[0] + cx]);
                out[base + ((size_t)cz * n[1] + cy) * n[0] + cx] = m * pm.scale;
            }
    }
}

pg_status pg_config_default(pg_config *c) {
    if (!c) return PG_ERR_INVALID;
    std::memset(c, 0, sizeof *c);
    c->device = 0;
    c->max_depth = -1;
    c->rr_depth = 5;
    c->use_nee = 1;
    c->hide_emitters = 0;
    c->strict_normals = 0;
    c->max_component_value = std::numeric_limits<float>::infinity();
    c->seed = 1337;
    c->guiding = 0;
    c->bsdf_sampling_fraction = 0.5f;
    c->s_tree_threshold = 12000.0f;
    c->d_tree_threshold = 0.01f;
    c->d_tree_max_depth = 20;
    c->record_max_vertices = 32;
    c->rank = 0;
    c->world_size = 1;
    c->tile_size = 32;
    c->max_paths_in_flight = 0;
    c->gpu_depth_cap = 1024;
    c->path_lanes = 0;
    c->integrator = PG_INTEGRATOR_PATH;
    c->distance_guiding = 0.25f;
    c->bsdf_fraction_bound = PG_FRACTION_FIXED;
    c->kernel_timing = 0;
    c->volpath_exact_mis = 0;
    c->tail_paths = 0;
    c->glossy_prior = 0;
    return PG_OK;
}

const char *pg_last_error(void *ctx) {
    if (!ctx) return g_tls_err.c_str();
    return ((Ctx *)ctx)->err.c_str();
}

pg_status pg_create(const pg_config *cfg, void **out) {
    if (!cfg || !out) return fail(nullptr, PG_ERR_INVALID, "pg_create: null argument");
    *out = nullptr;
    if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size)
        return fail(nullptr, PG_ERR_INVALID, "pg_create: bad rank/world_size");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(nullptr, PG_ERR_NO_DEVICE, "pg_create: no HIP device visible");
    if (cfg->device < 0 || cfg->device >= n) return fail(nullptr, PG_ERR_INVALID, "pg_create: bad device ordinal");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, PG_ERR_HIP, "pg_create: hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PG_ERR_NO_DEVICE, std::string("pg_create: device is ") + prop.gcnArchName + ", need gfx950");
    Ctx *c = new Ctx();
    c->cfg = *cfg;
    if (c->cfg.tile_size == 0) c->cfg.tile_size = 32;
    if (c->cfg.gpu_depth_cap <= 0) c->cfg.gpu_depth_cap = 1024;
    if (c->cfg.integrator == PG_INTEGRATOR_PATH) {  // the surface wavefront's per-bounce counter blocks
        if (c->cfg.gpu_depth_cap > (int32_t)kMaxBounces - 2) c->cfg.gpu_depth_cap = (int32_t)kMaxBounces - 2;
        if (c->cfg.max_depth > (int32_t)kMaxBounces - 3) {
            delete c;
            return fail(nullptr, PG_ERR_INVALID,
                        "pg_create: max_depth above " + std::to_string(kMaxBounces - 3) +
                            " is not supported by the path integrator (use -1 for unbounded paths)");
        }
    }
    if (c->cfg.path_lanes < 0 || c->cfg.path_lanes > PG_MAX_LANES) {
        delete c;
        return fail(nullptr, PG_ERR_INVALID, "pg_create: path_lanes must be 0..4");
    }
    c->nlanes = c->cfg.path_lanes ? c->cfg.path_lanes : PG_DEFAULT_LANES;
    if (c->cfg.integrator != PG_INTEGRATOR_PATH && c->cfg.integrator != PG_INTEGRATOR_VOLPATH) {
        delete c;
        return fail(nullptr, PG_ERR_INVALID, "pg_create: unknown integrator");
    }
    if (c->cfg.bsdf_fraction_bound < PG_FRACTION_FIXED || c->cfg.bsdf_fraction_bound > PG_FRACTION_LEARNED) {
        delete c;
        return fail(nullptr, PG_ERR_INVALID, "pg_create: unknown bsdf_fraction_bound");
    }
    if (c->cfg.volume_majorant != PG_MAJORANT_GRID && c->cfg.volume_majorant != PG_MAJORANT_GLOBAL) {
        delete c;
        return fail(nullptr, PG_ERR_INVALID, "pg_create: unknown volume_majorant");
    }
    if (c->cfg.aovs && c->cfg.integrator != PG_INTEGRATOR_PATH) {
        delete c;
        return fail(nullptr, PG_ERR_INVALID, "pg_create: aovs need the path integrator");
    }
    if (!(c->cfg.distance_guiding >= 0.0f && c->cfg.distance_guiding < 1.0f)) {
        delete c;
        return fail(nullptr, PG_ERR_INVALID, "pg_create: distance_guiding must be in [0, 1)");
    }
    if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->film_order, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->pass_start, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return fail(nullptr, PG_ERR_HIP, "pg_create: stream/pinned allocation failed");
    }
    *out = c;
    return PG_OK;
}

pg_status pg_destroy(void *ctx) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return PG_OK;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t &e : c->vw_ev)
        if (e) (void)hipEventDestroy(e);
    for (VolLane &l : c->vlanes) {
        if (l.nstream) (void)hipStreamSynchronize(l.nstream);
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        if (l.ready) (void)hipEventDestroy(l.ready);
        if (l.vdone) (void)hipEventDestroy(l.vdone);
        if (l.ndone) (void)hipEventDestroy(l.ndone);
        if (l.nstream) (void)hipStreamDestroy(l.nstream);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    for (Lane &l : c->lanes) {
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        for (auto &pool : l.ev)
            for (auto &e : pool) {
                (void)hipEventDestroy(e.a);
                (void)hipEventDestroy(e.b);
            }
        if (l.ready) (void)hipEventDestroy(l.ready);
        if (l.done) (void)hipEventDestroy(l.done);
        if (l.h_counts) (void)hipHostFree(l.h_counts);
        if (l.h_stats) (void)hipHostFree(l.h_stats);
        if (l.h_tail) (void)hipHostFree(l.h_tail);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    if (c->dn_ev.a) (void)hipEventDestroy(c->dn_ev.a);
    if (c->dn_ev.b) (void)hipEventDestroy(c->dn_ev.b);
    if (c->timing.a) (void)hipEventDestroy(c->timing.a);
    if (c->timing.b) (void)hipEventDestroy(c->timing.b);
    if (c->film_order) (void)hipEventDestroy(c->film_order);
    if (c->pass_start) (void)hipEventDestroy(c->pass_start);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return PG_OK;
}

pg_status pg_cancel(void *ctx) {
    if (!ctx) return PG_ERR_INVALID;
    ((Ctx *)ctx)->cancel.store(true);
    return PG_OK;
}

// ---- reconstruction-filtered film (pg_set_rfilter) ------------------------------------------------------
// device side of the filter: the table, the local tiles' pixel ranges and origins, and the zeroed sums
// (needs the scene's film size and tile shard; called by whichever of pg_set_rfilter / pg_upload_scene comes last)
static pg_status setupFiltered(Ctx *c) {
    const size_t n = (size_t)c->g.width * c->g.height * 4;
    HIPC(c, c->film_acc.alloc(n * 8));
    HIPC(c, hipMemsetAsync(c->film_acc.p, 0, n * 8, c->stream));
    HIPC(c, c->filter_tab.alloc(sizeof(c->filter_values)));
    HIPC(c, hipMemcpyAsync(c->filter_tab.p, c->filter_values, sizeof(c->filter_values), hipMemcpyHostToDevice, c->stream));
    pg_status s;
    if ((s = upload(c, c->tile_first, c->h_tile_first))) return s;
    if ((s = upload(c, c->tile_origin, c->h_tile_origin))) return s;
    HIPC(c, hipStreamSynchronize(c->stream));
    const char *e = std::getenv("PG_FILM_FILTER_DIRECT");
    const int border = (int)std::ceil(c->filter_radius - 0.5f);
    c->filter_direct = (e && std::atoi(e) != 0) || pg_film_filter_lds_bytes(c->cfg.tile_size, border) > 65536;
    return PG_OK;
}
pg_status pg_rfilter_table(int32_t type, float param, float *radius_out, float *values_out) {
    if (!radius_out || !values_out) return fail(nullptr, PG_ERR_INVALID, "pg_rfilter_table: null argument");
    float radius, stddev = 0.5f;
    switch (type) {
        case PG_RFILTER_BOX: radius = 0.5f; break;
        case PG_RFILTER_TENT: radius = 1.0f; break;
        case PG_RFILTER_GAUSSIAN:
            if (param != 0) stddev = param;
            if (!(stddev > 0) || !std::isfinite(stddev)) return fail(nullptr, PG_ERR_INVALID, "pg_rfilter_table: bad stddev");
            radius = 4 * stddev;
            break;
        default: return fail(nullptr, PG_ERR_INVALID, "pg_rfilter_table: unknown filter type");
    }
    // math::fastexp as pg_fastmath.h states it for the device: the double libm call rounded to float
    auto fastexp = [](float x) { return (float)std::exp((double)x); };
    auto eval = [&](float x) -> float {
        switch (type) {
            case PG_RFILTER_BOX: return std::fabs(x) <= radius ? 1.0f : 0.0f;                    // box.cpp:46-48
            case PG_RFILTER_TENT: return std::max(0.0f, 1.0f - std::fabs(x / radius));           // tent.cpp:42-44
            default: {                                                                            // gaussian.cpp:52-57
                const float alpha = -1.0f / (2.0f * stddev * stddev);
                return std::max(0.0f, fastexp(alpha * x * x) - fastexp(alpha * radius * radius));
            }
        }
    };
    // ReconstructionFilter::configure (rfilter.cpp:38-54)
    float sum = 0.0f;
    for (int i = 0; i < 31; ++i) {
        values_out[i] = eval((radius * i) / 31);
        sum += values_out[i];
    }
    values_out[31] = 0.0f;
    sum *= 2 * radius / 31;
    const float normalization = 1.0f / sum;
    for (int i = 0; i < 31; ++i) values_out[i] *= normalization;
    *radius_out = radius;
    return PG_OK;
}

pg_status pg_set_rfilter(void *ctx, float radius, const float *values) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_set_rfilter: null context");
    if (c->rendered) return fail(c, PG_ERR_STATE, "pg_set_rfilter: a render pass has already run");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!values) {  // off again: as if never set
        c->filtered = false;
        for (DevBuf *b : {&c->film_acc, &c->filter_tab, &c->tile_first, &c->tile_origin}) b->release();
        return PG_OK;
    }
    if (!(radius > 0) || !(radius <= 4)) return fail(c, PG_ERR_INVALID, "pg_set_rfilter: need 0 < radius <= 4");
    for (int i = 0; i < 32; ++i)
        if (!std::isfinite(values[i])) return fail(c, PG_ERR_INVALID, "pg_set_rfilter: non-finite table entry");
    if (cameraBands() > 0)
        return fail(c, PG_ERR_INVALID, "pg_set_rfilter: not supported with the banded camera map (PG_CAMERA_BANDS)");
    c->filter_radius = radius;
    std::memcpy(c->filter_values, values, sizeof(c->filter_values));
    c->filtered = true;
    return c->has_scene ? setupFiltered(c) : PG_OK;
}

// ---- thin lens (pg_capi.h pg_set_lens) ------------------------------------------------------------------------------
// The lens lives in the context's GParams, which every pass copies: pg_upload_scene's memset turns it off.
pg_status pg_set_lens(void *ctx, float aperture_radius, float focus_distance) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_set_lens: null context");
    if (!std::isfinite(aperture_radius) || aperture_radius < 0)
        return fail(c, PG_ERR_INVALID, "pg_set_lens: the aperture radius must be finite and >= 0");
    if (!std::isfinite(focus_distance)) return fail(c, PG_ERR_INVALID, "pg_set_lens: non-finite focus distance");
    if (aperture_radius > 0 && !(focus_distance > 0))
        return fail(c, PG_ERR_INVALID, "pg_set_lens: the focus distance of a lens must be > 0");
    c->g.lens_radius = aperture_radius;
    c->g.focus_dist = aperture_radius > 0 ? focus_distance : 0.0f;
    return PG_OK;
}

pg_status pg_get_lens(void *ctx, float *aperture_radius, float *focus_distance) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_get_lens: null context");
    if (aperture_radius) *aperture_radius = c->g.lens_radius;
    if (focus_distance) *focus_distance = c->g.focus_dist;
    return PG_OK;
}

pg_status pg_camera_rays(void *ctx, const uint32_t *pixels, const uint32_t *samples, uint32_t n, float *o_tmin,
                         float *d_tmax) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (n && (!pixels || !samples || !o_tmin || !d_tmax)))
        return fail(c, PG_ERR_INVALID, "pg_camera_rays: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_camera_rays: no scene");
    const uint64_t npix = (uint64_t)c->g.width * c->g.height;
    for (uint32_t i = 0; i < n; ++i)
        if (pixels[i] >= npix) return fail(c, PG_ERR_INVALID, "pg_camera_rays: pixel outside the film");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    GParams g = c->g;
    g.seed = c->cfg.seed;  // as the passes set it
    DevBuf p, s, o, d;
    HIPC(c, p.alloc((size_t)n * 4));
    HIPC(c, s.alloc((size_t)n * 4));
    HIPC(c, o.alloc((size_t)n * 16));
    HIPC(c, d.alloc((size_t)n * 16));
    HIPC(c, hipMemcpyAsync(p.p, pixels, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(s.p, samples, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    pg_launch_camera_rays(c->stream, g, p.as<uint32_t>(), s.as<uint32_t>(), n, o.as<float>(), d.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(o_tmin, o.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(d_tmax, d.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

// ---- textures (pg_capi.h pg_set_textures) ---------------------------------------------------------------------------
namespace {
// pg_texture -> GTex (texels left null) with its validation; err: what is wrong with it
bool makeGTex(const pg_texture &t, GTex &g, std::string &err) {
    g = GTex{};
    if (t.type > PG_TEXTURE_CHECKERBOARD) return err = "unknown texture type", false;
    if (t.filter > PG_TEXFILTER_BILINEAR) return err = "unknown filter", false;
    if (t.wrap_u > PG_TEXWRAP_ONE || t.wrap_v > PG_TEXWRAP_ONE) return err = "unknown wrap mode", false;
    for (float x : {t.uscale, t.vscale, t.uoffset, t.voffset})
        if (!std::isfinite(x)) return err = "non-finite uv scale or offset", false;
    if (t.type == PG_TEXTURE_BITMAP) {
        if (t.width == 0 || t.height == 0) return err = "zero-sized bitmap", false;
        if (t.width > (1u << 24) || t.height > (1u << 24) || (uint64_t)t.width * t.height > (1ull << 28))
            return err = "bitmap too large", false;
        if (!t.rgb) return err = "bitmap without texels", false;
        for (size_t i = 0; i < (size_t)3 * t.width * t.height; ++i)
            if (!std::isfinite(t.rgb[i]) || t.rgb[i] < 0) return err = "non-finite or negative texel", false;
        g.width = t.width;
        g.height = t.height;
    } else {
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(t.color0[k]) || t.color0[k] < 0 || !std::isfinite(t.color1[k]) || t.color1[k] < 0)
                return err = "non-finite or negative checkerboard colour", false;
    }
    g.mode = t.type | (t.filter << 4) | (t.wrap_u << 8) | (t.wrap_v << 12);
    g.uscale = t.uscale;
    g.vscale = t.vscale;
    g.uoffset = t.uoffset;
    g.voffset = t.voffset;
    for (int k = 0; k < 3; ++k) {
        g.color0[k] = t.color0[k];
        g.color1[k] = t.color1[k];
    }
    return true;
}
// float4 texels of a bitmap
void texelRows(const pg_texture &t, std::vector<float> &o) {
    o.assign((size_t)4 * t.width * t.height, 0.0f);
    for (size_t i = 0; i < (size_t)t.width * t.height; ++i)
        for (int k = 0; k < 3; ++k) o[4 * i + k] = t.rgb[3 * i + k];
}
// Texture::getAverage (the caller's, or the mean of the level-0 texels / of the two colours) and the per-channel
// maximum of the texture's values
void texAverageMax(const pg_texture &t, float avg[3], float mx[3]) {
    for (int k = 0; k < 3; ++k) {
        if (t.type == PG_TEXTURE_CHECKERBOARD) {
            avg[k] = (t.color0[k] + t.color1[k]) * 0.5f;
            mx[k] = std::max(t.color0[k], t.color1[k]);
        } else {
            double sum = 0;
            mx[k] = 0.0f;
            const size_t n = (size_t)t.width * t.height;
            for (size_t i = 0; i < n; ++i) {
                sum += t.rgb[3 * i + k];
                mx[k] = std::max(mx[k], t.rgb[3 * i + k]);
            }
            avg[k] = (float)(sum / (double)n);
        }
        // zero / one wrap modes add their constant to the range
        if (t.type == PG_TEXTURE_BITMAP && (t.wrap_u == PG_TEXWRAP_ONE || t.wrap_v == PG_TEXWRAP_ONE)) mx[k] = std::max(mx[k], 1.0f);
    }
    if (!(t.average[0] < 0))
        for (int k = 0; k < 3; ++k) avg[k] = t.average[k];
}
// TriMesh::computeUVTangents (trimesh.cpp:683-735) of one triangle, float32 without contraction: dpdu of pg_capi.h
// "normal maps".  uv: the three vertices' texcoords, or nullptr (no texcoords: p1 - p0)
void uvTangent(const float *p0, const float *p1, const float *p2, const float *uv, float dpdu[3]) {
    const float d1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, d2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    for (int a = 0; a < 3; ++a) dpdu[a] = d1[a];
    if (!uv) return;
    const float n[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    const float length = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (length == 0) return;
    const float u1[2] = {uv[2] - uv[0], uv[3] - uv[1]}, u2[2] = {uv[4] - uv[0], uv[5] - uv[1]};
    const float det = u1[0] * u2[1] - u1[1] * u2[0];
    if (det == 0) {  // coordinateSystem(n / length, dpdu, dpdv) (util.cpp:594-603): dpdu = cross(dpdv, a)
        const float a[3] = {n[0] / length, n[1] / length, n[2] / length};
        float c3[3];
        if (std::fabs(a[0]) > std::fabs(a[1])) {
            const float invLen = 1.0f / std::sqrt(a[0] * a[0] + a[2] * a[2]);
            c3[0] = a[2] * invLen, c3[1] = 0.0f, c3[2] = -a[0] * invLen;
        } else {
            const float invLen = 1.0f / std::sqrt(a[1] * a[1] + a[2] * a[2]);
            c3[0] = 0.0f, c3[1] = a[2] * invLen, c3[2] = -a[1] * invLen;
        }
        dpdu[0] = c3[1] * a[2] - c3[2] * a[1];
        dpdu[1] = c3[2] * a[0] - c3[0] * a[2];
        dpdu[2] = c3[0] * a[1] - c3[1] * a[0];
        return;
    }
    const float invDet = 1.0f / det;
    for (int a = 0; a < 3; ++a) dpdu[a] = (u2[1] * d1[a] - u1[1] * d2[a]) * invDet;
}
// What pg_set_textures and pg_set_normal_maps share, rebuilt from what each was given (Ctx::host_mtex / host_mnmap,
// tex_uv / nmap_uv): the per-triangle uv records, the triangle classes, mtex (all ~0 while only normal maps are
// bound: the kernels take mtex != nullptr for "the textured class exists") and the mapped triangles' tangents.
pg_status syncTexRows(Ctx *c) {
    pg_status s;
    if (!c->textured) c->mtex.release();
    if (!c->nmapped) c->ttan.release();
    if (!c->textured && !c->nmapped) {
        if ((s = upload(c, c->tclass, c->base_tclass))) return s;
        HIPC(c, hipStreamSynchronize(c->stream));
        c->tuv.release();
        return PG_OK;
    }
    const float *texcoords = !c->tex_uv.empty() ? c->tex_uv.data() : !c->nmap_uv.empty() ? c->nmap_uv.data() : nullptr;
    const std::vector<uint32_t> none(c->num_mats, 0xFFFFFFFFu);
    const std::vector<uint32_t> &mtex = c->textured ? c->host_mtex : none, &mnmap = c->nmapped ? c->host_mnmap : none;
    // per BVH-order triangle: the vertices' texcoords (pg_layout.h PG_TRI_UV_F4), the textured class, the tangent
    const uint32_t nt = c->num_tris;
    std::vector<float> tuv((size_t)4 * PG_TRI_UV_F4 * nt, 0.0f), ttan(c->nmapped ? (size_t)4 * nt : 0, 0.0f);
    std::vector<uint8_t> tclass = c->base_tclass;
    for (uint32_t k = 0; k < nt; ++k) {
        const float *rec = &c->host_shade[4 * PG_TRI_SHADE_STRIDE * (size_t)k];
        uint32_t bits, orig;
        std::memcpy(&bits, rec + 3, 4);
        std::memcpy(&orig, rec + 11, 4);
        float *o = &tuv[(size_t)4 * PG_TRI_UV_F4 * k];
        if (texcoords) {
            for (int v = 0; v < 3; ++v) {
                const uint32_t vi = c->host_indices[3 * (size_t)orig + v];
                o[2 * v] = texcoords[2 * (size_t)vi];
                o[2 * v + 1] = texcoords[2 * (size_t)vi + 1];
            }
        } else {  // Intersection::uv without texcoords: (b.y, b.z)
            o[2] = 1.0f;
            o[5] = 1.0f;
        }
        const uint32_t m = bits & 0xFFFFu;
        if (mtex[m] != 0xFFFFFFFFu || mnmap[m] != 0xFFFFFFFFu)
            tclass[k] = (uint8_t)(PG_CLASS_TEXTURED | (tclass[k] & PG_TCLASS_EMITTER));
        // unmapped triangles never read their row: p1 - p0, the frame they keep
        if (c->nmapped) uvTangent(rec, rec + 4, rec + 8, texcoords && mnmap[m] != 0xFFFFFFFFu ? o : nullptr, &ttan[4 * (size_t)k]);
    }
    if ((s = upload(c, c->tuv, tuv)) || (s = upload(c, c->mtex, mtex)) || (s = upload(c, c->tclass, tclass))) return s;
    if (c->nmapped && (s = upload(c, c->ttan, ttan))) return s;
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}
// the untextured scene's materials back on the device, and the shared rows without the textures
pg_status clearTextures(Ctx *c) {
    if (!c->textured) return PG_OK;
    c->textured = false;
    c->host_mats = c->base_mats;
    c->host_mtex.clear();
    c->tex_uv.clear();
    pg_status s;
    if ((s = upload(c, c->mats, c->host_mats)) || (s = syncTexRows(c))) return s;
    HIPC(c, hipStreamSynchronize(c->stream));
    for (DevBuf *b : {&c->tex, &c->texels}) b->release();
    return PG_OK;
}
// the scene without normal maps (they change no material record)
pg_status clearNormalMaps(Ctx *c) {
    if (!c->nmapped) return PG_OK;
    c->nmapped = false;
    c->host_mnmap.clear();
    c->nmap_uv.clear();
    if (pg_status s = syncTexRows(c)) return s;
    for (DevBuf *b : {&c->ntex, &c->mnmap, &c->ntexels}) b->release();
    return PG_OK;
}
// both calls' texcoords describe the same mesh: equal where both pass them
bool sameTexcoords(const std::vector<float> &other, const float *texcoords) {
    if (!texcoords || other.empty()) return true;
    for (size_t i = 0; i < other.size(); ++i)
        if (other[i] != texcoords[i]) return false;
    return true;
}
// the texel buffer of a texture set (each bitmap 256-B aligned) and the records pointing into it
pg_status uploadTexels(Ctx *c, const pg_texture *textures, uint32_t n_textures, DevBuf &buf, std::vector<GTex> &gtex) {
    std::vector<float> texels;
    std::vector<size_t> at(n_textures, 0);
    for (uint32_t i = 0; i < n_textures; ++i) {
        if (textures[i].type != PG_TEXTURE_BITMAP) continue;
        texels.resize((texels.size() + 63) & ~(size_t)63, 0.0f);
        at[i] = texels.size();
        std::vector<float> rows;
        texelRows(textures[i], rows);
        texels.insert(texels.end(), rows.begin(), rows.end());
    }
    if (pg_status s = upload(c, buf, texels)) return s;
    for (uint32_t i = 0; i < n_textures; ++i)
        if (textures[i].type == PG_TEXTURE_BITMAP) gtex[i].texels = buf.as<float>() + at[i];
    return PG_OK;
}
}  // namespace

pg_status pg_set_textures(void *ctx, const pg_texture *textures, uint32_t n_textures, const pg_texture_binding *bindings,
                          uint32_t n_bindings, const float *texcoords) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_set_textures: null context");
    if (c->cfg.integrator != PG_INTEGRATOR_PATH)
        return fail(c, PG_ERR_INVALID, "pg_set_textures: the volumetric integrator does not support textures");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_set_textures: no scene uploaded");
    if (c->scene_rendered) return fail(c, PG_ERR_STATE, "pg_set_textures: a render pass has already run on this scene");
    if ((n_textures && !textures) || (n_bindings && !bindings)) return fail(c, PG_ERR_INVALID, "pg_set_textures: null argument");
    HIPC(c, hipSetDevice(c->cfg.device));
    // validate everything before anything changes
    std::vector<GTex> gtex(n_textures);
    for (uint32_t i = 0; i < n_textures; ++i) {
        std::string err;
        if (!makeGTex(textures[i], gtex[i], err))
            return fail(c, PG_ERR_INVALID, "pg_set_textures: texture " + std::to_string(i) + ": " + err);
        if (!(textures[i].average[0] < 0))
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(textures[i].average[k]) || textures[i].average[k] < 0)
                    return fail(c, PG_ERR_INVALID, "pg_set_textures: texture " + std::to_string(i) + ": bad average");
    }
    std::vector<uint32_t> mtex(c->num_mats, 0xFFFFFFFFu);
    for (uint32_t b = 0; b < n_bindings; ++b) {
        const pg_texture_binding &tb = bindings[b];
        if (tb.material >= c->num_mats || tb.texture >= n_textures)
            return fail(c, PG_ERR_INVALID, "pg_set_textures: binding " + std::to_string(b) + ": index out of range");
        const uint32_t model = c->base_mats[tb.material].model;
        if (model != PG_BSDF_DIFFUSE && model != PG_BSDF_PLASTIC && model != PG_BSDF_ROUGHPLASTIC)
            return fail(c, PG_ERR_INVALID, "pg_set_textures: binding " + std::to_string(b) +
                                               ": the material's model has no diffuse reflectance");
        if (mtex[tb.material] != 0xFFFFFFFFu)
            return fail(c, PG_ERR_INVALID, "pg_set_textures: material " + std::to_string(tb.material) + " is bound twice");
        mtex[tb.material] = tb.texture;
    }
    if (texcoords)
        for (size_t i = 0; i < (size_t)2 * c->num_vertices; ++i)
            if (!std::isfinite(texcoords[i])) return fail(c, PG_ERR_INVALID, "pg_set_textures: non-finite texcoord");
    if (n_bindings && !sameTexcoords(c->nmap_uv, texcoords))
        return fail(c, PG_ERR_INVALID, "pg_set_textures: texcoords differ from those of pg_set_normal_maps");
    if (pg_status s = clearTextures(c)) return s;
    if (n_bindings == 0) return PG_OK;

    // from here on a failure puts the untextured scene back (restoreBase): the context never holds half a texture set
    auto restoreBase = [&](pg_status why) {
        const std::string msg = c->err;
        c->textured = true;  // so that clearTextures re-uploads the base records and classes
        (void)clearTextures(c);
        c->err = msg;
        return why;
    };
    pg_status s;
    if ((s = uploadTexels(c, textures, n_textures, c->texels, gtex))) return restoreBase(s);
    // the bound materials: specWeight from the texture's average (plastic.cpp:201-202, roughplastic.cpp:258-262) and
    // wbound from its per-channel maximum, an upper bound only (shadeOne computes the vertex's own)
    std::vector<GMat> mats = c->base_mats;
    for (uint32_t m = 0; m < c->num_mats; ++m) {
        if (mtex[m] == 0xFFFFFFFFu) continue;
        GMat &gm = mats[m];
        float avg[3], mx[3];
        texAverageMax(textures[mtex[m]], avg, mx);
        if (gm.model != PG_BSDF_DIFFUSE) {
            const float dAvg = luminance(avg), sAvg = luminance(gm.spec);
            gm.specWeight = sAvg / (dAvg + sAvg);
        }
        float a[3];
        for (int k = 0; k < 3; ++k) a[k] = gm.model == PG_BSDF_DIFFUSE ? mx[k] : mx[k] * 0.5f + gm.spec[k] * 0.5f;
        gm.wbound = std::max(std::max(a[0], a[1]), a[2]);
    }
    c->textured = true;  // syncTexRows reads the new set; restoreBase clears it again
    c->host_mtex = mtex;
    if (texcoords) c->tex_uv.assign(texcoords, texcoords + 2 * (size_t)c->num_vertices);
    if ((s = upload(c, c->tex, gtex)) || (s = upload(c, c->mats, mats)) || (s = syncTexRows(c))) return restoreBase(s);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return restoreBase(fail(c, PG_ERR_HIP, "pg_set_textures: upload failed"));
    c->host_mats = mats;
    c->textured = true;
    return PG_OK;
}

pg_status pg_texture_query(void *ctx, const pg_texture *texture, const float *uv, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !texture || (!uv && n) || (!out && n)) return fail(c, PG_ERR_INVALID, "pg_texture_query: null argument");
    if (n > 0xFFFFFFFFull / 3) return fail(c, PG_ERR_INVALID, "pg_texture_query: too many points");
    GTex g;
    std::string err;
    if (!makeGTex(*texture, g, err)) return fail(c, PG_ERR_INVALID, "pg_texture_query: " + err);
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf dt, dg, du, dout;
    if (texture->type == PG_TEXTURE_BITMAP) {
        std::vector<float> rows;
        texelRows(*texture, rows);
        HIPC(c, dt.alloc(rows.size() * 4));
        HIPC(c, hipMemcpy(dt.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        g.texels = dt.as<float>();
    }
    HIPC(c, dg.alloc(sizeof(GTex)));
    HIPC(c, du.alloc(n * 8));
    HIPC(c, dout.alloc(n * 12));
    HIPC(c, hipMemcpy(dg.p, &g, sizeof(GTex), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpyAsync(du.p, uv, n * 8, hipMemcpyHostToDevice, c->stream));
    pg_launch_texture_query(c->stream, dg.as<GTex>(), du.as<float>(), (uint32_t)n, dout.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, dout.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_hit_uvs(void *ctx, const float *rays, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!rays && n) || (!out && n)) return fail(c, PG_ERR_INVALID, "pg_hit_uvs: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_hit_uvs: no scene");
    if (n > 0xFFFFFFFFull) return fail(c, PG_ERR_INVALID, "pg_hit_uvs: too many rays");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf r, o, ovf;
    HIPC(c, r.alloc(n * 32));
    HIPC(c, o.alloc(n * 8));
    HIPC(c, ovf.alloc(pg_stack_overflow_words(pg_trace_rays_threads(n)) * 4));
    HIPC(c, hipMemcpyAsync(r.p, rays, n * 32, hipMemcpyHostToDevice, c->stream));
    pg_launch_hit_uvs(c->stream, sceneView(c), r.as<float>(), (uint32_t)n, o.as<float>(), ovf.as<uint32_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

// ---- normal maps (pg_capi.h pg_set_normal_maps) ----------------------------------------------------------------------
pg_status pg_set_normal_maps(void *ctx, const pg_texture *maps, uint32_t n_maps, const pg_texture_binding *bindings,
                             uint32_t n_bindings, const float *texcoords) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_set_normal_maps: null context");
    if (c->cfg.integrator != PG_INTEGRATOR_PATH)
        return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: the volumetric integrator does not support normal maps");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_set_normal_maps: no scene uploaded");
    if (c->scene_rendered) return fail(c, PG_ERR_STATE, "pg_set_normal_maps: a render pass has already run on this scene");
    if ((n_maps && !maps) || (n_bindings && !bindings)) return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: null argument");
    HIPC(c, hipSetDevice(c->cfg.device));
    // validate everything before anything changes
    std::vector<GTex> gtex(n_maps);
    for (uint32_t i = 0; i < n_maps; ++i) {
        std::string err;
        if (!makeGTex(maps[i], gtex[i], err))
            return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: map " + std::to_string(i) + ": " + err);
    }
    std::vector<uint32_t> mnmap(c->num_mats, 0xFFFFFFFFu);
    for (uint32_t b = 0; b < n_bindings; ++b) {
        const pg_texture_binding &tb = bindings[b];
        if (tb.material >= c->num_mats || tb.texture >= n_maps)
            return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: binding " + std::to_string(b) + ": index out of range");
        const uint32_t model = c->base_mats[tb.material].model;
        if (model != PG_BSDF_DIFFUSE && model != PG_BSDF_PLASTIC && model != PG_BSDF_ROUGHPLASTIC &&
            model != PG_BSDF_CONDUCTOR && model != PG_BSDF_ROUGHCONDUCTOR)
            return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: binding " + std::to_string(b) +
                                               ": the material's model (dielectric, roughdielectric or null) takes no normal map");
        if (mnmap[tb.material] != 0xFFFFFFFFu)
            return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: material " + std::to_string(tb.material) + " is bound twice");
        mnmap[tb.material] = tb.texture;
    }
    if (texcoords)
        for (size_t i = 0; i < (size_t)2 * c->num_vertices; ++i)
            if (!std::isfinite(texcoords[i])) return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: non-finite texcoord");
    if (n_bindings && !sameTexcoords(c->tex_uv, texcoords))
        return fail(c, PG_ERR_INVALID, "pg_set_normal_maps: texcoords differ from those of pg_set_textures");
    if (pg_status s = clearNormalMaps(c)) return s;
    if (n_bindings == 0) return PG_OK;

    // from here on a failure puts the scene without normal maps back, as pg_set_textures does for its set
    auto restoreBase = [&](pg_status why) {
        const std::string msg = c->err;
        c->nmapped = true;
        (void)clearNormalMaps(c);
        c->err = msg;
        return why;
    };
    pg_status s;
    if ((s = uploadTexels(c, maps, n_maps, c->ntexels, gtex))) return restoreBase(s);
    c->nmapped = true;
    c->host_mnmap = mnmap;
    if (texcoords) c->nmap_uv.assign(texcoords, texcoords + 2 * (size_t)c->num_vertices);
    if ((s = upload(c, c->ntex, gtex)) || (s = upload(c, c->mnmap, mnmap)) || (s = syncTexRows(c))) return restoreBase(s);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return restoreBase(fail(c, PG_ERR_HIP, "pg_set_normal_maps: upload failed"));
    return PG_OK;
}

pg_status pg_hit_frames(void *ctx, const float *rays, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!rays && n) || (!out && n)) return fail(c, PG_ERR_INVALID, "pg_hit_frames: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_hit_frames: no scene");
    if (n > 0xFFFFFFFFull / 12) return fail(c, PG_ERR_INVALID, "pg_hit_frames: too many rays");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf r, o, ovf;
    HIPC(c, r.alloc(n * 32));
    HIPC(c, o.alloc(n * 48));
    HIPC(c, ovf.alloc(pg_stack_overflow_words(pg_trace_rays_threads(n)) * 4));
    HIPC(c, hipMemcpyAsync(r.p, rays, n * 32, hipMemcpyHostToDevice, c->stream));
    pg_launch_hit_frames(c->stream, sceneView(c), r.as<float>(), (uint32_t)n, o.as<float>(), ovf.as<uint32_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 48, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

// ---- delta emitters (pg_capi.h pg_set_delta_emitters) ----------------------------------------------------------------
pg_status pg_set_delta_emitters(void *ctx, const pg_delta_emitter *emitters, uint32_t n) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_set_delta_emitters: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_set_delta_emitters: no scene uploaded");
    if (c->scene_rendered)
        return fail(c, PG_ERR_STATE, "pg_set_delta_emitters: a render pass has already run on this scene");
    if (n && !emitters) return fail(c, PG_ERR_INVALID, "pg_set_delta_emitters: null argument");
    if ((uint64_t)c->num_area + n + (c->has_env ? 1u : 0u) > 65534)
        return fail(c, PG_ERR_INVALID, "pg_set_delta_emitters: more than 65534 emitters");
    HIPC(c, hipSetDevice(c->cfg.device));
    // validate everything before anything changes
    float center[3];
    const float radius = pgh::boxSphere(c->tri_lo, c->tri_hi, center) * 1.1f;
    std::vector<GDelta> recs(n);
    for (uint32_t i = 0; i < n; ++i) {
        const pg_delta_emitter &e = emitters[i];
        const std::string id = "pg_set_delta_emitters: emitter " + std::to_string(i) + ": ";
        if (e.type != PG_EMITTER_POINT && e.type != PG_EMITTER_SPOT && e.type != PG_EMITTER_DIRECTIONAL)
            return fail(c, PG_ERR_INVALID, id + "unknown type");
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(e.position[k]) || !std::isfinite(e.direction[k]) || !std::isfinite(e.intensity[k]))
                return fail(c, PG_ERR_INVALID, id + "non-finite field");
            if (e.intensity[k] < 0) return fail(c, PG_ERR_INVALID, id + "negative intensity");
        }
        if (!std::isfinite(e.cutoff_angle) || !std::isfinite(e.beam_width))
            return fail(c, PG_ERR_INVALID, id + "non-finite field");
        GDelta &g = recs[i];
        g = GDelta{};
        g.type = (uint32_t)e.type;
        for (int k = 0; k < 3; ++k) g.intensity[k] = e.intensity[k];
        if (e.type != PG_EMITTER_POINT) {
            const float l = std::sqrt(e.direction[0] * e.direction[0] + e.direction[1] * e.direction[1] +
                                      e.direction[2] * e.direction[2]);
            if (!(l > 0) || !std::isfinite(l)) return fail(c, PG_ERR_INVALID, id + "zero direction");
            for (int k = 0; k < 3; ++k) g.dir[k] = e.direction[k] / l;
        }
        if (e.type == PG_EMITTER_DIRECTIONAL) {  // the disk's centre (directional.cpp:159-180)
            for (int k = 0; k < 3; ++k) g.pos[k] = center[k] - g.dir[k] * radius;
        } else {
            for (int k = 0; k < 3; ++k) g.pos[k] = e.position[k];
        }
        if (e.type == PG_EMITTER_SPOT) {  // SpotEmitter::configure (spot.cpp:105-112)
            if (!(e.beam_width >= 0 && e.beam_width < e.cutoff_angle && e.cutoff_angle < 3.14159265358979323846f))
                return fail(c, PG_ERR_INVALID, id + "a spot needs 0 <= beam_width < cutoff_angle < pi");
            g.cutoff = e.cutoff_angle;
            g.cos_cutoff = std::cos(e.cutoff_angle);
            g.cos_beam = std::cos(e.beam_width);
            g.inv_transition = 1.0f / (e.cutoff_angle - e.beam_width);
        }
    }
    if (n) {
        DevBuf nb;
        HIPC(c, nb.alloc((size_t)n * sizeof(GDelta)));
        HIPC(c, hipMemcpy(nb.p, recs.data(), (size_t)n * sizeof(GDelta), hipMemcpyHostToDevice));
        std::swap(c->delta.p, nb.p);
        std::swap(c->delta.bytes, nb.bytes);
    } else {
        c->delta.release();
    }
    c->num_delta = n;
    c->g.num_emitters = c->num_area + n + (c->has_env ? 1u : 0u);
    return resetBlockers(c);
}

// ---- homogeneous media (pg_capi.h pg_set_homogeneous_media) -----------------------------------------------------------
pg_status pg_set_homogeneous_media(void *ctx, const pg_homogeneous_medium *media, uint32_t n) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_set_homogeneous_media: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_set_homogeneous_media: no scene uploaded");
    if (c->scene_rendered)
        return fail(c, PG_ERR_STATE, "pg_set_homogeneous_media: a render pass has already run on this scene");
    if (c->cfg.integrator != PG_INTEGRATOR_VOLPATH)
        return fail(c, PG_ERR_INVALID, "pg_set_homogeneous_media: the path integrator has no media");
    if (n && !media) return fail(c, PG_ERR_INVALID, "pg_set_homogeneous_media: null argument");
    HIPC(c, hipSetDevice(c->cfg.device));
    // validate everything before anything changes
    std::vector<GMedium> recs = c->base_media;
    std::vector<uint8_t> mark(c->num_media, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const pg_homogeneous_medium &h = media[i];
        const std::string id = "pg_set_homogeneous_media: record " + std::to_string(i) + ": ";
        if (h.medium >= c->num_media) return fail(c, PG_ERR_INVALID, id + "medium index out of range");
        if (mark[h.medium]) return fail(c, PG_ERR_INVALID, id + "medium named twice");
        float sigmaT[3];
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(h.sigma_a[k]) || !std::isfinite(h.sigma_s[k]))
                return fail(c, PG_ERR_INVALID, id + "non-finite coefficient");
            if (h.sigma_a[k] < 0 || h.sigma_s[k] < 0) return fail(c, PG_ERR_INVALID, id + "negative coefficient");
            sigmaT[k] = h.sigma_a[k] + h.sigma_s[k];
            if (!std::isfinite(sigmaT[k])) return fail(c, PG_ERR_INVALID, id + "non-finite coefficient");
        }
        if (sigmaT[0] == 0 && sigmaT[1] == 0 && sigmaT[2] == 0)
            return fail(c, PG_ERR_INVALID, id + "sigma_t is zero in every channel");
        if (!(std::fabs(h.g) < 1)) return fail(c, PG_ERR_INVALID, id + "|g| must be below 1");
        float weight = h.medium_sampling_weight;
        if (weight == -1.0f) {  // the reference's default (homogeneous.cpp:168-183)
            weight = 0;
            for (int k = 0; k < 3; ++k)
                if (sigmaT[k] != 0) weight = std::max(weight, h.sigma_s[k] / sigmaT[k]);
            if (weight > 0) weight = std::max(weight, 0.5f);
        } else if (!(weight >= 0 && weight <= 1)) {
            return fail(c, PG_ERR_INVALID, id + "medium_sampling_weight outside [0, 1] and not -1");
        }
        mark[h.medium] = 1;
        GMedium &g = recs[h.medium];
        g.density = nullptr;
        g.maj = nullptr;
        g.bx = 1;
        g.g = h.g;
        g.scale = weight;
        for (int k = 0; k < 3; ++k) {
            g.gs[k] = sigmaT[k];
            g.go[k] = h.sigma_s[k];
        }
    }
    if (c->num_media)
        HIPC(c, hipMemcpy(c->media.p, recs.data(), recs.size() * sizeof(GMedium), hipMemcpyHostToDevice));
    c->is_homog = mark;
    c->num_homog = n;
    return PG_OK;
}

pg_status pg_homogeneous_query(void *ctx, uint32_t medium, int32_t op, const float *rays, const uint32_t *keys, uint64_t n,
                               float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!rays && n) || (!out && n) || (op == 0 && !keys && n))
        return fail(c, PG_ERR_INVALID, "pg_homogeneous_query: null argument");
    if (op < 0 || op > 1) return fail(c, PG_ERR_INVALID, "pg_homogeneous_query: bad op");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_homogeneous_query: no scene");
    if (medium >= c->num_media || !c->is_homog[medium])
        return fail(c, PG_ERR_INVALID, "pg_homogeneous_query: not a homogeneous medium");
    if (n > 0xFFFFFFFFull / 8) return fail(c, PG_ERR_INVALID, "pg_homogeneous_query: too many rays");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf a, k, o;
    HIPC(c, a.alloc(n * 32));
    HIPC(c, o.alloc(n * 32));
    HIPC(c, hipMemcpyAsync(a.p, rays, n * 32, hipMemcpyHostToDevice, c->stream));
    if (op == 0) {
        HIPC(c, k.alloc(n * 8));
        HIPC(c, hipMemcpyAsync(k.p, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    pg_launch_homog_query(c->stream, c->media.as<GMedium>() + medium, op, a.as<float>(),
                          op == 0 ? k.as<uint32_t>() : nullptr, (uint32_t)n, o.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_emitter_query(void *ctx, const float *ref, const float *samples, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (n && (!ref || !samples || !out))) return fail(c, PG_ERR_INVALID, "pg_emitter_query: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_emitter_query: no scene");
    if (n > 0xFFFFFFFFull / 8) return fail(c, PG_ERR_INVALID, "pg_emitter_query: too many points");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf r, s, o;
    HIPC(c, r.alloc(n * 12));
    HIPC(c, s.alloc(n * 8));
    HIPC(c, o.alloc(n * 32));
    HIPC(c, hipMemcpyAsync(r.p, ref, n * 12, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(s.p, samples, n * 8, hipMemcpyHostToDevice, c->stream));
    pg_launch_emitter_query(c->stream, c->g, sceneView(c), r.as<float>(), s.as<float>(), (uint32_t)n, o.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_read_film_filtered(void *ctx, float *rgbw, int64_t *raw) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_read_film_filtered: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_read_film_filtered: no scene");
    if (!c->filtered) return fail(c, PG_ERR_STATE, "pg_read_film_filtered: no filter set (pg_set_rfilter)");
    HIPC(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)c->g.width * c->g.height * 4;
    std::vector<int64_t> tmp;
    int64_t *dst = raw;
    if (!dst && rgbw) {
        tmp.resize(n);
        dst = tmp.data();
    }
    if (!dst) return PG_OK;
    HIPC(c, hipMemcpyAsync(dst, c->film_acc.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (rgbw)
        for (size_t i = 0; i < n; ++i) rgbw[i] = (float)((double)dst[i] * 0x1p-28);
    return PG_OK;
}

pg_status pg_upload_scene(void *ctx, const pg_scene_desc *d) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !d) return fail(c, PG_ERR_INVALID, "pg_upload_scene: null argument");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!d->positions || !d->indices || !d->shapes || !d->materials || d->num_triangles == 0)
        return fail(c, PG_ERR_INVALID, "pg_upload_scene: empty scene");
    if (d->camera.width == 0 || d->camera.height == 0) return fail(c, PG_ERR_INVALID, "pg_upload_scene: empty film");
    const uint32_t nt = d->num_triangles;
    for (uint64_t i = 0; i < 3ull * nt; ++i)
        if (d->indices[i] >= d->num_vertices) return fail(c, PG_ERR_INVALID, "pg_upload_scene: index out of range");
    if (d->num_materials > 65535 || d->num_emitters > 65534 || d->num_media > 65534)
        return fail(c, PG_ERR_INVALID, "pg_upload_scene: too many materials/emitters/media");
    for (uint32_t m = 0; m < d->num_materials; ++m)
        if (d->materials[m].type >= PG_BSDF_COUNT || d->materials[m].distribution > PG_DIST_GGX)
            return fail(c, PG_ERR_INVALID, "pg_upload_scene: bad material type");
    if (d->num_media && !d->media) return fail(c, PG_ERR_INVALID, "pg_upload_scene: media missing");
    if (d->camera_medium < -1 || d->camera_medium >= (int32_t)d->num_media)
        return fail(c, PG_ERR_INVALID, "pg_upload_scene: bad camera medium");
    if (d->envmap && c->cfg.integrator != PG_INTEGRATOR_PATH)
        return fail(c, PG_ERR_INVALID, "pg_upload_scene: the volumetric integrator does not support an environment emitter");
    std::vector<GMedium> gmed;
    std::vector<size_t> denOff;
    size_t denTotal = 0;
    for (uint32_t m = 0; m < d->num_media; ++m) {
        const pg_medium &pm = d->media[m];
        if (pg_status vs = validateMedium(c, pm, m)) return vs;
        GMedium gm{};
        gm.resx = pm.res[0];
        gm.resy = pm.res[1];
        gm.resz = pm.res[2];
        gm.scale = pm.scale;
        gm.invMax = 1.0f / (pm.scale * 1.0f);  // maxDensity = scale * getMaximumFloatValue() = scale
        gm.g = pm.g;
        for (int a = 0; a < 3; ++a) {
            gm.lo[a] = pm.aabb_min[a];
            gm.hi[a] = pm.aabb_max[a];
            gm.gs[a] = (float)(pm.res[a] - 1) / (pm.aabb_max[a] - pm.aabb_min[a]);
            gm.go[a] = gm.gs[a] * -pm.aabb_min[a];
            gm.albedo[a] = pm.albedo[a];
        }
        denOff.push_back(denTotal);
        denTotal += (size_t)pm.res[0] * pm.res[1] * pm.res[2];
        gm.mx = std::max(1u, (pm.res[0] - 1 + PG_MAJORANT_CELL - 1) / PG_MAJORANT_CELL);
        gm.my = std::max(1u, (pm.res[1] - 1 + PG_MAJORANT_CELL - 1) / PG_MAJORANT_CELL);
        gm.mz = std::max(1u, (pm.res[2] - 1 + PG_MAJORANT_CELL - 1) / PG_MAJORANT_CELL);
        gmed.push_back(gm);
    }
    // per-triangle (material | emitter+1 << 16) from the shape partition
    std::vector<uint32_t> triBits(nt, 0xFFFFFFFFu);
    for (uint32_t s = 0; s < d->num_shapes; ++s) {
        const pg_shape &sh = d->shapes[s];
        if ((uint64_t)sh.tri_begin + sh.tri_count > nt || sh.material >= d->num_materials ||
            (sh.emitter >= 0 && (uint32_t)sh.emitter >= d->num_emitters) || sh.interior_medium < -1 ||
            sh.interior_medium >= (int32_t)d->num_media || sh.exterior_medium < -1 ||
            sh.exterior_medium >= (int32_t)d->num_media)
            return fail(c, PG_ERR_INVALID, "pg_upload_scene: bad shape");
        uint32_t bits = sh.material | ((uint32_t)(sh.emitter + 1) << 16);
        for (uint32_t t = 0; t < sh.tri_count; ++t) triBits[sh.tri_begin + t] = bits;
    }
    for (uint32_t t = 0; t < nt; ++t)
        if (triBits[t] == 0xFFFFFFFFu) return fail(c, PG_ERR_INVALID, "pg_upload_scene: triangle without a shape");

    pgh::BvhOut bvh;
    if (!pgh::buildBvh(d->positions, d->indices, nt, kStackDepth, bvh))
        return fail(c, PG_ERR_INVALID, "pg_upload_scene: BVH deeper than the traversal stack");
    std::vector<float> shade((size_t)4 * PG_TRI_SHADE_STRIDE * nt, 0.0f);
    std::vector<uint8_t> tclass(nt), tcheap(nt);
    c->diffuse_null = true;
    for (uint32_t i = 0; i < d->num_materials; ++i)
        if (d->materials[i].type != PG_BSDF_DIFFUSE && d->materials[i].type != PG_BSDF_NULL) c->diffuse_null = false;
    for (uint32_t k = 0; k < nt; ++k) {
        uint32_t t = bvh.order[k];
        packShade(&shade[4 * PG_TRI_SHADE_STRIDE * (size_t)k], d->positions, d->normals, d->indices, t, triBits[t], t);
        // bit 7: an emitter's triangle, the one hit a doomed ray is kept for (pg_layout.h PF_DOOMED)
        tclass[k] = (uint8_t)(materialClass(d->materials[triBits[t] & 0xFFFFu].type) |
                              ((triBits[t] >> 16) != 0 ? PG_TCLASS_EMITTER : 0u));
        // volumetric wavefront: surfaces whose interaction skips the shadow walk through media (delta
        // BSDFs) or ends the path at once (emitters: black in the scenes here) -- VolDev::tcheap
        tcheap[k] = (tclass[k] & PG_TCLASS_MASK) == PG_CLASS_DELTA || (triBits[t] >> 16) != 0;
    }
    // per BVH-order triangle: the shape's medium transition, (interior + 1) | (exterior + 1) << 16
    std::vector<uint32_t> tmed(nt, 0);
    {
        std::vector<uint32_t> shapeMed(nt, 0);
        for (uint32_t sidx = 0; sidx < d->num_shapes; ++sidx) {
            const pg_shape &sh = d->shapes[sidx];
            const uint32_t bits = (uint32_t)(sh.interior_medium + 1) | ((uint32_t)(sh.exterior_medium + 1) << 16);
            for (uint32_t t = 0; t < sh.tri_count; ++t) shapeMed[sh.tri_begin + t] = bits;
        }
        for (uint32_t k = 0; k < nt; ++k) tmed[k] = shapeMed[bvh.order[k]];
    }
    // emitters: compact triangle array + area CDF (double accumulation of fp32 areas)
    std::vector<GEmitter> ems;
    std::vector<float> emtri, emcdf;
    for (uint32_t e = 0; e < d->num_emitters; ++e) {
        const pg_emitter &pe = d->emitters[e];
        if (pe.shape >= d->num_shapes) return fail(c, PG_ERR_INVALID, "pg_upload_scene: emitter without shape");
        const pg_shape &sh = d->shapes[pe.shape];
        GEmitter g{};
        g.tri_begin = (uint32_t)(emtri.size() / 20);
        g.tri_count = sh.tri_count;
        g.cdf_begin = (uint32_t)emcdf.size();
        std::vector<double> cum(sh.tri_count + 1, 0.0);
        double acc = 0;
        for (uint32_t i = 0; i < sh.tri_count; ++i) {
            uint32_t t = sh.tri_begin + i;
            const float *a = d->positions + 3 * (size_t)d->indices[3 * (size_t)t];
            const float *b = d->positions + 3 * (size_t)d->indices[3 * (size_t)t + 1];
            const float *cc = d->positions + 3 * (size_t)d->indices[3 * (size_t)t + 2];
            float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {cc[0] - a[0], cc[1] - a[1], cc[2] - a[2]};
            float x[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
            float area = 0.5f * std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
            acc += (double)area;
            cum[i + 1] = acc;
            size_t o = emtri.size();
            emtri.resize(o + 20);
            packShade(&emtri[o], d->positions, d->normals, d->indices, t, 0, t);
        }
        if (!(acc > 0)) return fail(c, PG_ERR_INVALID, "pg_upload_scene: emitter with zero area");
        for (uint32_t i = 0; i < sh.tri_count; ++i) emcdf.push_back((float)(cum[i] / acc));
        emcdf.push_back(1.0f);
        g.inv_area = 1.0f / (float)acc;
        for (int k = 0; k < 4; ++k) g.radiance[k] = pe.radiance[k];
        ems.push_back(g);
    }
    {  // padded boxes over the triangles that carry tclass' emitter bit (pg_layout.h "Doom probe")
        std::vector<uint32_t> triEmitter(nt);
        for (uint32_t t = 0; t < nt; ++t) triEmitter[t] = triBits[t] >> 16;
        c->num_em_boxes = pg_emitter_boxes(d->positions, d->indices, triEmitter.data(), nt, d->num_emitters, c->em_box,
                                           &c->em_absmax);
    }
    c->num_blockers = c->num_occluders = 0;
    c->blk_stopped = c->prb_stopped = false;
    c->absmax = 0.0f;
    for (size_t i = 0; i < (size_t)3 * d->num_vertices; ++i) c->absmax = std::max(c->absmax, std::fabs(d->positions[i]));
    // nt + 1 words for the shadow blockers (the last: the shadow rays counted), then as many for the probe occluders
    HIPC(c, c->blk_counts.alloc(2 * ((size_t)nt + 1) * 4));
    HIPC(c, hipMemsetAsync(c->blk_counts.p, 0, 2 * ((size_t)nt + 1) * 4, c->stream));
    c->host_tris = bvh.tris;
    c->host_shade = shade;
    // a new scene has no textures (pg_set_textures)
    c->textured = c->nmapped = false;
    c->scene_rendered = false;
    for (DevBuf *b : {&c->tuv, &c->tex, &c->mtex, &c->texels, &c->ntex, &c->mnmap, &c->ntexels, &c->ttan}) b->release();
    for (auto *v : {&c->host_mtex, &c->host_mnmap}) v->clear();
    for (auto *v : {&c->tex_uv, &c->nmap_uv}) v->clear();
    c->base_tclass = tclass;
    c->host_indices.assign(d->indices, d->indices + 3 * (size_t)nt);
    c->num_vertices = d->num_vertices;
    c->host_mats.clear();
    for (uint32_t m = 0; m < d->num_materials; ++m) c->host_mats.push_back(makeGMat(d->materials[m]));
    // roughplastic: rough-transmittance slice + internal diffuse Fresnel per material
    // (RoughPlastic::configure, roughplastic.cpp:283-299; ranges of rtrans.h checkEta/checkAlpha)
    std::vector<float> rtab;
    std::vector<std::pair<uint32_t, size_t>> rtabOf;
    for (uint32_t m = 0; m < d->num_materials; ++m) {
        const pg_material &pm = d->materials[m];
        if (pm.type != PG_BSDF_ROUGHPLASTIC) continue;
        GMat &gm = c->host_mats[m];
        if (pm.alpha_u != pm.alpha_v)
            return fail(c, PG_ERR_INVALID, "pg_upload_scene: roughplastic does not support anisotropic roughness");
        const float e = gm.eta < 1 ? 1 / gm.eta : gm.eta;
        if (!(e >= 1.0001f && e <= 4.0f) || !(gm.alpha_u <= 4.0f))
            return fail(c, PG_ERR_INVALID, "pg_upload_scene: roughplastic IOR or roughness outside the tabulated range");
        const size_t off = rtab.size();
        rtab.resize(off + pgh::kRoughTransSamples);
        pgh::roughTransmittance((int)pm.distribution, gm.alpha_u, gm.eta, &rtab[off], &gm.fdrInt);
        rtabOf.push_back({m, off});
    }

    pg_status s;
    if ((s = upload(c, c->rtab, rtab))) return s;
    for (auto &mo : rtabOf) c->host_mats[mo.first].rtrans = c->rtab.as<float>() + mo.second;
    c->base_mats = c->host_mats;
    c->bvh_top_nodes = std::min<uint32_t>(bvh.top_nodes, PG_BVH4_TOP_NODES);
    if ((s = upload(c, c->nodes, bvh.nodes)) || (s = upload(c, c->tris, bvh.tris)) ||
        (s = upload(c, c->wnodes, bvh.wnodes)) || (s = upload(c, c->tshade, shade)) ||
        (s = upload(c, c->tclass, tclass)) ||
        (s = upload(c, c->mats, c->host_mats)) || (s = upload(c, c->ems, ems)) || (s = upload(c, c->emtri, emtri)) ||
        (s = upload(c, c->emcdf, emcdf)) || (s = upload(c, c->tmed, tmed)) || (s = upload(c, c->tcheap, tcheap)))
        return s;
    // densities: one buffer, each grid 256-B aligned (corner-packed, see pg_layout.h GMedium)
    {
        size_t words = 0, linMax = 0;
        std::vector<size_t> at;
        // corner-packed grids (pg_layout.h "Corner-packed density"); a grid with a dimension of 1 has no
        // cell (every lookup is 0) and keeps no density
        for (uint32_t m = 0; m < d->num_media; ++m) {
            const pg_medium &pm = d->media[m];
            at.push_back(words);
            const size_t lin = (size_t)pm.res[0] * pm.res[1] * pm.res[2];
            const size_t cells = (size_t)(pm.res[0] - 1) * (pm.res[1] - 1) * (pm.res[2] - 1);
            const size_t n = cells * 8;
            if (cells) linMax = std::max(linMax, lin);
            words += (n + 63) & ~(size_t)63;
        }
        {
            // corner packing takes 8x the grid's memory plus a linear staging copy (pg_layout.h)
            const hipError_t e = c->density.grow(std::max<size_t>(words * 4, 256));
            if (e != hipSuccess)
                return fail(c, e == hipErrorOutOfMemory ? PG_ERR_OOM : PG_ERR_HIP,
                            "pg_upload_scene: cannot allocate " + std::to_string(words * 4) + " B of density (corner-packed: 8 floats per cell): " +
                                hipGetErrorString(e));
        }
        DevBuf linTmp;  // the linear grid of a corner-packed medium, expanded on the device
        if (linMax) HIPC(c, linTmp.alloc(linMax * 4));
        for (uint32_t m = 0; m < d->num_media; ++m) {
            const pg_medium &pm = d->media[m];
            const size_t n = (size_t)pm.res[0] * pm.res[1] * pm.res[2];
            HIPC(c, hipMemcpyAsync(linTmp.p, pm.density, n * 4, hipMemcpyHostToDevice, c->stream));
            pg_launch_density_corners(c->stream, linTmp.as<float>(), pm.res[0], pm.res[1], pm.res[2],
                                      c->density.as<float>() + at[m]);
            HIPC(c, hipGetLastError());
            HIPC(c, hipStreamSynchronize(c->stream));  // linTmp is reused by the next medium
            gmed[m].density = c->density.as<float>() + at[m];
        }
        // majorant grids (PG_MAJORANT_GRID tracking): one buffer, per-medium offsets
        std::vector<float> maj;
        std::vector<size_t> majAt;
        for (uint32_t m = 0; m < d->num_media; ++m) {
            majAt.push_back(maj.size());
            buildMajorants(d->media[m], gmed[m], maj);
        }
        if ((s = upload(c, c->majorant, maj))) return s;
        for (uint32_t m = 0; m < d->num_media; ++m) gmed[m].maj = c->majorant.as<float>() + majAt[m];
        HIPC(c, hipStreamSynchronize(c->stream));  // the host density arrays are caller-owned
        if ((s = upload(c, c->media, gmed))) return s;
        c->num_media = d->num_media;
        // a new scene has no homogeneous media (pg_set_homogeneous_media)
        c->base_media = gmed;
        c->is_homog.assign(d->num_media, 0);
        c->num_homog = 0;
        c->cam_medium = d->camera_medium;
    }

    // camera (Transform::lookAt, transform.cpp:191-214) and integrator constants
    GParams &g = c->g;
    std::memset(&g, 0, sizeof g);
    const pg_camera &cam = d->camera;
    float dir[3] = {cam.target[0] - cam.origin[0], cam.target[1] - cam.origin[1], cam.target[2] - cam.origin[2]};
    float l = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    for (int a = 0; a < 3; ++a) dir[a] /= l;
    const float *up = cam.up;
    float left[3] = {up[1] * dir[2] - up[2] * dir[1], up[2] * dir[0] - up[0] * dir[2], up[0] * dir[1] - up[1] * dir[0]};
    l = std::sqrt(left[0] * left[0] + left[1] * left[1] + left[2] * left[2]);
    for (int a = 0; a < 3; ++a) left[a] /= l;
    float nup[3] = {dir[1] * left[2] - dir[2] * left[1], dir[2] * left[0] - dir[0] * left[2],
                    dir[0] * left[1] - dir[1] * left[0]};
    for (int a = 0; a < 3; ++a) {
        g.cam_o[a] = cam.origin[a];
        g.cam_left[a] = left[a];
        g.cam_up[a] = nup[a];
        g.cam_dir[a] = dir[a];
    }
    g.tan_half = std::tan(cam.fov_x_deg * 3.14159265358979323846f / 360.0f);
    g.aspect = (float)cam.width / (float)cam.height;
    g.near_clip = cam.near_clip;
    g.far_clip = cam.far_clip;
    g.width = cam.width;
    g.height = cam.height;
    g.num_emitters = d->num_emitters + (d->envmap ? 1u : 0u);
    g.num_area = d->num_emitters;
    g.num_materials = d->num_materials;
    // a new scene has no delta emitters (pg_set_delta_emitters)
    c->num_area = d->num_emitters;
    c->num_delta = 0;
    c->delta.release();
    for (int a = 0; a < 3; ++a) {
        c->tri_lo[a] = bvh.lo[a];
        c->tri_hi[a] = bvh.hi[a];
    }

    // tile shard of this rank: 32x32 tiles dealt round-robin
    const uint32_t T = c->cfg.tile_size, tx = (cam.width + T - 1) / T, ty = (cam.height + T - 1) / T;
    c->local_pixels.clear();
    c->h_tile_first.clear();
    c->h_tile_origin.clear();
    for (uint32_t t = 0; t < tx * ty; ++t) {
        if ((int32_t)(t % (uint32_t)c->cfg.world_size) != c->cfg.rank) continue;
        uint32_t x0 = (t % tx) * T, y0 = (t / tx) * T;
        c->h_tile_first.push_back((uint32_t)c->local_pixels.size());
        c->h_tile_origin.push_back(x0);
        c->h_tile_origin.push_back(y0);
        const uint32_t x1 = std::min(x0 + T, cam.width), y1 = std::min(y0 + T, cam.height);
        // within a tile, PG_PIXEL_BLOCK^2 pixel blocks (one wave of camera rays per 8x8 block) in
        // row-major block order; 0 = plain row-major.  Per-pixel results do not depend on the order.
        const uint32_t B = PG_PIXEL_BLOCK > 0 ? PG_PIXEL_BLOCK : T;
        for (uint32_t by = y0; by < y1; by += B)
            for (uint32_t bx = x0; bx < x1; bx += B)
                for (uint32_t y = by; y < std::min(by + B, y1); ++y)
                    for (uint32_t x = bx; x < std::min(bx + B, x1); ++x) c->local_pixels.push_back(y * cam.width + x);
    }
    c->h_tile_first.push_back((uint32_t)c->local_pixels.size());
    if ((s = upload(c, c->d_local_pixels, c->local_pixels))) return s;
    {  // the surface path's pixel order: bands {r, r + 8, r + 16, ...} of the local pixels as the r-th eighth
        const uint32_t nb = cameraBands(), np = (uint32_t)c->local_pixels.size();
        std::vector<uint32_t> bp;
        bp.reserve(np);
        if (nb > 8 && np >= kBandMinPixels) {
            for (uint32_t r = 0; r < 8; ++r)
                for (uint32_t gb = r; gb < nb; gb += 8)
                    for (uint32_t i = (uint32_t)((uint64_t)gb * np / nb); i < (uint32_t)((uint64_t)(gb + 1) * np / nb); ++i)
                        bp.push_back(c->local_pixels[i]);
        } else {
            bp = c->local_pixels;
        }
        if ((s = upload(c, c->d_band_pixels, bp))) return s;
    }
    size_t fb = (size_t)cam.width * cam.height * 16;
    HIPC(c, c->film.alloc(fb));
    HIPC(c, c->film_sq.alloc(fb));
    HIPC(c, hipMemsetAsync(c->film.p, 0, fb, c->stream));
    HIPC(c, hipMemsetAsync(c->film_sq.p, 0, fb, c->stream));
    if (c->cfg.aovs) {
        HIPC(c, c->aov_albedo.alloc(fb));
        HIPC(c, c->aov_normal.alloc(fb));
        HIPC(c, hipMemsetAsync(c->aov_albedo.p, 0, fb, c->stream));
        HIPC(c, hipMemsetAsync(c->aov_normal.p, 0, fb, c->stream));
    }
    if (c->filtered && (s = setupFiltered(c))) return s;
    HIPC(c, c->rec_count.alloc(16));
    HIPC(c, hipMemsetAsync(c->rec_count.p, 0, 16, c->stream));
    c->rec_host_count = 0;
    c->num_tris = nt;
    c->num_mats = d->num_materials;
    // Scene::getAABB(): the kd-tree's slightly enlarged bounds (gkdtree.h:1213-1220,
    // MTS_KD_AABB_EPSILON = 1e-3); the SD-tree covers this box
    for (int a = 0; a < 3; ++a) {
        const float eps = 1e-3f;
        float lo = bvh.lo[a], hi = bvh.hi[a];
        lo = lo - ((hi - lo) * eps + eps);
        hi = hi + ((hi - lo) * eps + eps);
        c->scene_lo[a] = lo;
        c->scene_hi[a] = hi;
    }
    // environment emitter (EnvironmentMap::configure + createShape, envmap.cpp:260-356)
    c->has_env = false;
    if (d->envmap) {
        pgh::EnvTables et;
        std::string err;
        if (!pgh::buildEnvTables(*d->envmap, c->scene_lo, c->scene_hi, et, err))
            return fail(c, PG_ERR_INVALID, "pg_upload_scene: " + err);
        std::vector<float> tab;  // cdf_rows | cdf_cols | row_weights, each 16-B aligned
        auto put = [&](const std::vector<float> &v) {
            const size_t at = tab.size();
            tab.insert(tab.end(), v.begin(), v.end());
            tab.resize((tab.size() + 3) & ~(size_t)3, 0.0f);
            return at;
        };
        const size_t oRows = put(et.cdf_rows), oCols = put(et.cdf_cols), oW = put(et.row_weights);
        if ((s = upload(c, c->envtex, et.texels)) || (s = upload(c, c->envtab, tab))) return s;
        GEnv ge{};
        ge.texels = c->envtex.as<float>();
        ge.cdf_rows = c->envtab.as<float>() + oRows;
        ge.cdf_cols = c->envtab.as<float>() + oCols;
        ge.row_weights = c->envtab.as<float>() + oW;
        ge.width = et.width;
        ge.height = et.height;
        ge.scale = et.scale;
        ge.normalization = et.normalization;
        ge.pixel_size[0] = et.pixel_size[0];
        ge.pixel_size[1] = et.pixel_size[1];
        ge.radius = et.radius;
        for (int a = 0; a < 3; ++a) ge.center[a] = et.center[a];
        for (int k = 0; k < 9; ++k) ge.R[k] = et.R[k];
        if ((s = upload(c, c->env, std::vector<GEnv>{ge}))) return s;
        c->has_env = true;
    }
    c->sd.reset(c->scene_lo, c->scene_hi);
    // pinned staging for the tree transfers, sized once for a large tree here (growing it inside a
    // training loop re-pins memory, ~10-20 ms per growth)
    HIPC(c, c->sd_stage.reserve((size_t)48 << 20));
    if ((s = uploadSd(c))) return s;
    HIPC(c, hipStreamSynchronize(c->stream));
    c->has_scene = true;
    return PG_OK;
}

pg_status pg_rough_transmittance(uint32_t distribution, float alpha, float eta, float *table, float *fdr_int) {
    if (!table || !fdr_int) return fail(nullptr, PG_ERR_INVALID, "pg_rough_transmittance: null argument");
    if (distribution > PG_DIST_GGX || !(alpha >= 0) || !(eta > 0) || eta == 1.0f)
        return fail(nullptr, PG_ERR_INVALID, "pg_rough_transmittance: bad distribution, alpha or eta");
    pgh::roughTransmittance((int)distribution, std::max(alpha, 1e-4f), eta, table, fdr_int);
    return PG_OK;
}

pg_status pg_get_record_count(void *ctx, uint64_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !count) return fail(c, PG_ERR_INVALID, "pg_get_record_count: null argument");
    *count = c->rec_host_count;
    return PG_OK;
}

pg_status pg_get_records(void *ctx, void *dst, uint64_t max_records, int32_t dst_is_device, uint64_t *written) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!dst && max_records)) return fail(c, PG_ERR_INVALID, "pg_get_records: null argument");
    HIPC(c, hipSetDevice(c->cfg.device));
    uint64_t n = std::min(max_records, c->rec_host_count);
    if (n)
        HIPC(c, hipMemcpyAsync(dst, c->records.p, n * sizeof(pg_record),
                               dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (written) *written = n;
    return PG_OK;
}

pg_status pg_splat_records(void *ctx, const void *src, uint64_t count, int32_t src_is_device) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!src && count)) return fail(c, PG_ERR_INVALID, "pg_splat_records: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_splat_records: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!count) return PG_OK;
    const pg_record *dsrc = (const pg_record *)src;
    if (!src_is_device) {
        HIPC(c, c->ext_records.alloc(count * sizeof(pg_record)));
        HIPC(c, hipMemcpyAsync(c->ext_records.p, src, count * sizeof(pg_record), hipMemcpyHostToDevice, c->stream));
        dsrc = c->ext_records.as<pg_record>();
    }
    EventPair &e = c->timing;
    if (!e.a) {
        HIPC(c, hipEventCreate(&e.a));
        HIPC(c, hipEventCreate(&e.b));
    }
    HIPC(c, hipEventRecord(e.a, c->stream));
    pg_launch_splat(c->stream, sdView(c), dsrc, count);
    HIPC(c, hipEventRecord(e.b, c->stream));
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e.a, e.b);
    c->stats.other_ms += ms;
    return PG_OK;
}

pg_status pg_splat_local_records(void *ctx) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_splat_local_records: null context");
    if (c->rec_host_count == 0) return PG_OK;
    return pg_splat_records(ctx, c->records.p, c->rec_host_count, 1);
}

pg_status pg_refit(void *ctx, uint32_t iteration) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_refit: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_refit: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    pg_status s;
    const auto t0 = std::chrono::steady_clock::now();
    if ((s = downloadSd(c))) return s;
    const auto t1 = std::chrono::steady_clock::now();
    c->sd.refit(iteration, c->cfg.s_tree_threshold, c->cfg.d_tree_threshold, c->cfg.d_tree_max_depth,
                c->cfg.bsdf_fraction_bound == PG_FRACTION_LEARNED);
    const auto t2 = std::chrono::steady_clock::now();
    if ((s = uploadSd(c))) return s;
    HIPC(c, hipMemsetAsync(c->rec_count.p, 0, 8, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (std::getenv("PG_DEBUG_REFIT")) {
        const auto t3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "refit %u: download %.2f ms, refit %.2f ms, upload %.2f ms (%zu D-trees, %zu / %zu nodes)\n",
                     iteration, ms(t0, t1), ms(t1, t2), ms(t2, t3), c->sd.leaves.size(), c->sd.samplingNodes(),
                     c->sd.buildingNodes());
    }
    c->rec_host_count = 0;
    return PG_OK;
}

pg_status pg_get_tree_stats(void *ctx, void *dst, uint64_t capacity_words, int32_t dst_is_device, uint64_t *words) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !words) return fail(c, PG_ERR_INVALID, "pg_get_tree_stats: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_get_tree_stats: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    const size_t nb = c->sd.buildingNodes(), nl = c->sd.leaves.size();
    *words = 4 * nb + nl + pgh::kFracStats * nl;
    if (!dst) return PG_OK;
    if (capacity_words < *words) return fail(c, PG_ERR_INVALID, "pg_get_tree_stats: buffer too small");
    const hipMemcpyKind k = dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPC(c, hipMemcpyAsync(dst, c->sdp.bsum, 8 * *words, k, c->stream));  // bsum | count | frac, contiguous
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_put_tree_stats(void *ctx, const void *src, uint64_t words, int32_t src_is_device) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !src) return fail(c, PG_ERR_INVALID, "pg_put_tree_stats: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_put_tree_stats: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    const size_t nb = c->sd.buildingNodes(), nl = c->sd.leaves.size();
    if (words != 4 * nb + nl + pgh::kFracStats * nl)
        return fail(c, PG_ERR_INVALID, "pg_put_tree_stats: size does not match the tree");
    const hipMemcpyKind k = src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPC(c, hipMemcpyAsync(c->sdp.bsum, src, 8 * words, k, c->stream));  // bsum | count | frac, contiguous
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

// ---- multi-GPU inside the library (RCCL over xGMI).  Replaces what the reference's remote
// scheduler does for a distributed render (include/mitsuba/core/sched_remote.h:50-236: ship work
// units to other machines, merge their image blocks): here every rank renders its tile shard, and
// the only exchanges are the postprogression statistics all-reduce and the final film reduce.
#define NCCLC(c, expr)                                                                            \
    do {                                                                                          \
        ncclResult_t _r = (expr);                                                                 \
        if (_r != ncclSuccess) return fail(c, PG_ERR_HIP, std::string("RCCL: ") + #expr + ": " + \
                                                              ncclGetErrorString(_r));              \
    } while (0)

static_assert(PG_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "pg_comm id size");

pg_status pg_comm_unique_id(void *id_out) {
    if (!id_out) return fail(nullptr, PG_ERR_INVALID, "pg_comm_unique_id: null argument");
    ncclUniqueId id;
    NCCLC(nullptr, ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return PG_OK;
}

pg_status pg_comm_init(void *ctx, const void *id) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !id) return fail(c, PG_ERR_INVALID, "pg_comm_init: null argument");
    if (c->comm) return fail(c, PG_ERR_STATE, "pg_comm_init: communicator already initialised");
    if (c->cfg.world_size < 1 || c->cfg.rank < 0 || c->cfg.rank >= c->cfg.world_size)
        return fail(c, PG_ERR_INVALID, "pg_comm_init: rank / world_size of the config are inconsistent");
    HIPC(c, hipSetDevice(c->cfg.device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    NCCLC(c, ncclCommInitRank(&c->comm, c->cfg.world_size, uid, c->cfg.rank));
    return PG_OK;
}

pg_status pg_comm_allreduce_tree_stats(void *ctx) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_comm_allreduce_tree_stats: null context");
    if (!c->comm) return fail(c, PG_ERR_STATE, "pg_comm_allreduce_tree_stats: no communicator (pg_comm_init)");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_comm_allreduce_tree_stats: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    // the reduced vector IS the pg_get_tree_stats vector (u64 quadrant sums, per-D-tree record counts,
    // fraction statistics), which the device keeps contiguous: summed over ranks in place -- the
    // multi-rank arithmetic the torch.distributed / gloo exchange tests check.  Integer sums: every
    // rank ends with identical statistics.
    uint64_t words = 0;
    pg_status st;
    if ((st = pg_get_tree_stats(ctx, nullptr, 0, 1, &words))) return st;
    if (words) NCCLC(c, ncclAllReduce(c->sdp.bsum, c->sdp.bsum, words, ncclUint64, ncclSum, c->comm, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_comm_reduce_film(void *ctx, int32_t root) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_comm_reduce_film: null context");
    if (!c->comm) return fail(c, PG_ERR_STATE, "pg_comm_reduce_film: no communicator (pg_comm_init)");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_comm_reduce_film: no scene");
    if (root < 0 || root >= c->cfg.world_size) return fail(c, PG_ERR_INVALID, "pg_comm_reduce_film: bad root");
    HIPC(c, hipSetDevice(c->cfg.device));
    const size_t nf = (size_t)c->g.width * c->g.height * 4;
    // disjoint tile shards: every pixel has one non-zero contributor, so the f32 sum is exact
    NCCLC(c, ncclGroupStart());
    NCCLC(c, ncclReduce(c->film.p, c->film.p, nf, ncclFloat32, ncclSum, root, c->comm, c->stream));
    NCCLC(c, ncclReduce(c->film_sq.p, c->film_sq.p, nf, ncclFloat32, ncclSum, root, c->comm, c->stream));
    if (c->aov_albedo.p) {
        NCCLC(c, ncclReduce(c->aov_albedo.p, c->aov_albedo.p, nf, ncclFloat32, ncclSum, root, c->comm, c->stream));
        NCCLC(c, ncclReduce(c->aov_normal.p, c->aov_normal.p, nf, ncclFloat32, ncclSum, root, c->comm, c->stream));
    }
    // the filtered sums overlap at tile borders; integer sums are exact in any order
    if (c->filtered) NCCLC(c, ncclReduce(c->film_acc.p, c->film_acc.p, nf, ncclInt64, ncclSum, root, c->comm, c->stream));
    NCCLC(c, ncclGroupEnd());
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_comm_allreduce_f64(void *ctx, double *values, uint64_t n) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!values && n)) return fail(c, PG_ERR_INVALID, "pg_comm_allreduce_f64: null argument");
    if (!c->comm) return fail(c, PG_ERR_STATE, "pg_comm_allreduce_f64: no communicator (pg_comm_init)");
    if (!n) return PG_OK;
    HIPC(c, hipSetDevice(c->cfg.device));
    DevBuf b;
    HIPC(c, b.alloc(n * 8));
    HIPC(c, hipMemcpyAsync(b.p, values, n * 8, hipMemcpyHostToDevice, c->stream));
    NCCLC(c, ncclAllReduce(b.p, b.p, n, ncclFloat64, ncclSum, c->comm, c->stream));
    HIPC(c, hipMemcpyAsync(values, b.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_comm_allgather_records(void *ctx, uint64_t *counts_out) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_comm_allgather_records: null context");
    if (!c->comm) return fail(c, PG_ERR_STATE, "pg_comm_allgather_records: no communicator (pg_comm_init)");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_comm_allgather_records: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    const int W = c->cfg.world_size;
    // 1. every rank's record count
    DevBuf cnt;
    HIPC(c, cnt.alloc((size_t)(W + 1) * 8));
    const uint64_t mine = c->rec_host_count;
    HIPC(c, hipMemcpyAsync(cnt.as<uint64_t>() + W, &mine, 8, hipMemcpyHostToDevice, c->stream));
    NCCLC(c, ncclAllGather(cnt.as<uint64_t>() + W, cnt.p, 1, ncclUint64, c->comm, c->stream));
    std::vector<uint64_t> counts(W);
    HIPC(c, hipMemcpyAsync(counts.data(), cnt.p, (size_t)W * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    const uint64_t maxn = *std::max_element(counts.begin(), counts.end());
    if (counts_out) std::copy(counts.begin(), counts.end(), counts_out);
    if (maxn == 0) return PG_OK;
    // 2. the records, all-gathered in slices of at most kGatherSlice records per rank: round k gathers
    //    every rank's records [k S, (k + 1) S) (the local record buffer, padded to whole slices, is the
    //    send buffer) into ext_records (W S records, allocated once and reused by every round and every
    //    iteration), and every rank's valid part of the round is splatted, in rank order, before the next
    //    round overwrites it (same stream).  A single padded all-gather would need W x the largest count:
    //    ~13.6 GB per rank, re-allocated each iteration, for C3's 16-spp pass at W = 8.  Integer sums:
    //    the tree does not depend on the splat order.
    uint64_t slice = 1ull << 22;  // 128 MiB of records per rank and round
    if (const char *e = std::getenv("PG_GATHER_SLICE")) slice = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));  // tests
    const uint64_t S = std::min<uint64_t>(maxn, slice), rounds = (maxn + S - 1) / S;
    pg_status st;
    if ((st = ensureRecords(c, rounds * S))) return st;
    HIPC(c, c->ext_records.alloc((size_t)W * S * sizeof(pg_record)));
    const SDDev sd = sdView(c);
    for (uint64_t k = 0; k < rounds; ++k) {
        NCCLC(c, ncclAllGather(c->records.as<pg_record>() + k * S, c->ext_records.p, S * sizeof(pg_record), ncclUint8,
                               c->comm, c->stream));
        for (int r = 0; r < W; ++r) {
            const uint64_t lo = k * S, n = counts[r] > lo ? std::min(S, counts[r] - lo) : 0;
            if (n) pg_launch_splat(c->stream, sd, c->ext_records.as<pg_record>() + (size_t)r * S, n);
        }
        HIPC(c, hipGetLastError());
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_get_sdtree(void *ctx, void *buf, uint64_t capacity, uint64_t *size) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !size) return fail(c, PG_ERR_INVALID, "pg_get_sdtree: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_get_sdtree: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    pg_status s;
    if ((s = downloadSd(c))) return s;
    std::vector<uint8_t> blob = c->sd.serialize();
    *size = blob.size();
    if (buf) {
        if (capacity < blob.size()) return fail(c, PG_ERR_INVALID, "pg_get_sdtree: buffer too small");
        std::memcpy(buf, blob.data(), blob.size());
    }
    return PG_OK;
}

pg_status pg_put_sdtree(void *ctx, const void *buf, uint64_t size) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !buf) return fail(c, PG_ERR_INVALID, "pg_put_sdtree: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_put_sdtree: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    pgh::SdTree t;
    if (!t.deserialize((const uint8_t *)buf, size)) return fail(c, PG_ERR_INVALID, "pg_put_sdtree: malformed blob");
    c->sd = std::move(t);
    if (pg_status s = resetBlockers(c)) return s;  // a tree from outside starts a new job: nothing learned carries over
    return uploadSd(c);
}

pg_status pg_sdtree_pdf(void *ctx, const float *pos, const float *dir, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !pos || !dir || !out) return fail(c, PG_ERR_INVALID, "pg_sdtree_pdf: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_sdtree_pdf: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    DevBuf a, b, o;
    HIPC(c, a.alloc(n * 12 + 16));
    HIPC(c, b.alloc(n * 12 + 16));
    HIPC(c, o.alloc(n * 4 + 16));
    HIPC(c, hipMemcpyAsync(a.p, pos, n * 12, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(b.p, dir, n * 12, hipMemcpyHostToDevice, c->stream));
    pg_launch_sd_pdf(c->stream, sdView(c), a.as<float>(), b.as<float>(), (uint32_t)n, o.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_sdtree_sample(void *ctx, const float *pos, const float *u, uint64_t n, float *dir_out, float *pdf_out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !pos || !u || !dir_out || !pdf_out) return fail(c, PG_ERR_INVALID, "pg_sdtree_sample: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_sdtree_sample: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    DevBuf a, b, d, p;
    HIPC(c, a.alloc(n * 12 + 16));
    HIPC(c, b.alloc(n * 8 + 16));
    HIPC(c, d.alloc(n * 12 + 16));
    HIPC(c, p.alloc(n * 4 + 16));
    HIPC(c, hipMemcpyAsync(a.p, pos, n * 12, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(b.p, u, n * 8, hipMemcpyHostToDevice, c->stream));
    pg_launch_sd_sample(c->stream, sdView(c), a.as<float>(), b.as<float>(), (uint32_t)n, d.as<float>(), p.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(dir_out, d.p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(pdf_out, p.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_read_film(void *ctx, float *rgbw, float *sumsq) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_read_film: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_read_film: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    size_t fb = (size_t)c->g.width * c->g.height * 16;
    if (rgbw) HIPC(c, hipMemcpyAsync(rgbw, c->film.p, fb, hipMemcpyDeviceToHost, c->stream));
    if (sumsq) HIPC(c, hipMemcpyAsync(sumsq, c->film_sq.p, fb, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_reset_film(void *ctx) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_reset_film: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_reset_film: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    size_t fb = (size_t)c->g.width * c->g.height * 16;
    HIPC(c, hipMemsetAsync(c->film.p, 0, fb, c->stream));
    HIPC(c, hipMemsetAsync(c->film_sq.p, 0, fb, c->stream));
    if (c->aov_albedo.p) {
        HIPC(c, hipMemsetAsync(c->aov_albedo.p, 0, fb, c->stream));
        HIPC(c, hipMemsetAsync(c->aov_normal.p, 0, fb, c->stream));
    }
    if (c->filtered) HIPC(c, hipMemsetAsync(c->film_acc.p, 0, fb * 2, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_read_aovs(void *ctx, float *albedo, float *normal) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_read_aovs: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_read_aovs: no scene");
    if (!c->cfg.aovs) return fail(c, PG_ERR_STATE, "pg_read_aovs: the context was created with aovs = 0");
    HIPC(c, hipSetDevice(c->cfg.device));
    size_t fb = (size_t)c->g.width * c->g.height * 16;
    if (albedo) HIPC(c, hipMemcpyAsync(albedo, c->aov_albedo.p, fb, hipMemcpyDeviceToHost, c->stream));
    if (normal) HIPC(c, hipMemcpyAsync(normal, c->aov_normal.p, fb, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

// ---- denoiser (pg_capi.h "denoiser"; kernels in pg_denoise.hip) ----------------------------------------------------
pg_status pg_denoise_default_params(pg_denoise_params *params) {
    if (!params) return fail(nullptr, PG_ERR_INVALID, "pg_denoise_default_params: null argument");
    params->levels = 5;
    params->sigma_l = 4.0f;
    params->sigma_n = 0.1f;
    params->sigma_a = 0.1f;
    return PG_OK;
}

static pg_status denoiseParams(Ctx *c, const pg_denoise_params *in, pg_denoise_params *p) {
    if (in) *p = *in;
    else (void)pg_denoise_default_params(p);
    if (p->levels < 1 || p->levels > 6) return fail(c, PG_ERR_INVALID, "pg_denoise: levels must be 1..6");
    for (float s : {p->sigma_l, p->sigma_n, p->sigma_a})
        if (!(s > 0) || !std::isfinite(s)) return fail(c, PG_ERR_INVALID, "pg_denoise: the sigmas must be finite and > 0");
    return PG_OK;
}

// prepare + the levels on c->stream over device rows; scratch: 4 x width x height float4.  The result is left in
// one of the first two scratch rows and copied to `out` (host).
static pg_status denoiseRun(Ctx *c, const pg_denoise_params &p, uint32_t W, uint32_t H, const float4 *rgbw,
                            const float4 *sumsq, const float4 *albedo, const float4 *normal, float4 *scratch, float *out) {
    const size_t npix = (size_t)W * H;
    if (!c->dn_ev.a) {
        HIPC(c, hipEventCreate(&c->dn_ev.a));
        HIPC(c, hipEventCreate(&c->dn_ev.b));
    }
    // steps 1 and 2 from an LDS tile: 0.51 against 0.61 ms for the five levels of a 1280 x 720 film, same bits
    // (profiles/r22_denoise); PG_DENOISE_TILED=0 gathers every level from memory, for A/B
    const char *e = std::getenv("PG_DENOISE_TILED");
    const bool tiled = !(e && std::atoi(e) == 0);
    float4 *ev[2] = {scratch, scratch + npix}, *fn = scratch + 2 * npix, *fa = scratch + 3 * npix;
    HIPC(c, hipEventRecord(c->dn_ev.a, c->stream));
    pg_launch_denoise_prepare(c->stream, W, H, rgbw, sumsq, albedo, normal, ev[0], fn, fa);
    for (int i = 0; i < p.levels; ++i)
        pg_launch_denoise_level(c->stream, W, H, 1 << i, p.sigma_l, p.sigma_n, p.sigma_a, i == p.levels - 1, ev[i & 1], fn,
                                fa, ev[(i + 1) & 1], tiled);
    HIPC(c, hipGetLastError());
    HIPC(c, hipEventRecord(c->dn_ev.b, c->stream));
    HIPC(c, hipMemcpyAsync(out, ev[p.levels & 1], npix * 16, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->dn_timed = true;
    return PG_OK;
}

pg_status pg_denoise(void *ctx, const pg_denoise_params *params, float *out_rgbv) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_denoise: null context");
    if (!out_rgbv) return fail(c, PG_ERR_INVALID, "pg_denoise: null output");
    pg_denoise_params p;
    if (pg_status s = denoiseParams(c, params, &p)) return s;
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_denoise: no scene");
    if (!c->cfg.aovs) return fail(c, PG_ERR_STATE, "pg_denoise: the context was created with aovs = 0");
    HIPC(c, hipSetDevice(c->cfg.device));
    HIPC(c, c->dn_scratch.alloc((size_t)c->g.width * c->g.height * 64));
    return denoiseRun(c, p, c->g.width, c->g.height, c->film.as<float4>(), c->film_sq.as<float4>(),
                      c->aov_albedo.as<float4>(), c->aov_normal.as<float4>(), c->dn_scratch.as<float4>(), out_rgbv);
}

pg_status pg_denoise_arrays(void *ctx, const pg_denoise_params *params, uint32_t width, uint32_t height,
                            const float *rgbw, const float *sumsq, const float *albedo, const float *normal,
                            float *out_rgbv) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_denoise_arrays: null context");
    if (!rgbw || !sumsq || !albedo || !normal || !out_rgbv) return fail(c, PG_ERR_INVALID, "pg_denoise_arrays: null array");
    if (!width || !height || width > 65536u || height > 65536u || (uint64_t)width * height > ((uint64_t)1 << 28))
        return fail(c, PG_ERR_INVALID, "pg_denoise_arrays: need 1 <= width, height <= 65536 and at most 2^28 pixels");
    pg_denoise_params p;
    if (pg_status s = denoiseParams(c, params, &p)) return s;
    HIPC(c, hipSetDevice(c->cfg.device));
    const size_t npix = (size_t)width * height, row = npix * 16;
    DevBuf in, scratch;  // freed on return: the sizes are the caller's, not the scene's
    HIPC(c, in.alloc(4 * row));
    HIPC(c, scratch.alloc(4 * row));
    const float *host[4] = {rgbw, sumsq, albedo, normal};
    for (int k = 0; k < 4; ++k)
        HIPC(c, hipMemcpyAsync(in.as<float4>() + k * npix, host[k], row, hipMemcpyHostToDevice, c->stream));
    const float4 *d = in.as<float4>();
    return denoiseRun(c, p, width, height, d, d + npix, d + 2 * npix, d + 3 * npix, scratch.as<float4>(), out_rgbv);
}

pg_status pg_denoise_time(void *ctx, float *ms_out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !ms_out) return fail(c, PG_ERR_INVALID, "pg_denoise_time: null argument");
    if (!c->dn_timed) return fail(c, PG_ERR_STATE, "pg_denoise_time: no pg_denoise call yet");
    HIPC(c, hipSetDevice(c->cfg.device));
    HIPC(c, hipEventElapsedTime(ms_out, c->dn_ev.a, c->dn_ev.b));
    return PG_OK;
}

pg_status pg_envmap_query(void *ctx, int32_t op, const float *in, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!in && n) || (!out && n)) return fail(c, PG_ERR_INVALID, "pg_envmap_query: null argument");
    if (op < 0 || op > 2) return fail(c, PG_ERR_INVALID, "pg_envmap_query: bad op");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_envmap_query: no scene");
    if (!c->has_env) return fail(c, PG_ERR_STATE, "pg_envmap_query: the scene has no environment emitter");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    const size_t inBytes = n * (op == 0 ? 8 : 12), outBytes = n * (op == 0 ? 32 : op == 1 ? 4 : 12);
    DevBuf a, o;
    HIPC(c, a.alloc(inBytes));
    HIPC(c, o.alloc(outBytes));
    HIPC(c, hipMemcpyAsync(a.p, in, inBytes, hipMemcpyHostToDevice, c->stream));
    pg_launch_envmap_query(c->stream, sceneView(c), op, a.as<float>(), (uint32_t)n, o.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, outBytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_get_stats(void *ctx, pg_stats *st) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !st) return fail(c, PG_ERR_INVALID, "pg_get_stats: null argument");
    *st = c->stats;
    return PG_OK;
}

pg_status pg_get_probes(void *ctx, uint64_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !count) return fail(c, PG_ERR_INVALID, "pg_get_probes: null argument");
    *count = c->probes;
    return PG_OK;
}
pg_status pg_get_culled(void *ctx, uint64_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !count) return fail(c, PG_ERR_INVALID, "pg_get_culled: null argument");
    *count = c->culled;
    return PG_OK;
}

pg_status pg_get_shadow_culled(void *ctx, uint64_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !count) return fail(c, PG_ERR_INVALID, "pg_get_shadow_culled: null argument");
    *count = c->shadow_culled;
    return PG_OK;
}
pg_status pg_get_probes_resolved(void *ctx, uint64_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !count) return fail(c, PG_ERR_INVALID, "pg_get_probes_resolved: null argument");
    *count = c->probes_resolved;
    return PG_OK;
}
pg_status pg_get_occluders(void *ctx, uint32_t *tri_ids, uint32_t *orig_ids, uint32_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !tri_ids || !count) return fail(c, PG_ERR_INVALID, "pg_get_occluders: null argument");
    *count = c->num_occluders;
    for (uint32_t i = 0; i < c->num_occluders; ++i) {
        tri_ids[i] = c->prb_ids[i];
        if (orig_ids) orig_ids[i] = c->prb_orig[i];
    }
    return PG_OK;
}
pg_status pg_get_blockers(void *ctx, uint32_t *tri_ids, uint32_t *orig_ids, uint32_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !tri_ids || !count) return fail(c, PG_ERR_INVALID, "pg_get_blockers: null argument");
    *count = c->num_blockers;
    for (uint32_t i = 0; i < c->num_blockers; ++i) {
        tri_ids[i] = c->blk_ids[i];
        if (orig_ids) orig_ids[i] = c->blk_orig[i];
    }
    return PG_OK;
}

pg_status pg_local_pixel_count(void *ctx, uint64_t *count) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !count) return fail(c, PG_ERR_INVALID, "pg_local_pixel_count: null argument");
    *count = c->local_pixels.size();
    return PG_OK;
}

pg_status pg_trace_rays(void *ctx, const float *rays, uint64_t n, int32_t any_hit, float *hits) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!rays && n) || (!hits && n)) return fail(c, PG_ERR_INVALID, "pg_trace_rays: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_trace_rays: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf r, h, ovf;
    HIPC(c, r.alloc(n * 32));
    HIPC(c, h.alloc(n * 16));
    HIPC(c, ovf.alloc(pg_stack_overflow_words(pg_trace_rays_threads(n)) * 4));
    HIPC(c, hipMemcpyAsync(r.p, rays, n * 32, hipMemcpyHostToDevice, c->stream));
    pg_launch_trace_rays(c->stream, sceneView(c), r.as<float>(), (uint32_t)n, any_hit ? 1 : 0, h.as<float>(),
                         ovf.as<uint32_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(hits, h.p, n * 16, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_blocker_test(void *ctx, const float *rays, uint64_t n, const uint32_t *tri_ids, uint32_t k, uint32_t *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!rays && n) || (!out && n) || (!tri_ids && k)) return fail(c, PG_ERR_INVALID, "pg_blocker_test: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_blocker_test: no scene");
    if (k > PG_MAX_BLOCKERS) return fail(c, PG_ERR_INVALID, "pg_blocker_test: more than PG_MAX_BLOCKERS triangles");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    SceneDev sc = sceneView(c);
    uint32_t ids[PG_MAX_BLOCKERS];
    if (pg_status s = installBlockers(c, tri_ids, k, sc.blk, ids, nullptr, &sc.num_blockers)) return s;
    DevBuf r, o;
    HIPC(c, r.alloc(n * 32));
    HIPC(c, o.alloc(n * 4));
    HIPC(c, hipMemcpyAsync(r.p, rays, n * 32, hipMemcpyHostToDevice, c->stream));
    pg_launch_blocker_test(c->stream, sc, r.as<float>(), (uint32_t)n, o.as<uint32_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_occluder_test(void *ctx, const float *rays, uint64_t n, const uint32_t *tri_ids, uint32_t k, uint32_t *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!rays && n) || (!out && n) || (!tri_ids && k)) return fail(c, PG_ERR_INVALID, "pg_occluder_test: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_occluder_test: no scene");
    if (k > PG_PROBE_LIST_MAX) return fail(c, PG_ERR_INVALID, "pg_occluder_test: more than PG_PROBE_LIST_MAX triangles");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    SceneDev sc = sceneView(c);
    uint32_t ids[PG_PROBE_LIST_MAX];
    if (pg_status s = installBlockers(c, tri_ids, k, sc.prb, ids, nullptr, &sc.num_occluders, PG_PROBE_LIST_MAX)) return s;
    DevBuf r, o, ovf;
    HIPC(c, r.alloc(n * 32));
    HIPC(c, o.alloc(n * 8));
    HIPC(c, ovf.alloc(pg_stack_overflow_words(pg_trace_rays_threads(n)) * 4));
    HIPC(c, hipMemcpyAsync(r.p, rays, n * 32, hipMemcpyHostToDevice, c->stream));
    pg_launch_occluder_test(c->stream, sc, r.as<float>(), (uint32_t)n, o.as<uint32_t>(), ovf.as<uint32_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_hit_records(void *ctx, const float *rays, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!rays && n) || (!out && n)) return fail(c, PG_ERR_INVALID, "pg_hit_records: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_hit_records: no scene");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf r, h, ovf;
    HIPC(c, r.alloc(n * 32));
    HIPC(c, h.alloc(n * 64));
    HIPC(c, ovf.alloc(pg_stack_overflow_words(pg_trace_rays_threads(n)) * 4));
    HIPC(c, hipMemcpyAsync(r.p, rays, n * 32, hipMemcpyHostToDevice, c->stream));
    pg_launch_trace_rays(c->stream, sceneView(c), r.as<float>(), (uint32_t)n, 2, h.as<float>(), ovf.as<uint32_t>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, h.p, n * 64, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_bsdf_query(void *ctx, uint32_t material, const float *wi, const float *u, const float *wo_given, uint64_t n,
                        float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!wi && n) || (!u && n) || (!out && n)) return fail(c, PG_ERR_INVALID, "pg_bsdf_query: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_bsdf_query: no scene");
    if (material >= c->num_mats) return fail(c, PG_ERR_INVALID, "pg_bsdf_query: bad material");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf a, b, g, o;
    HIPC(c, a.alloc(n * 12));
    HIPC(c, b.alloc(n * 12));
    HIPC(c, o.alloc(n * 48));
    HIPC(c, hipMemcpyAsync(a.p, wi, n * 12, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(b.p, u, n * 12, hipMemcpyHostToDevice, c->stream));
    if (wo_given) {
        HIPC(c, g.alloc(n * 12));
        HIPC(c, hipMemcpyAsync(g.p, wo_given, n * 12, hipMemcpyHostToDevice, c->stream));
    }
    pg_launch_bsdf_query(c->stream, c->mats.as<GMat>() + material, a.as<float>(), b.as<float>(),
                         wo_given ? g.as<float>() : nullptr, (uint32_t)n, o.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 48, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_phase_query(void *ctx, uint32_t medium, const float *in, const float *wo_given, uint64_t n, float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!in && n) || (!out && n)) return fail(c, PG_ERR_INVALID, "pg_phase_query: null argument");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_phase_query: no scene");
    if (medium >= c->num_media) return fail(c, PG_ERR_INVALID, "pg_phase_query: bad medium");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    DevBuf a, g, o;
    HIPC(c, a.alloc(n * 20));
    HIPC(c, o.alloc(n * 20));
    HIPC(c, hipMemcpyAsync(a.p, in, n * 20, hipMemcpyHostToDevice, c->stream));
    if (wo_given) {
        HIPC(c, g.alloc(n * 12));
        HIPC(c, hipMemcpyAsync(g.p, wo_given, n * 12, hipMemcpyHostToDevice, c->stream));
    }
    pg_launch_phase_query(c->stream, c->media.as<GMedium>() + medium, a.as<float>(), wo_given ? g.as<float>() : nullptr,
                          (uint32_t)n, o.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, n * 20, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_medium_query(void *ctx, uint32_t medium, int32_t op, const float *in, const uint32_t *keys, uint64_t n,
                          float *out) {
    Ctx *c = (Ctx *)ctx;
    if (!c || (!in && n) || (!out && n) || (op != 0 && !keys && n))
        return fail(c, PG_ERR_INVALID, "pg_medium_query: null argument");
    if (op < 0 || op > 4) return fail(c, PG_ERR_INVALID, "pg_medium_query: bad op");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_medium_query: no scene");
    if (medium >= c->num_media) return fail(c, PG_ERR_INVALID, "pg_medium_query: bad medium");
    if (c->is_homog[medium])
        return fail(c, PG_ERR_INVALID, "pg_medium_query: a homogeneous medium has no grid (pg_homogeneous_query)");
    HIPC(c, hipSetDevice(c->cfg.device));
    if (!n) return PG_OK;
    const size_t inBytes = n * (op == 0 ? 12 : 32), outBytes = n * (op == 0 ? 4 : 16);
    DevBuf a, k, o;
    HIPC(c, a.alloc(inBytes));
    HIPC(c, o.alloc(outBytes));
    HIPC(c, hipMemcpyAsync(a.p, in, inBytes, hipMemcpyHostToDevice, c->stream));
    if (op != 0) {
        HIPC(c, k.alloc(n * 8));
        HIPC(c, hipMemcpyAsync(k.p, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    }
    pg_launch_medium_query(c->stream, c->media.as<GMedium>() + medium, op, a.as<float>(),
                           op != 0 ? k.as<uint32_t>() : nullptr, (uint32_t)n, o.as<float>());
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(out, o.p, outBytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return PG_OK;
}

}  // extern "C"
