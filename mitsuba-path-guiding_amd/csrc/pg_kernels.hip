// gfx950 kernels of the guided path-tracing wavefront (DESIGN.md §"Kernels").
//
// One bounce of the reference's ProgressiveMIPathTracer::Li (progressive_path.cpp:133-314) is
// split into:  trace (closest hit over the live-path queue) -> shade (emission/MIS of the previous
// segment, Russian roulette, NEE sampling, BSDF / SD-tree one-sample-MIS direction sampling,
// training-vertex write, queue compaction by wave ballot) -> shadow (any hit; adds the NEE
// contribution).  Camera rays, film accumulation, record commit and SD-tree splat are separate
// kernels.  Path state is SoA float4/uint4 arrays indexed by path slot.
#include <algorithm>
#include <cstdlib>

#include "pg_trace.h"

// LDS staging of material tiles (measured, off by default: profiles/r02k_lds_ab/ -- C3
// within noise to -1 %: the few materials already hit in L1, and the block
// fill + barrier is paid by every short-lived shading block)
#ifndef SHADE_LDS_MATS
#define SHADE_LDS_MATS 0   // > 0: k_shade stages up to this many materials in LDS (64 = 8 KiB)
#endif

// =============================================================================================
// camera rays (cameraRay, pg_device.h) for (pixel, sample) slots.  LENS: a thin lens is set (pg_set_lens); the
// pinhole launches k_camera<false>, the kernel as it was
template <bool LENS>
__global__ __launch_bounds__(256) void k_camera(GParams g, PathDev p, const uint32_t *__restrict__ local_pixels,
                                                uint32_t pix_begin, uint32_t npix, uint32_t nlayers,
                                                uint32_t sample_base, Queue q, bool banded) {
    uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = npix * nlayers;
    if (slot < PG_QSHARDS) q.counts[slot] = pg_camera_count(banded, npix, nlayers, slot);
    if (slot >= n) return;
    uint32_t layer = slot / npix, lp = slot - layer * npix;
    uint32_t pix = local_pixels[pix_begin + lp];
    uint32_t sample = sample_base + layer;
    f3 o, wd;
    float tmin, tmax;
    cameraRay<LENS>(g, pix, rngKey(pix, g.seed), sample, o, wd, tmin, tmax);
    stS(pathRayO(p, slot), f4(o, tmin));
    stS(pathRayD(p, slot), f4(wd, tmax));
    // throughput (1, eta 1) is implied by depth 1: the first bounce's readers (shadeOne, envEscapeRadiance) do not
    // load it.  ray_d.w is the far clip along the ray; a bounce ray keeps woPdf there (pg_layout.h "Path state").
    // L = 0 is stored: a camera ray that escapes is
    // never shaded and k_film reads its L.
    stS(&p.rad[slot], make_float4(0.f, 0.f, 0.f, 0.f));
    stS(pathInfo(p, slot), make_uint4(pix, sample, 1u | (PF_EMITTED_QUERY << 16), 0u));
    if (banded) {  // pg_kernels.h pg_banded_shard_count: band r of the local pixels -> shards r, r + 8, ...
        const uint32_t r = (uint32_t)(((uint64_t)lp * 8u) / npix);
        const uint32_t b0 = pg_band_start(r, npix), m = pg_band_start(r + 1, npix) - b0;
        const uint32_t k = layer * m + (lp - b0);
        q.items[(r + 8u * ((k >> 6) & 7u)) * q.stride + (((k >> 9) << 6) | (k & 63u))] = slot;
    } else {  // pg_kernels.h pg_camera_slot: the fused first launch (cameraRows) computes this entry instead
        q.items[pg_camera_shard(slot) * q.stride + pg_camera_entry(slot)] = slot;
    }
}
// the interleaved camera queue alone: what k_camera stores in q, for the one reader the fused first launch leaves it
// (k_tail, when it takes a chunk over straight after the camera rays' hits)
__global__ __launch_bounds__(256) void k_camera_queue(uint32_t n, Queue q) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot < PG_QSHARDS) q.counts[slot] = pg_camera_shard_count(n, slot);
    if (slot < n) q.items[pg_camera_shard(slot) * q.stride + pg_camera_entry(slot)] = slot;
}

// BSDF::getAlbedo of the config BSDFs (diffuse.cpp:112, conductor.cpp:225, roughconductor.cpp:264,
// dielectric.cpp:230, roughdielectric.cpp:272, plastic.cpp:266, roughplastic.cpp:354; null: the
// BSDF default 0, bsdf.h:361).  twosided picks the nested BSDF by side, which is the same BSDF here.
__device__ __forceinline__ f3 bsdfAlbedo(const GMat &M) {
    const f3 diff = mk(M.diff[0], M.diff[1], M.diff[2]), spec = mk(M.spec[0], M.spec[1], M.spec[2]);
    const f3 trans = mk(M.trans[0], M.trans[1], M.trans[2]);
    switch (M.model) {
        case PG_BSDF_DIFFUSE: return diff;
        case PG_BSDF_CONDUCTOR:
        case PG_BSDF_ROUGHCONDUCTOR: return spec;
        case PG_BSDF_DIELECTRIC: return trans * 0.5f + spec * (1 - 0.5f);
        case PG_BSDF_ROUGHDIELECTRIC: return spec * 0.5f + trans * (1 - 0.5f);
        case PG_BSDF_PLASTIC: return diff * 0.5f + spec * (1 - 0.5f);
        case PG_BSDF_ROUGHPLASTIC: return spec * 0.5f + diff * (1 - 0.5f);
        default: return mk1(0.f);
    }
}

// A path whose extension ray escaped (progressive_path.cpp:150-158 for the camera ray, :252-267 +
// :276-284 after a bounce): the environment emitter's radiance, MIS-weighted against its NEE pdf.
// radiance an escaped path picks up from the environment emitter.  k_trace stores it in the path's
// hit record (t, u, v of a miss; the escape ends the path), and k_film / k_commit add it to L
// (envHitRadiance): the sum (L + NEE of the last vertex) + environment keeps its order while the
// last vertex's shadow ray may run in the same launch (k_rays)
// word: the escaped ray's depth | flags << 16 (pinfo.z; kCameraWord for a camera ray), woPdf: a bounce ray's ray_d.w
constexpr uint32_t kCameraWord = 1u | (PF_EMITTED_QUERY << 16);  // what k_camera writes to pinfo.z
__device__ __forceinline__ f3 envEscapeRadiance(const GParams &g, const SceneDev &sc, const PathDev &p, uint32_t slot,
                                                f3 rd, uint32_t word, float woPdf) {
    const uint32_t depth = word & 0xFFFFu, flags = word >> 16;
    f3 add;
    if (depth == 1) {  // camera ray (throughput 1): the loop-top miss with EEmittedRadiance
        if (!(flags & PF_EMITTED_QUERY) || (g.hide_emitters && !(flags & PF_SCATTERED))) return mk1(0.f);
        add = envEval(*sc.env, rd);
    } else {
        const float4 T4 = ldS(pathThr(p, slot));
        if (g.hide_emitters && !(flags & PF_SCATTERED)) return mk1(0.f);
        float w = 1.0f;
        if (g.use_nee) {
            const float lumPdf = (flags & PF_PREV_DELTA) ? 0.0f : envPdf(*sc.env, rd) * (1.0f / (float)g.num_emitters);
            w = miWeight(woPdf, lumPdf);
        }
        add = xyz(T4) * envEval(*sc.env, rd) * w;
    }
    return add;
}
// L of a finished path plus the environment radiance its escape left in the hit record
__device__ __forceinline__ float4 envHitRadiance(float4 L, float4 hv) {
    if (__float_as_uint(hv.y) == 0xFFFFFFFFu) {
        L.x += hv.x;
        L.y += hv.z;
        L.z += hv.w;
    }
    return L;
}


// A bounce ray's rows (pg_layout.h "Path state"): o = (p, +-tmin), d = (wo, woPdf); its tmax is +inf.
// PF_DOOMED on the ray: shadeOne stores a doomed extension ray's tmin negated
__device__ __forceinline__ bool rayDoomed(float4 o) { return (__float_as_uint(o.w) >> 31) != 0; }
static_assert(PG_RAY_EPSILON == kEpsilon, "pg_ray_tmin uses the ray epsilon");
// class-queue row of a traced ray: the hit triangle's material class, PG_CLASS_ESCAPED for a miss, or
// PG_CLASS_CULLED for a doomed ray that hit a non-emitter -- its vertex would do nothing, so the path ends
// here and its hit record becomes a miss without environment radiance (k_film / k_commit add exact zeros)
__device__ __forceinline__ int hitClass(const SceneDev &sc, bool h, uint32_t tri, bool doomed, float4 &hr) {
    if (!h) return PG_CLASS_ESCAPED;
    const uint32_t tc = sc.tclass[tri];
    if (doomed && !(tc & PG_TCLASS_EMITTER)) {
        hr = make_float4(0.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f);
        return PG_CLASS_CULLED;
    }
    return (int)(tc & PG_TCLASS_MASK);
}

// closest hit for every queued path: hit[slot] = (t, BVH-order triangle | ~0, u, v).
// Grid-stride over the queue shard blockIdx % PG_QSHARDS.  (A persistent variant with dynamic
// ray fetch into finished lanes measured slower once traversal was made while-while.)
struct ClassQueues {
    Queue q[PG_CLASS_ROWS];
};

// wave-aggregated append of `slot` to class queue `cls` (< 0: none), shard s: one atomic per class
// present in the wave; the rows from PG_NUM_CLASSES on (escaped rays, culled hits) are counted only
__device__ __forceinline__ void classAppend(int cls, uint32_t slot, const ClassQueues &cqs, uint32_t s) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(cls >= 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int c = __shfl(cls, leader);
        const unsigned long long mine = __ballot(cls == c);
        const Queue &cq = cqs.q[c];
        uint32_t b = 0;
        if (lane == leader) b = atomicAdd(cq.counts + s, (uint32_t)__popcll(mine));
        b = __shfl(b, leader);
        if (cls == c && c < PG_NUM_CLASSES)
            cq.items[(size_t)s * cq.stride + b + __popcll(mine & ((1ull << lane) - 1ull))] = slot;
        pending &= ~mine;
    }
}

// closest hits of the rows of queue shard bid % PG_QSHARDS that block bid of nblk takes (a
// grid-stride loop: k_trace, or the trace blocks of k_rays).
// ENV: the scene has an environment emitter (escaped paths pick up its radiance)
// CAM: the rows are camera rays (the chunk's first launch), whose tmin / tmax are in the rows; bounce rays otherwise
// first: the camera rays' bounce with denoiser features on (pg_config.aovs): the hit record of every
// path also goes to p.aov, which k_film resolves into albedo and normal (nullptr: off)
template <bool ENV, bool CAM>
__device__ __forceinline__ void traceRows(const GParams &g, const SceneDev &sc, const PathDev &p, const Queue &q,
                                          const ClassQueues &cqs, float4 *first, uint32_t bid, uint32_t nblk,
                                          const TStack &stk) {
    const uint32_t s = bid & (PG_QSHARDS - 1);
    const uint32_t n = q.counts[s];
    const uint32_t *items = q.items + (size_t)s * q.stride;
    // block-uniform loop bound, so whole waves reach the class ballots together
    for (uint32_t base = (bid / PG_QSHARDS) * TRACE_BLOCK; base < n; base += nblk / PG_QSHARDS * TRACE_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        int cls = -1;
        uint32_t slot = 0;
        if (i < n) {
            slot = items[i];
            float4 o = ldS(pathRayO(p, slot)), d = ldS(pathRayD(p, slot));
            // the doomed bit rides through the walk in the slot's top bit (slots are < 2^31): no register of its own
            // under k_rays' 64-VGPR cap
            slot |= rayDoomed(o) ? 0x80000000u : 0u;
            const float tmin = fabsf(o.w);
            float tmax = CAM ? d.w : __builtin_huge_valf();
            uint32_t tri = 0xFFFFFFFFu;
            float u = 0, v = 0;
            const bool h = traverse<false>(sc.nodes, sc.tris, xyz(o), xyz(d), tmin, tmax, tri, u, v, stk);
            const bool doomed = (slot >> 31) != 0;
            slot &= 0x7FFFFFFFu;
            float4 hr = make_float4(h ? tmax : 0.0f, __uint_as_float(h ? tri : 0xFFFFFFFFu), u, v);
            if (first) first[slot] = hr;
            if (ENV && !h) {
                const f3 e = envEscapeRadiance(g, sc, p, slot, xyz(d), CAM ? kCameraWord : pathInfo(p, slot)->z, d.w);
                hr = make_float4(e.x, hr.y, e.y, e.z);
            }
            cls = hitClass(sc, h, tri, doomed, hr);
            stS(&p.hit[slot], hr);
        }
        classAppend(cls, slot, cqs, s);
    }
}

template <bool ENV, bool CAM>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace(GParams g, SceneDev sc, PathDev p, Queue q, ClassQueues cqs,
                                                       float4 *first) {
    __shared__ uint32_t stack[LDS_STACK * TRACE_BLOCK];
    traceRows<ENV, CAM>(g, sc, p, q, cqs, first, blockIdx.x, gridDim.x, threadStack(stack, p.stack_ovf));
}

// A chunk's camera rays, generated where they are traced (the chunk's first launch; k_camera + k_trace<ENV, true> in one,
// DESIGN.md section 5 "Camera fusion").  The rows are those of the interleaved camera queue, which is never stored: entry
// i of shard s is slot pg_camera_slot(s, i) and the shard holds pg_camera_shard_count entries, so blocks, waves and
// lanes take the slots they took when the queue was read back.  Of k_camera's rows ray_d, pinfo and rad = 0 are stored
// (pg_layout.h "Path state"); ray_o, the near clip and the queue entry have no reader after this launch.
struct CameraChunk {
    const uint32_t *local_pixels;
    uint32_t pix_begin, npix, nlayers, sample_base;
};
template <bool ENV, bool LENS>
__device__ __forceinline__ void cameraRows(const GParams &g, const SceneDev &sc, const PathDev &p, const CameraChunk &cam,
                                           const ClassQueues &cqs, float4 *first, uint32_t bid, uint32_t nblk,
                                           const TStack &stk) {
    const uint32_t s = bid & (PG_QSHARDS - 1);
    const uint32_t n = pg_camera_shard_count(cam.npix * cam.nlayers, s);
    // block-uniform loop bound, as traceRows'
    for (uint32_t base = (bid / PG_QSHARDS) * TRACE_BLOCK; base < n; base += nblk / PG_QSHARDS * TRACE_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        int cls = -1;
        uint32_t slot = 0;
        if (i < n) {
            slot = pg_camera_slot(s, i);
            f3 o, wd;
            float tmin, tmax;
            {  // k_camera's rows
                const uint32_t layer = slot / cam.npix, lp = slot - layer * cam.npix;
                const uint32_t pix = cam.local_pixels[cam.pix_begin + lp];
                const uint32_t sample = cam.sample_base + layer;
                cameraRay<LENS>(g, pix, rngKey(pix, g.seed), sample, o, wd, tmin, tmax);
                stS(pathRayD(p, slot), f4(wd, tmax));
                stS(&p.rad[slot], make_float4(0.f, 0.f, 0.f, 0.f));
                stS(pathInfo(p, slot), make_uint4(pix, sample, kCameraWord, 0u));
            }
            const float far = tmax;
            uint32_t tri = 0xFFFFFFFFu;
            float u = 0, v = 0;
            const bool h = traverse<false>(sc.nodes, sc.tris, o, wd, tmin, tmax, tri, u, v, stk);
            float4 hr = make_float4(h ? tmax : 0.0f, __uint_as_float(h ? tri : 0xFFFFFFFFu), u, v);
            if (first) first[slot] = hr;
            if (ENV && !h) {
                const f3 e = envEscapeRadiance(g, sc, p, slot, wd, kCameraWord, far);
                hr = make_float4(e.x, hr.y, e.y, e.z);
            }
            cls = hitClass(sc, h, tri, false, hr);
            stS(&p.hit[slot], hr);
        }
        classAppend(cls, slot, cqs, s);
    }
}
template <bool ENV, bool LENS>
__global__ __launch_bounds__(TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(LENS ? 4 : ENV ? 5 : 6))) void k_camera_trace(GParams g, SceneDev sc, PathDev p, CameraChunk cam,
                                                              ClassQueues cqs, float4 *first) {
    __shared__ uint32_t stack[LDS_STACK * TRACE_BLOCK];
    cameraRows<ENV, LENS>(g, sc, p, cam, cqs, first, blockIdx.x, gridDim.x, threadStack(stack, p.stack_ovf));
}

// shadow-ray mint at the shading point o (the extension ray's origin): Epsilon * max |o_i|
// (progressive_path.cpp via DirectSamplingRecord / Scene::sampleEmitterDirect's shadow ray)
__device__ __forceinline__ float shadowTmin(float4 o) {
    return kEpsilon * fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
}

template <class T>
__device__ __forceinline__ void waveKeyedAdd(T *base, uint32_t key, T v, bool valid);
// the rows (a block's share of a queue shard) whose shadow rays the recording passes count (pg_layout.h PG_BLOCKER_SAMPLE)
__device__ __forceinline__ bool blockerRowCounted(uint32_t row) { return row % PG_BLOCKER_SAMPLE == 0; }
// any hit for queued shadow rays; unoccluded -> add the NEE contribution to L (and to the
// training vertex's radiance snapshot, so its record excludes light arriving from elsewhere)
// COUNT (recording passes without an environment emitter, pg_layout.h "Shadow blockers"): every occluded ray adds one
// to sc.blk_counts[the triangle the walk accepted], wave-aggregated by triangle (a few triangles take nearly all the
// counts).  An instantiation of its own, so the final render's kernels carry none of it.
// an unoccluded shadow ray's contribution (sh_c) to its path's L and to its training vertex's snapshot
__device__ __forceinline__ void shadowAdd(const PathDev &p, uint32_t slot) {
    float4 c = ldS(&p.sh_c[slot]);
    float4 L = ldS(&p.rad[slot]);
    stS(&p.rad[slot], make_float4(L.x + c.x, L.y + c.y, L.z + c.z, L.w));
    uint32_t vi = __float_as_uint(c.w);
    if (vi != 0xFFFFFFFFu) {
        float4 *vl = p.vtx + ((size_t)vi * p.vtxP + slot) * PG_VTX_F4 + 2;
        float4 a = *vl;
        *vl = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w);
    }
}
template <bool COUNT>
__device__ __forceinline__ void shadowRows(const SceneDev &sc, const PathDev &p, const Queue &q, uint32_t bid,
                                           uint32_t nblk, const WStack &stk) {
    const uint32_t s = bid & (PG_QSHARDS - 1);
    const uint32_t n = q.counts[s];
    const uint32_t *items = q.items + (size_t)s * q.stride;
    if constexpr (COUNT) {
        // block-uniform loop bound: whole waves reach the keyed add together
        for (uint32_t base = (bid / PG_QSHARDS) * TRACE_BLOCK; base < n; base += nblk / PG_QSHARDS * TRACE_BLOCK) {
            const uint32_t i = base + threadIdx.x;
            uint32_t tri = 0xFFFFFFFFu;
            if (i < n) {
                const uint32_t slot = items[i];
                const float4 o = ldS(pathRayO(p, slot)), d = ldS(&p.sh_d[slot]);
                if (!occluded(sc, xyz(o), xyz(d), shadowTmin(o), d.w, stk, tri)) shadowAdd(p, slot);
            }
            if (sc.blk_counts && blockerRowCounted(base / TRACE_BLOCK)) {  // pg_layout.h PG_BLOCKER_SAMPLE
                waveKeyedAdd<uint32_t>(sc.blk_counts, tri, 1u, tri != 0xFFFFFFFFu);
                const unsigned long long rays = __ballot(i < n);
                if ((threadIdx.x & 63) == 0 && rays) atomicAdd(sc.blk_total, (uint32_t)__popcll(rays));
            }
        }
        return;
    }
    for (uint32_t i = (bid / PG_QSHARDS) * TRACE_BLOCK + threadIdx.x; i < n; i += nblk / PG_QSHARDS * TRACE_BLOCK) {
        uint32_t slot = items[i];
        // the shadow ray starts at the shading point, which is also the extension ray's origin
        float4 o = ldS(pathRayO(p, slot)), d = ldS(&p.sh_d[slot]);
        if (!occluded(sc, xyz(o), xyz(d), shadowTmin(o), d.w, stk)) shadowAdd(p, slot);
    }
}

template <bool COUNT>
__global__ __launch_bounds__(TRACE_BLOCK) void k_shadow(SceneDev sc, PathDev p, Queue q) {
    __shared__ uint32_t stack[2 * WIDE_LDS_STACK * TRACE_BLOCK];
    shadowRows<COUNT>(sc, p, q, blockIdx.x, gridDim.x, threadWideStack(stack, p.stack_ovf));
}

// Doom probe (pg_layout.h): does the doomed ray (o, d) hit anything?  The closest-hit walk's own 4-wide nodes, padded
// box tests, tmin and TriAccel records with tmax = inf, stopped at the first accepted triangle.  Until its first
// accepted triangle a closest-hit walk visits the same nodes and leaves in the same order (its culling distance is
// still inf), so "hit" here is exactly "the closest-hit walk would have returned a hit".  (The shadow rays' 8-wide
// tree culls boxes differently and could disagree on a grazing ray.)
__device__ __forceinline__ bool probeHit(const SceneDev &sc, float4 o, float4 d, const TStack &stk) {
    float tmax = __builtin_huge_valf(), u = 0, v = 0;
    uint32_t tri = 0xFFFFFFFFu;
    return traverse<true>(sc.nodes, sc.tris, xyz(o), xyz(d), fabsf(o.w), tmax, tri, u, v, stk);
}
// the probes of queue shard bid % PG_QSHARDS that block bid of nblk takes (a grid-stride loop as shadowRows'): no hit
// record, no class queue; a wave adds its hits to the culled row and its misses to the escaped row of the counter
// block the same launch's closest hits use, so the host's accounting sees them as it did when they were traced
// Probe occluders (pg_layout.h): a probe the listed triangles resolve (pg_ray_hits_occluders: the walk is certain to
// return a hit) is a hit without the walk, also counted in the queue's `dropped` row (pg_get_probes_resolved).  A walk
// costs its wave what its slowest lane costs, so resolving most lanes of a wave saves nothing by itself: the probes a
// row leaves unresolved are gathered in the wave's `pend` (PG_PROBE_PEND entries of LDS, the slot with bit 31 set on a
// counted row) and walked 64 at a time by full waves, the rest after the last row.  An empty list costs the one
// uniform branch: every row walks at once, as it did.
// COUNT (the recording passes' instantiation, as shadowRows'): on the sampled rows every probe adds one to
// sc.prb_counts[the triangle that answered it] -- the one its walk accepted, or the listed one that resolved it, so a
// listed triangle keeps its share -- and the row's probes, hit or miss, to sc.prb_total.
#define PG_PROBE_PEND 128u
template <bool COUNT>
__device__ __forceinline__ void probeRows(const SceneDev &sc, const PathDev &p, const Queue &q, const ClassQueues &cqs,
                                          uint32_t bid, uint32_t nblk, const TStack &stk, uint32_t *pend) {
    const uint32_t s = bid & (PG_QSHARDS - 1);
    const uint32_t n = q.counts[s];
    const uint32_t *items = q.items + (size_t)s * q.stride;
    const uint32_t lane = threadIdx.x & 63u;
    const bool learn = COUNT && sc.prb_counts != nullptr;
    uint32_t hits = 0, misses = 0, resolved = 0;
    uint32_t held = 0;  // entries in pend (wave-uniform)
    const uint32_t step = nblk / PG_QSHARDS * TRACE_BLOCK;
    uint32_t base = (bid / PG_QSHARDS) * TRACE_BLOCK;
    // block-uniform loop bounds: whole waves reach the ballots and the keyed adds together.  One iteration takes a row
    // (while any is left), then walks at most once -- the row itself under an empty list, else 64 gathered probes, or
    // what is left of them after the last row -- so the walk is compiled once.
    while (base < n || held) {
        float4 o = make_float4(0, 0, 0, 0), d = o;
        bool active = false, counted = false, go = false;
        if (base < n) {
            const uint32_t i = base + threadIdx.x;
            const bool rowCounted = learn && blockerRowCounted(base / TRACE_BLOCK);  // pg_layout.h PG_BLOCKER_SAMPLE
            base += step;
            uint32_t slot = 0;
            if (i < n) {
                slot = items[i];
                o = ldS(pathRayO(p, slot));
                d = ldS(pathRayD(p, slot));
            }
            if (rowCounted) {
                const unsigned long long rays = __ballot(i < n);
                if (lane == 0 && rays) atomicAdd(sc.prb_total, (uint32_t)__popcll(rays));
            }
            if (!sc.num_occluders) {
                active = i < n;
                counted = rowCounted;
                go = true;
            } else {
                uint32_t listed = 0;
                if (i < n) {
                    const float po[3] = {o.x, o.y, o.z}, pd[3] = {d.x, d.y, d.z};
                    listed = pg_ray_hits_occluders(sc.prb, sc.num_occluders, sc.absmax, po, pd, fabsf(o.w));
                }
                if (listed) {
                    ++resolved;
                    ++hits;
                }
                if (rowCounted) waveKeyedAdd<uint32_t>(sc.prb_counts, listed - 1u, 1u, listed != 0);
                const bool open = i < n && !listed;
                const unsigned long long m = __ballot(open);
                // held < 64 here, so held + popc(m) <= 127 < PG_PROBE_PEND
                if (open) pend[held + __popcll(m & ((1ull << lane) - 1ull))] = slot | (rowCounted ? 0x80000000u : 0u);
                held += (uint32_t)__popcll(m);
                // pend is the wave's own and a wave's LDS accesses complete in program order on gfx950 (lockstep lanes,
                // one in-order LDS queue per wave), so a wavefront-scope fence is all that keeps the compiler from
                // moving the reads below over these writes; no barrier, no other wave ever touches this part
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
        }
        if (sc.num_occluders && (held >= 64u || (base >= n && held))) {  // the top min(held, 64) entries of pend
            const uint32_t m = held < 64u ? held : 64u;
            held -= m;
            active = lane < m;
            if (active) {
                const uint32_t e = pend[held + lane];
                counted = (e >> 31) != 0;
                o = ldS(pathRayO(p, e & 0x7FFFFFFFu));
                d = ldS(pathRayD(p, e & 0x7FFFFFFFu));
            }
            go = true;
        }
        if (go) {
            uint32_t tri = 0xFFFFFFFFu;
            if (active) {
                float tmax = __builtin_huge_valf(), u = 0, v = 0;
                if (traverse<true>(sc.nodes, sc.tris, xyz(o), xyz(d), fabsf(o.w), tmax, tri, u, v, stk)) ++hits;
                else ++misses;
            }
            if (learn) waveKeyedAdd<uint32_t>(sc.prb_counts, tri, 1u, counted && tri != 0xFFFFFFFFu);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        hits += __shfl_xor(hits, off);
        misses += __shfl_xor(misses, off);
        resolved += __shfl_xor(resolved, off);
    }
    if (lane == 0) {
        if (hits) atomicAdd(cqs.q[PG_CLASS_CULLED].counts + s, hits);
        if (misses) atomicAdd(cqs.q[PG_CLASS_ESCAPED].counts + s, misses);
        if (resolved) atomicAdd(q.dropped + s, resolved);
    }
}
// the probes in a launch of their own (the unfused launches, PG_NO_RAYS_FUSION)
template <bool COUNT>
__global__ __launch_bounds__(TRACE_BLOCK) void k_probe(SceneDev sc, PathDev p, Queue q, ClassQueues cqs) {
    __shared__ uint32_t stack[LDS_STACK * TRACE_BLOCK];
    __shared__ uint32_t pend[PG_PROBE_PEND * (TRACE_BLOCK / 64)];
    probeRows<COUNT>(sc, p, q, cqs, blockIdx.x, gridDim.x, threadStack(stack, p.stack_ovf),
                     pend + PG_PROBE_PEND * (threadIdx.x / 64));
}

// a bounce's shadow rays and the next closest hits in one launch: blocks [0, shadow_blocks) run
// k_shadow's rows, the rest k_trace's (an escaped path's environment radiance goes to its hit
// record, not to L, so it cannot race with the same path's NEE add).  Blocks past those two ranges run the doom probes
// (probeRows) of the bounce just shaded: rays of paths that are in neither of the other queues' next vertices, and
// blocks of their own, so they do not lengthen the closest-hit waves.  All parts are grid-stride loops over their
// shards; the overflow ring holds three launches' worth of threads (3 x pg_stack_overflow_words(0)).
static_assert(2 * WIDE_LDS_STACK >= LDS_STACK, "k_rays / k_trace_rays share one LDS stack array");
#ifndef PG_RAYS_WAVES
#define PG_RAYS_WAVES 8
#endif
// COUNT: the recording passes' instantiation, whose shadow rows count blockers (shadowRows)
template <bool ENV, bool COUNT = false>
__global__ __launch_bounds__(TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(PG_RAYS_WAVES))) void k_rays(GParams g, SceneDev sc, PathDev p, Queue q, ClassQueues cqs,
                                                      Queue shq, uint32_t shadow_blocks, Queue pq, uint32_t probe_blocks) {
    // >= LDS_STACK words per thread
    __shared__ uint32_t stack[2 * WIDE_LDS_STACK * TRACE_BLOCK];
    __shared__ uint32_t pend[PG_PROBE_PEND * (TRACE_BLOCK / 64)];  // probeRows' unresolved probes, per wave
    // the probe blocks come last
    if (blockIdx.x >= gridDim.x - probe_blocks) {
        probeRows<COUNT>(sc, p, pq, cqs, blockIdx.x - (gridDim.x - probe_blocks), probe_blocks,
                         threadStack(stack, p.stack_ovf), pend + PG_PROBE_PEND * (threadIdx.x / 64));
        return;
    }
    const uint32_t trace_blocks = gridDim.x - probe_blocks - shadow_blocks;
    if (blockIdx.x >= trace_blocks) {
        shadowRows<COUNT>(sc, p, shq, blockIdx.x - trace_blocks, shadow_blocks, threadWideStack(stack, p.stack_ovf));
    } else {
        const TStack sa = threadStack(stack, p.stack_ovf);
        traceRows<ENV, false>(g, sc, p, q, cqs, nullptr, blockIdx.x, trace_blocks, sa);
    }
}

// ray order key of a new extension ray (PG_RAY_SORT): direction octant, then the Morton code of the
// origin's cell in an 8^3 grid over the SD-tree cube (the scene bounds)
__device__ __forceinline__ uint32_t rayOrderKey(const SDDev &sd, f3 o, f3 d) {
    const float inv = 8.0f / sd.extent;
    const int cx = min(max((int)((o.x - sd.lo[0]) * inv), 0), 7);
    const int cy = min(max((int)((o.y - sd.lo[1]) * inv), 0), 7);
    const int cz = min(max((int)((o.z - sd.lo[2]) * inv), 0), 7);
    uint32_t m = 0;
    for (int b = 0; b < 3; ++b)
        m |= (((cx >> b) & 1) << (3 * b)) | (((cy >> b) & 1) << (3 * b + 1)) | (((cz >> b) & 1) << (3 * b + 2));
    const uint32_t oct = (d.x < 0 ? 1u : 0u) | (d.y < 0 ? 2u : 0u) | (d.z < 0 ? 4u : 0u);
    return (oct << 9) | m;
}

// one bounce of Li for every queued path (progressive_path.cpp:149-306 + guiding)
// MODEL >= 0 compiles only that BSDF model's code (material-class queues filled by k_trace);
// CAN_GUIDE = false drops the SD-tree code for classes that are never guided (delta lobes).
// ENV compiles in environment-emitter sampling for NEE (kept out of the other instantiations: it
// costs 4-8 VGPRs).
// one bounce of Li for the path in `slot` (progressive_path.cpp:149-306 + guiding): reads its state,
// writes the next one; alive = an extension ray was written, shadow = a shadow ray was written (sh_*)
// mats: the material table (global memory, or a block's LDS copy); wantKey: compute rkey (PG_RAY_SORT)

// the per-bounce half of a path's info record (depth | flags, vertex count): pixel and sample never
// change after k_camera, so an 8-B store replaces the 16-B rewrite
__device__ __forceinline__ void stPinfoZW(uint4 *p, uint32_t z, uint32_t w) {
    reinterpret_cast<uint2 *>(p)[1] = make_uint2(z, w);
}

#if PG_TRAV_STATS
extern "C" int pg_debug_trav_stats(unsigned long long *out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pgTravStats), 8 * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pgTravStats), z, 8 * 8) != hipSuccess) return -1;
    }
    return 0;
}
#endif
// Debug build only (PG_WATCH=1, make watch -> build/libpgamd_watch.so; tools/diverge_c3.py): shadeOne
// logs every vertex of one (pixel, sample) path, the same record the oracle's Li writes (oracle.cpp
// g_vtxLog): depth, original triangle, p, T, alpha, guided, mode, woPdf, weight, wo, L, NEE
// contribution and pdfs, RR q / outcome, alive, shadow, b0, b1.  The product build has none of it.
#ifndef PG_WATCH
#define PG_WATCH 0
#endif
#if PG_WATCH
#define PG_WATCH_F 32
#define PG_WATCH_MAX 256
__device__ uint32_t pgWatch[3];  // pixel, sample, records written
__device__ float pgWatchLog[PG_WATCH_MAX * PG_WATCH_F];
extern "C" int pg_debug_watch(uint32_t pixel, uint32_t sample) {
    const uint32_t w[3] = {pixel, sample, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(pgWatch), w, sizeof(w)) == hipSuccess ? 0 : -1;
}
extern "C" int pg_debug_watch_read(float *out, uint32_t max, uint32_t *n) {
    uint32_t w[3];
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(w, HIP_SYMBOL(pgWatch), sizeof(w)) != hipSuccess) return -1;
    *n = w[2] < PG_WATCH_MAX ? w[2] : PG_WATCH_MAX;
    const uint32_t k = *n < max ? *n : max;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(pgWatchLog), (size_t)k * PG_WATCH_F * 4) == hipSuccess ? 0 : -1;
}
#define WSET(i, v) (wr[i] = (float)(v))
#define WSET3(i, v) (wr[i] = (v).x, wr[(i) + 1] = (v).y, wr[(i) + 2] = (v).z)
#else
#define WSET(i, v) ((void)0)
#define WSET3(i, v) ((void)0)
#endif

// TEX (the textured class, pg_layout.h PG_CLASS_TEXTURED): the vertex's material has a texture as its diffuse
// reflectance.  The lookup replaces the register copy of GMat::diff and the albedo bound, and the BSDF code runs on
// that copy unchanged; with TEX = false none of it is compiled.  A material of that class may also carry a normal map
// (pg_set_normal_maps): every BSDF call of the vertex then runs in the perturbed frame under normalmap.cpp's hemisphere
// rule, and the side tests keep the unperturbed normal.
// DELTA: delta emitters are set (pg_set_delta_emitters): sampleEmitter's point / spot / directional branches and the
// discrete-measure rule of the NEE below; with DELTA = false none of it is compiled.
template <int MODEL, bool CAN_GUIDE, bool ENV, bool TEX = false, bool DELTA = false>
__device__ __forceinline__ void shadeOne(const GParams &g, const SceneDev &sc, const SDDev &sd, const PathDev &p,
                                         uint32_t slot, const GMat *mats, bool wantKey, bool &alive, bool &shadow,
                                         bool &probe, uint32_t &rkey, uint32_t &blocked) {
    bool dirtyL = false;
    f3 L = mk1(0.f);
    // the watch build logs every vertex with its own roulette draw, as the oracle does
    const bool cull = !PG_WATCH && g.path_cull;
#if PG_WATCH
    float wr[PG_WATCH_F];
    for (int i = 0; i < PG_WATCH_F; ++i) wr[i] = -1.0f;
    bool watched = false;
#endif
    do {
        const uint4 pi = ldS(pathInfo(p, slot));
        const uint32_t pix = pi.x, sample = pi.y;
#if PG_WATCH
        watched = pix == pgWatch[0] && sample == pgWatch[1];
#endif
        const float4 rd4 = ldS(pathRayD(p, slot));
        float4 hv = ldS(&p.hit[slot]);
        uint32_t depth = pi.z & 0xFFFFu, flags = pi.z >> 16, nv = pi.w;
        // a camera ray's state is implied (k_camera stores no throughput)
        float4 T4 = depth == 1 ? make_float4(1.f, 1.f, 1.f, 1.f) : ldS(pathThr(p, slot));
        f3 T = xyz(T4);
        // L is loaded where the vertex first needs it: before it adds emission or snapshots a training vertex.  Most
        // vertices of a non-recording pass do neither, and the dirtyL store below is the only one either way.
        bool haveL = depth == 1;
        auto loadL = [&]() {
            if (!haveL) {
                L = xyz(ldS(&p.rad[slot]));
                haveL = true;
            }
        };
        if (PG_WATCH) loadL();
        float eta = T4.w;
        uint32_t tri = __float_as_uint(hv.y);
        if (tri == 0xFFFFFFFFu) break;  // escaped: no environment emitter
        const uint32_t key = rngKey(pix, g.seed);
        f3 rd = xyz(rd4);
        Hit h;
        fetchHit(sc, tri, hv.z, hv.w, rd, h);
        WSET(0, depth);
        WSET(1, __float_as_uint(sc.tshade[(size_t)PG_TRI_SHADE_STRIDE * tri + 2].w));
        WSET3(2, h.p);
        f3 Le = mk1(0.f);
        if (h.emitter >= 0 && dot(h.shN, -rd) > 0) {  // AreaLight::eval (area.cpp)
            const GEmitter &em = sc.ems[h.emitter];
            Le = mk(em.radiance[0], em.radiance[1], em.radiance[2]);
        }
        // ---- finish the previous bounce: emitter hit by the sampled direction (MIS), then RR
        if (depth > 1) {
            if (h.emitter >= 0) {
                // the pdf the previous vertex sampled this direction with, and the side it left that vertex on
                const float prevPdf = rd4.w;  // a bounce ray's row (pg_layout.h "Path state")
                float lumPdf = 0.0f;
                if (g.use_nee && !(flags & PF_PREV_DELTA)) {
                    if ((flags & PF_PREV_FRONT) && dot(rd, h.shN) < 0) {
                        const GEmitter &em = sc.ems[h.emitter];
                        lumPdf = em.inv_area * (hv.x * hv.x) / absDot(rd, h.shN) * (1.0f / (float)g.num_emitters);
                    }
                }
                float w = g.use_nee ? miWeight(prevPdf, lumPdf) : 1.0f;
                loadL();
                L = L + T * Le * w;
                dirtyL = true;
            }
            // PF_DOOMED (pg_layout.h): the previous vertex's shader made this vertex's exits for it, and the
            // tracer kept the path only because it hit an emitter
            if (flags & PF_DOOMED) break;
            if (depth - 1 >= (uint32_t)g.rr_depth) {
                float q = fminf(maxc(T) * eta * eta, 0.95f);
                WSET(26, q);
                WSET3(18, L);
                WSET3(5, T);
                WSET(27, 0);
                // with the cull on, a vertex that got here has already survived this draw
                if (!cull && rng1(key, sample, dimOf(depth - 1, SLOT_RR)) >= q) break;
                WSET(27, 1);
                T = T / q;
            }
        }
        WSET3(5, T);
        if (depth > g.depth_cap) break;
        // the next vertex's roulette draw (PF_DOOMED), made where this vertex's own used to be: here Philox costs
        // the registers it always did (k_shade_all spills 4 VGPRs); next to the extension-ray stores it spilled 49
        float rrNext = 0.0f;
        if (cull && depth >= (uint32_t)g.rr_depth) rrNext = rng1(key, sample, dimOf(depth, SLOT_RR));
        GMat M = mats[h.mat];
        if constexpr (TEX) {
            const uint32_t ti = sc.mtex[h.mat];
            if (ti != 0xFFFFFFFFu) {
                float tu, tv;
                hitUV(sc, tri, hv.z, hv.w, tu, tv);
                const f3 c = texEval(sc.tex[ti], tu, tv);
                M.diff[0] = c.x;
                M.diff[1] = c.y;
                M.diff[2] = c.z;
                M.wbound = maxc(bsdfAlbedo(M));  // the host's makeGMat bound, of the looked-up reflectance
            }
        }
        if ((flags & PF_EMITTED_QUERY) && h.emitter >= 0 && (!g.hide_emitters || (flags & PF_SCATTERED))) {
            loadL();
            L = L + T * Le;
            dirtyL = true;
        }
        if ((g.max_depth > 0 && (int)depth >= g.max_depth) ||
            (g.strict_normals && dot(rd, h.geoN) * h.wi.z >= 0))
            break;
        // a normal-mapped material: from here on h.sh and h.wi are the perturbed frame and -d in it; h.shN stays
        bool mapped = false;
        if constexpr (TEX) {
            mapped = nmapFrame(sc, tri, hv.z, hv.w, h.mat, h.shN, h.sh);
            if (mapped) h.wi = h.sh.toLocal(-rd);
        }
        // normalmap.cpp:215,233,258,280: wo on opposite sides of the unperturbed and the perturbed tangent plane
        auto wrongSide = [&](f3 woW, float woZ) { return TEX && mapped && dot(woW, h.shN) * woZ <= 0; };
        WSET3(18, L);
        const f3 refN = (M.type & (ETransmission | EBackSide)) == 0 ? h.shN : mk1(0.f);
        // glossy prior (pg_config.glossy_prior): r = BSDF::getGlossySamplingRate; r = 1 is not guided
        const float gRate = (CAN_GUIDE && g.glossy_prior) ? glossyRate<MODEL>(M, h.wi.z) : 0.0f;
        const bool guide = CAN_GUIDE && g.guiding && sd.built && (M.type & ESmooth) && !(M.type & EDelta) && gRate < 1.0f;
        const SDView sv = sdv(sd);
        uint4 meta = make_uint4(0, 0, 0, 0);
        if (guide) meta = sd.meta[sdLookup(sv, h.p)];
        // one-sample-MIS BSDF fraction of this vertex (pg_config.bsdf_fraction_bound; oracle guideFraction):
        // PG_FRACTION_LEARNED reads the leaf's learned fraction (meta.z; 0 = not learned yet)
        const float leafAlpha = __uint_as_float(meta.z);
        float alpha = g.fraction_bound == PG_FRACTION_LEARNED ? (leafAlpha > 0 ? leafAlpha : g.bsdf_fraction)
                                                               : guideFraction(g.fraction_bound, g.bsdf_fraction,
                                                                               M.wbound, maxc(T));
        if (gRate > 0.0f) {
#pragma clang fp contract(off)
            alpha = gRate + (1.0f - gRate) * alpha;
        }
        float pgWo = -1.0f;  // p_guide of the sampled direction at a guided vertex (training record)

        // ---- NEE (progressive_path.cpp:193-219); the shadow ray is deferred to k_shadow.  With
        // guiding, the D-tree pdf of the light direction is resolved below, in one lockstep walk
        // with the direction-sampling descent (sdDual).
        f3 neeC = mk1(0.f), neeD = mk1(0.f), neeV = mk1(0.f);
        float neeDist = 0, neeEmPdf = 0, neeBp = 0;
        bool neePending = false;
        if (g.use_nee && (M.type & ESmooth)) {
            float s0, s1;
            rng2(key, sample, dimOf(depth, SLOT_NEE), s0, s1);
            float emPdf;
            bool discrete = false;  // a delta emitter's sample: MIS weight 1, no D-tree pdf of its direction
            f3 value = sampleEmitter<ENV, DELTA>(g, sc, h.p, refN, s0, s1, neeD, neeDist, emPdf, nullptr, &discrete);
            if (!isZero(value)) {
                f3 woL = h.sh.toLocal(neeD);
                f3 bsdfVal = wrongSide(neeD, woL.z) ? mk1(0.f) : bsdfEval<MODEL>(M, h.wi, woL);
                // strict normals test bRec.wo, a direction of the unperturbed frame
                const float woZ = TEX && mapped ? dot(neeD, h.shN) : woL.z;
                if (!isZero(bsdfVal) && (!g.strict_normals || dot(h.geoN, neeD) * woZ > 0)) {
                    neeBp = bsdfPdf<MODEL>(M, h.wi, woL);
                    neeEmPdf = emPdf;
                    neeV = T * value * bsdfVal;
                    shadow = true;
                    // shadow blockers (pg_layout.h): the ray shadowRows would trace, (h.p, neeD, shadowTmin, the tmax
                    // stored in sh_d.w below), tested against the listed triangles before anything is stored.  A
                    // certain hit: no shadow ray; its contribution is dropped as shadowRows would drop it.
                    if (!ENV && sc.num_blockers) {
                        const float po[3] = {h.p.x, h.p.y, h.p.z}, pd[3] = {neeD.x, neeD.y, neeD.z};
                        blocked = pg_ray_hits_blockers(sc.blk, sc.num_blockers, sc.absmax, po, pd,
                                                       shadowTmin(f4(h.p, 0.0f)), neeDist * (1 - kShadowEpsilon));
                        shadow = blocked == 0;
                    }
                    if (DELTA && discrete) neeC = neeV;
                    else if (guide) neePending = shadow;  // a resolved ray's contribution is never used
                    else neeC = neeV * miWeight(emPdf, neeBp);
                }
            }
        }

        // ---- direction sampling: BSDF, or one-sample MIS between BSDF and the D-tree
        BS bs;
        f3 weight;
        float woPdf;
        bool ok = true;
        {
            float b0, b1;
            rng2(key, sample, dimOf(depth, SLOT_BSDF), b0, b1);
            float b2 = rng1(key, sample, dimOf(depth, SLOT_COMP));
            WSET(30, b0);
            WSET(31, b1);
            int mode = 0;  // D-tree walk of the sampled direction: 0 none, 1 pdf (BSDF sample), 2 sample
            float bu = 0, bw = 0;
            if (!guide) {
                weight = bsdfSample<MODEL>(M, h.wi, b0, b1, b2, bs);
                if (!isZero(weight) && wrongSide(h.sh.toWorld(bs.wo), bs.wo.z)) weight = mk1(0.f);
                woPdf = bs.pdf;
            } else if (rng1(key, sample, dimOf(depth, SLOT_GUIDE_CHOICE)) < alpha) {
                weight = bsdfSample<MODEL>(M, h.wi, b0, b1, b2, bs);
                if (!isZero(weight) && wrongSide(h.sh.toWorld(bs.wo), bs.wo.z)) weight = mk1(0.f);
                if (isZero(weight)) {
                    ok = false;
                } else {
                    mode = 1;
                    dirToCanonical(h.sh.toWorld(bs.wo), bu, bw);
                }
            } else {
                mode = 2;
                rng2(key, sample, dimOf(depth, SLOT_GUIDE), bu, bw);
            }
            if (guide) {
                float au = 0, aw = 0, aPdf, dPdf, cu, cv;
                if (neePending) dirToCanonical(neeD, au, aw);
                sdDual(sv, meta, neePending, au, aw, aPdf, mode != 0, mode == 2, bu, bw, cu, cv, dPdf);
                if (neePending) neeC = neeV * miWeight(neeEmPdf, alpha * neeBp + (1 - alpha) * aPdf);
                pgWo = dPdf;
                if (mode == 1) {
                    woPdf = alpha * bs.pdf + (1 - alpha) * dPdf;
                    weight = weight * (bs.pdf / woPdf);
                } else if (mode == 2) {
                    f3 dW = canonicalToDir(cu, cv);
                    f3 woL = h.sh.toLocal(dW);
                    const bool wrong = wrongSide(dW, woL.z);
                    f3 f = wrong ? mk1(0.f) : bsdfEval<MODEL>(M, h.wi, woL);
                    float bp = wrong ? 0.0f : bsdfPdf<MODEL>(M, h.wi, woL);
                    woPdf = alpha * bp + (1 - alpha) * dPdf;
                    if (!(woPdf > 0) || isZero(f)) {
                        ok = false;
                    } else {
                        weight = f / woPdf;
                        bs.wo = woL;
                        bs.pdf = bp;
                        bool refl = h.wi.z * woL.z > 0;
                        bs.type = refl ? ((M.type & EDiffuseReflection) ? EDiffuseReflection : EGlossyReflection)
                                       : EGlossyTransmission;
                        bs.eta = refl ? 1.0f : (h.wi.z > 0 ? M.eta : M.invEta);
                    }
                }
            }
            WSET(10, mode + (ok ? 0 : 10));
        }
        uint32_t vtxIndex = 0xFFFFFFFFu;
        WSET(8, alpha);
        WSET(9, guide ? 1 : 0);
        WSET(11, woPdf);
        WSET3(12, weight);
        WSET3(15, h.sh.toWorld(bs.wo));
        WSET3(21, neeC);
        WSET(24, neeEmPdf);
        WSET(25, neeBp);
        if (ok && !isZero(weight)) {
            if (bs.type != ENull) flags |= PF_SCATTERED;
            f3 wo = h.sh.toWorld(bs.wo);
            const float woZ = TEX && mapped ? dot(wo, h.shN) : bs.wo.z;  // bRec.wo.z of the unperturbed frame
            if (!(g.strict_normals && dot(h.geoN, wo) * woZ <= 0)) {
                f3 Tn = T * weight;
                // training vertex: (x, wo, woPdf, T after this bounce, L snapshot)
                if (g.record && !(bs.type & EDelta) && nv < (uint32_t)g.max_vertices) {
                    float cu, cv;
                    dirToCanonical(wo, cu, cv);
                    loadL();
                    float4 *vb = p.vtx + ((size_t)nv * p.vtxP + slot) * PG_VTX_F4;
                    stS(vb + 0, f4(h.p, woPdf));
                    stS(vb + 1, f4(Tn, __uint_as_float(packCanonical(cu, cv))));
                    stS(vb + 2, f4(L, 0.0f));
                    // learned-fraction statistics only from vertices whose fraction is the leaf's (r = 0)
                    stS(vb + 3, f4(T, guide && gRate == 0.0f ? pgWo : -1.0f));
                    vtxIndex = nv;
                    nv++;
                }
                const float tmin = pg_ray_tmin(h.p.x, h.p.y, h.p.z);
                const float etaN = eta * bs.eta;
                // the next vertex's exits, decided here (PF_DOOMED): its depth tests, and its roulette draw against
                // the throughput and eta it will load from its vst record
                bool doomed = false;
                if (cull) {
                    const uint32_t D = depth + 1;
                    doomed = D > g.depth_cap || (g.max_depth > 0 && (int)D >= g.max_depth) ||
                             (D - 1 >= (uint32_t)g.rr_depth && rrNext >= fminf(maxc(Tn) * etaN * etaN, 0.95f));
                }
                // doom probe (pg_layout.h): a doomed ray that misses every emitter box cannot end on an emitter, so
                // only whether it hits anything is still wanted (culled against escaped)
                if (!ENV && doomed && g.doom_probe) {
                    const float po[3] = {h.p.x, h.p.y, h.p.z}, pd[3] = {wo.x, wo.y, wo.z};
                    probe = pg_ray_misses_boxes(sc.em_box, sc.num_em_boxes, sc.em_absmax, po, pd, tmin);
                }
                // the bounce ray's rows (pg_layout.h "Path state")
                stS(pathRayO(p, slot), f4(h.p, doomed ? -tmin : tmin));
                stS(pathRayD(p, slot), f4(wo, woPdf));
                if (probe) {  // the path ends here: the hit record a culled hit gets, no state for a next vertex
                    stS(&p.hit[slot], make_float4(0.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f));
                } else {
                    stS(pathThr(p, slot), f4(Tn, etaN));
                    flags = (flags & ~(PF_EMITTED_QUERY | PF_PREV_DELTA | PF_PREV_FRONT)) |
                        ((bs.type & EDelta) ? PF_PREV_DELTA : 0u) | (doomed ? PF_DOOMED : 0u) |
                        (pg_prev_front(wo.x, wo.y, wo.z, refN.x, refN.y, refN.z) ? PF_PREV_FRONT : 0u);
                    stPinfoZW(pathInfo(p, slot), (depth + 1) | (flags << 16), nv);
                    alive = true;
                    if (wantKey) rkey = rayOrderKey(sd, h.p, wo);
                }
            }
        }
        if (shadow) {  // origin: ray_o (the extension ray's, written above when the path goes on)
            if (!alive && !probe) stS(pathRayO(p, slot), f4(h.p, 0.0f));
            stS(&p.sh_d[slot], f4(neeD, neeDist * (1 - kShadowEpsilon)));
            stS(&p.sh_c[slot], f4(neeC, __uint_as_float(vtxIndex)));
        }
        if (!alive && nv != pi.w) stPinfoZW(pathInfo(p, slot), pi.z, nv);
    } while (false);
    if (dirtyL) stS(&p.rad[slot], f4(L, 0.0f));
#if PG_WATCH
    if (watched) {
        wr[28] = alive ? 1.0f : 0.0f;
        wr[29] = shadow ? 1.0f : 0.0f;
        const uint32_t k = atomicAdd(&pgWatch[2], 1u);
        if (k < PG_WATCH_MAX)
            for (int i = 0; i < PG_WATCH_F; ++i) pgWatchLog[k * PG_WATCH_F + i] = wr[i];
    }
#endif
}

template <int MODEL, bool CAN_GUIDE, bool ENV, bool TEX = false, bool DELTA = false>
__device__ __forceinline__ void shadeBlock(const GParams &g, const SceneDev &sc, const SDDev &sd, const PathDev &p,
                                           const Queue &in, const Queue &out, const Queue &shq, const Queue &pq,
                                           uint32_t bid) {
    // one item per thread (a grid-stride loop here cost ~45 VGPRs of hoisted invariants): block b
    // takes row b / PG_QSHARDS of shard b % PG_QSHARDS; rows past the shard's count exit at once
    const uint32_t s = bid & (PG_QSHARDS - 1);
    const uint32_t n = in.counts[s];
    {
    const uint32_t base = (bid / PG_QSHARDS) * SHADE_BLOCK;
    if (base >= n) return;
    const uint32_t i = base + threadIdx.x;
    bool alive = false, shadow = false, probe = false;
    uint32_t slot = 0, rkey = 0, blocked = 0;
    if (i < n) slot = in.items[(size_t)s * in.stride + i];
    // the material table, staged in LDS once per block (the material read sits on the dependent chain
    // hit -> triangle -> material of every shaded vertex); larger tables stay in global memory
    __shared__ float4 smat[(SHADE_LDS_MATS > 0 ? SHADE_LDS_MATS : 1) * (sizeof(GMat) / 16)];
    const bool ldsMats = SHADE_LDS_MATS > 0 && g.num_materials <= SHADE_LDS_MATS;
    if (ldsMats) {
        const float4 *src = reinterpret_cast<const float4 *>(sc.mats);
        for (uint32_t k = threadIdx.x; k < g.num_materials * (uint32_t)(sizeof(GMat) / 16); k += SHADE_BLOCK) smat[k] = src[k];
        __syncthreads();
    }
    if (i < n)
        shadeOne<MODEL, CAN_GUIDE, ENV, TEX, DELTA>(g, sc, sd, p, slot, ldsMats ? reinterpret_cast<const GMat *>(smat) : sc.mats,
                                        out.keys != nullptr, alive, shadow, probe, rkey, blocked);
    if (out.keys)
        waveAppendKey(alive, slot, (uint16_t)rkey, out.items + (size_t)s * out.stride, out.keys + (size_t)s * out.stride,
                      out.counts + s);
    else
        waveAppend(alive, slot, out.items + (size_t)s * out.stride, out.counts + s);
    waveAppend(shadow, slot, shq.items + (size_t)s * shq.stride, shq.counts + s);
    // shadow rays resolved against the blocker list: counted only (they stay in pg_stats.shadow_rays), and in the
    // recording passes added to their blocker's count, as the any-hit rows would have
    if (!ENV && sc.num_blockers) {
        const unsigned long long m = __ballot(blocked != 0);
        if (m) {
            if ((threadIdx.x & 63) == 0) atomicAdd(shq.dropped + s, (uint32_t)__popcll(m));
            if (sc.blk_counts && blockerRowCounted(bid / PG_QSHARDS)) {
                waveKeyedAdd<uint32_t>(sc.blk_counts, blocked - 1u, 1u, blocked != 0);  // blocked: 1 + the triangle
                if ((threadIdx.x & 63) == 0) atomicAdd(sc.blk_total, (uint32_t)__popcll(m));
            }
        }
    }
    // doomed rays that miss every emitter box: the tracer's probe rows (never set with ENV or without the probe)
    if (!ENV && g.doom_probe) waveAppend(probe, slot, pq.items + (size_t)s * pq.stride, pq.counts + s);
    }
}

template <int MODEL, bool CAN_GUIDE, bool ENV, bool TEX = false, bool DELTA = false>
__global__ __launch_bounds__(SHADE_BLOCK) void k_shade(GParams g, SceneDev sc, SDDev sd, PathDev p, Queue in,
                                                       Queue out, Queue shq, Queue pq) {
    shadeBlock<MODEL, CAN_GUIDE, ENV, TEX, DELTA>(g, sc, sd, p, in, out, shq, pq, blockIdx.x);
}

// every material class of a bounce in one launch (no environment emitter): blocks
// [end[c-1], end[c]) shade class c.  All class bodies fit 128 VGPRs, so the shared register budget
// keeps the 4 waves/SIMD each class kernel has alone.
struct ShadeRanges {
    uint32_t end[PG_NUM_CLASSES];
};
#ifndef PG_SHADE_WAVES
#define PG_SHADE_WAVES 4
#endif
// TEX: the scene has textures bound (pg_set_textures): the instantiation with the textured class' body.  Scenes
// without textures launch k_shade_all<false>, which holds the six bodies it always did and nothing else.
// DELTA: delta emitters are set (pg_set_delta_emitters): every body with the delta NEE compiled in.
template <bool TEX, bool DELTA = false>
__global__ __launch_bounds__(SHADE_BLOCK) __attribute__((amdgpu_waves_per_eu(PG_SHADE_WAVES))) void k_shade_all(
    GParams g, SceneDev sc, SDDev sd, PathDev p, ClassQueues in, Queue out, Queue shq, Queue pq, ShadeRanges r) {
    static_assert(PG_NUM_CLASSES == 7, "class ranges");
    const uint32_t b = blockIdx.x;
    if (b < r.end[0]) shadeBlock<PG_BSDF_DIFFUSE, true, false, false, DELTA>(g, sc, sd, p, in.q[0], out, shq, pq, b);
    else if (b < r.end[1]) shadeBlock<PG_BSDF_ROUGHCONDUCTOR, true, false, false, DELTA>(g, sc, sd, p, in.q[1], out, shq, pq, b - r.end[0]);
    else if (b < r.end[2]) shadeBlock<PG_BSDF_ROUGHDIELECTRIC, true, false, false, DELTA>(g, sc, sd, p, in.q[2], out, shq, pq, b - r.end[1]);
    else if (b < r.end[3]) shadeBlock<PG_BSDF_PLASTIC, false, false, false, DELTA>(g, sc, sd, p, in.q[3], out, shq, pq, b - r.end[2]);
    else if (b < r.end[4]) shadeBlock<PG_BSDF_ROUGHPLASTIC, true, false, false, DELTA>(g, sc, sd, p, in.q[4], out, shq, pq, b - r.end[3]);
    else if (!TEX || b < r.end[5]) shadeBlock<-1, false, false, false, DELTA>(g, sc, sd, p, in.q[5], out, shq, pq, b - r.end[4]);
    else if constexpr (TEX)
        shadeBlock<PG_MODELS_TEXTURED, true, false, true, DELTA>(g, sc, sd, p, in.q[6], out, shq, pq, b - r.end[5]);
}

// ---- counting sort of a queue's shards by ray order key (PG_RAY_SORT): the next closest-hit launch
// then traces each shard's rays grouped by direction octant and origin cell.  Within a key the order
// follows LDS/global atomics (nondeterministic), which is harmless: every path is a pure function of
// (pixel, sample), whatever the order its bounces are traced in.
#define RSORT_TILE 4096  // queue entries per block (256 threads x 16)
template <uint32_t BINS>
__global__ __launch_bounds__(256) void k_rsort_hist(Queue q, uint32_t *hist) {
    __shared__ uint32_t h[BINS];
    const uint32_t s = blockIdx.x & (PG_QSHARDS - 1), tile = blockIdx.x / PG_QSHARDS;
    const uint32_t n = q.counts[s], b0 = tile * RSORT_TILE;
    if (b0 >= n) return;
    for (uint32_t k = threadIdx.x; k < BINS; k += 256) h[k] = 0;
    __syncthreads();
    const uint16_t *keys = q.keys + (size_t)s * q.stride;
    const uint32_t e = min(n, b0 + RSORT_TILE);
    for (uint32_t i = b0 + threadIdx.x; i < e; i += 256) atomicAdd(&h[keys[i]], 1u);
    __syncthreads();
    uint32_t *g = hist + (size_t)s * BINS;
    for (uint32_t k = threadIdx.x; k < BINS; k += 256)
        if (h[k]) atomicAdd(&g[k], h[k]);
}
// exclusive scan of every shard's histogram in place (one block per shard)
template <uint32_t BINS>
__global__ __launch_bounds__(256) void k_rsort_scan(uint32_t *hist) {
    __shared__ uint32_t part[256];
    uint32_t *g = hist + (size_t)blockIdx.x * BINS;
    constexpr int PER = BINS / 256;
    uint32_t v[PER], sum = 0;
    for (int j = 0; j < PER; ++j) {
        v[j] = g[threadIdx.x * PER + j];
        sum += v[j];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // Hillis-Steele inclusive scan of the thread sums
        const uint32_t x = threadIdx.x >= (uint32_t)off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += x;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (int j = 0; j < PER; ++j) {
        g[threadIdx.x * PER + j] = run;
        run += v[j];
    }
}
template <uint32_t BINS>
__global__ __launch_bounds__(256) void k_rsort_scatter(Queue q, uint32_t *hist, uint32_t *sorted) {
    __shared__ uint32_t cnt[BINS];
    const uint32_t s = blockIdx.x & (PG_QSHARDS - 1), tile = blockIdx.x / PG_QSHARDS;
    const uint32_t n = q.counts[s], b0 = tile * RSORT_TILE;
    if (b0 >= n) return;
    for (uint32_t k = threadIdx.x; k < BINS; k += 256) cnt[k] = 0;
    __syncthreads();
    const uint16_t *keys = q.keys + (size_t)s * q.stride;
    const uint32_t *items = q.items + (size_t)s * q.stride;
    const uint32_t e = min(n, b0 + RSORT_TILE);
    constexpr int PER = RSORT_TILE / 256;
    uint32_t rank[PER], key[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {  // fixed trip count: the per-thread arrays stay in registers
        const uint32_t i = b0 + threadIdx.x + 256u * j;
        key[j] = i < e ? keys[i] : 0u;
        rank[j] = i < e ? atomicAdd(&cnt[key[j]], 1u) : 0u;
    }
    __syncthreads();
    uint32_t *g = hist + (size_t)s * BINS;
    for (uint32_t k = threadIdx.x; k < BINS; k += 256)  // this tile's range of every key
        if (cnt[k]) cnt[k] = atomicAdd(&g[k], cnt[k]);
    __syncthreads();
    uint32_t *out = sorted + (size_t)s * q.stride;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const uint32_t i = b0 + threadIdx.x + 256u * j;
        if (i < e) out[cnt[key[j]] + rank[j]] = items[i];
    }
}

// ---- the tail of a chunk: once few paths are alive, the host stops the per-bounce launches and
// count readbacks and one launch finishes every remaining path, each thread looping shade (the
// class's specialised body) -> shadow ray -> closest hit until its path ends.  Every step is the
// wavefront's own code on the path's own state and random numbers, in the same order (a path's NEE
// is added before its next vertex is shaded), so films, records and trees are bit-identical with
// the bounce-by-bounce loop.  Input: the queue of the bounce just traced (hits already in p.hit).
// stats: [0] traced segments, [1] escaped segments, [2] shadow rays, [3] culled hits, [4] probed segments (u64,
// device atomics; a probe is also a segment and either a culled hit or an escape).
template <bool ENV, bool TEX, bool DELTA>
__device__ __forceinline__ void tailShade(const GParams &g, const SceneDev &sc, const SDDev &sd, const PathDev &p,
                                          uint32_t slot, uint32_t tri, bool &alive, bool &shadow, bool &probe,
                                          uint32_t &blocked) {
    uint32_t rk = 0;
    // the textured class: only scenes with textures bound have such triangles, and they run k_tail<.., TEX = true>
    if constexpr (TEX) {
        if ((sc.tclass[tri] & PG_TCLASS_MASK) == PG_CLASS_TEXTURED) {
            shadeOne<PG_MODELS_TEXTURED, true, ENV, true, DELTA>(g, sc, sd, p, slot, sc.mats, false, alive, shadow, probe, rk, blocked);
            return;
        }
    }
    switch (sc.tclass[tri] & PG_TCLASS_MASK) {
        case PG_CLASS_DIFFUSE: shadeOne<PG_BSDF_DIFFUSE, true, ENV, false, DELTA>(g, sc, sd, p, slot, sc.mats, false, alive, shadow, probe, rk, blocked); break;
        case PG_CLASS_ROUGHCONDUCTOR:
            shadeOne<PG_BSDF_ROUGHCONDUCTOR, true, ENV, false, DELTA>(g, sc, sd, p, slot, sc.mats, false, alive, shadow, probe, rk, blocked);
            break;
        case PG_CLASS_ROUGHDIELECTRIC:
            shadeOne<PG_BSDF_ROUGHDIELECTRIC, true, ENV, false, DELTA>(g, sc, sd, p, slot, sc.mats, false, alive, shadow, probe, rk, blocked);
            break;
        case PG_CLASS_PLASTIC: shadeOne<PG_BSDF_PLASTIC, false, ENV, false, DELTA>(g, sc, sd, p, slot, sc.mats, false, alive, shadow, probe, rk, blocked); break;
        case PG_CLASS_ROUGHPLASTIC:
            shadeOne<PG_BSDF_ROUGHPLASTIC, true, ENV, false, DELTA>(g, sc, sd, p, slot, sc.mats, false, alive, shadow, probe, rk, blocked);
            break;
        default: shadeOne<-1, false, ENV, false, DELTA>(g, sc, sd, p, slot, sc.mats, false, alive, shadow, probe, rk, blocked);
    }
}
#ifndef PG_TAIL_WAVES
#define PG_TAIL_WAVES 0  // 0: the compiler's budget (A/B: 3)
#endif
// COUNT: the recording passes' instantiation (shadowRows).  On the sampled rows, one plain add per occluded ray to its
// triangle's counter and one per shadow ray, occluded or not, to the single total: the one-address pattern that is too
// slow for the bounce launches' rows, affordable here because the tail holds few paths
template <bool ENV, bool COUNT = false, bool TEX = false, bool DELTA = false>
__global__ __launch_bounds__(TRACE_BLOCK) __attribute__((amdgpu_waves_per_eu(PG_TAIL_WAVES > 0 ? PG_TAIL_WAVES : 1))) void k_tail(GParams g, SceneDev sc, SDDev sd, PathDev p, Queue q,
                                                      unsigned long long *stats) {
    __shared__ uint32_t stack[2 * WIDE_LDS_STACK * TRACE_BLOCK];  // >= LDS_STACK words per thread
    const TStack stk = threadStack(stack, p.stack_ovf);
    const WStack wstk = threadWideStack(stack, p.stack_ovf);
    const uint32_t s = blockIdx.x & (PG_QSHARDS - 1);
    const uint32_t rows = gridDim.x / PG_QSHARDS;  // grid capped at TRACE_MAX_BLOCKS: the overflow ring's size
    const uint32_t n = q.counts[s];
    uint32_t segs = 0, esc = 0, shadows = 0, culled = 0, probes = 0, drops = 0;
    for (uint32_t i = (blockIdx.x / PG_QSHARDS) * TRACE_BLOCK + threadIdx.x; i < n; i += rows * TRACE_BLOCK) {
        const uint32_t slot = q.items[(size_t)s * q.stride + i];
        uint32_t tri = __float_as_uint(ldS(&p.hit[slot]).y);
        while (tri != 0xFFFFFFFFu) {
            bool alive = false, shadow = false, probe = false;
            uint32_t blocked = 0;
            tailShade<ENV, TEX, DELTA>(g, sc, sd, p, slot, tri, alive, shadow, probe, blocked);
            if (!ENV && blocked) {  // a shadow ray the blocker list resolved: counted, not traced
                ++shadows;
                ++drops;
                if (COUNT && blockerRowCounted(i / TRACE_BLOCK)) {
                    atomicAdd(sc.blk_counts + (blocked - 1u), 1u);
                    atomicAdd(sc.blk_total, 1u);
                }
            }
            if (shadow) {  // shadowRows for this path
                ++shadows;
                const float4 o = ldS(pathRayO(p, slot)), d = ldS(&p.sh_d[slot]);
                uint32_t btri;
                const bool occ = occluded(sc, xyz(o), xyz(d), shadowTmin(o), d.w, wstk, btri);
                if (COUNT && blockerRowCounted(i / TRACE_BLOCK)) {
                    if (btri != 0xFFFFFFFFu) atomicAdd(sc.blk_counts + btri, 1u);
                    atomicAdd(sc.blk_total, 1u);
                }
                if (!occ) {
                    const float4 c = ldS(&p.sh_c[slot]);
                    const float4 L = ldS(&p.rad[slot]);
                    stS(&p.rad[slot], make_float4(L.x + c.x, L.y + c.y, L.z + c.z, L.w));
                    const uint32_t vi = __float_as_uint(c.w);
                    if (vi != 0xFFFFFFFFu) {
                        float4 *vl = p.vtx + ((size_t)vi * p.vtxP + slot) * PG_VTX_F4 + 2;
                        const float4 a = *vl;
                        *vl = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w);
                    }
                }
            }
            if (!ENV && probe) {  // probeRows for this path: its last segment, a culled hit or an escape
                const float4 o = ldS(pathRayO(p, slot)), d = ldS(pathRayD(p, slot));
                ++segs;
                ++probes;
                if (probeHit(sc, o, d, stk)) ++culled;
                else ++esc;
            }
            if (!alive) break;
            // traceRows for this path
            const float4 o = ldS(pathRayO(p, slot)), d = ldS(pathRayD(p, slot));
            float tmax = __builtin_huge_valf(), u = 0, v = 0;
            tri = 0xFFFFFFFFu;
            const bool h = traverse<false>(sc.nodes, sc.tris, xyz(o), xyz(d), fabsf(o.w), tmax, tri, u, v, stk);
            float4 hr = make_float4(h ? tmax : 0.0f, __uint_as_float(h ? tri : 0xFFFFFFFFu), u, v);
            if (ENV && !h) {
                const f3 e = envEscapeRadiance(g, sc, p, slot, xyz(d), pathInfo(p, slot)->z, d.w);
                hr = make_float4(e.x, hr.y, e.y, e.z);
            }
            const int cls = hitClass(sc, h, tri, rayDoomed(o), hr);
            stS(&p.hit[slot], hr);
            ++segs;
            if (cls == PG_CLASS_ESCAPED) ++esc;
            if (cls == PG_CLASS_CULLED) ++culled;
            if (cls >= PG_NUM_CLASSES) tri = 0xFFFFFFFFu;  // the path ended with this segment
        }
    }
    // wave-summed counters
    unsigned long long a = segs, b = esc, c = shadows, e = culled, f = probes, dr = drops;
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
        c += __shfl_xor(c, off);
        e += __shfl_xor(e, off);
        f += __shfl_xor(f, off);
        dr += __shfl_xor(dr, off);
    }
    if ((threadIdx.x & 63) == 0 && (a | b | c)) {
        atomicAdd(stats + 0, a);
        atomicAdd(stats + 1, b);
        atomicAdd(stats + 2, c);
        if (e) atomicAdd(stats + 3, e);
        if (f) atomicAdd(stats + 4, f);
        if (dr) atomicAdd(stats + 5, dr);
    }
}

// the sample the film takes from item i of a chunk (ProgressiveMonteCarloIntegrator::renderBlock clamp +
// ImageBlock::put validity check); false: put rejects it.  Shared by k_film and k_film_filtered.
__device__ __forceinline__ bool filmSample(const GParams &g, const SceneDev &sc, const PathDev &p, size_t i, float4 &L) {
    L = p.rad[i];
    if (sc.env && p.hit) L = envHitRadiance(L, p.hit[i]);  // surface path (volpath: no hit)
    float m = fmaxf(L.x, fmaxf(L.y, L.z));
    if (m > g.max_component_value) {
        float s = g.max_component_value / m;
        L.x *= s;
        L.y *= s;
        L.z *= s;
    }
    return isfinite(L.x) && isfinite(L.y) && isfinite(L.z) && L.x >= 0 && L.y >= 0 && L.z >= 0;
}

// film: box-filtered accumulation of every layer's sample into its pixel, in sample order
// TEX: textures are bound (pg_set_textures): the first-hit albedo of a textured material is the looked-up value.
// Scenes without textures launch k_film<false>, the kernel as it was.
template <bool TEX>
__global__ __launch_bounds__(256) void k_film(GParams g, SceneDev sc, PathDev p, const uint32_t *__restrict__ local_pixels,
                                              uint32_t pix_begin, uint32_t npix, uint32_t nlayers,
                                              float4 *__restrict__ film, float4 *__restrict__ sumsq,
                                              float4 *__restrict__ aov_albedo, float4 *__restrict__ aov_normal) {
    uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npix) return;
    uint32_t pix = local_pixels[pix_begin + lp];
    if (p.aov) {  // feature sums of every sample (Denoiser::add averages all of them, denoiser.cpp:138-144)
        float4 sa = aov_albedo[pix], sn = aov_normal[pix];
        for (uint32_t l = 0; l < nlayers; ++l) {
            const float4 hv = p.aov[(size_t)l * npix + lp];
            const uint32_t tri = __float_as_uint(hv.y);
            f3 a = mk1(0.f), n = mk(0.f, 0.f, -1.f);  // Denoiser::Sample defaults (denoiser.h:12-16): escaped ray
            if (tri != 0xFFFFFFFFu) {
                const float4 *r = sc.tshade + (size_t)PG_TRI_SHADE_STRIDE * tri;
                const float4 s1 = r[1], s3 = r[3], s4 = r[4];
                const float b0 = 1 - hv.z - hv.w;
                n = normalize(xyz(s3) * b0 + mk(s3.w, s4.x, s4.y) * hv.z + mk(s4.z, s4.w, s1.w) * hv.w);  // fetchHit's shN
                a = bsdfAlbedo(sc.mats[__float_as_uint(r[0].w) & 0xFFFFu]);
                if constexpr (TEX) {
                    const uint32_t mi = __float_as_uint(r[0].w) & 0xFFFFu, ti = sc.mtex[mi];
                    if (ti != 0xFFFFFFFFu) {  // a textured reflectance: the albedo of the looked-up value, as shadeOne's
                        GMat M = sc.mats[mi];
                        float tu, tv;
                        hitUV(sc, tri, hv.z, hv.w, tu, tv);
                        const f3 c = texEval(sc.tex[ti], tu, tv);
                        M.diff[0] = c.x;
                        M.diff[1] = c.y;
                        M.diff[2] = c.z;
                        a = bsdfAlbedo(M);
                    }
                }
            }
            sa = make_float4(sa.x + a.x, sa.y + a.y, sa.z + a.z, sa.w + 1.0f);
            sn = make_float4(sn.x + n.x, sn.y + n.y, sn.z + n.z, 0.0f);
        }
        aov_albedo[pix] = sa;
        aov_normal[pix] = sn;
    }
    float4 a = film[pix], q = sumsq[pix];
    for (uint32_t l = 0; l < nlayers; ++l) {
        float4 L;
        if (!filmSample(g, sc, p, (size_t)l * npix + lp, L)) continue;
        a.x += L.x;
        a.y += L.y;
        a.z += L.z;
        a.w += 1.0f;
        q.x += L.x * L.x;
        q.y += L.y * L.y;
        q.z += L.z * L.z;
    }
    film[pix] = a;
    sumsq[pix] = q;
}

// ---- reconstruction-filtered film (pg_set_rfilter): ImageBlock::put (imageblock.h:151-196) over the whole image
// with the filter's 32-entry table (rfilter.h:76-77), every tap added as a signed 2^-28 fixed-point integer, so
// the sums do not depend on the order, the chunking or the launch variant (pg_capi.h "filtered film").
// One tap's add: to the block's LDS tile when `lds` is set and the tap lies inside it, else to the global sums.
__device__ __forceinline__ void filterAdd(unsigned long long *acc, unsigned long long *lds, uint32_t width, int x, int y,
                                          int lx0, int ly0, int pw, int c, long long v) {
    if (v == 0) return;
    const int ix = x - lx0, iy = y - ly0;
    if (lds && ix >= 0 && iy >= 0 && ix < pw && iy < pw) atomicAdd(lds + (size_t)c * pw * pw + iy * pw + ix, (unsigned long long)v);
    else atomicAdd(acc + ((size_t)y * width + x) * 4 + c, (unsigned long long)v);
}
// one sample's splat; the jitter is the camera's (k_camera / volCamera: dimension 0 of the path's stream).
// Float32 without contraction, then exact products in double (pg_capi.h spells out each step).
__device__ __forceinline__ void filterSplat(const GParams &g, const FilmFilter &f, const float *tab, uint32_t pix,
                                            uint32_t sample, float4 L, unsigned long long *lds, int lx0, int ly0, int pw) {
#pragma clang fp contract(off)
    float jx, jy;
    rng2(rngKey(pix, g.seed), sample, 0, jx, jy);
    const float px = (float)(pix % g.width) + jx, py = (float)(pix / g.width) + jy;
    const float posx = px - 0.5f, posy = py - 0.5f;
    const int xa = max((int)ceilf(posx - f.radius), 0), xb = min((int)floorf(posx + f.radius), (int)g.width - 1);
    const int ya = max((int)ceilf(posy - f.radius), 0), yb = min((int)floorf(posy + f.radius), (int)g.height - 1);
    for (int y = ya; y <= yb; ++y) {
        const float wy = tab[(int)fminf(fabsf(((float)y - posy) * f.scale), 31.0f)];
        for (int x = xa; x <= xb; ++x) {
            const float wx = tab[(int)fminf(fabsf(((float)x - posx) * f.scale), 31.0f)];
            const float w = wx * wy;
            if (w == 0.0f) continue;  // every add would be an exact zero
            const double dw = (double)w;
            filterAdd(f.acc, lds, g.width, x, y, lx0, ly0, pw, 0, __double2ll_rn(dw * (double)L.x * 268435456.0));
            filterAdd(f.acc, lds, g.width, x, y, lx0, ly0, pw, 1, __double2ll_rn(dw * (double)L.y * 268435456.0));
            filterAdd(f.acc, lds, g.width, x, y, lx0, ly0, pw, 2, __double2ll_rn(dw * (double)L.z * 268435456.0));
            filterAdd(f.acc, lds, g.width, x, y, lx0, ly0, pw, 3, __double2ll_rn(dw * 268435456.0));
        }
    }
}
// LDS = true: block b takes the chunk's pixels of local tile tile0 + b for all the chunk's layers and stages its
// taps in a (tile + 2 border)^2 x 4 int64 tile (channel-major: neighbouring pixels' sums sit 8 B apart, so a
// wave's adds spread over the banks), then adds every non-zero entry to the global sums once.  A tap outside
// the padded tile (float rounding at pos +- radius can reach one pixel past the border) goes straight to the
// global sums.  LDS = false: one thread per sample and global adds only (tiles too large for 64 KiB of LDS).
template <bool LDS>
__global__ __launch_bounds__(256) void k_film_filtered(GParams g, SceneDev sc, PathDev p, FilmFilter f,
                                                       const uint32_t *__restrict__ local_pixels, uint32_t pix_begin,
                                                       uint32_t npix, uint32_t nlayers, uint32_t sample_base,
                                                       uint32_t tile0) {
    extern __shared__ unsigned long long tile_acc[];
    __shared__ float tab[32];
    if (threadIdx.x < 32) tab[threadIdx.x] = f.values[threadIdx.x];
    if (LDS) {
        const int pw = (int)f.tile + 2 * f.border, pp = pw * pw;
        for (int e = threadIdx.x; e < 4 * pp; e += blockDim.x) tile_acc[e] = 0;
        __syncthreads();
        const uint32_t t = tile0 + blockIdx.x;
        const uint32_t lo = max(f.tile_first[t], pix_begin), hi = min(f.tile_first[t + 1], pix_begin + npix);
        const uint32_t cnt = hi > lo ? hi - lo : 0;
        const uint2 org = f.tile_origin[t];
        const int lx0 = (int)org.x - f.border, ly0 = (int)org.y - f.border;
        for (uint32_t i = threadIdx.x; i < cnt * nlayers; i += blockDim.x) {
            const uint32_t layer = i / cnt, lp = (lo - pix_begin) + (i - layer * cnt);
            float4 L;
            if (!filmSample(g, sc, p, (size_t)layer * npix + lp, L)) continue;
            filterSplat(g, f, tab, local_pixels[pix_begin + lp], sample_base + layer, L, tile_acc, lx0, ly0, pw);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 4 * pp; e += blockDim.x) {
            const unsigned long long v = tile_acc[e];
            if (!v) continue;
            const int c = e / pp, q = e - c * pp, x = lx0 + q % pw, y = ly0 + q / pw;
            if (x >= 0 && y >= 0 && x < (int)g.width && y < (int)g.height)
                atomicAdd(f.acc + ((size_t)y * g.width + x) * 4 + c, v);
        }
    } else {
        __syncthreads();
        const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
        if (slot >= npix * nlayers) return;
        const uint32_t layer = slot / npix, lp = slot - layer * npix;
        float4 L;
        if (!filmSample(g, sc, p, slot, L)) return;
        filterSplat(g, f, tab, local_pixels[pix_begin + lp], sample_base + layer, L, nullptr, 0, 0, 0);
    }
}

// training records of finished paths: radiance along wo_i = (L_final - L_i) / T_i (channel-wise)
// env_hits: the surface path of a scene with an environment emitter (envHitRadiance)
__global__ __launch_bounds__(256) void k_commit(PathDev p, uint32_t nslots, int maxV, pg_record *__restrict__ recs,
                                                unsigned long long *__restrict__ rec_count,
                                                unsigned long long capacity, int env_hits) {
    uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nv = 0;
    if (slot < nslots) nv = min(p.vst ? pathInfo(p, slot)->w : __float_as_uint(p.rad[slot].w), (uint32_t)maxV);
    // wave inclusive scan of nv
    int lane = threadIdx.x & 63;
    uint32_t incl = nv;
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t y = __shfl_up(incl, off);
        if (lane >= off) incl += y;
    }
    uint32_t total = __shfl(incl, 63);
    unsigned long long base = 0;
    if (lane == 63 && total) base = atomicAdd(rec_count, (unsigned long long)total);
    base = __shfl(base, 63);
    if (nv == 0) return;
    unsigned long long o = base + (incl - nv);
    float4 L = p.rad[slot];
    if (env_hits) L = envHitRadiance(L, p.hit[slot]);
    for (uint32_t k = 0; k < nv; ++k, ++o) {
        if (o >= capacity) return;
        const float4 *vb = p.vtx + ((size_t)k * p.vtxP + slot) * PG_VTX_F4;
        float4 a = vb[0], b = vb[1], c = vb[2], e = vb[3];
        float woPdf = a.w;
        float lr = (b.x * woPdf > 1e-4f) ? (L.x - c.x) / b.x : 0.0f;
        float lg = (b.y * woPdf > 1e-4f) ? (L.y - c.y) / b.y : 0.0f;
        float lb = (b.z * woPdf > 1e-4f) ? (L.z - c.z) / b.z : 0.0f;
        // f L_i / woPdf per channel = (L_final - L_snapshot) / T_before (oracle: the same guards)
        float wr = (b.x * woPdf > 1e-4f) ? (L.x - c.x) / e.x : 0.0f;
        float wg = (b.y * woPdf > 1e-4f) ? (L.y - c.y) / e.y : 0.0f;
        float wb = (b.z * woPdf > 1e-4f) ? (L.z - c.z) / e.z : 0.0f;
        pg_record r;
        r.pos[0] = a.x;
        r.pos[1] = a.y;
        r.pos[2] = a.z;
        r.dir = __float_as_uint(b.w);
        r.radiance = (lr + lg + lb) * (1.0f / 3.0f);
        r.wo_pdf = woPdf;
        r.product = e.w >= 0.0f ? (wr + wg + wb) * (1.0f / 3.0f) : 0.0f;
        r.weight = e.w;
        float4 *dst = reinterpret_cast<float4 *>(recs + o);
        dst[0] = make_float4(r.pos[0], r.pos[1], r.pos[2], __uint_as_float(r.dir));
        dst[1] = make_float4(r.radiance, r.wo_pdf, r.product, r.weight);
    }
}

// SD-tree splat: records -> building-tree leaf quadrants (2^-24 fixed point, u64 atomics)
// Wave-aggregated atomic add: lanes with equal keys are summed in registers and one lane adds the
// sum.  Early training iterations splat ~1M records into a handful of D-tree nodes, where plain
// per-record atomics serialize on one address (53 ms for iteration 0).  Integer adds make the
// result independent of the grouping, so trees stay bit-identical.  Call with the whole wave active.
template <class T>
__device__ __forceinline__ void waveKeyedAdd(T *base, uint32_t key, T v, bool valid) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(valid);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t k = __shfl(key, leader);
        const bool mine = valid && key == k;
        const unsigned long long m = __ballot(mine);
        T sum = mine ? v : (T)0;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == leader) atomicAdd(base + k, sum);
        pending &= ~m;
    }
}

// the learned-fraction statistics of a wave's guided records: per group of lanes with one D-tree,
// kFracCandidates wave-summed fixed-point values and the group's record count, added by its leader
__device__ __forceinline__ void waveKeyedFracAdd(unsigned long long *base, uint32_t key, float w, float pb, float pg,
                                                 float q0, bool valid) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(valid);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t k = __shfl(key, leader);
        const bool mine = valid && key == k;
        const unsigned long long m = __ballot(mine);
        unsigned long long *dst = base + (size_t)k * (kFracCandidates + 1);
        for (int c = 0; c < kFracCandidates; ++c) {
            unsigned long long v = mine ? fracStat(w, pb, pg, q0, c) : 0ull;
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == leader) atomicAdd(dst + c, v);
        }
        if (lane == leader) atomicAdd(dst + kFracCandidates, (unsigned long long)__popcll(m));
        pending &= ~m;
    }
}

__global__ __launch_bounds__(256) void k_splat(SDDev sd, const pg_record *__restrict__ recs, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = i < n, found = false;
    unsigned long long fx = 0;
    uint32_t dt = 0, slot = 0;
    if (valid) {
        const float4 *src = reinterpret_cast<const float4 *>(recs + i);
        float4 a = src[0], b = src[1];
        float woPdf = b.y;
        float val = 0.0f;
        {
#pragma clang fp contract(off)
            if (woPdf > 0) val = b.x / woPdf;
        }
        valid = woPdf > 0 && val >= 0 && val < 1e30f;
        if (valid) {
            float s = val * 16777216.0f;
            // cap 2^48 (value <= 2^24; oracle kSplatCap).  A leaf quadrant's u64 atomic sum over all
            // records and ranks of an iteration wraps only past 2^40 value units (e.g. 2^16 records at
            // the cap); the host refit's interior sums saturate (pg_sdtree.cpp propagate)
            if (s >= 281474976710656.0f) s = 281474976710656.0f;
            fx = (unsigned long long)s;
            const SDView sv = sdv(sd);
            dt = sdLookup(sv, mk(a.x, a.y, a.z));
            uint32_t dirw = __float_as_uint(a.w);
            float u = ((float)(dirw & 0xFFFFu) + 0.5f) * (1.0f / 65536.0f);
            float v = ((float)(dirw >> 16) + 0.5f) * (1.0f / 65536.0f);
            uint32_t node = sd.meta[dt].y;
            for (int guard = 0; guard < 64; ++guard) {
                int q = childIndex(u, v);
                uint32_t c = c4(sd.bchild[node], q);
                if (c == 0) {
                    slot = 4 * node + q;
                    found = true;
                    break;
                }
                node = c;
            }
        }
    }
    waveKeyedAdd<unsigned long long>(sd.count, dt, 1ull, valid);
    waveKeyedAdd<unsigned long long>(sd.bsum, slot, fx, found);
    if (!sd.learned) return;
    // learned BSDF-sampling fraction (pg_device.h fracStat): a guided record (weight = p_guide >= 0)
    // with a contribution adds w log2(q_k / q0) for every candidate k, and 1 to its guided count.  p_bsdf
    // comes back from q0 = a0 p_bsdf + (1 - a0) p_guide with a0 the leaf's fraction that sampled it.
    bool stat = false;
    float w = 0, pb = 0, pg = 0, q0 = 0;
    if (valid) {
        const float4 b = reinterpret_cast<const float4 *>(recs + i)[1];
        pg = b.w;
        w = b.z;
        q0 = b.y;
        if (pg >= 0.0f && w > 0.0f && w < 1e30f) {
#pragma clang fp contract(off)
            const float la = __uint_as_float(sd.meta[dt].z);
            const float a0 = la > 0 ? la : sd.alpha0;
            pb = fmaxf((q0 - (1.0f - a0) * pg) / a0, 0.0f);
            stat = true;
        }
    }
    waveKeyedFracAdd(sd.frac, dt, w, pb, pg, q0, stat);
}

// Block-private splat (PG_SPLAT_LDS, default): a grid of at most ~1k blocks walks the records in
// block-strided rounds and sums the per-D-tree record counts and per-leaf-quadrant fixed-point values
// in two LDS hash tables (open addressing, 8 probes); keys that find no slot go straight to the global
// atomics.  Each block then adds its table entries to the global sums once.  A hot D-tree (one near
// the camera gets ~10 % of an iteration's records) thus costs one global atomic per block instead of
// one per wave.  Integer sums: the trees are bit-identical to the wave-aggregated k_splat.
// 1024 + 4096 entries (60 KiB, 2 blocks per CU): C3 W = 1 training 77 -> 70 ms against 512 + 2048
// (iteration 4's splat 7.5 -> 2.9 ms); 2048 + 8192 (1 block per CU) 74 ms (profiles/r03y_splat_tables_ab/)
#ifndef SPLAT_CNT_SLOTS
#define SPLAT_CNT_SLOTS 1024
#endif
#ifndef SPLAT_SUM_SLOTS
#define SPLAT_SUM_SLOTS 4096
#endif
#define SPLAT_EMPTY 0xFFFFFFFFu
__device__ __forceinline__ bool ldsTableAdd(uint32_t *keys, unsigned long long *vals, uint32_t mask, uint32_t key,
                                            unsigned long long v) {
    uint32_t h = (key * 2654435761u) >> 7;
    for (int probe = 0; probe < 8; ++probe, ++h) {
        h &= mask;
        uint32_t k = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
        if (k == SPLAT_EMPTY) k = atomicCAS(&keys[h], SPLAT_EMPTY, key);
        if (k == SPLAT_EMPTY || k == key) {
            atomicAdd(&vals[h], v);
            return true;
        }
    }
    return false;
}

__global__ __launch_bounds__(256) void k_splat_lds(SDDev sd, const pg_record *__restrict__ recs, unsigned long long n) {
    __shared__ uint32_t ckey[SPLAT_CNT_SLOTS], skey[SPLAT_SUM_SLOTS];
    __shared__ unsigned long long cval[SPLAT_CNT_SLOTS], sval[SPLAT_SUM_SLOTS];
    for (uint32_t e = threadIdx.x; e < SPLAT_SUM_SLOTS; e += blockDim.x) {
        skey[e] = SPLAT_EMPTY;
        sval[e] = 0;
        if (e < SPLAT_CNT_SLOTS) {
            ckey[e] = SPLAT_EMPTY;
            cval[e] = 0;
        }
    }
    __syncthreads();
    const SDView sv = sdv(sd);
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    // uniform trip count per block (waveKeyedFracAdd needs the whole wave)
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        bool valid = i < n, found = false;
        unsigned long long fx = 0;
        uint32_t dt = 0, slot = 0;
        float4 b = make_float4(0, 0, 0, 0);
        if (valid) {
            const float4 *src = reinterpret_cast<const float4 *>(recs + i);
            const float4 a = src[0];
            b = src[1];
            const float woPdf = b.y;
            float val = 0.0f;
            {
#pragma clang fp contract(off)
                if (woPdf > 0) val = b.x / woPdf;
            }
            valid = woPdf > 0 && val >= 0 && val < 1e30f;
            if (valid) {
                float s = val * 16777216.0f;
                if (s >= 281474976710656.0f) s = 281474976710656.0f;  // cap 2^48, as k_splat
                fx = (unsigned long long)s;
                dt = sdLookup(sv, mk(a.x, a.y, a.z));
                const uint32_t dirw = __float_as_uint(a.w);
                float u = ((float)(dirw & 0xFFFFu) + 0.5f) * (1.0f / 65536.0f);
                float v = ((float)(dirw >> 16) + 0.5f) * (1.0f / 65536.0f);
                uint32_t node = sd.meta[dt].y;
                for (int guard = 0; guard < 64; ++guard) {
                    const int q = childIndex(u, v);
                    const uint32_t c = c4(sd.bchild[node], q);
                    if (c == 0) {
                        slot = 4 * node + q;
                        found = true;
                        break;
                    }
                    node = c;
                }
            }
        }
        if (valid && !ldsTableAdd(ckey, cval, SPLAT_CNT_SLOTS - 1, dt, 1ull)) atomicAdd(sd.count + dt, 1ull);
        if (found && fx && !ldsTableAdd(skey, sval, SPLAT_SUM_SLOTS - 1, slot, fx)) atomicAdd(sd.bsum + slot, fx);
        if (sd.learned) {  // learned-fraction statistics as in k_splat (wave-aggregated global atomics)
            bool stat = false;
            float w = 0, pb = 0, pg = 0, q0 = 0;
            if (valid) {
                pg = b.w;
                w = b.z;
                q0 = b.y;
                if (pg >= 0.0f && w > 0.0f && w < 1e30f) {
#pragma clang fp contract(off)
                    const float la = __uint_as_float(sd.meta[dt].z);
                    const float a0 = la > 0 ? la : sd.alpha0;
                    pb = fmaxf((q0 - (1.0f - a0) * pg) / a0, 0.0f);
                    stat = true;
                }
            }
            waveKeyedFracAdd(sd.frac, dt, w, pb, pg, q0, stat);
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < SPLAT_SUM_SLOTS; e += blockDim.x) {
        if (skey[e] != SPLAT_EMPTY && sval[e]) atomicAdd(sd.bsum + skey[e], sval[e]);
        if (e < SPLAT_CNT_SLOTS && ckey[e] != SPLAT_EMPTY) atomicAdd(sd.count + ckey[e], cval[e]);
    }
}

// ---- unit-level kernels used by the parity tests ---------------------------------------------
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_rays(SceneDev sc, const float *__restrict__ rays, uint32_t n,
                                                            int any, float *__restrict__ hits, uint32_t *ovf) {
    __shared__ uint32_t stack[2 * WIDE_LDS_STACK * TRACE_BLOCK];  // >= LDS_STACK words per thread
    const TStack stk = threadStack(stack, ovf);
    const WStack wstk = threadWideStack(stack, ovf);
    uint32_t i = blockIdx.x * TRACE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + 8 * (size_t)i;
    f3 o = mk(r[0], r[1], r[2]), d = mk(r[4], r[5], r[6]);
    float tmax = r[7];
    uint32_t tri = 0xFFFFFFFFu;
    float u = 0, v = 0;
    float *h = hits + 4 * (size_t)i;
    if (any == 1) {
        bool occ = occluded(sc, o, d, r[3], tmax, wstk);
        h[0] = occ ? 1.0f : 0.0f;
        h[1] = h[2] = h[3] = 0.0f;
        return;
    }
    bool hit = traverse<false>(sc.nodes, sc.tris, o, d, r[3], tmax, tri, u, v, stk);
    if (any == 2) {  // pg_hit_records: the hit record the shading kernels build (fetchHit), 16 floats per ray
        float *q = hits + 16 * (size_t)i;
        if (!hit) {
            for (int k = 0; k < 16; ++k) q[k] = 0.0f;
            return;
        }
        Hit hr;
        fetchHit(sc, tri, u, v, d, hr);
        const float rec[16] = {hr.p.x,    hr.p.y,    hr.p.z,    tmax,       hr.geoN.x, hr.geoN.y, hr.geoN.z, hr.shN.x,
                               hr.shN.y,  hr.shN.z,  hr.sh.s.x, hr.sh.s.y,  hr.sh.s.z, hr.wi.x,   hr.wi.y,   hr.wi.z};
        for (int k = 0; k < 16; ++k) q[k] = rec[k];
        return;
    }
    uint32_t orig = hit ? __float_as_uint(sc.tshade[(size_t)PG_TRI_SHADE_STRIDE * tri + 2].w) : 0xFFFFFFFFu;
    h[0] = hit ? tmax : 0.0f;
    h[1] = __uint_as_float(orig);
    h[2] = u;
    h[3] = v;
}

// pg_texture_query: texEval on raw uv
__global__ __launch_bounds__(256) void k_texture_query(const GTex *tex, const float *__restrict__ uv, uint32_t n,
                                                       float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 c = texEval(*tex, uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
    out[3 * (size_t)i] = c.x;
    out[3 * (size_t)i + 1] = c.y;
    out[3 * (size_t)i + 2] = c.z;
}
// pg_hit_uvs: the closest hit's interpolated uv (hitUV), rows as k_trace_rays'
__global__ __launch_bounds__(TRACE_BLOCK) void k_hit_uvs(SceneDev sc, const float *__restrict__ rays, uint32_t n,
                                                         float *__restrict__ out, uint32_t *ovf) {
    __shared__ uint32_t stack[2 * WIDE_LDS_STACK * TRACE_BLOCK];  // >= LDS_STACK words per thread
    const TStack stk = threadStack(stack, ovf);
    const uint32_t i = blockIdx.x * TRACE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + 8 * (size_t)i;
    const f3 o = mk(r[0], r[1], r[2]), d = mk(r[4], r[5], r[6]);
    float tmax = r[7], u = 0, v = 0, tu = 0, tv = 0;
    uint32_t tri = 0xFFFFFFFFu;
    if (traverse<false>(sc.nodes, sc.tris, o, d, r[3], tmax, tri, u, v, stk)) hitUV(sc, tri, u, v, tu, tv);
    out[2 * (size_t)i] = tu;
    out[2 * (size_t)i + 1] = tv;
}
// pg_hit_frames: the frame the closest hit's BSDF calls run in and -d in it, as shadeOne forms them (fetchHit, then
// nmapFrame where the material carries a normal map); rows as k_trace_rays', 12 floats per ray, zeros for a miss
__global__ __launch_bounds__(TRACE_BLOCK) void k_hit_frames(SceneDev sc, const float *__restrict__ rays, uint32_t n,
                                                            float *__restrict__ out, uint32_t *ovf) {
    __shared__ uint32_t stack[2 * WIDE_LDS_STACK * TRACE_BLOCK];  // >= LDS_STACK words per thread
    const TStack stk = threadStack(stack, ovf);
    const uint32_t i = blockIdx.x * TRACE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + 8 * (size_t)i;
    const f3 o = mk(r[0], r[1], r[2]), d = mk(r[4], r[5], r[6]);
    float tmax = r[7], u = 0, v = 0;
    uint32_t tri = 0xFFFFFFFFu;
    float *f = out + 12 * (size_t)i;
    if (!traverse<false>(sc.nodes, sc.tris, o, d, r[3], tmax, tri, u, v, stk)) {
        for (int k = 0; k < 12; ++k) f[k] = 0.0f;
        return;
    }
    Hit h;
    fetchHit(sc, tri, u, v, d, h);
    if (nmapFrame(sc, tri, u, v, h.mat, h.shN, h.sh)) h.wi = h.sh.toLocal(-d);
    const f3 rows[4] = {h.sh.n, h.sh.s, h.sh.t, h.wi};
    for (int k = 0; k < 4; ++k) {
        f[3 * k] = rows[k].x;
        f[3 * k + 1] = rows[k].y;
        f[3 * k + 2] = rows[k].z;
    }
}

// pg_blocker_test: the shader's blocker test on given rays (rows as k_trace_rays')
__global__ __launch_bounds__(256) void k_blocker_test(SceneDev sc, const float *__restrict__ rays, uint32_t n,
                                                      uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + 8 * (size_t)i;
    const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]};
    out[i] = pg_ray_hits_blockers(sc.blk, sc.num_blockers, sc.absmax, o, d, r[3], r[7]) ? 1u : 0u;
}

// pg_occluder_test: the tracer's occluder test and the probe walk on given rays (rows as k_trace_rays'; tmin in [3]):
// out[2 i] = the test's answer, out[2 i + 1] = probeHit's
__global__ __launch_bounds__(TRACE_BLOCK) void k_occluder_test(SceneDev sc, const float *__restrict__ rays, uint32_t n,
                                                               uint32_t *__restrict__ out, uint32_t *ovf) {
    __shared__ uint32_t stack[LDS_STACK * TRACE_BLOCK];
    const TStack stk = threadStack(stack, ovf);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + 8 * (size_t)i;
    const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]};
    out[2 * (size_t)i] = pg_ray_hits_occluders(sc.prb, sc.num_occluders, sc.absmax, o, d, fabsf(r[3])) ? 1u : 0u;
    out[2 * (size_t)i + 1] = probeHit(sc, make_float4(r[0], r[1], r[2], r[3]), make_float4(r[4], r[5], r[6], 0.0f), stk) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_bsdf_query(const GMat *mat, const float *wi, const float *u, const float *wog,
                                                    uint32_t n, float *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GMat M = *mat;
    f3 w = mk(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]);
    BS bs;
    f3 wt = bsdfSample(M, w, u[3 * i], u[3 * i + 1], u[3 * i + 2], bs);
    float *o = out + 12 * (size_t)i;
    bool z = isZero(wt);
    o[0] = bs.wo.x;
    o[1] = bs.wo.y;
    o[2] = bs.wo.z;
    o[3] = z ? 0.0f : bs.pdf;
    o[4] = wt.x;
    o[5] = wt.y;
    o[6] = wt.z;
    o[7] = z ? 0.0f : (float)bs.type;
    if (wog) {
        f3 g = mk(wog[3 * i], wog[3 * i + 1], wog[3 * i + 2]);
        f3 e = bsdfEval(M, w, g);
        o[8] = e.x;
        o[9] = e.y;
        o[10] = e.z;
        o[11] = bsdfPdf(M, w, g);
    } else {
        o[8] = o[9] = o[10] = o[11] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_sd_pdf(SDDev sd, const float *pos, const float *dir, uint32_t n, float *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SDView sv = sdv(sd);
    uint4 meta = sd.meta[sdLookup(sv, mk(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]))];
    out[i] = sdPdf(sv, meta, mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]));
}

__global__ __launch_bounds__(256) void k_sd_sample(SDDev sd, const float *pos, const float *u, uint32_t n, float *dir,
                                                   float *pdf) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SDView sv = sdv(sd);
    uint4 meta = sd.meta[sdLookup(sv, mk(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]))];
    float cu, cv, pd;
    sdSampleCanon(sv, meta, u[2 * i], u[2 * i + 1], cu, cv, pd);
    f3 d = canonicalToDir(cu, cv);
    dir[3 * i] = d.x;
    dir[3 * i + 1] = d.y;
    dir[3 * i + 2] = d.z;
    pdf[i] = pd;
}

// =============================================================================================
static inline uint32_t blocks(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

size_t pg_stack_overflow_words(uint64_t max_threads) {
    if (max_threads == 0) max_threads = (uint64_t)TRACE_MAX_BLOCKS * TRACE_BLOCK;
    const size_t words = std::max<size_t>(std::max(STACK_DEPTH, PG_QSTACK_DEPTH) - LDS_STACK,
                                          2 * (STACK_DEPTH - WIDE_LDS_STACK));
    return words * max_threads;
}
// threads k_trace_rays launches for n rays: its overflow stride is gridDim.x * TRACE_BLOCK
uint64_t pg_trace_rays_threads(uint64_t n) { return (uint64_t)blocks(n, TRACE_BLOCK) * TRACE_BLOCK; }

void pg_launch_camera(hipStream_t s, const GParams &g, const PathDev &p, const uint32_t *local_pixels,
                      uint32_t pix_begin, uint32_t npix, uint32_t nlayers, uint32_t sample_base, Queue q, bool banded) {
    uint64_t n = (uint64_t)npix * nlayers;
    if (!n) return;
    if (g.lens_radius > 0)
        hipLaunchKernelGGL(k_camera<true>, dim3(blocks(n, 256)), dim3(256), 0, s, g, p, local_pixels, pix_begin, npix,
                           nlayers, sample_base, q, pg_camera_banded(banded, npix));
    else
        hipLaunchKernelGGL(k_camera<false>, dim3(blocks(n, 256)), dim3(256), 0, s, g, p, local_pixels, pix_begin, npix,
                           nlayers, sample_base, q, pg_camera_banded(banded, npix));
}
// pg_camera_rays: cameraRay for given (global pixel, sample) pairs; out: (o, tmin) and (d, tmax) per pair
template <bool LENS>
__global__ __launch_bounds__(256) void k_camera_rays(GParams g, const uint32_t *__restrict__ pixels,
                                                     const uint32_t *__restrict__ samples, uint32_t n,
                                                     float4 *__restrict__ o_tmin, float4 *__restrict__ d_tmax) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t pix = pixels[i];
    f3 o, wd;
    float tmin, tmax;
    cameraRay<LENS>(g, pix, rngKey(pix, g.seed), samples[i], o, wd, tmin, tmax);
    o_tmin[i] = f4(o, tmin);
    d_tmax[i] = f4(wd, tmax);
}
void pg_launch_camera_rays(hipStream_t s, const GParams &g, const uint32_t *pixels, const uint32_t *samples, uint32_t n,
                           float *o_tmin, float *d_tmax) {
    if (!n) return;
    float4 *o = reinterpret_cast<float4 *>(o_tmin), *d = reinterpret_cast<float4 *>(d_tmax);
    if (g.lens_radius > 0)
        hipLaunchKernelGGL(k_camera_rays<true>, dim3(blocks(n, 256)), dim3(256), 0, s, g, pixels, samples, n, o, d);
    else
        hipLaunchKernelGGL(k_camera_rays<false>, dim3(blocks(n, 256)), dim3(256), 0, s, g, pixels, samples, n, o, d);
}
// grid of a sharded launch: PG_QSHARDS x rows (rows capped for persistent grid-stride kernels)
static inline dim3 shardGrid(uint32_t max_shard, uint32_t block, uint32_t max_rows) {
    const uint32_t rows = blocks(max_shard, block);
    return dim3(PG_QSHARDS * (rows < max_rows ? rows : max_rows));
}
void pg_launch_trace(hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p, Queue q, uint32_t max_shard,
                     const Queue *class_queues, bool first_bounce) {
    if (!max_shard) return;
    ClassQueues cq;
    for (int c = 0; c < PG_CLASS_ROWS; ++c) cq.q[c] = class_queues[c];
    const dim3 grid = shardGrid(max_shard, TRACE_BLOCK, TRACE_MAX_BLOCKS / PG_QSHARDS);
    float4 *first = first_bounce ? p.aov : nullptr;
    // the chunk's first launch traces k_camera's rows, every later one shadeOne's (pg_layout.h "Path state")
    if (first_bounce) {
        if (sc.env) hipLaunchKernelGGL((k_trace<true, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, p, q, cq, first);
        else hipLaunchKernelGGL((k_trace<false, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, p, q, cq, first);
    } else {
        if (sc.env) hipLaunchKernelGGL((k_trace<true, false>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, p, q, cq, first);
        else hipLaunchKernelGGL((k_trace<false, false>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, p, q, cq, first);
    }
}
void pg_launch_camera_trace(hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p,
                            const uint32_t *local_pixels, uint32_t pix_begin, uint32_t npix, uint32_t nlayers,
                            uint32_t sample_base, const Queue *class_queues) {
    const uint32_t max_shard = pg_camera_bound(false, npix, nlayers);
    if (!max_shard) return;
    ClassQueues cq;
    for (int c = 0; c < PG_CLASS_ROWS; ++c) cq.q[c] = class_queues[c];
    const dim3 grid = shardGrid(max_shard, TRACE_BLOCK, TRACE_MAX_BLOCKS / PG_QSHARDS), block(TRACE_BLOCK);
    const CameraChunk cam{local_pixels, pix_begin, npix, nlayers, sample_base};
    const bool lens = g.lens_radius > 0;
    if (sc.env) {
        if (lens) hipLaunchKernelGGL((k_camera_trace<true, true>), grid, block, 0, s, g, sc, p, cam, cq, p.aov);
        else hipLaunchKernelGGL((k_camera_trace<true, false>), grid, block, 0, s, g, sc, p, cam, cq, p.aov);
    } else {
        if (lens) hipLaunchKernelGGL((k_camera_trace<false, true>), grid, block, 0, s, g, sc, p, cam, cq, p.aov);
        else hipLaunchKernelGGL((k_camera_trace<false, false>), grid, block, 0, s, g, sc, p, cam, cq, p.aov);
    }
}
void pg_launch_camera_queue(hipStream_t s, uint32_t npix, uint32_t nlayers, Queue q) {
    const uint64_t n = (uint64_t)npix * nlayers;
    if (!n) return;
    hipLaunchKernelGGL(k_camera_queue, dim3(blocks(n, 256)), dim3(256), 0, s, (uint32_t)n, q);
}
template <bool ENV, bool DELTA>
static void launchShade(hipStream_t s, int cls, dim3 grid, const GParams &g, const SceneDev &sc, const SDDev &sd,
                        const PathDev &p, Queue in, Queue out, Queue shq, Queue pq) {
    const dim3 block(SHADE_BLOCK);
    switch (cls) {
        case PG_CLASS_DIFFUSE:
            hipLaunchKernelGGL((k_shade<PG_BSDF_DIFFUSE, true, ENV, false, DELTA>), grid, block, 0, s, g, sc, sd, p, in, out, shq, pq);
            break;
        case PG_CLASS_ROUGHCONDUCTOR:
            hipLaunchKernelGGL((k_shade<PG_BSDF_ROUGHCONDUCTOR, true, ENV, false, DELTA>), grid, block, 0, s, g, sc, sd, p, in, out, shq, pq);
            break;
        case PG_CLASS_ROUGHDIELECTRIC:
            hipLaunchKernelGGL((k_shade<PG_BSDF_ROUGHDIELECTRIC, true, ENV, false, DELTA>), grid, block, 0, s, g, sc, sd, p, in, out, shq, pq);
            break;
        case PG_CLASS_PLASTIC:
            hipLaunchKernelGGL((k_shade<PG_BSDF_PLASTIC, false, ENV, false, DELTA>), grid, block, 0, s, g, sc, sd, p, in, out, shq, pq);
            break;
        case PG_CLASS_ROUGHPLASTIC:
            hipLaunchKernelGGL((k_shade<PG_BSDF_ROUGHPLASTIC, true, ENV, false, DELTA>), grid, block, 0, s, g, sc, sd, p, in, out, shq, pq);
            break;
        case PG_CLASS_TEXTURED:  // a textured diffuse reflectance (diffuse, plastic, roughplastic at run time)
            hipLaunchKernelGGL((k_shade<PG_MODELS_TEXTURED, true, ENV, true, DELTA>), grid, block, 0, s, g, sc, sd, p, in, out, shq, pq);
            break;
        default:  // delta lobes: conductor, dielectric (runtime switch, never guided)
            hipLaunchKernelGGL((k_shade<-1, false, ENV, false, DELTA>), grid, block, 0, s, g, sc, sd, p, in, out, shq, pq);
    }
}
void pg_launch_shade_class(hipStream_t s, int cls, const GParams &g, const SceneDev &sc, const SDDev &sd,
                           const PathDev &p, Queue in, uint32_t max_shard, Queue out, Queue shq, Queue pq) {
    if (!max_shard) return;
    const dim3 grid = shardGrid(max_shard, SHADE_BLOCK, 0xFFFFFFFFu);
    // sc.delta: delta emitters are set (pg_set_delta_emitters); scenes without them launch the kernels they always did
    if (sc.delta) {
        if (sc.env) launchShade<true, true>(s, cls, grid, g, sc, sd, p, in, out, shq, pq);
        else launchShade<false, true>(s, cls, grid, g, sc, sd, p, in, out, shq, pq);
    } else if (sc.env) launchShade<true, false>(s, cls, grid, g, sc, sd, p, in, out, shq, pq);
    else launchShade<false, false>(s, cls, grid, g, sc, sd, p, in, out, shq, pq);
}
void pg_launch_shade_all(hipStream_t s, const GParams &g, const SceneDev &sc, const SDDev &sd, const PathDev &p,
                         const Queue *class_queues, const uint32_t *max_shard, Queue out, Queue shq, Queue pq) {
    ClassQueues cq;
    ShadeRanges r;
    uint32_t total = 0;
    for (int c = 0; c < PG_NUM_CLASSES; ++c) {
        cq.q[c] = class_queues[c];
        total += max_shard[c] ? shardGrid(max_shard[c], SHADE_BLOCK, 0xFFFFFFFFu).x : 0;
        r.end[c] = total;
    }
    for (int c = PG_NUM_CLASSES; c < PG_CLASS_ROWS; ++c) cq.q[c] = class_queues[c];
    if (!total) return;
    if (sc.delta) {
        if (sc.mtex) hipLaunchKernelGGL((k_shade_all<true, true>), dim3(total), dim3(SHADE_BLOCK), 0, s, g, sc, sd, p, cq, out, shq, pq, r);
        else hipLaunchKernelGGL((k_shade_all<false, true>), dim3(total), dim3(SHADE_BLOCK), 0, s, g, sc, sd, p, cq, out, shq, pq, r);
    } else if (sc.mtex) hipLaunchKernelGGL(k_shade_all<true>, dim3(total), dim3(SHADE_BLOCK), 0, s, g, sc, sd, p, cq, out, shq, pq, r);
    else hipLaunchKernelGGL(k_shade_all<false>, dim3(total), dim3(SHADE_BLOCK), 0, s, g, sc, sd, p, cq, out, shq, pq, r);
}
// the recording passes count shadow blockers (sc.blk_counts is set only for them, never with an environment emitter)
static inline bool blockersCounted(const GParams &g, const SceneDev &sc) { return g.record && sc.blk_counts && !sc.env; }
// ... and the probe rows their occluders (sc.prb_counts, set as blk_counts is).  k_rays<false, true> serves either, so
// its rows check their own pointer.
static inline bool probesCounted(const SceneDev &sc) { return sc.prb_counts && !sc.env; }
void pg_launch_rays(hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p, Queue q, uint32_t max_shard,
                    const Queue *class_queues, Queue shq, uint32_t max_shadow_shard, Queue pq) {
    ClassQueues cq;
    for (int c = 0; c < PG_CLASS_ROWS; ++c) cq.q[c] = class_queues[c];
    const uint32_t sb = max_shadow_shard ? shardGrid(max_shadow_shard, TRACE_BLOCK, TRACE_MAX_BLOCKS / PG_QSHARDS).x : 0;
    const bool count = blockersCounted(g, sc), pcount = probesCounted(sc);
    // the probe queue's shards are bounded as the shadow queue's (both hold vertices of the bounce just shaded)
    const uint32_t pb = (g.doom_probe && !sc.env) ? sb : 0;
    const uint32_t tb =
        max_shard ? shardGrid(max_shard, TRACE_BLOCK, TRACE_MAX_BLOCKS / PG_QSHARDS).x : 0;
    if (sb + tb == 0) return;
    if (tb == 0) {  // no trace rows: k_rays needs at least one trace block per shard to stay sharded
        if (count) hipLaunchKernelGGL(k_shadow<true>, dim3(sb), dim3(TRACE_BLOCK), 0, s, sc, p, shq);
        else hipLaunchKernelGGL(k_shadow<false>, dim3(sb), dim3(TRACE_BLOCK), 0, s, sc, p, shq);
        if (pb && pcount) hipLaunchKernelGGL(k_probe<true>, dim3(pb), dim3(TRACE_BLOCK), 0, s, sc, p, pq, cq);
        else if (pb) hipLaunchKernelGGL(k_probe<false>, dim3(pb), dim3(TRACE_BLOCK), 0, s, sc, p, pq, cq);
        return;
    }
    // sb + tb + pb <= 3 TRACE_MAX_BLOCKS: the overflow ring's size (pg_host.cpp ensurePaths)
    if (sc.env) hipLaunchKernelGGL(k_rays<true>, dim3(sb + tb + pb), dim3(TRACE_BLOCK), 0, s, g, sc, p, q, cq, shq, sb, pq, pb);
    else if (count || pcount) hipLaunchKernelGGL((k_rays<false, true>), dim3(sb + tb + pb), dim3(TRACE_BLOCK), 0, s, g, sc, p, q, cq, shq, sb, pq, pb);
    else hipLaunchKernelGGL(k_rays<false>, dim3(sb + tb + pb), dim3(TRACE_BLOCK), 0, s, g, sc, p, q, cq, shq, sb, pq, pb);
}
void pg_launch_probe(hipStream_t s, const SceneDev &sc, const PathDev &p, Queue pq, uint32_t max_shard,
                     const Queue *class_queues) {
    if (!max_shard) return;
    ClassQueues cq;
    for (int c = 0; c < PG_CLASS_ROWS; ++c) cq.q[c] = class_queues[c];
    const dim3 grid = shardGrid(max_shard, TRACE_BLOCK, TRACE_MAX_BLOCKS / PG_QSHARDS);
    if (probesCounted(sc)) hipLaunchKernelGGL(k_probe<true>, grid, dim3(TRACE_BLOCK), 0, s, sc, p, pq, cq);
    else hipLaunchKernelGGL(k_probe<false>, grid, dim3(TRACE_BLOCK), 0, s, sc, p, pq, cq);
}
void pg_launch_shadow(hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p, Queue q, uint32_t max_shard) {
    if (!max_shard) return;
    const dim3 grid = shardGrid(max_shard, TRACE_BLOCK, TRACE_MAX_BLOCKS / PG_QSHARDS);
    if (blockersCounted(g, sc)) hipLaunchKernelGGL(k_shadow<true>, grid, dim3(TRACE_BLOCK), 0, s, sc, p, q);
    else hipLaunchKernelGGL(k_shadow<false>, grid, dim3(TRACE_BLOCK), 0, s, sc, p, q);
}
void pg_launch_tail(hipStream_t s, const GParams &g, const SceneDev &sc, const SDDev &sd, const PathDev &p, Queue q,
                    uint32_t max_shard, unsigned long long *stats) {
    if (!max_shard) return;
    // at most TRACE_MAX_BLOCKS blocks (a grid-stride loop over each shard): the traversal stacks' overflow
    // ring (threadStack / threadWideStack, stride gridDim.x * TRACE_BLOCK) holds that many threads
    const dim3 grid = shardGrid(max_shard, TRACE_BLOCK, TRACE_MAX_BLOCKS / PG_QSHARDS);
    if (sc.delta) {  // delta emitters set: the instantiations with their NEE compiled in
        const bool count = blockersCounted(g, sc);
        if (sc.mtex) {
            if (sc.env) hipLaunchKernelGGL((k_tail<true, false, true, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
            else if (count) hipLaunchKernelGGL((k_tail<false, true, true, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
            else hipLaunchKernelGGL((k_tail<false, false, true, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
        } else if (sc.env) hipLaunchKernelGGL((k_tail<true, false, false, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
        else if (count) hipLaunchKernelGGL((k_tail<false, true, false, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
        else hipLaunchKernelGGL((k_tail<false, false, false, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
        return;
    }
    if (sc.mtex) {  // textures bound: the instantiations with the textured class' body
        if (sc.env) hipLaunchKernelGGL((k_tail<true, false, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
        else if (blockersCounted(g, sc)) hipLaunchKernelGGL((k_tail<false, true, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
        else hipLaunchKernelGGL((k_tail<false, false, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
        return;
    }
    if (sc.env) hipLaunchKernelGGL(k_tail<true>, grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
    else if (blockersCounted(g, sc)) hipLaunchKernelGGL((k_tail<false, true>), grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
    else hipLaunchKernelGGL(k_tail<false>, grid, dim3(TRACE_BLOCK), 0, s, g, sc, sd, p, q, stats);
}
template <uint32_t BINS>
static void raySort(hipStream_t s, Queue q, uint32_t max_shard, uint32_t *sorted_items, uint32_t *hist) {
    (void)hipMemsetAsync(hist, 0, (size_t)PG_QSHARDS * BINS * 4, s);
    const dim3 grid(PG_QSHARDS * blocks(max_shard, RSORT_TILE));
    hipLaunchKernelGGL(k_rsort_hist<BINS>, grid, dim3(256), 0, s, q, hist);
    hipLaunchKernelGGL(k_rsort_scan<BINS>, dim3(PG_QSHARDS), dim3(256), 0, s, hist);
    hipLaunchKernelGGL(k_rsort_scatter<BINS>, grid, dim3(256), 0, s, q, hist, sorted_items);
}
void pg_launch_ray_sort(hipStream_t s, Queue q, uint32_t max_shard, uint32_t *sorted_items, uint32_t *hist,
                        uint32_t bins) {
    if (!max_shard) return;
    if (bins == 512) raySort<512>(s, q, max_shard, sorted_items, hist);
    else raySort<PG_RAY_SORT_BINS>(s, q, max_shard, sorted_items, hist);
}
void pg_launch_film(hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p, const uint32_t *local_pixels, uint32_t pix_begin,
                    uint32_t npix, uint32_t nlayers, float4 *film_rgbw, float4 *film_sumsq, float4 *aov_albedo,
                    float4 *aov_normal) {
    if (!npix) return;
    if (sc.mtex)
        hipLaunchKernelGGL(k_film<true>, dim3(blocks(npix, 256)), dim3(256), 0, s, g, sc, p, local_pixels, pix_begin, npix,
                           nlayers, film_rgbw, film_sumsq, aov_albedo, aov_normal);
    else
        hipLaunchKernelGGL(k_film<false>, dim3(blocks(npix, 256)), dim3(256), 0, s, g, sc, p, local_pixels, pix_begin, npix,
                           nlayers, film_rgbw, film_sumsq, aov_albedo, aov_normal);
}
void pg_launch_film_filtered(hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p, const FilmFilter &f,
                             const uint32_t *local_pixels, uint32_t pix_begin, uint32_t npix, uint32_t nlayers,
                             uint32_t sample_base, uint32_t tile0, uint32_t ntiles) {
    if (!npix || !nlayers) return;
    if (ntiles) {  // the LDS tile; the caller checked pg_film_filter_lds_bytes against the 64 KiB limit
        hipLaunchKernelGGL(k_film_filtered<true>, dim3(ntiles), dim3(256), pg_film_filter_lds_bytes(f.tile, f.border), s, g,
                           sc, p, f, local_pixels, pix_begin, npix, nlayers, sample_base, tile0);
    } else {
        hipLaunchKernelGGL(k_film_filtered<false>, dim3(blocks(npix * nlayers, 256)), dim3(256), 0, s, g, sc, p, f,
                           local_pixels, pix_begin, npix, nlayers, sample_base, 0u);
    }
}

// op 0: sampleDirect from the bounding-sphere centre (in: n x 2 samples; out n x 8: d, pdf, value/pdf, dist)
// op 1: pdfDirect (in: n x 3 world directions; out n); op 2: evalEnvironment (in n x 3; out n x 3)
__global__ __launch_bounds__(256) void k_envmap_query(SceneDev sc, int op, const float *in, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !sc.env) return;
    const GEnv &e = *sc.env;
    if (op == 0) {
        f3 d = mk1(0.f);
        float dist = 0, pdf;
        const f3 v = envSampleDirect(e, mk(e.center[0], e.center[1], e.center[2]), in[2 * i], in[2 * i + 1], d, dist, pdf);
        float *o = out + 8 * (size_t)i;
        o[0] = d.x;
        o[1] = d.y;
        o[2] = d.z;
        o[3] = pdf;
        o[4] = v.x;
        o[5] = v.y;
        o[6] = v.z;
        o[7] = dist;
    } else if (op == 1) {
        out[i] = envPdf(e, mk(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
    } else {
        const f3 v = envEval(e, mk(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
        out[3 * (size_t)i] = v.x;
        out[3 * (size_t)i + 1] = v.y;
        out[3 * (size_t)i + 2] = v.z;
    }
}
void pg_launch_envmap_query(hipStream_t s, const SceneDev &sc, int op, const float *in, uint32_t n, float *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_envmap_query, dim3(blocks(n, 256)), dim3(256), 0, s, sc, op, in, n, out);
}
// unit-level emitter sampling (pg_emitter_query): the shaders' sampleEmitter over the scene's whole emitter set at
// ref[i] with refN = 0; out n x 8: d, dist, value / pdf, measure (0 failed, 1 solid angle, 2 discrete)
template <bool ENV>
__global__ __launch_bounds__(256) void k_emitter_query(GParams g, SceneDev sc, const float *ref, const float *smp, uint32_t n,
                                                       float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f3 d = mk1(0.f);
    float dist = 0, pdf;
    bool discrete = false;
    const f3 v = sampleEmitter<ENV, true>(g, sc, mk(ref[3 * (size_t)i], ref[3 * (size_t)i + 1], ref[3 * (size_t)i + 2]), mk1(0.f),
                                          smp[2 * (size_t)i], smp[2 * (size_t)i + 1], d, dist, pdf, nullptr, &discrete);
    const bool ok = pdf != 0 && !isZero(v);
    float *o = out + 8 * (size_t)i;
    o[0] = ok ? d.x : 0.0f;
    o[1] = ok ? d.y : 0.0f;
    o[2] = ok ? d.z : 0.0f;
    o[3] = ok ? dist : 0.0f;
    o[4] = ok ? v.x : 0.0f;
    o[5] = ok ? v.y : 0.0f;
    o[6] = ok ? v.z : 0.0f;
    o[7] = !ok ? 0.0f : discrete ? 2.0f : 1.0f;
}
void pg_launch_emitter_query(hipStream_t s, const GParams &g, const SceneDev &sc, const float *ref, const float *smp,
                             uint32_t n, float *out) {
    if (!n) return;
    if (sc.env) hipLaunchKernelGGL(k_emitter_query<true>, dim3(blocks(n, 256)), dim3(256), 0, s, g, sc, ref, smp, n, out);
    else hipLaunchKernelGGL(k_emitter_query<false>, dim3(blocks(n, 256)), dim3(256), 0, s, g, sc, ref, smp, n, out);
}
void pg_launch_commit(hipStream_t s, const PathDev &p, uint32_t nslots, int max_vertices, pg_record *records,
                      unsigned long long *rec_count, unsigned long long rec_capacity, int env_hits) {
    if (!nslots) return;
    hipLaunchKernelGGL(k_commit, dim3(blocks(nslots, 256)), dim3(256), 0, s, p, nslots, max_vertices, records, rec_count,
                       rec_capacity, env_hits);
}
// the host's fillJump (pg_sdtree.cpp) per cell: level d splits axis d % 3 by bit (bits - 1 - d / 3) of
// the cell's coordinate on that axis
__global__ __launch_bounds__(256) void k_sd_jump(const uint2 *__restrict__ snodes, int bits, uint32_t *__restrict__ jump) {
    const uint32_t R = 1u << bits, cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= R * R * R) return;
    const uint32_t xyz[3] = {cell % R, (cell / R) % R, cell / (R * R)};
    uint32_t n = 0;
    for (int d = 0; d < 3 * bits; ++d) {
        const uint2 nd = snodes[n];
        if (nd.x == 0xFFFFFFFFu) break;
        n = ((xyz[d % 3] >> (bits - 1 - d / 3)) & 1u) ? nd.y : nd.x;
    }
    // a cell inside one leaf holds the leaf's D-tree id, flagged (pg_device.h sdLookup: one load, not two)
    const uint2 nd = snodes[n];
    jump[cell] = nd.x == 0xFFFFFFFFu ? (0x80000000u | nd.y) : n;
}
void pg_launch_sd_jump(hipStream_t s, const uint32_t *snodes, int bits, uint32_t *jump) {
    const uint32_t n = 1u << (3 * bits);
    hipLaunchKernelGGL(k_sd_jump, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint2 *>(snodes), bits,
                       jump);
}
void pg_launch_splat(hipStream_t s, const SDDev &sd, const pg_record *recs, unsigned long long n) {
    if (!n) return;
    static const bool lds = [] {
        const char *e = std::getenv("PG_SPLAT_LDS");
        return !e || std::atoi(e) != 0;
    }();
    if (lds) {  // ~16 records per thread, at most 1024 blocks (4 per CU)
        const unsigned long long nb = std::min<unsigned long long>(1024, std::max<unsigned long long>(1, n / 4096));
        hipLaunchKernelGGL(k_splat_lds, dim3((uint32_t)nb), dim3(256), 0, s, sd, recs, n);
    } else {
        hipLaunchKernelGGL(k_splat, dim3(blocks(n, 256)), dim3(256), 0, s, sd, recs, n);
    }
}
void pg_launch_trace_rays(hipStream_t s, const SceneDev &sc, const float *rays, uint32_t n, int any, float *hits,
                          uint32_t *ovf) {
    if (!n) return;
    hipLaunchKernelGGL(k_trace_rays, dim3(blocks(n, TRACE_BLOCK)), dim3(TRACE_BLOCK), 0, s, sc, rays, n, any, hits, ovf);
}
void pg_launch_texture_query(hipStream_t s, const GTex *tex, const float *uv, uint32_t n, float *out) {
    if (n) hipLaunchKernelGGL(k_texture_query, dim3(blocks(n, 256)), dim3(256), 0, s, tex, uv, n, out);
}
void pg_launch_hit_uvs(hipStream_t s, const SceneDev &sc, const float *rays, uint32_t n, float *out, uint32_t *ovf) {
    if (n) hipLaunchKernelGGL(k_hit_uvs, dim3(blocks(n, TRACE_BLOCK)), dim3(TRACE_BLOCK), 0, s, sc, rays, n, out, ovf);
}
void pg_launch_hit_frames(hipStream_t s, const SceneDev &sc, const float *rays, uint32_t n, float *out, uint32_t *ovf) {
    if (n) hipLaunchKernelGGL(k_hit_frames, dim3(blocks(n, TRACE_BLOCK)), dim3(TRACE_BLOCK), 0, s, sc, rays, n, out, ovf);
}
void pg_launch_blocker_test(hipStream_t s, const SceneDev &sc, const float *rays, uint32_t n, uint32_t *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_blocker_test, dim3(blocks(n, 256)), dim3(256), 0, s, sc, rays, n, out);
}
// n rays in blocks(n, TRACE_BLOCK) blocks, as k_trace_rays: ovf holds pg_stack_overflow_words(pg_trace_rays_threads(n))
void pg_launch_occluder_test(hipStream_t s, const SceneDev &sc, const float *rays, uint32_t n, uint32_t *out, uint32_t *ovf) {
    if (!n) return;
    hipLaunchKernelGGL(k_occluder_test, dim3(blocks(n, TRACE_BLOCK)), dim3(TRACE_BLOCK), 0, s, sc, rays, n, out, ovf);
}
void pg_launch_bsdf_query(hipStream_t s, const GMat *mat, const float *wi, const float *u, const float *wog, uint32_t n,
                          float *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_bsdf_query, dim3(blocks(n, 256)), dim3(256), 0, s, mat, wi, u, wog, n, out);
}
void pg_launch_sd_pdf(hipStream_t s, const SDDev &sd, const float *pos, const float *dir, uint32_t n, float *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_sd_pdf, dim3(blocks(n, 256)), dim3(256), 0, s, sd, pos, dir, n, out);
}
void pg_launch_sd_sample(hipStream_t s, const SDDev &sd, const float *pos, const float *u, uint32_t n, float *dir,
                         float *pdf) {
    if (!n) return;
    hipLaunchKernelGGL(k_sd_sample, dim3(blocks(n, 256)), dim3(256), 0, s, sd, pos, u, n, dir, pdf);
}
