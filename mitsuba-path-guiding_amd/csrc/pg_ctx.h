// Internal host header: the device context behind the C-ABI (include/pg_capi.h) and what the pass
// drivers (pg_pass.cpp) need from the context side (pg_host.cpp).  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/pg_capi.h"
#include "pg_kernels.h"
#include "pg_layout.h"
#include "pg_sdtree.h"

namespace pgh __attribute__((visibility("hidden"))) {  // the library exports the pg_* entry points only

constexpr uint32_t kMaxBounces = 1100;     // > gpu_depth_cap default (1024) + 2
// per-bounce device counters (words): [0, 64) shard counts of the live queue entering the bounce,
// [64, 128) shadow-queue shard counts, [128, 704) shard counts of the PG_NUM_CLASSES material-class
// queues followed by the escaped-ray and the culled-hit counts (PG_CLASS_ROWS rows), [704, 768) shard counts of the
// probe queue the bounce's shading fills (pg_layout.h "Doom probe"), [768, 832) the dropped shadow rays, [832, 896) the
// probes of that queue resolved against the occluder list
constexpr uint32_t kBounceWords = 896;
constexpr uint32_t kShadowCounts = PG_QSHARDS, kClassCounts = 2 * PG_QSHARDS;
constexpr uint32_t kProbeCounts = kClassCounts + PG_CLASS_ROWS * PG_QSHARDS;
// shadow rays the shader resolved against the blocker list (Queue::dropped of the shadow queue)
constexpr uint32_t kDropCounts = kProbeCounts + PG_QSHARDS;
// probes the tracer resolved against the occluder list (Queue::dropped of the probe queue; pg_layout.h "Probe occluders")
constexpr uint32_t kResolvedCounts = kDropCounts + PG_QSHARDS;
static_assert(kResolvedCounts + PG_QSHARDS <= kBounceWords, "counter layout");
constexpr uint32_t kCounterWords = kBounceWords * (kMaxBounces + 1);
constexpr size_t kTailStats = 6;  // k_tail: segments, escaped, shadow rays, culled, probes, blocker-resolved shadow rays

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        else p = nullptr;
        return e;
    }
    // growth with headroom, for buffers re-sized every training iteration (SD-tree): freeing and
    // re-allocating device memory per refit stalled the next stream operation by up to ~20 ms
    hipError_t grow(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        return alloc(std::max(n, bytes + bytes / 2));
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Pinned host staging buffer (reused): pageable-memory copies are pinned on demand by the runtime.
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        n = std::max(n, (size_t)1 << 20);
        n += n / 2;
        hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
        if (e == hipSuccess) bytes = n;
        return e;
    }
};

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
};
// what a timed launch ran (pg_stats buckets)
enum LaunchKind { KT_TRACE = 0, KT_SHADE = 1, KT_SHADOW = 2, KT_RAYS = 3 };

// One in-flight chunk of paths: its own stream, path state, queues and counters.  pg_render_pass
// interleaves pg_config.path_lanes lanes, so while the host waits for one lane's per-bounce class counts the
// GPU runs the other lane's kernels (and a lane's sparse late bounces overlap the other's).
#define PG_MAX_LANES 4
#define PG_DEFAULT_LANES 3
struct Lane {
    hipStream_t stream = nullptr;
    uint32_t P = 0;
    int vtx_slots = 0;
    uint32_t vtxP = 0;  // slot stride of vtx (recording passes only allocate it)
    DevBuf ray, hit, rad, vst, sh_d, sh_c, vtx, q0, q1, qs, qp, class_q, counters, stack_ovf;
    DevBuf qkey, qsorted, rsort_hist;  // ray-sorted trace queues (PG_RAY_SORT): keys, sorted entries, histograms
    bool sorted = false;               // the queue of the next trace launch is qsorted
    DevBuf tail_stats;                 // k_tail counters of the running chunk (kTailStats u64), copied to h_tail
    uint64_t *h_tail = nullptr;        // pinned: k_tail counters of the last finished chunk
    DevBuf aov;  // denoiser features per slot (pg_config.aovs), 2 x float4
    uint32_t *h_counts = nullptr;  // pinned: per-bounce class counts of the running chunk
    uint32_t *h_stats = nullptr;   // pinned: counters of the last finished chunk
    std::vector<EventPair> ev[2];  // kernel-timing events: running chunk / last finished chunk
    std::vector<uint8_t> evkind[2];  // LaunchKind of each used pair
    size_t evused[2] = {0, 0};
    int evcur = 0;
    hipEvent_t ready = nullptr;    // class counts of the current bounce are on the host
    hipEvent_t done = nullptr;     // last finished chunk's statistics copy
    bool stats_pending = false;
    uint32_t stats_bounces = 0;
    // PG_DEBUG_COUNTS: per-bounce segment totals the host read (running chunk / last finished chunk),
    // checked against the device counters of the finished chunk
    std::vector<uint64_t> used_cur, used_prev;
    // running chunk
    bool active = false;
    bool traced = false;  // every path of the chunk terminated; film waits for its turn
    uint32_t chunk = 0;   // chunk index within the pass (films accumulate in this order)
    uint32_t b = 0, bound = 0, pb = 0, np = 0, nl = 0, sample_base = 0;
};

// One in-flight chunk of the volumetric wavefront (renderVolpath): its own stream, SoA path state
// (VolWave, 7 x 16 B per slot), five sharded queues (flight / surface for two iterations, medium
// vertices) with their counters and host copy, per-item radiance and stack overflow ring.  Several
// lanes overlap one chunk's sparse late iterations and k_vtail with the next chunk's full ones.
struct VolLane {
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr;  // the counters' host copy landed
    // the deferred transmittance walks (k_vnee) on a stream of their own, overlapping the next iteration's
    // free flights (PG_VOL_NEE_OVERLAP): vdone = this iteration's interactions done, ndone = its walks done
    hipStream_t nstream = nullptr;
    hipEvent_t vdone = nullptr, ndone = nullptr;
    bool npending = false;
    DevBuf state, items, counts, rad, ovf;
    DevBuf keys, sorted, hist;  // flight order keys of both flight queues, a sorted copy, histograms (PG_VOL_SORT)
    PinnedBuf host;
    uint32_t cap = 0;
    int stateF4 = 0;  // float4 arrays per slot in `state` (7, or 14 with the k_vnee stage's records)
    // the chunk in flight
    bool active = false, waved = false;  // waved: its paths are done, its film waits for its turn
    uint32_t chunk = 0, pb = 0, np = 0, nl = 0, sample_base = 0;
    int it = 0;
    EventPair span;                      // chunk start .. film (pg_stats volume_ms; moved to the pass's list)
};

struct Ctx {
    pg_config cfg{};
    std::string err;
    std::atomic<bool> cancel{false};
    hipStream_t stream = nullptr;
    // scene
    bool has_scene = false;
    GParams g{};
    DevBuf nodes, tris, wnodes, tshade, tclass, mats, rtab, ems, emtri, emcdf;  // tris: both BVHs' triangles
    DevBuf env, envtex, envtab;  // environment emitter: GEnv record, texels, CDFs + row weights
    bool has_env = false;
    // media (volpath)
    DevBuf media, density, tmed, majorant, tcheap;
    bool diffuse_null = false;  // every material diffuse or null: VolDev::models (PG_VOL_MODELS=0 turns it off)
    int32_t cam_medium = -1;
    uint32_t num_media = 0;
    DevBuf vol_rad, vol_ovf, vol_work;  // per-item radiance, traversal-stack overflow, counter + stats
    DevBuf vol_vtx;                     // guided volpath training vertices (48 B each)
    uint64_t vol_vtx_cap = 0;
    // volumetric wavefront (PG_VOL_WAVEFRONT) lanes
    VolLane vlanes[PG_MAX_LANES];
    hipEvent_t vw_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // stage timing (kernel_timing)
    uint32_t vol_cap = 0;
    uint32_t num_tris = 0, num_mats = 0;
    uint32_t bvh_top_nodes = 0;  // breadth-first top levels of the 4-wide BVH (SceneDev::top_nodes: no reader)
    // padded boxes over the emitter triangles (pg_layout.h "Doom probe"): SceneDev::em_box
    uint32_t num_em_boxes = 0;
    float em_absmax = 0.0f;
    float em_box[PG_EMBOX_MAX][6] = {};
    // shadow blockers (pg_layout.h "Shadow blockers"): the per-triangle counts of the recording passes and the list
    // chosen from them (SceneDev::blk); both empty after an upload and after pg_put_sdtree (a new job)
    DevBuf blk_counts;
    PinnedBuf h_blk_counts;     // the counts' host copy (learnBlockers)
    std::vector<float> host_tris, host_shade;  // host copies of tris and tshade: the listed triangles' records
    bool blk_stopped = false;   // no more counting in this job, the list stays (learnBlockers)
    // probe occluders (pg_layout.h "Probe occluders"): counted in the second half of blk_counts (num_tris + 1 words
    // each, one readback for both), learned and reset with the blockers
    bool prb_stopped = false;
    uint32_t num_occluders = 0;
    uint32_t prb_ids[PG_PROBE_LIST_MAX] = {}, prb_orig[PG_PROBE_LIST_MAX] = {};
    float prb[PG_PROBE_LIST_MAX][12] = {};
    uint32_t num_blockers = 0;
    uint32_t blk_ids[PG_MAX_BLOCKERS] = {}, blk_orig[PG_MAX_BLOCKERS] = {};  // BVH-order and original ids
    float blk[PG_MAX_BLOCKERS][12] = {};
    float absmax = 0.0f;  // the scene's largest |coordinate|
    std::vector<GMat> host_mats;
    // textures (pg_set_textures): nothing is allocated while `textured` is false.  base_mats / base_tclass: the
    // untextured scene's material records and triangle classes, put back when the textures are turned off
    bool textured = false;
    bool scene_rendered = false;  // a render pass ran on the uploaded scene: its textures can no longer change
    DevBuf tuv, tex, mtex, texels;
    std::vector<GMat> base_mats;
    std::vector<uint8_t> base_tclass;
    std::vector<uint32_t> host_indices;  // the uploaded scene's triangles (their vertices' texcoords)
    uint32_t num_vertices = 0;
    // normal maps (pg_set_normal_maps): nothing is allocated while `nmapped` is false.  The two calls share the uv
    // records, the triangle classes and mtex (syncTexRows), so each keeps what it was given: the per-material indices
    // (empty: off) and the texcoords (empty: none passed)
    bool nmapped = false;
    DevBuf ntex, mnmap, ntexels, ttan;
    std::vector<uint32_t> host_mtex, host_mnmap;
    std::vector<float> tex_uv, nmap_uv;
    float scene_lo[3] = {0, 0, 0}, scene_hi[3] = {0, 0, 0};
    // delta emitters (pg_set_delta_emitters): nothing is allocated while num_delta is 0.  tri_lo / tri_hi: the
    // uploaded triangles' box, whose bounding sphere a directional emitter's disk lies on
    DevBuf delta;
    uint32_t num_delta = 0, num_area = 0;
    float tri_lo[3] = {0, 0, 0}, tri_hi[3] = {0, 0, 0};
    // homogeneous media (pg_set_homogeneous_media): base_media is the uploaded scene's records, which `media` holds
    // while num_homog is 0; is_homog marks the entries the records replaced
    std::vector<GMedium> base_media;
    std::vector<uint8_t> is_homog;
    uint32_t num_homog = 0;
    // shard
    std::vector<uint32_t> local_pixels;
    DevBuf d_local_pixels;
    DevBuf d_band_pixels;  // the surface path's order of the same pixels (cameraBands)
    // path state
    Lane lanes[PG_MAX_LANES];
    int nlanes = PG_DEFAULT_LANES;
    hipEvent_t film_order = nullptr;  // last chunk's film + record commit (keeps them in chunk order)
    hipEvent_t pass_start = nullptr;
    uint64_t rec_bound = 0;           // upper bound of the device-side record count
    EventPair timing;                 // context-stream kernel timing (splat)
    // film
    DevBuf film, film_sq;
    DevBuf aov_albedo, aov_normal;  // per-pixel denoiser feature sums (pg_config.aovs)
    // reconstruction-filtered film (pg_set_rfilter): nothing is allocated or launched while `filtered` is false
    bool filtered = false;
    bool filter_direct = false;  // PG_FILM_FILTER_DIRECT=1, or the padded tile exceeds 64 KiB of LDS
    bool rendered = false;       // a render pass ran: the filter can no longer change
    float filter_radius = 0;
    float filter_values[32] = {};
    DevBuf film_acc, filter_tab, tile_first, tile_origin;
    std::vector<uint32_t> h_tile_first;  // local tile k = local pixels [h_tile_first[k], h_tile_first[k + 1])
    std::vector<uint32_t> h_tile_origin; // (x, y) pairs
    // denoiser (pg_denoise): nothing is allocated or created before the first call
    DevBuf dn_scratch;                  // pg_denoise's four rows per pixel: ev ping, ev pong, fn, fa
    EventPair dn_ev;                    // around the last call's launches (pg_denoise_time)
    bool dn_timed = false;
    // records
    DevBuf records, rec_count;
    uint64_t rec_capacity = 0;
    uint64_t rec_host_count = 0;
    DevBuf ext_records;
    // sd-tree
    pgh::SdTree sd;
    // the device SD-tree lives in one allocation (uploadSd): snodes | meta | qnode {energies, children} |
    // bchild | bsum | count | frac | jump.  bsum, count and frac are contiguous -- the pg_get_tree_stats
    // vector -- so the statistics move in one copy (download, all-reduce in place), the host-built
    // part in one upload, and the jump grid is built on the device from the S-tree.
    DevBuf sd_blob;
    struct {
        uint32_t *snodes = nullptr, *meta = nullptr, *qnode = nullptr, *bchild = nullptr, *jump = nullptr;
        uint64_t *bsum = nullptr, *count = nullptr, *frac = nullptr;  // frac: pgh::kFracStats u64 per leaf
    } sdp;
    int sd_jump_bits = 0;
    PinnedBuf sd_stage;
    bool sd_dirty = true;
    // multi-GPU: RCCL communicator over the job's ranks (pg_comm_init), one per context/device
    ncclComm_t comm = nullptr;
    // stats
    pg_stats stats{};
    uint64_t culled = 0;  // segments whose hit the tracer culled (pg_get_culled); counted in stats.segments
    uint64_t probes = 0;  // segments answered by an any-hit probe (pg_get_probes); counted in culled or escaped
    uint64_t probes_resolved = 0;  // probes answered by the occluder list without a walk (pg_get_probes_resolved); counted in probes
    uint64_t shadow_culled = 0;  // shadow rays resolved against the blocker list; counted in stats.shadow_rays
};

// records the message on the context (or, without one, for pg_last_error(NULL)) and returns `code`
pg_status fail(Ctx *c, pg_status code, const std::string &msg);

#define HIPC(c, expr)                                                                                              \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess)                                                                                      \
            return fail((c), e_ == hipErrorOutOfMemory ? PG_ERR_OOM : PG_ERR_HIP,                                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                                        \
    } while (0)

// ---- the context side (pg_host.cpp), as the pass drivers use it ----
SceneDev sceneView(const Ctx *c);
SDDev sdView(const Ctx *c);
PathDev pathView(const Lane *l);
pg_status ensurePaths(Ctx *c, uint32_t want, bool rec);
void releasePaths(Ctx *c);
pg_status ensureRecords(Ctx *c, uint64_t want);
pg_status learnBlockers(Ctx *c, bool blockers, bool occluders);
bool probeListEnabled(const Ctx *c);
void launchFilmFiltered(Ctx *c, hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &p,
                        const uint32_t *pixels, uint32_t pb, uint32_t np, uint32_t nl, uint32_t sample_base);
int vertexSlots(const Ctx *c, bool rec);
uint32_t deviceDepthCap(const pg_config &cfg);
uint32_t cameraBands();
bool raySortEnabled();  // pg_pass.cpp (PG_RAY_SORT): ensurePaths allocates the sort's buffers

}  // namespace pgh
