// The pass drivers behind pg_render_pass (ProgressiveMonteCarloIntegrator::renderSamples / renderBlock,
// src/librender/progressiveintegrator.cpp:65-114,222-282, re-expressed as GPU schedulers): the surface wavefront
// (renderPass), the volumetric wavefront (volWavefrontPass), the megakernel loop (renderVolpath), their shared steps.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_chunks.h"
#include "pg_ctx.h"

namespace pgh __attribute__((visibility("hidden"))) {

// ---- scheduling knobs -----------------------------------------------------------------------------------------------
#ifndef PG_SMALL_PASS
#define PG_SMALL_PASS (1u << 21)  // paths: passes up to this size run as one chunk (0: always one per lane)
#endif
// the same threshold at run time (A/B: PG_SMALL_PASS_PATHS overrides)
uint64_t smallPass() {
    static const char *e = std::getenv("PG_SMALL_PASS_PATHS");
    static const uint64_t n = e ? (uint64_t)std::strtoull(e, nullptr, 10) : (uint64_t)PG_SMALL_PASS;
    return n;
}

// ray-sorted trace queues (A/B switch PG_RAY_SORT=1): k_shade writes a ray order key per queued path and
// a counting sort groups every shard of the next closest-hit queue by direction octant + origin cell
bool raySortEnabled() {
    static const char *e = std::getenv("PG_RAY_SORT");
    static const bool on = e && std::atoi(e) != 0;
    return on;
}
constexpr uint32_t kRaySortMinShard = 1024;  // smaller bounces trace unsorted (the sort's launches cost more)

// the tail of a chunk (k_tail): at most this many live paths left -> one launch finishes them all
// instead of one launch pair + count readback per bounce (PG_TAIL_PATHS overrides; 0 = off)
uint32_t tailPaths() {
    static const char *e = std::getenv("PG_TAIL_PATHS");  // profiles/r03n_*: 2^17 vs 2^16 +0.3 %
    static const uint32_t n = e ? (uint32_t)std::strtoul(e, nullptr, 10) : (uint32_t)1 << 17;
    return n;
}

// an integer knob read from the environment when called (unset or empty: def), so tests can switch it in-process
long long envInt(const char *name, long long def) {
    const char *e = std::getenv(name);
    return e && *e ? std::strtoll(e, nullptr, 10) : def;
}

// The volumetric path as a wavefront (pg_volpath.hip k_vcam / k_vflight / k_vvertex / k_vtail) or as the
// persistent megakernel k_volpath (PG_VOL_WAVEFRONT=0): the same per-path arithmetic and random
// streams, so the same films and trees
// (read per chunk, so tests can compare both in one process)
bool volWavefront() { return envInt("PG_VOL_WAVEFRONT", 1) != 0; }
// the interactions' transmittance walks (NEE shadow walks, emitter walks through media) as a stage of their
// own (k_vnee, after each k_vvertex; PG_VOL_NEE_STAGE=1) or inline at the end of each k_vvertex interaction
// (default): both give the same films and trees (the walks draw from their own sub-streams either way).  The
// stage takes the walks out of k_vvertex (medium interactions at 3 waves/SIMD, 166 VGPRs, no scratch) but the
// walks then run 45 % slower on their own: C5 328.8 / 326.4 Mpaths/s as a stage, 334.7 / 335.6 with the stage
// overlapping the next iteration's flights, 373.7 / 373.9 inline on one box (profiles/r05c_vol_nee_stage/)
bool volNeeStage() { return envInt("PG_VOL_NEE_STAGE", 0) != 0; }
// VolLane path state: VolWave's 14 float4 per slot (7 path columns, 6 deferred-walk columns and their flags /
// key / sample column; the first 7 when the walks run inline); its queues (pg_volpath.hip)
constexpr int kVolStateF4 = 14, kVolStateF4Inline = 7, kVolQueues = 8;
// k_vnee of iteration i on the lane's second stream, concurrent with iteration i + 1's k_vflight (which reads
// no state the walks write); k_vvertex of i + 1 waits for it.  PG_VOL_NEE_OVERLAP=0: on the lane's stream
bool volNeeOverlap() { return envInt("PG_VOL_NEE_OVERLAP", 1) != 0; }
// below this many live paths a chunk's remaining paths finish in one k_vtail launch (PG_VOL_TAIL_PATHS): 2^17
// with three lanes (C5 398.7 / 399.4 against 396.6 / 397.5 at 2^18, profiles/r04al_vol_tail/)
uint32_t volTailPaths() { return (uint32_t)envInt("PG_VOL_TAIL_PATHS", 1 << 17); }
// flight queues sorted by the 16^3 cell of the flight's start before k_vflight, for shards of at least this
// many flights (PG_VOL_SORT; 0 = off, the default since round 5).  Round 4: C5 351.5 / 350.0 against
// 346.3 / 345.7 Mpaths/s unsorted (profiles/r04s_vol_sort/, r04t_vol_ab/).  With round 5's 3-wave interaction
// launches the sort no longer pays: 442.9 / 442.5 sorted (4096) against 445.0 / 445.8 unsorted, k_vflight
// 45.3 against 48.9 ms per calibration pass but k_vvertex 136.4 against 133.8 (its state reads no longer
// scattered) plus the sort kernels (profiles/r05t_vol_tune/)
uint32_t volSortMin() { return (uint32_t)envInt("PG_VOL_SORT", 0); }
// volumetric wavefront lanes in flight: pg_config.path_lanes (default 3, as for the path integrator; C5 at
// the round-4 kernels: 393.7 / 397.0 / 389.7 Mpaths/s with 2 / 3 / 4 lanes, profiles/r04aj_vol_lanes/);
// PG_VOL_LANES overrides (A/B)
int volLanes(const Ctx *c) { return std::max(1, std::min(PG_MAX_LANES, (int)envInt("PG_VOL_LANES", c->nlanes))); }

// ---- steps the schedulers share -------------------------------------------------------------------------------------
// the device's record count, read once every stream that commits records is idle: into the statistics, and the new bound
pg_status foldRecordCount(Ctx *c) {
    unsigned long long rc = 0;
    HIPC(c, hipMemcpy(&rc, c->rec_count.p, 8, hipMemcpyDeviceToHost));
    c->stats.records += rc - c->rec_host_count;
    c->rec_host_count = c->rec_bound = rc;
    return PG_OK;
}

// Record commit of a finished chunk of `items` paths on stream s.  Every path can emit at most maxV records; when that
// bound could overflow the record buffer, the streams `busy` (whatever may be committing: every surface lane, the
// volumetric lane itself, the megakernel's context stream) are waited for, the true count read and the buffer grown.
pg_status commitRecords(Ctx *c, hipStream_t s, const PathDev &pv, uint32_t items, int maxV, int env,
                        const hipStream_t *busy, int nbusy) {
    const uint64_t add = (uint64_t)items * (uint64_t)maxV;
    if (c->rec_bound + add > c->rec_capacity) {
        for (int i = 0; i < nbusy; ++i) HIPC(c, hipStreamSynchronize(busy[i]));
        pg_status st;
        if ((st = foldRecordCount(c)) || (st = ensureRecords(c, c->rec_host_count + add))) return st;
    }
    c->rec_bound += add;
    pg_launch_commit(s, pv, items, maxV, c->records.as<pg_record>(), c->rec_count.as<unsigned long long>(),
                     c->rec_capacity, env);
    return PG_OK;
}

// Film of a finished chunk on stream s: k_film and, with a reconstruction filter, k_film_filtered over the same rows
// (the tail, when it ran, left them as the bounce launches do).  albedo / normal: the surface path's AOV sums.  A lane
// brackets this and its commit with Ctx::film_order (surface: film, commit; volumetric: commit, film): the callers do.
void chunkFilm(Ctx *c, hipStream_t s, const GParams &g, const SceneDev &sc, const PathDev &pv, const uint32_t *pixels,
               const VChunk &ch, float4 *albedo = nullptr, float4 *normal = nullptr) {
    pg_launch_film(s, g, sc, pv, pixels, ch.pb, ch.np, ch.nl, c->film.as<float4>(), c->film_sq.as<float4>(), albedo, normal);
    if (c->filtered) launchFilmFiltered(c, s, g, sc, pv, pixels, ch.pb, ch.np, ch.nl, ch.sample_base);
}

// the context's GParams with the pg_config fields every pass sets; each scheduler adds those only it sets
GParams passParams(const Ctx *c, bool record, int maxV) {
    GParams g = c->g;
    g.max_depth = c->cfg.max_depth;
    g.rr_depth = c->cfg.rr_depth;
    g.use_nee = c->cfg.use_nee;
    g.hide_emitters = c->cfg.hide_emitters;
    g.strict_normals = c->cfg.strict_normals;
    g.max_component_value = c->cfg.max_component_value;
    g.seed = c->cfg.seed;
    g.depth_cap = deviceDepthCap(c->cfg);
    g.guiding = c->cfg.guiding;
    g.bsdf_fraction = c->cfg.bsdf_sampling_fraction;
    g.fraction_bound = c->cfg.bsdf_fraction_bound;
    g.record = record ? 1 : 0;
    g.max_vertices = maxV;
    return g;
}

// ---- the volumetric schedulers --------------------------------------------------------------------------------------
// The chunks of one pass through the wavefront: per chunk the camera rays, then per iteration the
// free flights and the interactions, until at most volTailPaths() paths live; the tail finishes them.
// The host reads a chunk's queue counters once per iteration (grid sizes; the kernels read the counts)
// and advances whichever lane's counters have landed, so one chunk's readback and sparse last
// iterations overlap another's full ones.  Films (and record commits) run in chunk order, so every
// pixel's float sums are those of one lane.  Recording passes use two lanes (each with its own region of
// training vertices), per-stage timing one.
pg_status volWavefrontPass(Ctx *c, const GParams &g, const SceneDev &sc, const VolDev &v, const SDDev &sd,
                           const PathDev &pv, const std::vector<VChunk> &chunks, uint32_t want, int maxV,
                           uint32_t vtxLanes, std::vector<EventPair> &evs) {
    const bool evt = c->cfg.kernel_timing != 0;
    const int nl = evt ? 1 : std::min<int>(g.record ? (int)vtxLanes : volLanes(c), (int)chunks.size());
    // training vertices of lane li (recording passes): region li of vtxLanes, want items each
    auto laneVtx = [&](const VolLane &l) -> float4 * {
        return v.vtx ? v.vtx + (size_t)(&l - c->vlanes) * want * (size_t)maxV * PG_VTX_F4 : nullptr;
    };
    const size_t cbytes = (size_t)PG_QSHARDS * 4 * kVolQueues;
    const bool neeStage = volNeeStage(), neeOverlap = neeStage && volNeeOverlap() && !evt;
    auto joinNee = [&](VolLane &l) -> pg_status {  // the lane's stream waits for its pending walks
        if (l.npending) {
            HIPC(c, hipStreamWaitEvent(l.stream, l.ndone, 0));
            l.npending = false;
        }
        return PG_OK;
    };
    const uint32_t sortMin = volSortMin();
    HIPC(c, hipEventRecord(c->pass_start, c->stream));  // lanes start after the context stream's work
    for (int li = 0; li < nl; ++li) {
        VolLane &l = c->vlanes[li];
        if (!l.stream) {
            HIPC(c, hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
            HIPC(c, hipEventCreateWithFlags(&l.ready, hipEventDisableTiming));
        }
        // the second stream only when the overlapped k_vnee stage runs: HIP maps a process's streams onto
        // GPU_MAX_HW_QUEUES (4) hardware queues, and with one more stream per lane two lanes shared a queue
        // and serialized (C5 380 against 400 Mpaths/s, profiles/r05h_vol_streams/)
        if (neeOverlap && !l.nstream) {
            HIPC(c, hipStreamCreateWithFlags(&l.nstream, hipStreamNonBlocking));
            HIPC(c, hipEventCreateWithFlags(&l.vdone, hipEventDisableTiming));
            HIPC(c, hipEventCreateWithFlags(&l.ndone, hipEventDisableTiming));
        }
        l.npending = false;
        const int f4 = neeStage ? kVolStateF4 : kVolStateF4Inline;  // the stage's records only when it runs
        if (l.cap < want || l.stateF4 != f4) {
            const uint32_t lc = std::max(want, l.cap);
            HIPC(c, l.state.alloc((size_t)lc * 16 * f4));
            l.stateF4 = f4;
            HIPC(c, l.items.alloc((size_t)pg_queue_stride(lc) * PG_QSHARDS * 4 * kVolQueues));
            HIPC(c, l.rad.alloc((size_t)lc * 16));
            l.cap = lc;
        }
        HIPC(c, l.counts.alloc(cbytes));
        HIPC(c, l.host.reserve(cbytes));
        if (sortMin) {
            const size_t qstride = (size_t)pg_queue_stride(l.cap) * PG_QSHARDS;
            HIPC(c, l.keys.alloc(qstride * 2 * 2));
            HIPC(c, l.sorted.alloc(qstride * 4));
            HIPC(c, l.hist.alloc((size_t)PG_QSHARDS * PG_RAY_SORT_BINS * 4));
        }
        if (!l.ovf.p) HIPC(c, l.ovf.alloc(pg_stack_overflow_words(0) * 4));
        HIPC(c, hipStreamWaitEvent(l.stream, c->pass_start, 0));
        l.active = l.waved = false;
    }
    HIPC(c, hipEventRecord(c->film_order, c->stream));
    const uint32_t tail = volTailPaths();
    uint32_t next = 0, filmNext = 0;
    auto views = [&](VolLane &l, VolDev &lv, VolWave &w, Queue *q) {  // q: kVolQueues queues
        lv = v;
        lv.rad = l.rad.as<float4>();
        lv.stack_ovf = l.ovf.as<uint32_t>();
        lv.vtx = laneVtx(l);
        float4 *st = l.state.as<float4>();
        const size_t cap = l.cap;
        w = VolWave{st, st + cap, reinterpret_cast<uint4 *>(st + 2 * cap), st + 3 * cap, st + 4 * cap,
                    reinterpret_cast<uint4 *>(st + 5 * cap), st + 6 * cap};
        if (l.stateF4 == kVolStateF4) {  // the k_vnee stage's deferred-walk records
            w.n0 = st + 7 * cap;
            w.n1 = st + 8 * cap;
            w.n2 = st + 9 * cap;
            w.h0 = st + 10 * cap;
            w.h1 = st + 11 * cap;
            w.h2 = st + 12 * cap;
            w.nflags = reinterpret_cast<uint4 *>(st + 13 * cap);
        }
        // queues 0/1: flight of even / odd iterations, 2/3: surface, 4: medium vertices, 5/6: delta surface,
        // 7: deferred transmittance walks (k_vnee)
        const size_t qstride = (size_t)pg_queue_stride(l.cap) * PG_QSHARDS;
        const uint32_t stride = pg_queue_stride(l.np * l.nl);
        for (int k = 0; k < kVolQueues; ++k)
            q[k] = Queue{l.items.as<uint32_t>() + k * qstride, l.counts.as<uint32_t>() + k * PG_QSHARDS, stride};
        if (sortMin)
            for (int k = 0; k < 2; ++k) q[k].keys = l.keys.as<uint16_t>() + k * qstride;
    };
    auto readback = [&](VolLane &l) -> pg_status {
        HIPC(c, hipMemcpyAsync(l.host.p, l.counts.p, cbytes, hipMemcpyDeviceToHost, l.stream));
        HIPC(c, hipEventRecord(l.ready, l.stream));
        return PG_OK;
    };
    auto start = [&](VolLane &l) -> pg_status {
        l.active = false;
        if (next >= chunks.size()) return PG_OK;
        const VChunk &ch = chunks[next];
        l.chunk = next++;
        l.pb = ch.pb, l.np = ch.np, l.nl = ch.nl, l.sample_base = ch.sample_base;
        l.it = 0;
        l.active = true;
        l.waved = false;
        HIPC(c, hipEventCreate(&l.span.a));
        HIPC(c, hipEventCreate(&l.span.b));
        HIPC(c, hipEventRecord(l.span.a, l.stream));
        VolDev lv;
        VolWave w;
        Queue q[kVolQueues];
        views(l, lv, w, q);
        HIPC(c, hipMemsetAsync(l.counts.p, 0, cbytes, l.stream));
        pg_launch_vol_camera(l.stream, g, sc, lv, w, c->d_local_pixels.as<uint32_t>(), l.pb, l.np, l.nl, l.sample_base,
                             q[0], q[2], q[5]);
        HIPC(c, hipGetLastError());
        return readback(l);
    };
    // record commit + film of a chunk whose paths are done (its turn in chunk order), then its next chunk
    auto finish = [&](VolLane &l) -> pg_status {
        HIPC(c, hipStreamWaitEvent(l.stream, c->film_order, 0));
        PathDev lp = pv;
        lp.rad = l.rad.as<float4>();
        lp.vtx = laneVtx(l);
        if (g.record)
            if (pg_status st = commitRecords(c, l.stream, lp, l.np * l.nl, maxV, 0, &l.stream, 1)) return st;
        chunkFilm(c, l.stream, g, sc, lp, c->d_local_pixels.as<uint32_t>(), VChunk{l.pb, l.np, l.nl, l.sample_base});
        HIPC(c, hipGetLastError());
        HIPC(c, hipEventRecord(c->film_order, l.stream));
        HIPC(c, hipEventRecord(l.span.b, l.stream));
        evs.push_back(l.span);
        l.span = EventPair{};
        c->stats.paths += (uint64_t)l.np * l.nl;
        return start(l);
    };
    // one iteration of lane l (its counters are on the host)
    auto advance = [&](VolLane &l) -> pg_status {
        if (c->cancel.load()) return fail(c, PG_ERR_CANCELLED, "cancelled");
        const uint32_t *hc = reinterpret_cast<const uint32_t *>(l.host.p);
        auto maxShard = [&](int k) {
            uint32_t m = 0, t = 0;
            for (int i = 0; i < PG_QSHARDS; ++i) {
                m = std::max(m, hc[k * PG_QSHARDS + i]);
                t += hc[k * PG_QSHARDS + i];
            }
            return std::make_pair(m, t);
        };
        VolDev lv;
        VolWave w;
        Queue q[kVolQueues];
        views(l, lv, w, q);
        const int cur = l.it & 1, nxt = cur ^ 1;
        const auto f = maxShard(cur), su = maxShard(2 + cur), sdl = maxShard(5 + cur);
        if (f.second + su.second + sdl.second <= tail) {
            if (pg_status js = joinNee(l)) return js;
            if (f.second + su.second + sdl.second) {
                pg_launch_vol_tail(l.stream, g, sc, lv, sd, w, q[cur], f.first, q[2 + cur], su.first, q[5 + cur],
                                   sdl.first);
                HIPC(c, hipGetLastError());
            }
            l.waved = true;
            // finish this chunk and every waiting one whose turn comes after it
            for (int k = 0; k < nl; ++k) {
                VolLane &o = c->vlanes[k];
                if (!(o.active && o.waved && o.chunk == filmNext)) continue;
                ++filmNext;
                if (pg_status st = finish(o)) return st;
                k = -1;  // the next chunk in film order may wait on any lane
            }
            return PG_OK;
        }
        // the next iteration's output queues and the medium queue start empty
        HIPC(c, hipMemsetAsync(q[nxt].counts, 0, PG_QSHARDS * 4, l.stream));
        HIPC(c, hipMemsetAsync(q[2 + nxt].counts, 0, PG_QSHARDS * 4, l.stream));
        HIPC(c, hipMemsetAsync(q[4].counts, 0, PG_QSHARDS * 4, l.stream));
        HIPC(c, hipMemsetAsync(q[5 + nxt].counts, 0, PG_QSHARDS * 4, l.stream));
        // per-stage device time (pg_config.kernel_timing, one lane): events around each launch
        if (evt && !c->vw_ev[0])
            for (hipEvent_t &e : c->vw_ev) HIPC(c, hipEventCreate(&e));
        Queue fq = q[cur];
        if (sortMin && f.first >= sortMin) {  // the flights in cell order (same shards and counts)
            pg_launch_ray_sort(l.stream, fq, f.first, l.sorted.as<uint32_t>(), l.hist.as<uint32_t>(), PG_VOL_SORT_BINS);
            fq.items = l.sorted.as<uint32_t>();
        }
        if (evt) HIPC(c, hipEventRecord(c->vw_ev[0], l.stream));
        pg_launch_vol_flight(l.stream, g, sc, lv, sd, w, fq, f.first, q[4], q[2 + cur], q[5 + cur]);
        if (evt) HIPC(c, hipEventRecord(c->vw_ev[1], l.stream));
        // shard bounds without a readback: a medium vertex came from a flight; a surface vertex from a
        // flight or from the previous iteration's interactions; no shard exceeds the queue stride
        const uint32_t mm = f.first, ms = std::min(q[0].stride, f.first + su.first + sdl.first);
        // the previous iteration's walks write L: done before this iteration's interactions read it
        if (pg_status js = joinNee(l)) return js;
        if (neeStage) HIPC(c, hipMemsetAsync(q[7].counts, 0, PG_QSHARDS * 4, l.stream));
        const int vk = pg_launch_vol_vertex(l.stream, g, sc, lv, sd, w, q[4], mm, q[2 + cur], ms, q[5 + cur], ms,
                                            q[nxt], q[2 + nxt], q[5 + nxt], neeStage ? &q[7] : nullptr);
        if (evt) HIPC(c, hipEventRecord(c->vw_ev[2], l.stream));
        // the deferred walks: at most one entry per path live in this iteration (<= ms per shard)
        if (neeOverlap) {
            HIPC(c, hipEventRecord(l.vdone, l.stream));
            HIPC(c, hipStreamWaitEvent(l.nstream, l.vdone, 0));
            pg_launch_vol_nee(l.nstream, g, sc, lv, w, q[7], ms);
            HIPC(c, hipEventRecord(l.ndone, l.nstream));
            l.npending = true;
        } else if (neeStage) {
            pg_launch_vol_nee(l.stream, g, sc, lv, w, q[7], ms);
        }
        if (evt) {
            HIPC(c, hipEventRecord(c->vw_ev[3], l.stream));
            HIPC(c, hipEventSynchronize(c->vw_ev[3]));
            float a = 0, b = 0, e = 0;
            if (f.first) {
                HIPC(c, hipEventElapsedTime(&a, c->vw_ev[0], c->vw_ev[1]));
                c->stats.vol_flight_ms += a;
                c->stats.vol_flight_launches++;
            }
            HIPC(c, hipEventElapsedTime(&b, c->vw_ev[1], c->vw_ev[2]));
            c->stats.vol_vertex_ms += b;
            c->stats.vol_vertex_launches += vk;  // kernels, not stages: the medium and surface launches
            if (neeStage) {
                HIPC(c, hipEventElapsedTime(&e, c->vw_ev[2], c->vw_ev[3]));
                c->stats.vol_nee_ms += e;
                c->stats.vol_nee_launches++;
            }
        }
        HIPC(c, hipGetLastError());
        ++l.it;
        return readback(l);
    };
    pg_status s;
    for (int li = 0; li < nl; ++li)
        if ((s = start(c->vlanes[li]))) return s;
    // advance whichever lane has its counters first
    for (uint32_t rr = 0;; ++rr) {
        int active = 0, picked = -1;
        for (int k = 0; k < nl && picked < 0; ++k) {
            VolLane &l = c->vlanes[(rr + k) % nl];
            if (!l.active) continue;
            ++active;
            if (l.waved) continue;  // waiting for an earlier chunk's film
            const hipError_t qr = hipEventQuery(l.ready);
            if (qr == hipSuccess) picked = (int)((rr + k) % nl);
            else if (qr != hipErrorNotReady) HIPC(c, qr);
        }
        if (!active) break;
        if (picked >= 0 && (s = advance(c->vlanes[picked]))) return s;
    }
    for (int li = 0; li < nl; ++li) HIPC(c, hipStreamSynchronize(c->vlanes[li].stream));
    return PG_OK;
}

// progressive_volpath: chunks of (pixel, sample) items through the wavefront or k_volpath, films in chunk order
pg_status renderVolpath(Ctx *c, uint32_t spp, uint32_t sample_offset, bool rec) {
    const uint32_t npix = (uint32_t)c->local_pixels.size();
    // 2^25 items per launch: fewer persistent-kernel tails (C5 guided: 177.8 -> 189.8 Mpaths/s
    // against 2^22, profiles/r01h_c5_*.log); 50 GB of training vertices when guided
    const uint32_t cap = c->cfg.max_paths_in_flight ? c->cfg.max_paths_in_flight : (1u << 25);
    const uint64_t total = (uint64_t)npix * spp;
    uint32_t want = (uint32_t)std::min<uint64_t>(total, cap);
    const bool wave = volWavefront();  // the wavefront's lanes hold their own radiance and overflow rings
    const int maxV = std::min(std::max(c->cfg.record_max_vertices, 0), 64);
    // a recording pass through the wavefront runs as (at least) two chunks on two lanes, each lane with
    // its own region of training vertices (indexed by item within the chunk): the same vertex memory as
    // one chunk of the whole pass
    const char *rl = std::getenv("PG_VOL_REC_LANES");  // 1: one lane (A/B)
    const uint32_t vtxLanes = (wave && rec && maxV > 0 && !c->cfg.kernel_timing && volLanes(c) >= 2 && total > 1 &&
                               !(rl && std::atoi(rl) == 1)) ? 2u : 1u;
    if (vtxLanes == 2) want = (uint32_t)std::min<uint64_t>(want, (total + 1) / 2);
    if (!wave && c->vol_cap < want) {
        HIPC(c, c->vol_rad.alloc((size_t)want * 16));
        c->vol_cap = want;
    }
    if (rec && maxV > 0 && c->vol_vtx_cap < (uint64_t)want * maxV * vtxLanes) {
        HIPC(c, c->vol_vtx.alloc((size_t)want * maxV * vtxLanes * 16 * PG_VTX_F4));
        c->vol_vtx_cap = (uint64_t)want * maxV * vtxLanes;
    }
    if (!wave && !c->vol_ovf.p) HIPC(c, c->vol_ovf.alloc(pg_stack_overflow_words(0) * 4));
    HIPC(c, c->vol_work.alloc(128));  // work counter, then 7 u64 statistics from byte 16
    HIPC(c, hipMemsetAsync(c->vol_work.p, 0, 128, c->stream));
    GParams g = passParams(c, rec && maxV > 0, maxV);
    g.exact_mis = c->cfg.volpath_exact_mis;
    const SceneDev sc = sceneView(c);
    const SDDev sd = sdView(c);
    VolDev v{};
    v.grid = c->cfg.volume_majorant == PG_MAJORANT_GRID ? 1 : 0;
    v.media = c->media.as<GMedium>();
    v.tmed = c->tmed.as<uint32_t>();
    v.tcheap = c->tcheap.as<uint8_t>();
    {  // the surface launches specialised to diffuse / null materials (read per pass: tests A/B it in-process)
        const char *e = std::getenv("PG_VOL_MODELS");
        v.models = c->diffuse_null && !(e && *e && std::atoi(e) == 0) ? 1u : 0u;
    }
    v.cam_medium = c->cam_medium;
    v.num_media = c->num_media;
    v.homog = c->num_homog ? 1u : 0u;  // the launchers' HOMOG instantiations (pg_set_homogeneous_media)
    v.rad = c->vol_rad.as<float4>();
    v.next = c->vol_work.as<uint32_t>();
    v.stats = (unsigned long long *)(c->vol_work.as<uint8_t>() + 16);
    v.stack_ovf = c->vol_ovf.as<uint32_t>();
    v.vtx = g.record ? c->vol_vtx.as<float4>() : nullptr;
    v.vtx_P = want;
    v.dist_beta = c->cfg.distance_guiding;
    {  // refill threshold of the persistent volumetric kernel: C5 198 / 212 / 227 / 243 / 248 / 247 / 242 /
       // 211 Mpaths/s at 1 / 8 / 16 / 32 / 40 / 48 / 56 / 64 idle lanes (profiles/r03p_vol_refill/);
       // PG_VOL_REFILL overrides (A/B)
        const char *e = std::getenv("PG_VOL_REFILL");
        v.refill_min = e ? (uint32_t)std::max(1, std::min(64, std::atoi(e))) : 40u;
    }
    PathDev pv{};
    pv.rad = v.rad;
    pv.vtx = v.vtx;
    pv.P = want;
    pv.vtxP = want;
    pv.vst = nullptr;  // k_commit reads the vertex count from rad[item].w
    const std::vector<VChunk> chunks = planChunks(npix, spp, want, sample_offset);
    std::vector<EventPair> evs;
    struct EventsGuard {  // the chunk spans, on every exit (an error or cancellation returns early)
        std::vector<EventPair> &v;
        ~EventsGuard() {
            for (EventPair &e : v) {
                (void)hipEventDestroy(e.a);
                (void)hipEventDestroy(e.b);
            }
        }
    } evsGuard{evs};
    if (wave)
        if (pg_status ws = volWavefrontPass(c, g, sc, v, sd, pv, chunks, want, maxV, vtxLanes, evs)) return ws;
    for (size_t ci = 0; !wave && ci < chunks.size(); ++ci) {  // the persistent megakernel
        if (c->cancel.load()) return fail(c, PG_ERR_CANCELLED, "cancelled");
        const VChunk &ch = chunks[ci];
        EventPair e;
        HIPC(c, hipEventCreate(&e.a));
        HIPC(c, hipEventCreate(&e.b));
        evs.push_back(e);
        HIPC(c, hipEventRecord(e.a, c->stream));
        pg_launch_volpath(c->stream, g, sc, v, sd, c->d_local_pixels.as<uint32_t>(), ch.pb, ch.np, ch.nl, ch.sample_base);
        HIPC(c, hipEventRecord(e.b, c->stream));
        if (g.record)
            if (pg_status st = commitRecords(c, c->stream, pv, ch.np * ch.nl, maxV, 0, &c->stream, 1)) return st;
        chunkFilm(c, c->stream, g, sc, pv, c->d_local_pixels.as<uint32_t>(), ch);
        HIPC(c, hipGetLastError());
        c->stats.paths += (uint64_t)ch.np * ch.nl;
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    unsigned long long st[9];
    HIPC(c, hipMemcpy(st, c->vol_work.as<uint8_t>() + 16, 72, hipMemcpyDeviceToHost));
    c->stats.vol_nee_walks += st[7];
    c->stats.vol_nee_lookups += st[8];
    c->stats.vol_flights += st[3];
    c->stats.vol_flight_lookups += st[4];
    c->stats.vol_vertices += st[5];
    c->stats.vol_vertex_lookups += st[6];
    c->stats.segments += st[0];
    c->stats.shadow_rays += st[1];
    c->stats.density_lookups += st[2];
    if (g.record)
        if (pg_status rs = foldRecordCount(c)) return rs;
    for (EventPair &e : evs) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e.a, e.b);
        c->stats.volume_ms += ms;
        c->stats.volume_launches++;
    }
    return PG_OK;
}

// ---- the surface scheduler ------------------------------------------------------------------------------------------
EventPair nextEvents(Lane *l, LaunchKind kind) {
    std::vector<EventPair> &pool = l->ev[l->evcur];
    std::vector<uint8_t> &kinds = l->evkind[l->evcur];
    kinds.resize(l->evused[l->evcur] + 1);
    kinds[l->evused[l->evcur]] = (uint8_t)kind;
    if (l->evused[l->evcur] == pool.size()) {
        EventPair e;
        (void)hipEventCreate(&e.a);
        (void)hipEventCreate(&e.b);
        pool.push_back(e);
    }
    return pool[l->evused[l->evcur]++];
}

// fold the last finished chunk's shadow counts and kernel times into the statistics
pg_status collectStats(Ctx *c, Lane &l) {
    if (!l.stats_pending) return PG_OK;
    HIPC(c, hipEventSynchronize(l.done));
    for (uint32_t k = 0; k < l.stats_bounces; ++k)
        for (int sh = 0; sh < PG_QSHARDS; ++sh) {
            c->stats.shadow_rays += l.h_stats[(size_t)kBounceWords * k + kShadowCounts + sh];
            c->probes += l.h_stats[(size_t)kBounceWords * k + kProbeCounts + sh];
            // shadow rays the shader resolved: never queued, still shadow rays of the job
            c->stats.shadow_rays += l.h_stats[(size_t)kBounceWords * k + kDropCounts + sh];
            c->shadow_culled += l.h_stats[(size_t)kBounceWords * k + kDropCounts + sh];
            c->probes_resolved += l.h_stats[(size_t)kBounceWords * k + kResolvedCounts + sh];
        }
    c->stats.segments += l.h_tail[0];  // the chunk's tail (k_tail)
    c->stats.escaped += l.h_tail[1];
    c->stats.shadow_rays += l.h_tail[2];
    c->culled += l.h_tail[3];
    c->probes += l.h_tail[4];
    c->shadow_culled += l.h_tail[5];
    if (std::getenv("PG_DEBUG_COUNTS")) {
        for (uint32_t k = 0; k < l.stats_bounces && k < l.used_prev.size(); ++k) {
            uint64_t t = 0;
            for (int w = 0; w < PG_CLASS_ROWS * PG_QSHARDS; ++w)
                t += l.h_stats[(size_t)kBounceWords * k + kClassCounts + w];
            if (t != l.used_prev[k])
                std::fprintf(stderr, "PG_DEBUG_COUNTS: chunk bounce %u: host read %llu segments, device %llu\n", k,
                             (unsigned long long)l.used_prev[k], (unsigned long long)t);
        }
    }
    const int prev = l.evcur ^ 1;
    std::vector<EventPair> &pool = l.ev[prev];
    for (size_t e = 0; e < l.evused[prev]; ++e) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, pool[e].a, pool[e].b);
        switch (l.evkind[prev][e]) {
            case KT_TRACE: c->stats.trace_ms += ms; c->stats.trace_launches++; break;
            case KT_SHADE: c->stats.shade_ms += ms; break;
            case KT_SHADOW: c->stats.shadow_ms += ms; c->stats.shadow_launches++; break;
            default: c->stats.rays_ms += ms; c->stats.rays_launches++;
        }
    }
    l.evused[prev] = 0;
    l.stats_pending = false;
    return PG_OK;
}

// Paths per chunk of a surface pass of npix x spp paths (*want), with every lane's path state allocated for it.
pg_status surfaceChunkPaths(Ctx *c, uint32_t npix, uint32_t spp, bool rec, uint32_t *want) {
    // 2^25 paths per chunk by default: bigger chunks mean fewer sparse tail bounces (each costs a
    // class-count readback) per path.  C3 with 3 lanes: 2^22 491, 2^23 552, 2^24 569, 2^25 587
    // Mpaths/s (DESIGN.md "Lanes"; round 2: 2^26 / 2^27 within noise, profiles/r02zq_chunk_ab).  Round 6, with
    // the faster kernels, C3's final render (943.7 M paths, 3 lanes) by chunk count: 30 (2^25) 633-644, 15
    // (2^26) 646-650, 12 655-660, 9 (2^27) 637-648 Mpaths/s (profiles/r06_chunk/, r06_chunk2/).  So a pass of at
    // least 3 x lanes x 2^26 paths is cut into four rounds of lanes (whole sample layers, at most 2^27 paths a
    // chunk); smaller passes (training, an N-GPU shard) keep 2^25 so every lane still gets several chunks.
    // A non-recording lane holds ~6.1 GB per 2^25 paths; recording lanes add 32 training vertices per path.
    const uint64_t total = (uint64_t)npix * spp;
    uint32_t cap = c->cfg.max_paths_in_flight ? c->cfg.max_paths_in_flight : (1u << 25);
    if (!c->cfg.max_paths_in_flight && total >= 3ull * (uint64_t)c->nlanes * (1ull << 26)) {
        const uint32_t rounds = 4u * (uint32_t)c->nlanes;
        cap = (uint32_t)std::min<uint64_t>((uint64_t)((spp + rounds - 1) / rounds) * npix, 1ull << 27);
    }
    if (!c->cfg.max_paths_in_flight) {
        // ... but at most 70 % of the device memory this context can use for path state (free memory
        // plus what its lanes already hold), e.g. when several contexts or ranks share one GPU
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB > 0) {
            size_t held = 0;
            for (int li = 0; li < c->nlanes; ++li) {
                const Lane &l = c->lanes[li];
                for (const DevBuf *b : {&l.ray, &l.hit, &l.rad, &l.vst,
                                        &l.sh_d, &l.sh_c, &l.vtx, &l.q0, &l.q1, &l.qs, &l.qp, &l.class_q, &l.aov})
                    held += b->bytes;
            }
            const int vs = vertexSlots(c, rec);
            const double perPath = 8.0 * 16 + (4 + PG_NUM_CLASSES) * 4.0 + vs * 16.0 * PG_VTX_F4 + (c->cfg.aovs ? 16.0 : 0.0);
            const double fit = 0.7 * (double)(freeB + held) / (perPath * c->nlanes);
            if (fit < (double)cap) cap = std::max<uint32_t>(1u << 20, (uint32_t)fit & ~4095u);
        }
    }
    for (;;) {
        // chunk count rounded up to whole rounds of lanes, so that the last round keeps every lane busy
        // (a rank of an N-GPU job may get only a few chunks of the final render); small passes split
        // into one chunk per lane
        uint64_t chunks = std::max<uint64_t>(1, (total + cap - 1) / cap);
        chunks = (chunks + c->nlanes - 1) / c->nlanes * c->nlanes;
        // a small pass (early training iterations, a rank's shard of them) runs as ONE chunk: three
        // lanes would each pay the whole bounce tail of launches and count readbacks for a third of
        // the paths.  Per-pixel sums keep their layer order either way.
        if (total <= smallPass()) chunks = 1;
        if ((uint64_t)npix * chunks <= total) {  // whole sample layers per chunk
            const uint64_t layers = (spp + chunks - 1) / chunks;
            *want = (uint32_t)std::min<uint64_t>(layers * npix, cap);
        } else {
            *want = (uint32_t)std::min<uint64_t>((total + chunks - 1) / chunks, cap);
        }
        const pg_status s = ensurePaths(c, *want, rec);
        if (s != PG_ERR_OOM || cap <= (1u << 20)) return s;
        // out of device memory (e.g. contexts sharing a GPU sized their chunks from the same free
        // memory): release the lanes and retry with half the chunk size, down to 2^20 paths
        releasePaths(c);
        (void)hipGetLastError();
        cap = std::max<uint32_t>(1u << 20, (cap / 2) & ~4095u);
    }
}

// one pass: the volumetric drivers above, or the surface wavefront (per bounce a trace, a count readback, a shading launch)
pg_status renderPass(Ctx *c, uint32_t spp, uint32_t sample_offset, int32_t record) {
    const uint32_t npix = (uint32_t)c->local_pixels.size();
    c->scene_rendered = true;
    if (npix == 0 || spp == 0) return PG_OK;
    if (c->cfg.integrator == PG_INTEGRATOR_VOLPATH) return renderVolpath(c, spp, sample_offset, record && c->cfg.guiding);
    const bool rec = record && c->cfg.guiding;
    uint32_t want;
    pg_status s;
    if ((s = surfaceChunkPaths(c, npix, spp, rec, &want))) return s;
    GParams g = passParams(c, rec, rec ? std::min(vertexSlots(c, rec), c->lanes[0].vtx_slots) : 0);
    g.glossy_prior = c->cfg.glossy_prior;
    SceneDev sc = sceneView(c);
    // recording passes count the triangles that block shadow rays (pg_layout.h "Shadow blockers")
    const bool learn = rec && !c->has_env && g.use_nee && !c->blk_stopped && !std::getenv("PG_NO_SHADOW_CULL");
    if (learn) {
        sc.blk_counts = c->blk_counts.as<uint32_t>();
        sc.blk_total = sc.blk_counts + c->num_tris;
    }
    const SDDev sd = sdView(c);
    const uint32_t maxBounces = std::min<uint32_t>(g.depth_cap + 2, kMaxBounces);
    const bool evt = c->cfg.kernel_timing != 0;  // per-launch HIP events (pg_stats trace/shade/shadow_ms)
    // the fused launches (k_rays: shadow rays + next closest hits; k_shade_all: every material class)
    // are what a render runs; with kernel_timing they are timed as launched (pg_stats rays_ms /
    // shade_ms), so a one-lane calibration context measures the shipped kernels
    const bool fuseRays = !std::getenv("PG_NO_RAYS_FUSION");
    // PF_DOOMED (pg_layout.h): roulette and depth exits decided one bounce early, doomed non-emitter hits culled
    // by the tracer; PG_NO_PATH_CULL=1 runs every vertex through the shader as before (same results)
    g.path_cull = std::getenv("PG_NO_PATH_CULL") ? 0 : 1;
    // doom probe (pg_layout.h): doomed rays that miss every emitter box get an any-hit probe instead of the closest-hit
    // walk; PG_NO_DOOM_PROBE=1 (or no path cull) traces them all as before (same results).  Never with an environment
    // emitter: an escaping doomed ray picks up its radiance.
    g.doom_probe = (g.path_cull && !c->has_env && !std::getenv("PG_NO_DOOM_PROBE")) ? 1 : 0;
    // ... and count the triangles their probes end on (pg_layout.h "Probe occluders"), in the second half of blk_counts
    const bool learnProbes = rec && g.doom_probe && !c->prb_stopped && probeListEnabled(c);
    if (learnProbes) {
        sc.prb_counts = c->blk_counts.as<uint32_t>() + c->num_tris + 1;
        sc.prb_total = sc.prb_counts + c->num_tris;
    }
    const bool bands = cameraBands() > 0;
    // a chunk's first launch generates the camera rays it traces (k_camera_trace, DESIGN.md section 5 "Camera fusion");
    // PG_NO_CAMERA_FUSION=1 launches the pair k_camera + k_trace as before (same results), and so does the banded
    // camera map, which has no closed-form inverse
    const bool fuseCamera = !bands && !std::getenv("PG_NO_CAMERA_FUSION");
    const bool fuseShade = !c->has_env && !std::getenv("PG_NO_SHADE_FUSION");
    // chunks: whole sample layers over the local pixels when they fit, else pixel ranges
    const std::vector<VChunk> chunks = planChunks(npix, spp, want, sample_offset);
    // filmNext: chunk whose film is next (films run in chunk order, so the float sums of a pixel do not depend on
    // which lane finishes first)
    uint32_t nextChunk = 0, filmNext = 0;
    // the lanes start after everything already queued on the context stream (film reset, uploads)
    HIPC(c, hipEventRecord(c->pass_start, c->stream));
    HIPC(c, hipEventRecord(c->film_order, c->stream));
    c->rec_bound = c->rec_host_count;
    hipStream_t laneStreams[PG_MAX_LANES];
    for (int li = 0; li < c->nlanes; ++li) laneStreams[li] = c->lanes[li].stream;
    auto lqueue = [](const Lane &l, uint32_t *items, uint32_t *counts) { return Queue{items, counts, pg_queue_stride(l.P)}; };
    // the queue bounce b's trace reads (sorted, or the shader's output of the bounce's parity) with the bounce's counters
    auto traceQueue = [&](const Lane &l, uint32_t b) {
        return lqueue(l, l.sorted ? l.qsorted.as<uint32_t>() : (b & 1) ? l.q1.as<uint32_t>() : l.q0.as<uint32_t>(),
                      l.counters.as<uint32_t>() + (size_t)kBounceWords * b);
    };
    auto classQueues = [&](const Lane &l, uint32_t *cb, Queue *cls) {
        for (int k = 0; k < PG_CLASS_ROWS; ++k)
            cls[k] = lqueue(l, k < PG_NUM_CLASSES ? l.class_q.as<uint32_t>() + (size_t)k * PG_QSHARDS * pg_queue_stride(l.P)
                                                 : nullptr,
                            cb + kClassCounts + k * PG_QSHARDS);
    };
    // trace of bounce l.b (closest hit + material-class partition), then the class counts to the host;
    // shq, pq: the previous bounce's shadow and probe queues, traced in the same launch (k_rays)
    auto launchTrace = [&](Lane &l, const Queue *shq, const Queue *pq) -> pg_status {
        uint32_t *cb = l.counters.as<uint32_t>() + (size_t)kBounceWords * l.b;
        Queue cls[PG_CLASS_ROWS];
        classQueues(l, cb, cls);
        EventPair et{};
        if (evt) et = nextEvents(&l, shq ? KT_RAYS : KT_TRACE);
        if (evt) HIPC(c, hipEventRecord(et.a, l.stream));
        const Queue tq = traceQueue(l, l.b);
        if (shq) pg_launch_rays(l.stream, g, sc, pathView(&l), tq, l.bound, cls, *shq, l.bound, *pq);
        else if (l.b == 0 && fuseCamera)  // the chunk's trace launch, the camera rays generated in it
            pg_launch_camera_trace(l.stream, g, sc, pathView(&l), c->d_band_pixels.as<uint32_t>(), l.pb, l.np, l.nl,
                                   l.sample_base, cls);
        else pg_launch_trace(l.stream, g, sc, pathView(&l), tq, l.bound, cls, l.b == 0);
        if (evt) HIPC(c, hipEventRecord(et.b, l.stream));
        HIPC(c, hipMemcpyAsync(l.h_counts + (size_t)kBounceWords * l.b + kClassCounts, cb + kClassCounts,
                               PG_CLASS_ROWS * PG_QSHARDS * 4, hipMemcpyDeviceToHost, l.stream));
        HIPC(c, hipEventRecord(l.ready, l.stream));
        return PG_OK;
    };
    // start the next chunk on lane l (none left: the lane goes inactive)
    auto startChunk = [&](Lane &l) -> pg_status {
        l.active = false;
        if (nextChunk >= chunks.size()) return PG_OK;
        if (c->cancel.load()) return fail(c, PG_ERR_CANCELLED, "cancelled");
        const VChunk &ch = chunks[nextChunk];
        l.pb = ch.pb, l.np = ch.np, l.nl = ch.nl, l.sample_base = ch.sample_base;
        l.b = 0;
        l.sorted = false;  // camera rays: their queue order is already coherent
        l.bound = pg_camera_bound(pg_camera_banded(bands, l.np), l.np, l.nl);
        l.active = true;
        l.traced = false;
        l.chunk = nextChunk++;
        HIPC(c, hipStreamWaitEvent(l.stream, c->pass_start, 0));
        HIPC(c, hipMemsetAsync(l.counters.p, 0, (size_t)kBounceWords * (maxBounces + 1) * 4, l.stream));
        HIPC(c, hipMemsetAsync(l.tail_stats.p, 0, kTailStats * 8, l.stream));
        if (!fuseCamera)
            pg_launch_camera(l.stream, g, pathView(&l), c->d_band_pixels.as<uint32_t>(), l.pb, l.np, l.nl, l.sample_base,
                             lqueue(l, l.q0.as<uint32_t>(), l.counters.as<uint32_t>()), bands);
        return launchTrace(l, nullptr, nullptr);
    };
    // film + record commit (in chunk order across lanes), statistics copy; then the next chunk
    auto finishChunk = [&](Lane &l) -> pg_status {
        pg_status st;
        if ((st = collectStats(c, l))) return st;
        const PathDev pv = pathView(&l);
        HIPC(c, hipMemcpyAsync(l.h_stats, l.counters.p, (size_t)kBounceWords * l.b * 4, hipMemcpyDeviceToHost, l.stream));
        HIPC(c, hipMemcpyAsync(l.h_tail, l.tail_stats.p, kTailStats * 8, hipMemcpyDeviceToHost, l.stream));
        HIPC(c, hipStreamWaitEvent(l.stream, c->film_order, 0));
        chunkFilm(c, l.stream, g, sc, pv, c->d_band_pixels.as<uint32_t>(), VChunk{l.pb, l.np, l.nl, l.sample_base},
                  c->aov_albedo.as<float4>(), c->aov_normal.as<float4>());
        if (rec && (st = commitRecords(c, l.stream, pv, l.np * l.nl, g.max_vertices, c->has_env ? 1 : 0, laneStreams, c->nlanes)))
            return st;
        HIPC(c, hipEventRecord(c->film_order, l.stream));
        HIPC(c, hipEventRecord(l.done, l.stream));
        HIPC(c, hipGetLastError());
        l.stats_pending = true;
        l.stats_bounces = l.b;
        l.used_prev.swap(l.used_cur);
        l.used_cur.clear();
        l.evcur ^= 1;
        c->stats.paths += (uint64_t)l.np * l.nl;
        return startChunk(l);
    };
    // one bounce's shading + shadow rays + next trace on lane l (class counts already on the host)
    auto advance = [&](Lane &l) -> pg_status {
        HIPC(c, hipEventSynchronize(l.ready));
        uint32_t *cb = l.counters.as<uint32_t>() + (size_t)kBounceWords * l.b;
        const uint32_t *hc = l.h_counts + (size_t)kBounceWords * l.b + kClassCounts;
        uint32_t clsMax[PG_NUM_CLASSES], shardLive[PG_QSHARDS] = {};
        uint64_t nlive = 0;
        for (int k = 0; k < PG_CLASS_ROWS; ++k) {
            uint32_t m = 0;
            for (int sh = 0; sh < PG_QSHARDS; ++sh) {
                const uint32_t v = hc[k * PG_QSHARDS + sh];
                c->stats.segments += v;
                if (k >= PG_NUM_CLASSES) {  // counted only: neither shaded nor alive
                    (k == PG_CLASS_ESCAPED ? c->stats.escaped : c->culled) += v;
                    continue;
                }
                m = std::max(m, v);
                shardLive[sh] += v;
                nlive += v;
            }
            if (k < PG_NUM_CLASSES) clsMax[k] = m;
        }
        {
            uint64_t t = 0;
            for (int w = 0; w < PG_CLASS_ROWS * PG_QSHARDS; ++w) t += hc[w];
            l.used_cur.push_back(t);
        }
        ++l.b;
        const uint32_t tailMax = c->cfg.tail_paths < 0 ? 0u : c->cfg.tail_paths > 0 ? (uint32_t)c->cfg.tail_paths : tailPaths();
        const bool tail = nlive > 0 && nlive <= tailMax && l.b < maxBounces;
        if (tail) {  // one launch finishes every remaining path (shading starts at the hits just traced)
            // straight after the camera rays it walks the camera queue, which the fused first launch did not store
            if (l.b == 1 && fuseCamera) pg_launch_camera_queue(l.stream, l.np, l.nl, traceQueue(l, 0));
            pg_launch_tail(l.stream, g, sc, sd, pathView(&l), traceQueue(l, l.b - 1), l.bound,
                           l.tail_stats.as<unsigned long long>());
            c->stats.tail_launches += 1;
        }
        if (nlive == 0 || tail || l.b >= maxBounces) {
            l.traced = true;
            // finish this lane and every waiting lane whose turn comes after it, in chunk order
            for (int k = 0; k < c->nlanes; ++k) {
                Lane &o = c->lanes[k];
                if (!(o.active && o.traced && o.chunk == filmNext)) continue;
                ++filmNext;
                if (pg_status st = finishChunk(o)) return st;
                k = -1;  // the next chunk in film order may wait on any lane
            }
            return PG_OK;
        }
        Queue cls[PG_CLASS_ROWS];
        classQueues(l, cb, cls);
        const PathDev pv = pathView(&l);
        Queue next = lqueue(l, (l.b & 1) ? l.q1.as<uint32_t>() : l.q0.as<uint32_t>(), cb + kBounceWords);
        Queue shq = lqueue(l, l.qs.as<uint32_t>(), cb + kShadowCounts);
        shq.dropped = cb + kDropCounts;
        Queue pq = lqueue(l, l.qp.as<uint32_t>(), cb + kProbeCounts);
        pq.dropped = cb + kResolvedCounts;
        const uint32_t nextBound = *std::max_element(shardLive, shardLive + PG_QSHARDS);
        const bool sortNext = raySortEnabled() && nextBound >= kRaySortMinShard;
        if (sortNext) next.keys = l.qkey.as<uint16_t>();
        EventPair es{}, ew{};
        if (evt) es = nextEvents(&l, KT_SHADE);
        if (evt) HIPC(c, hipEventRecord(es.a, l.stream));
        if (fuseShade) {  // one launch for every class present
            pg_launch_shade_all(l.stream, g, sc, sd, pv, cls, clsMax, next, shq, pq);
            c->stats.shade_launches += 1;
        } else {
            for (int k = 0; k < PG_NUM_CLASSES; ++k) {
                pg_launch_shade_class(l.stream, k, g, sc, sd, pv, cls[k], clsMax[k], next, shq, pq);
                c->stats.shade_launches += clsMax[k] ? 1 : 0;
            }
        }
        if (evt) HIPC(c, hipEventRecord(es.b, l.stream));
        l.bound = nextBound;
        if (sortNext)  // group every shard of the next closest-hit queue by ray order key
            pg_launch_ray_sort(l.stream, next, l.bound, l.qsorted.as<uint32_t>(), l.rsort_hist.as<uint32_t>());
        l.sorted = sortNext;
        // without per-launch timing the shadow rays share the next trace's launch
        if (fuseRays) return launchTrace(l, &shq, &pq);
        if (evt) ew = nextEvents(&l, KT_SHADOW);
        if (evt) HIPC(c, hipEventRecord(ew.a, l.stream));
        pg_launch_shadow(l.stream, g, sc, pv, shq, l.bound);
        if (g.doom_probe) {  // the probes of this bounce, counted with the closest hits of the trace that follows
            Queue ncls[PG_CLASS_ROWS];
            classQueues(l, cb + kBounceWords, ncls);
            pg_launch_probe(l.stream, sc, pv, pq, l.bound, ncls);
        }
        if (evt) HIPC(c, hipEventRecord(ew.b, l.stream));
        return launchTrace(l, nullptr, nullptr);
    };
    for (int li = 0; li < c->nlanes; ++li)
        if ((s = startChunk(c->lanes[li]))) return s;
    // advance whichever lane has its counts first (waiting on a fixed lane order leaves the GPU idle
    // whenever the other lane is already ready)
    for (uint32_t rr = 0;; ++rr) {
        int active = 0, picked = -1;
        for (int k = 0; k < c->nlanes && picked < 0; ++k) {
            Lane &l = c->lanes[(rr + k) % c->nlanes];
            if (!l.active) continue;
            ++active;
            if (l.traced) continue;  // waiting for an earlier chunk's film
            const hipError_t q = hipEventQuery(l.ready);
            if (q == hipSuccess) picked = (int)((rr + k) % c->nlanes);
            else if (q != hipErrorNotReady) HIPC(c, q);
        }
        if (!active) break;
        if (picked >= 0 && (s = advance(c->lanes[picked]))) return s;
    }
    for (int li = 0; li < c->nlanes; ++li) {
        Lane &l = c->lanes[li];
        HIPC(c, hipStreamSynchronize(l.stream));
        if ((s = collectStats(c, l))) return s;
    }
    if (rec && (s = foldRecordCount(c))) return s;
    HIPC(c, hipStreamSynchronize(c->stream));
    if ((learn || learnProbes) && (s = learnBlockers(c, learn, learnProbes))) return s;
    return PG_OK;
}

// Every exit of a pass that did not complete (cancellation, a HIP error): the lane streams are created
// non-blocking, so nothing queued later on c->stream (pg_read_film, pg_reset_film) orders after them.
// Wait for them, so that no lane kernel still writes the film or the records once pg_render_pass has
// returned, and release the chunk span events a volumetric lane had not handed over yet.
void drainLanes(Ctx *c) {
    for (int li = 0; li < c->nlanes; ++li)
        if (c->lanes[li].stream) (void)hipStreamSynchronize(c->lanes[li].stream);
    for (VolLane &l : c->vlanes) {
        if (l.nstream) (void)hipStreamSynchronize(l.nstream);
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        l.npending = false;
        if (l.span.a) (void)hipEventDestroy(l.span.a);
        if (l.span.b) (void)hipEventDestroy(l.span.b);
        l.span = EventPair{};
        l.active = l.waved = false;
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
}

}  // namespace pgh

using namespace pgh;

extern "C" {

pg_status pg_render_pass(void *ctx, uint32_t spp, uint32_t sample_offset, int32_t record) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return fail(nullptr, PG_ERR_INVALID, "pg_render_pass: null context");
    if (!c->has_scene) return fail(c, PG_ERR_STATE, "pg_render_pass: no scene uploaded");
    if (c->cancel.load()) return fail(c, PG_ERR_CANCELLED, "cancelled");
    HIPC(c, hipSetDevice(c->cfg.device));
    c->rendered = true;
    const pg_status s = renderPass(c, spp, sample_offset, record);
    if (s) drainLanes(c);
    return s;
}

// ProgressiveMonteCarloIntegrator::renderTime (progressiveintegrator.cpp:117-168): whole
// progressions until the wall-clock budget is spent.  The reference checks the timer after every
// progression of a 128-progression batch and cancels the rest; here consecutive progressions are
// merged into one pg_render_pass (the film adds samples in sample order, so a merged pass equals
// its progressions bit for bit), each merge covering at most half the remaining budget at the
// measured rate, so the overshoot stays below one progression plus one readback.  Only whole
// progressions reach the film: every pixel holds the same sample count (the reference may cancel
// a progression midway, leaving some blocks with one progression more).
pg_status pg_render_time(void *ctx, double seconds, uint32_t spp_per_progression, uint32_t sample_offset,
                         uint32_t max_spp, uint32_t *spp_done) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !spp_done) return fail(c, PG_ERR_INVALID, "pg_render_time: null argument");
    *spp_done = 0;
    if (!(seconds > 0) || spp_per_progression == 0)
        return fail(c, PG_ERR_INVALID, "pg_render_time: need seconds > 0 and spp_per_progression > 0");
    const uint32_t limit = max_spp ? max_spp : 0x7FFFFFFFu;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t done = 0, batch = std::min(spp_per_progression, limit);
    while (done < limit) {
        pg_status s = pg_render_pass(ctx, batch, sample_offset + done, 0);
        if (s) return s;
        done += batch;
        *spp_done = done;
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el >= seconds) break;
        const double perProg = el / (done / spp_per_progression);
        const double progs = std::floor(0.5 * (seconds - el) / std::max(perProg, 1e-9));
        const uint64_t want = (uint64_t)std::max(1.0, std::min(progs, 1e6)) * spp_per_progression;
        batch = (uint32_t)std::min<uint64_t>(want, limit - done);
        batch -= batch % spp_per_progression;  // whole progressions
        if (batch == 0) break;
    }
    return PG_OK;
}

}  // extern "C"
