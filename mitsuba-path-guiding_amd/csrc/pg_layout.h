// GPU record layouts shared by the host driver (pg_host.cpp) and the kernels (pg_kernels.hip).
// Sizes are static_asserted; DESIGN.md §"Data layout in HBM" documents them.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pg_capi.h"

// Material record: 128 B (8 x 16 B), derived constants precomputed on the host (BSDF::configure()).
struct GMat {
    uint32_t model, dist, flags, type;  // pg BSDF model, microfacet distribution, PG_MAT_* flags, EBSDFType bits
    float alpha_u, alpha_v, eta, invEta;
    float invEta2, fdrInt, specWeight, wbound;  // wbound: max channel of BSDF::getAlbedo (guide-fraction bound)
    float diff[4];
    float spec[4];
    float trans[4];
    union {
        float ceta[4];
        struct {
            const float *rtrans;  // roughplastic: external rough-transmittance table (device)
            float pad1[2];
        };
    };
    float ck[4];
};
static_assert(sizeof(GMat) == 128, "GMat layout");

// Area emitter record: 32 B.  Triangles of emitter e are em_tri[tri_begin, tri_begin + tri_count),
// each with its normalized area-CDF entry em_cdf[tri_begin + 1 + i] (em_cdf[tri_begin] = 0 slot
// lives at index tri_begin + e, see pg_host.cpp: cdf arrays are stored with one leading zero each).
struct GEmitter {
    uint32_t tri_begin;   // into em_tri
    uint32_t tri_count;
    uint32_t cdf_begin;   // into em_cdf (tri_count + 1 entries)
    float inv_area;
    float radiance[4];
};
static_assert(sizeof(GEmitter) == 32, "GEmitter layout");

// Environment emitter record: 128 B (EnvironmentMap, envmap.cpp:260-329).  texels: width x height
// float4 (rgb rounded to half precision, as the reference's SpectrumHalf MIP level 0; w = 0), row
// y = theta.  cdf_rows: height + 1 marginal CDF entries; cdf_cols: height rows of width + 1
// conditional CDF entries; row_weights: sin((y + 0.5) pi / height).  R: toWorld rotation,
// row-major (world = R local, local = R^T world).  center/radius: the scene's bounding sphere
// enlarged by 1.5 (EnvironmentMap::createShape, envmap.cpp:331-356).
struct GEnv {
    const float *texels;  // float4 per texel
    const float *cdf_rows;
    const float *cdf_cols;
    const float *row_weights;
    uint32_t width, height;
    float scale, normalization;
    float pixel_size[2];
    float radius, pad0;
    float center[3], pad1;
    float R[9];
    float pad2[3];
};
static_assert(sizeof(GEnv) == 128, "GEnv layout");

// Delta emitter record: 64 B (pg_set_delta_emitters; pg_capi.h pg_delta_emitter).  type: PG_EMITTER_*.  dir: the
// spot's axis / the direction a directional light travels, unit length.  Spot: cos_cutoff, cos_beam and
// inv_transition = 1 / (cutoff - beam) as SpotEmitter::configure precomputes them (spot.cpp:105-125).  Directional:
// pos is the centre of the disk the light leaves from (bounding-sphere centre - dir * radius, directional.cpp:159-180)
// and intensity the irradiance on a surface normal to dir.
struct GDelta {
    float pos[3];
    uint32_t type;
    float dir[3];
    float cutoff;
    float intensity[3];
    float cos_cutoff;
    float cos_beam, inv_transition;
    float pad[2];
};
static_assert(sizeof(GDelta) == 64, "GDelta layout");

// Texture record: 64 B (pg_set_textures; pg_capi.h pg_texture).  texels: width x height float4 (rgb, 0), row y at
// texels + 4 * y * width; nullptr for a checkerboard.  mode: type | filter << 4 | wrap_u << 8 | wrap_v << 12.
struct GTex {
    const float *texels;
    uint32_t width, height;
    uint32_t mode, pad0;
    float uscale, vscale, uoffset, voffset;
    float color0[3], color1[3];
};
static_assert(sizeof(GTex) == 64, "GTex layout");
// Per BVH-order triangle uv record (SceneDev::tuv, allocated only while textures are set): t0.xy, t1.xy | t2.xy, 0, 0;
// 2 x float4 = 32 B, so both 16-B loads stay within one 128-B line.  Without texcoords: (0, 0), (1, 0), (0, 1).
#define PG_TRI_UV_F4 2

// Heterogeneous medium record: 128 B (volpath).  World -> grid is g = p * gs + go
// (gridvolume.cpp:186-198); invMax = 1 / (scale * maxFloatValue), maxFloatValue = 1
// (gridvolume.cpp:583-585, heterogeneous.cpp:236-242).  density: res x*y*z floats, x fastest.
// maj: the majorant grid, mx*my*mz cells of PG_MAJORANT_CELL^3 voxels, each scale * the maximum
// voxel over the cell extended by one voxel per side.
// A homogeneous entry (pg_set_homogeneous_media; pg_volpath.hip "homogeneous medium") reuses the record, so VolDev::media
// stays one array indexed by the shapes' medium ids: bx = 1 marks it, gs holds sigma_t, go sigma_s and scale the
// medium sampling weight; g, lo and hi keep their meaning (lo / hi: the flight queue's order key only), the other
// grid fields are not read.
#ifndef PG_MAJORANT_CELL
#define PG_MAJORANT_CELL 16  // voxels per majorant cell and axis (oracle: orc_medium.h kCell)
#endif
struct GMedium {
    const float *density;
    uint32_t resx, resy;
    uint32_t resz;
    float scale, invMax, g;
    float lo[3];
    uint32_t mx;
    float hi[3];
    uint32_t my;
    float gs[3];
    uint32_t mz;
    float go[3];
    uint32_t bx;  // 1: a homogeneous entry (above); 0: a density grid
    float albedo[3];
    uint32_t by;  // unused (0)
    const float *maj;
    uint32_t pad4, pad5;
};
static_assert(sizeof(GMedium) == 128, "GMedium layout");
// Corner-packed density (the only layout lookupDensity reads; an upload that cannot hold it fails with
// PG_ERR_OOM): cell (x, y, z) of the
// (rx-1)(ry-1)(rz-1) cells between voxel centres stores its 8 corner voxels, 32 B in lookup order
// (z, y, x bits: d000 d001 d010 d011 | d100 d101 d110 d111), so a trilinear lookup is two aligned
// 16-B loads instead of eight scattered 4-B loads over four cache lines.  8x the memory of the grid
// (530 MB for 256^3): a trade the 288 GB of HBM3E affords.

// Triangle records of both BVHs (48 B = 3 x float4 per BVH-order triangle, three consecutive rows): the
// reference's own triangle test, TriAccel (include/mitsuba/render/triaccel.h:37-157; the oracle's
// orc_scene.h TriAccel): (n_u, n_v, n_d, bits(k)), (a_u, a_v, b_nu, b_nv), (c_nu, c_nv, bits(original
// triangle id), 0), built in fp32 as TriAccel::load builds it and tested with contraction off, so a hit's
// t and barycentrics are the oracle's bit for bit; k = 3 marks a degenerate triangle (NaN plane: never
// hit).
// float4 index of row r (0-2) of BVH-order triangle tr; PG_TRI_F4(nt) float4 for nt triangles
#define PG_TRI_ROW(tr, r) (3u * (uint32_t)(tr) + (r))
#define PG_TRI_F4(nt) (3u * (uint32_t)(nt))

// Volumetric flight order key (pg_volpath.hip flightKey): 8^3 cells, 512 sort bins
#define PG_VOL_SORT_BINS 512u

// Per-triangle shading record (5 x float4 = 80 B), indexed by BVH-order triangle id:
//   [0] p0.xyz, bits(material | (emitter + 1) << 16)
//   [1] p1.xyz, n2.z
//   [2] p2.xyz, bits(original triangle id)
//   [3] n0.xyz, n1.x
//   [4] n1.y, n1.z, n2.x, n2.y
// The same layout is used for the compact emitter-triangle array.
#define PG_TRI_SHADE_F4 5
// float4 per triangle in the BVH-order array (tshade).  The emitter-triangle array keeps PG_TRI_SHADE_F4.
#define PG_TRI_SHADE_STRIDE PG_TRI_SHADE_F4

// 4-wide BVH node for closest-hit rays (4 x float4 = 64 B), collapsed from the binary tree the 8-wide BVH
// is collapsed from (C3 +1.5 %, kitchen +6.9 %, C5 +3.1 % over binary nodes, identical results;
// profiles/r03za_bvh4_ab), with child boxes quantised to bytes in the node's frame (as the 8-wide shadow nodes):
//   [0] origin.xyz (the node box's lo corner), bits((e_x + 127) | (e_y + 127) << 8 | (e_z + 127) << 16)
//   [1] bits(child[4]): child >= 0: inner node index; child < 0: leaf, ~child = (first_tri << 4) | count
//       (count <= 15); PG_QNODE_EMPTY: unused slot
//   [2] u32 lo.x, hi.x, lo.y, hi.y  [3] u32 lo.z, hi.z, 0, 0   -- byte s of each word: slot s's plane
// plane = origin + q * 2^e, rounded outward (floor / ceil, checked against the fp32 reconstruction);
// an empty slot has lo = 255, hi = 0 (an inverted box) and the PG_QNODE_EMPTY ref
#define PG_QNODE_F4 4
#define PG_QNODE_EMPTY 0x7ffffffe
// The 4-wide nodes of the top PG_BVH4_TOP_LEVELS + 1 levels come first, breadth first (round 5; the rest
// depth first): nodes [0, SceneDev.top_nodes), at most 1 + 4 + 16 = 21.  No kernel reads the count; the
// order decides the node indices.
#ifndef PG_BVH4_TOP_LEVELS
#define PG_BVH4_TOP_LEVELS 2
#endif
#define PG_BVH4_TOP_NODES 21
// closest-hit stack entries a 4-wide traversal may need (the builder checks its trees against it;
// the global overflow ring already holds PG_QSTACK_DEPTH - LDS_STACK words per thread)
#define PG_QSTACK_DEPTH 96
// host-side accessors of a 4-wide node (tests/csrc/bvh_shim.cpp): slot s's ref and box
inline int32_t pg_qnode_ref(const float *node, int s) {
    int32_t r;
    __builtin_memcpy(&r, node + 4 + s, 4);
    return r;
}
inline void pg_qnode_box(const float *node, int s, float lo[3], float hi[3]) {
    uint32_t e, w[6];
    __builtin_memcpy(&e, node + 3, 4);
    __builtin_memcpy(w, node + 8, 24);
    for (int a = 0; a < 3; ++a) {
        uint32_t eb = ((e >> (8 * a)) & 0xFFu) << 23;
        float scale;
        __builtin_memcpy(&scale, &eb, 4);
        lo[a] = node[a] + (float)((w[2 * a] >> (8 * s)) & 0xFFu) * scale;
        hi[a] = node[a] + (float)((w[2 * a + 1] >> (8 * s)) & 0xFFu) * scale;
    }
}

// 8-wide BVH node for shadow rays, with quantised child boxes (5 x float4 = 80 B; after Ylitie et al. 2017):
//   [0] p.xyz (quantisation origin = node box min), bits(ex | ey << 8 | ez << 16 | imask << 24)
//       child box coordinate = p + q * 2^(e - 127) per axis; imask bit s: slot s is an inner node
//   [1] child_base (inner children are consecutive nodes, in slot order), tri_base (leaf triangles
//       are consecutive BVH-order triangles, in slot order), meta[8] (bytes): leaf slot s =
//       offset from tri_base | count << 5 (count 1..3), 0 = empty slot
//   [2] qlo.x[8] qlo.y[8]   [3] qlo.z[8] qhi.x[8]   [4] qhi.y[8] qhi.z[8]   (uint8, slot order)
// Slot s holds the child that rays of direction octant s (bit a = negative along axis a) should
// visit first, so traversal orders hits by slot ^ (7 - octant) without sorting.
// PG_WIDE_NODE_F4: float4 per node
#define PG_WIDE_NODE_F4 5
#define PG_WIDE_LEAF_MAX 3

// Material classes of the per-bounce shading queues (k_classify -> k_shade<MODEL>)
#define PG_CLASS_DIFFUSE 0
#define PG_CLASS_ROUGHCONDUCTOR 1
#define PG_CLASS_ROUGHDIELECTRIC 2
#define PG_CLASS_PLASTIC 3
#define PG_CLASS_ROUGHPLASTIC 4
#define PG_CLASS_DELTA 5
// materials whose diffuse reflectance is a texture (pg_set_textures), whatever their model: the run-time-model body
// with the lookup compiled in (shadeOne's TEX flag).  Empty unless textures are bound, so the other classes' bodies
// never see a textured vertex.
#define PG_CLASS_TEXTURED 6
#define PG_NUM_CLASSES 7
// counted-only rows after the class queues' shard counts: escaped rays, then culled hits (PF_DOOMED below)
#define PG_CLASS_ESCAPED PG_NUM_CLASSES
#define PG_CLASS_CULLED (PG_NUM_CLASSES + 1)
#define PG_CLASS_ROWS (PG_NUM_CLASSES + 2)
// SceneDev::tclass[tri]: the class in the low bits, bit 7 set on an emitter's triangles
#define PG_TCLASS_EMITTER 0x80u
#define PG_TCLASS_MASK 0x7Fu

// Path state of the surface wavefront, 16-B rows per slot (PathDev, pg_kernels.h).  The rows that are always touched
// together are the halves of one 32-B record, so a slot of a sparse wave costs one sector for both (DESIGN.md
// section 5 "Paired state"); hit, rad, sh_d and sh_c are arrays of their own, one row per slot:
//   ray[2 slot] = ray_o, ray[2 slot + 1] = ray_d     (pathRayO, pathRayD)
//   vst[2 slot] = pinfo, vst[2 slot + 1] = thr       (pathInfo, pathThr)
//   camera ray (k_camera_trace, the chunk's first launch: generated and traced there, DESIGN.md section 5 "Camera
//                           fusion"):  ray_d = (direction, far clip); the far clip has no reader (the walk that takes
//                           it is in the same launch), a depth-1 vertex reads the direction only
//                           pinfo = (pixel, sample, 1 | PF_EMITTED_QUERY << 16, 0)   rad = 0   thr: implied (1, eta 1),
//                           its half of the record keeps what the slot's previous path left there, and so does ray_o:
//                           the origin and the near clip are not stored (shadeOne recomputes the hit point from the
//                           barycentrics and stores ray_o before anything reads it), nor is the camera queue
//                           (pg_kernels.h pg_camera_slot).  PG_NO_CAMERA_FUSION=1 and PG_CAMERA_BANDS run k_camera +
//                           k_trace<., true>: k_camera stores ray_o = (camera position, near clip along the ray) and
//                           the queue as well, and k_trace reads them back
//   bounce ray (shadeOne):  ray_o = (p, +-tmin)   ray_d = (wo, woPdf)   thr = (T, eta)
//                           pinfo.zw = (depth | flags << 16, training-vertex count), an 8-B store: with thr one
//                           contiguous 24-B span of the vst record
// A bounce ray's tmax is +inf, so the tracers take it as a constant (their CAM template flag tells camera rows from
// bounce rows) and ray_d.w carries woPdf, the solid-angle pdf wo was sampled with.  It is read only by a vertex that
// lands on an emitter and by an escape into the environment emitter, for the MIS weight against next-event
// estimation; both hold ray_d already.  tmin = pg_ray_tmin(p) stays in ray_o.w with PF_DOOMED in its sign: recomputing
// it in the tracers and moving depth | flags into ray_d.w (so that pinfo is not rewritten) was built and measured,
// and cost k_rays<false> seven more spilled VGPRs and 15 % of its time (DESIGN.md section 5 "Lean state").
// There is no row for the previous vertex: PF_PREV_FRONT below replaces its reference normal.  L (rad) is loaded
// only by a vertex that adds emission or snapshots a training vertex.
// A path that ends while it still owes a shadow ray keeps ray_o = (p, 0): the shadow rows derive their own tmin.
//
// Path-state flags (pinfo.z high bits; stPinfoZW writes depth | flags << 16 with the vertex count)
#define PF_SCATTERED 0x1u
#define PF_EMITTED_QUERY 0x2u
#define PF_PREV_DELTA 0x4u
// The extension ray leaves the vertex that wrote it on the side of that vertex's reference normal:
// pg_prev_front(wo, refN), with refN = 0 (transmissive or back-side lobes: always true) as the emitter-hit MIS of
// the next vertex wants it.  That vertex's ray direction is this vertex's wo bit for bit, so the writer evaluates
// the test and the reader needs neither the normal nor a row to keep it in.
#define PF_PREV_FRONT 0x10u
// The vertex this ray leads to ends before it samples anything: the shader that wrote the ray already made its
// Russian-roulette draw (same key, sample, dimension, throughput and eta the vertex would use) and lost, or the
// vertex is past depth_cap / at max_depth.  Such a vertex can only add the emission of an emitter it hits, so
//   - the ray carries the bit in the sign of ray_o.w (tmin > 0; the closest-hit walks take |w|), and a doomed ray
//     that hits a non-emitter is culled by the tracer: its hit record is stored as a miss (0, ~0, 0, 0), it joins
//     no class queue and is counted in the PG_CLASS_CULLED row;
//   - a doomed ray that hits an emitter is shaded: shadeOne adds the MIS-weighted emission, sees PF_DOOMED and
//     stops where the roulette draw used to be;
//   - without an environment emitter, a doomed ray that misses every emitter box is not traced at all ("Doom probe"
//     below): its path ends in the shader and an any-hit probe decides culled against escaped.
// Set only while GParams::path_cull is on; then a vertex without the flag has survived its roulette.
#define PF_DOOMED 0x8u

// Doom probe: emitter bounds (SceneDev::em_box, scenes without an environment emitter).  A doomed ray matters only
// if its closest hit is an emitter triangle, so shadeOne slab-tests it against up to PG_EMBOX_MAX axis-aligned boxes
// over the emitter triangles (one per emitter, or their union beyond PG_EMBOX_MAX).  A ray that misses every box
// cannot end on an emitter: it is not queued for the closest-hit walk, and an any-hit probe of the same 4-wide
// nodes only decides `culled` against `escaped` (pg_kernels.hip probeRows).
// Why the test never rejects a ray the walk could return an emitter for: TriAccel accepts a hit at its fp32 t >=
// tmin when the ray's point at t projects into the triangle, up to the rounding of (o + t d), and the plane solve
// leaves that point off the triangle's plane by at most ~100 ulps of max(|o|, |vertex|) (grazing
// rays far from the origin).  So the exact ray passes within ~6e-6 max(|o|, |vertex|) of the triangle at some
// t >= tmin.  Every box is padded on all sides by 1e-3 of its largest extent plus 1e-3 of its largest absolute
// coordinate (160 times that bound for an origin no farther out than the box), and the slab test widens every
// interval by 2^-16 (max|o| + the boxes' largest |coordinate|) along each axis, which covers both an origin far
// outside the boxes and the rounding of (plane - o) idir; intervals are compared with a relative slack of 2^-20 and
// NaNs (inf - inf for axis-parallel rays) drop out of fminf / fmaxf, which can only widen the interval.
#define PG_EMBOX_MAX 8
#if defined(__HIPCC__)
#define PG_HD __host__ __device__
#else
#define PG_HD
#endif
// tmin of a ray that leaves a surface at p (Epsilon * max(max |p_i|, Epsilon), the reference's ray epsilon; Epsilon
// is pg_device.h kEpsilon).  shadeOne computes it once per extension ray, for its box test and for ray_o.w.
#define PG_RAY_EPSILON 1e-4f
PG_HD inline float pg_ray_tmin(float px, float py, float pz) {
    return PG_RAY_EPSILON * fmaxf(fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)), PG_RAY_EPSILON);
}
// PF_PREV_FRONT of an extension ray wo written at a vertex with reference normal n: dot(wo, n) >= 0, summed in
// pg_device.h dot's order and never contracted
PG_HD inline bool pg_prev_front(float wx, float wy, float wz, float nx, float ny, float nz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return wx * nx + wy * ny + wz * nz >= 0;
}
// boxes: (lo.xyz, hi.xyz) each, padded; absmax: the largest |coordinate| of any of them.  True: the ray o + t d,
// t >= tmin, misses every box.
PG_HD inline bool pg_ray_misses_boxes(const float (*boxes)[6], uint32_t n, float absmax, const float o[3], const float d[3],
                                      float tmin) {
    const float eps = 1e-30f;  // slabRay's guard of a zero direction component
    const float s = 1.52587891e-5f * (fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2])) + absmax);  // 2^-16
    float idir[3], pad[3];
    for (int a = 0; a < 3; ++a) {
        idir[a] = 1.0f / (fabsf(d[a]) > eps ? d[a] : copysignf(eps, d[a]));
        pad[a] = s * fabsf(idir[a]);
    }
    for (uint32_t b = 0; b < n; ++b) {
        float tn = tmin, tf = __builtin_huge_valf();
        for (int a = 0; a < 3; ++a) {
            const float t0 = (boxes[b][a] - o[a]) * idir[a], t1 = (boxes[b][3 + a] - o[a]) * idir[a];
            tn = fmaxf(tn, fminf(t0, t1) - pad[a]);
            tf = fminf(tf, fmaxf(t0, t1) + pad[a]);
        }
        if (tn <= tf + 9.53674316e-7f * fabsf(tf)) return false;
    }
    return true;
}
// Host: the padded boxes of a scene's emitter triangles.  tri_emitter[t]: emitter index + 1 of triangle t, 0 for
// none.  Returns the number of boxes (0: no emitter triangle) and their largest |coordinate| in *absmax.
inline uint32_t pg_emitter_boxes(const float *positions, const uint32_t *indices, const uint32_t *tri_emitter, uint32_t nt,
                                 uint32_t num_emitters, float (*boxes)[6], float *absmax) {
    const float inf = __builtin_huge_valf();
    uint32_t n = 0;
    // one box per emitter while they fit; from the first emitter past PG_EMBOX_MAX on, one union of all
    const bool single = num_emitters > PG_EMBOX_MAX;
    for (uint32_t e = 0; e < (single ? 1u : num_emitters); ++e) {
        float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
        for (uint32_t t = 0; t < nt; ++t) {
            if (tri_emitter[t] == 0 || (!single && tri_emitter[t] != e + 1)) continue;
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) {
                    const float x = positions[3 * (size_t)indices[3 * (size_t)t + k] + a];
                    lo[a] = fminf(lo[a], x);
                    hi[a] = fmaxf(hi[a], x);
                }
        }
        if (!(lo[0] <= hi[0])) continue;  // an emitter without triangles
        float ext = 0.0f, mag = 0.0f;
        for (int a = 0; a < 3; ++a) {
            ext = fmaxf(ext, hi[a] - lo[a]);
            mag = fmaxf(mag, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
        }
        const float padding = 1e-3f * ext + 1e-3f * mag;
        for (int a = 0; a < 3; ++a) {
            boxes[n][a] = lo[a] - padding;
            boxes[n][3 + a] = hi[a] + padding;
        }
        ++n;
    }
    *absmax = 0.0f;
    for (uint32_t b = 0; b < n; ++b)
        for (int a = 0; a < 6; ++a) *absmax = fmaxf(*absmax, fabsf(boxes[b][a]));
    return n;
}

// Shadow blockers (SceneDev::blk): where next-event estimation almost always fails (an emitter behind a small
// opening), nearly every shadow ray ends on one of a few large triangles.  The any-hit rows of the recording passes
// count, per triangle, the shadow rays it blocked; after each recording pass the host lists up to PG_MAX_BLOCKERS
// triangles that each blocked at least 1 / PG_BLOCKER_MIN_SHARE of all shadow rays of the recording passes, and
// keeps the list only if together they blocked at least half of those rays (pg_select_blockers): where the light is
// mostly visible the tests would cost every NEE vertex more than the few walks they save.  Then
// shadeOne tests a new shadow ray against the listed TriAccel records before it stores anything: a certain hit drops
// the ray (its stores, its queue entry and its any-hit walk), exactly as shadowRows would have dropped its
// contribution.  The list only decides which rays are resolved early, never a result.
//
// "Certain" (pg_ray_hits_blockers): the shortcut may say "occluded" only where the 8-wide walk says it too.  The
// walk's leaf test of the blocker is this test bit for bit (same record, o, d, tmin, tmax), so the walk accepts the
// blocker if it reaches its leaf, i.e. if every ancestor slot passes max(tn_x, tn_y, tn_z, tmin) <= min(tf_x, tf_y,
// tf_z, tmax) with tn_a = fma(q, 2^e idir_a, fma(p_a, idir_a, -(o_a idir_a)) - pad_a) and tf_a the same + pad_a,
// pad_a = 2^-21 (|o_a idir_a| + |p_a idir_a| + 256 |2^e idir_a|) (pg_trace.h traverseWide, wideRay).  The planes
// X = p + q 2^e are rounded outward, so they enclose the triangle; q 2^e idir is exact, and the roundings of idir,
// o idir, the padded addends and the fmas displace a computed plane by at most 5 * 2^-24 of those three terms, i.e.
// by less than d_pos = 2^-21 E along its axis, E = the scene's largest |coordinate| + max |o_i| (an origin inside
// the scene: |p|, |o|, |X - o| <= E).  In t that is d_pos / |d_a|.  The pad is larger than these roundings and
// moves the near plane earlier and the far plane later only, so it never closes a slot that the exact planes leave
// open: "blocker says occluded => walk says occluded" holds as it did for the unpadded walk this derivation was
// first written for, whose margins are kept.  They make the exact hit point P clear every plane displaced by d_pos:
//   - barycentrics u, v, 1 - u - v >= 2^-10.  TriAccel's own t carries at most 2^-22 E / |den| of cancellation
//     (den = d.n / n_k), with |den| >= max|d| / 16 below that moves the point by <= 2^-18 E and, for a triangle whose
//     box is at least E / 32 wide on both axes other than k (rec[11], set by the host: pg_blocker_record), its
//     barycentrics by <= 2^-12: P's true weights are >= 2^-11, so P is at least 2^-11 W >= 2^-16 E inside the
//     triangle's box on those two axes;
//   - |d_k| >= max|d| / 16 (k = the record's projection axis, the one axis the box may be flat on).  A pair of slabs
//     (a, b) stays ordered when one of them has slack >= d_pos (1 + |d_a| / |d_b|): with the flat axis as b that is
//     17 d_pos = 2^-17 E on the other axis, half of what the barycentric margin leaves; the two wide axes cover
//     each other with 2 d_pos;
//   - t in [tmin + 2^-10 tmax, tmax - 2^-10 tmax] and tmax max|d| >= E / 32: the flat axis' planes sit at t -+
//     (d_pos / |d_k| + the error of t) <= 1.5 * 2^-17 E / max|d| <= 2^-10 tmax / 2.6, inside [tmin, tmax].  (The shrink
//     is absolute at both ends: tmin is only 1e-4 of the origin, so a shrink relative to tmin would be far less than a
//     plane's rounding.)
//   - every |d_a| > 1e-30: the walk replaces a smaller component by +-1e-30 (and picks near / far by the sign of
//     that reciprocal, -0.0 included) -- such a ray is left to the walk.
// A ray that fails any margin is queued and walked as before.  The margins cost a negligible share of the culls.
// Only every PG_BLOCKER_SAMPLE-th row (a block's share of a queue shard) is counted, with the number of shadow rays in those rows as
// the total the shares refer to: a few triangles take nearly all the counts, and one add per wave and triangle on so
// few addresses serialises in L2 (C3's training went from 70 to 112 ms with every row counted).  The selection needs
// shares, not exact counts.  The counts are uint32 and cumulative over a job; once the total reaches 2^31 the host
// stops counting and keeps the list it has (PG_BLOCKER_COUNT_STOP), so no counter wraps.  It also stops, with an empty
// list, once PG_BLOCKER_DECIDE counted rays or more gave no list: such a scene pays for one or two small passes' counting.
#define PG_MAX_BLOCKERS 8
#define PG_BLOCKER_MIN_SHARE 64
#define PG_BLOCKER_COUNT_STOP 0x80000000u
#define PG_BLOCKER_SAMPLE 16u
// counted shadow rays after which an empty selection is final for the job: each listed share is then known to about
// 1 / sqrt(4096 / 64) of itself at the 1/64 threshold and the half-share bound to 1.6 %
#define PG_BLOCKER_DECIDE 4096u
#define PG_BLOCKER_MARGIN 9.765625e-4f  // 2^-10
// blk: the listed records, 12 floats each: TriAccel rows 0-2 with [10] = bits(BVH-order id) and [11] = the smaller
// width of the triangle's box on the two axes other than k.  absmax: the scene's largest |coordinate|.
// Returns 1 + the id ([10]) of the first listed triangle that certainly blocks o + t d, t in [tmin, tmax]; 0: none.
// The listed-record loop of both certain-hit tests (this one and pg_ray_hits_occluders below): the first record whose
// TriAccel test, in triHitRow0's arithmetic, puts the hit at t in [tlo, thi] with every barycentric weight >=
// PG_BLOCKER_MARGIN, on a triangle wide enough for E and not grazed by d.  1 + its id ([10]); 0: none.
PG_HD inline uint32_t pg_ray_hits_records(const float (*blk)[12], uint32_t n, float E, float dmax, const float o[3],
                                          const float d[3], float tlo, float thi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (uint32_t b = 0; b < n; ++b) {
        const float *r = blk[b];
        uint32_t k;
        __builtin_memcpy(&k, r + 3, 4);
        if (k > 2u || !(r[11] * 32.0f >= E)) continue;
        // triHitRow0's arithmetic (pg_trace.h), in its order
        const float ou = k == 0 ? o[1] : (k == 1 ? o[2] : o[0]), ov = k == 0 ? o[2] : (k == 1 ? o[0] : o[1]);
        const float ok = k == 0 ? o[0] : (k == 1 ? o[1] : o[2]);
        const float du = k == 0 ? d[1] : (k == 1 ? d[2] : d[0]), dv = k == 0 ? d[2] : (k == 1 ? d[0] : d[1]);
        const float dk = k == 0 ? d[0] : (k == 1 ? d[1] : d[2]);
        const float den = du * r[0] + dv * r[1] + dk;
        if (!(fabsf(dk) * 16.0f >= dmax && fabsf(den) * 16.0f >= dmax)) continue;
        const float tt = (r[2] - ou * r[0] - ov * r[1] - ok) / den;
        if (!(tt >= tlo && tt <= thi)) continue;
        const float hu = ou + tt * du - r[4], hv = ov + tt * dv - r[5];
        const float u = hv * r[6] + hu * r[7];
        const float v = hu * r[8] + hv * r[9];
        if (u >= PG_BLOCKER_MARGIN && v >= PG_BLOCKER_MARGIN && u + v <= 1.0f - PG_BLOCKER_MARGIN) {
            uint32_t id;
            __builtin_memcpy(&id, r + 10, 4);
            return id + 1;  // ids are < 2^31
        }
    }
    return 0;
}
PG_HD inline uint32_t pg_ray_hits_blockers(const float (*blk)[12], uint32_t n, float absmax, const float o[3],
                                           const float d[3], float tmin, float tmax) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float E = absmax + fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
    const float dmax = fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2]));
    const float dmin = fminf(fminf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2]));
    if (!(dmin > 1e-30f && tmax * dmax * 32.0f >= E)) return 0;
    const float shrink = PG_BLOCKER_MARGIN * tmax;
    return pg_ray_hits_records(blk, n, E, dmax, o, d, tmin + shrink, tmax - shrink);
}
// Host: the listed record of BVH-order triangle `id`: its TriAccel rows (3 float4), p0 / p1 / p2 its vertices
inline void pg_blocker_record(const float *rows, const float *p0, const float *p1, const float *p2, uint32_t id,
                              float *rec) {
    __builtin_memcpy(rec, rows, 48);
    uint32_t k;
    __builtin_memcpy(&k, rows + 3, 4);
    float w = __builtin_huge_valf();
    for (uint32_t a = 0; a < 3; ++a) {
        if (a == k) continue;
        const float lo = fminf(fminf(p0[a], p1[a]), p2[a]), hi = fmaxf(fmaxf(p0[a], p1[a]), p2[a]);
        w = fminf(w, hi - lo);
    }
    __builtin_memcpy(rec + 10, &id, 4);
    rec[11] = k <= 2u ? w : 0.0f;
}
// Host: up to PG_MAX_BLOCKERS triangle ids by descending count, each with count * PG_BLOCKER_MIN_SHARE >= total, the
// number of shadow rays (occluded or not) the counts were taken from: below that share eight tests per NEE vertex
// cannot pay for themselves.  Equal counts go to the lower id, so the list is reproducible.  The list is empty
// unless its triangles together blocked at least half of the total.  Returns the number written to ids.
// pg_select_listed: the rule with the list's capacity `cap` as a parameter (the probe occluders' list is longer)
inline uint32_t pg_select_listed(const uint32_t *counts, uint32_t n, uint64_t total, uint32_t cap, uint32_t *ids) {
    uint32_t m = 0;
    if (!total) return 0;
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t c = counts[t];
        if (c == 0 || (uint64_t)c * PG_BLOCKER_MIN_SHARE < total) continue;
        // insertion into the descending list; strict > keeps the lower id first among equals
        uint32_t at = m;
        while (at > 0 && c > counts[ids[at - 1]]) --at;
        if (at >= cap) continue;
        const uint32_t last = m < cap ? m : cap - 1;
        for (uint32_t j = last; j > at; --j) ids[j] = ids[j - 1];
        ids[at] = t;
        if (m < cap) ++m;
    }
    uint64_t listed = 0;
    for (uint32_t j = 0; j < m; ++j) listed += counts[ids[j]];
    return 2 * listed >= total ? m : 0;
}
inline uint32_t pg_select_blockers(const uint32_t *counts, uint32_t n, uint64_t total, uint32_t *ids) {
    return pg_select_listed(counts, n, total, PG_MAX_BLOCKERS, ids);
}

// Probe occluders (SceneDev::prb): a doom probe (above) only asks whether its ray hits anything, and in a closed
// room nearly every probe does -- after a nearest-first descent almost as long as a closest-hit walk's.  The probe
// rows of the recording passes count, per triangle, the probes whose walk accepted it (every PG_BLOCKER_SAMPLE-th row,
// counters of their own beside the shadow blockers', the same selection rule: pg_select_listed with up to
// PG_PROBE_LIST_MAX triangles).  The tracing kernels then test a probe against the listed records first
// (pg_kernels.hip probeRows): a certain hit is counted as the hit the walk would have returned, without the walk.
// Any listed triangle hit anywhere along the ray will do, whatever lies in front of it: the walk cannot end without a
// hit while a triangle it is certain to accept is still ahead.  The list only decides which probes skip the walk,
// never a counter: `culled`, `escaped` and `probes` keep their values, a resolved probe is also counted in a row of
// its own (pg_get_probes_resolved).
//
// "Certain" (pg_ray_hits_occluders): "hit" only where probeHit -- the any-hit form of the 4-wide closest-hit walk
// (pg_trace.h traverse4), tmin = |ray_o.w|, tmax = +inf -- says it too.  That walk returns only at its first accepted
// triangle or with an empty stack (the builder holds its trees under PG_QSTACK_DEPTH), so it either accepts some
// triangle first or reaches every leaf whose ancestor slots all pass; in the listed triangle's leaf its test is
// pg_ray_hits_records' arithmetic bit for bit (same record, o, d, tmin; t <= inf, and t < inf always accepts), whose
// margins are stricter than the leaf's u, v >= 0, u + v <= 1, t >= tmin.  So it is enough that every ancestor slot
// passes cmin <= cmax (1 + 2^-21), cmin = max(tn_x, tn_y, tn_z, tmin), cmax = min(tf_x, tf_y, tf_z, inf).  The slot's
// planes X = origin + q 2^e are rounded outward, so they enclose the triangle.  The walk computes t = fma(q, 2^e idir,
// fma(origin, idir, -(o idir) -+ pad_o) -+ pad_n): 2^e idir is exact, and the roundings of idir, o idir, the padded
// addend, both fmas and the last subtraction displace a plane by at most 6 * 2^-24 E < d_pos = 2^-21 E along its axis
// (E as for the blockers: |origin|, |X - o| <= E to first order).  Its paddings (2^-21 |o_a|, 2^-22 |origin_a|) only
// move the near plane earlier and the far plane later, and (1 + 2^-21) only loosens the comparison where cmax > 0.
// The 8-wide walk of the blockers' derivation pads the same way (its planes by 2^-21 of |o_a idir_a|, |origin_a
// idir_a| and the node's width, without the relative (1 + 2^-21)); the margins were derived for planes displaced by
// d_pos with no padding at all, the stricter case for either walk, and the same margins hold: barycentrics >= 2^-10 on a triangle at least E / 32 wide off its axis k (the hit point is >= 2^-16 E inside
// the box on both wide axes, 2 d_pos between them, 17 d_pos against the flat axis), |d_k|, |den| >= max|d| / 16, no
// |d_a| <= 1e-30.  What changes is the interval: there is no tmax, so the blockers' shrink 2^-10 tmax with tmax max|d|
// >= E / 32 becomes its smallest admissible value, t >= tmin + 2^-15 E / max|d|: the flat axis' far plane is computed at
// t - (d_pos / |d_k| + the error of t) >= t - 1.5 * 2^-17 E / max|d| >= tmin, so cmax >= tmin > 0 and tmin never cuts
// the slot; t must be finite.
// A probe that fails any margin, or hits no listed triangle, walks as before.
#define PG_PROBE_LIST_MAX 16
#define PG_PROBE_TMIN_MARGIN 3.0517578125e-5f  // 2^-15
// prb: the listed records (pg_blocker_record's form).  Returns 1 + the id of the first listed triangle the probe
// walk of o + t d, t >= tmin, is certain to end on or before; 0: none (the walk decides).
PG_HD inline uint32_t pg_ray_hits_occluders(const float (*prb)[12], uint32_t n, float absmax, const float o[3],
                                            const float d[3], float tmin) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float E = absmax + fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
    const float dmax = fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2]));
    const float dmin = fminf(fminf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2]));
    if (!(dmin > 1e-30f)) return 0;
    const float tlo = tmin + PG_PROBE_TMIN_MARGIN * E / dmax;
    // one record per call, the loop unrolled: every index into the by-value list is then a constant and the records
    // are read from the kernel arguments (a run-time index had the kernels copy the list to 1.6 KB of scratch per lane)
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t b = 0; b < PG_PROBE_LIST_MAX; ++b) {
        if (b >= n) break;
        const uint32_t hit = pg_ray_hits_records(prb + b, 1, E, dmax, o, d, tlo, 3.40282347e38f);
        if (hit) return hit;
    }
    return 0;
}

// Kernel-side constants of one render context.
struct GParams {
    // camera
    float cam_o[3], cam_left[3], cam_up[3], cam_dir[3];
    float tan_half, aspect, near_clip, far_clip;
    uint32_t width, height;
    // integrator
    int32_t max_depth, rr_depth, use_nee, hide_emitters, strict_normals, guiding, record, max_vertices;
    float max_component_value, bsdf_fraction;
    uint32_t seed, num_emitters, num_materials, depth_cap;  // num_emitters counts the environment emitter
    int32_t fraction_bound;  // pg_config.bsdf_fraction_bound (PG_FRACTION_*)
    int32_t exact_mis;       // pg_config.volpath_exact_mis
    int32_t glossy_prior;    // pg_config.glossy_prior
    int32_t path_cull;       // 1: shadeOne decides PF_DOOMED one bounce early and the tracer culls (PG_NO_PATH_CULL: 0)
    int32_t doom_probe;      // 1: a doomed ray that misses every emitter box is probed, not traced (PG_NO_DOOM_PROBE: 0)
    // thin lens (pg_set_lens): world-space aperture radius, 0 = pinhole (the lens kernels are not launched), and
    // the distance of the focal plane along the viewing direction
    float lens_radius, focus_dist;
    // the area emitters among num_emitters: emitter ei < num_area is sc.ems[ei], the delta emitters
    // (pg_set_delta_emitters) follow as sc.delta[ei - num_area], the environment emitter is last
    uint32_t num_area;
};
