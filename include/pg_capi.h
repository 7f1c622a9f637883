/*
 * pg_capi.h — the drop-in boundary of the MI355X guided path-tracing integrator.
 *
 * A thin C ABI (plain pointers, sizes and integer status codes; no C++ types, no exceptions)
 * between a host integrator plugin and the HIP/gfx950 hot path.  It replaces the CPU side of
 * the reference's progressive Monte-Carlo integrator for ONE job:
 *
 *   reference surface                                    replaced by
 *   ------------------------------------------------------------------------------------------
 *   Integrator::preprocess            include/mitsuba/render/integrator.h:61   pg_create + pg_upload_scene
 *   ProgressiveMonteCarloIntegrator::render / renderSamples
 *                                     src/librender/progressiveintegrator.cpp:65-114,170-220
 *                                                                              pg_render_pass (one progression)
 *   ProgressiveMonteCarloIntegrator::renderBlock (per-pixel sample loop, clamp, ImageBlock::put)
 *                                     src/librender/progressiveintegrator.cpp:222-282   (inside pg_render_pass)
 *   ProgressiveMIPathTracer::Li       src/integrators/path/progressive_path.cpp:133-314 (inside pg_render_pass)
 *   ProgressiveMonteCarloIntegrator::postprogression (guiding refit slot)
 *                                     src/librender/progressiveintegrator.cpp:314-317  pg_splat_* + pg_refit
 *   Integrator::cancel                integrator.h:84; progressiveintegrator.cpp:319-326  pg_cancel
 *   Film::develop / ImageBlock readback  src/librender/renderproc.cpp:142-149        pg_read_film
 *   Integrator::postprocess           integrator.h:96                             pg_get_stats + pg_destroy
 *
 * Every function returns a pg_status; on failure pg_last_error() holds a message (the Mitsuba
 * adapter turns it into Log(EError, ...), which throws: include/mitsuba/core/formatter.h:33).
 * All host arrays passed in are caller-owned and copied; all device memory is owned by the
 * context and released by pg_destroy.  One context per render job; calls come from one thread
 * except pg_cancel, which may be called from any thread.
 */
#ifndef PG_CAPI_H
#define PG_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 12

typedef int32_t pg_status;
enum {
    PG_OK = 0,
    PG_ERR_INVALID = 1,    /* bad argument / inconsistent scene */
    PG_ERR_HIP = 2,        /* HIP runtime error */
    PG_ERR_OOM = 3,        /* device allocation failed */
    PG_ERR_STATE = 4,      /* call out of order (e.g. render before upload) */
    PG_ERR_CANCELLED = 5,  /* pg_cancel() was called */
    PG_ERR_NO_DEVICE = 6   /* no gfx950 device visible */
};

/* BSDF models (reference: EBSDFModel, include/mitsuba/render/bsdf.h:287-297; plugins in src/bsdfs/). */
enum {
    PG_BSDF_DIFFUSE = 0,          /* src/bsdfs/diffuse.cpp          */
    PG_BSDF_CONDUCTOR = 1,        /* src/bsdfs/conductor.cpp        */
    PG_BSDF_ROUGHCONDUCTOR = 2,   /* src/bsdfs/roughconductor.cpp   */
    PG_BSDF_DIELECTRIC = 3,       /* src/bsdfs/dielectric.cpp       */
    PG_BSDF_ROUGHDIELECTRIC = 4,  /* src/bsdfs/roughdielectric.cpp  */
    PG_BSDF_PLASTIC = 5,          /* src/bsdfs/plastic.cpp          */
    PG_BSDF_ROUGHPLASTIC = 6,     /* src/bsdfs/roughplastic.cpp     */
    PG_BSDF_NULL = 7,             /* src/bsdfs/null.cpp: index-matched medium boundary */
    PG_BSDF_COUNT = 8
};
/* Microfacet distributions (src/bsdfs/microfacet.h:48-58). */
enum { PG_DIST_BECKMANN = 0, PG_DIST_GGX = 1 };
/* Material flags. */
#define PG_MAT_TWOSIDED 1u    /* wrap in the 'twosided' adapter (src/bsdfs/twosided.cpp) */
#define PG_MAT_NONLINEAR 2u   /* plastic: 'nonlinear' (src/bsdfs/plastic.cpp) */
#define PG_MAT_SAMPLE_ALL 4u  /* microfacet: sampleVisible=false (microfacet.h:112) */

/* One material; 112 bytes.  Conductor eta/k are RGB and already divided by extEta
 * (roughconductor.cpp:173-188).  Dielectric/plastic use int_ior/ext_ior. */
typedef struct pg_material {
    uint32_t type;
    uint32_t distribution;
    uint32_t flags;
    uint32_t pad0;
    float alpha_u, alpha_v;
    float int_ior, ext_ior;
    float diffuse_reflectance[4];    /* diffuse.reflectance, plastic.diffuseReflectance */
    float specular_reflectance[4];
    float specular_transmittance[4];
    float eta[4];
    float k[4];
} pg_material;

/* A shape = a contiguous triangle range with one BSDF and optionally one area emitter
 * (reference: Shape/TriMesh + AreaLight, src/librender/trimesh.cpp, src/emitters/area.cpp). */
typedef struct pg_shape {
    uint32_t tri_begin;
    uint32_t tri_count;
    uint32_t material;
    int32_t emitter;          /* index into emitters, or -1 */
    int32_t interior_medium;  /* Shape::getInteriorMedium (shape.h), index into media or -1 */
    int32_t exterior_medium;  /* Shape::getExteriorMedium; the side is the geometric normal's */
} pg_shape;

/* Participating medium (volpath integrator only).  PG_MEDIUM_HETEROGENEOUS is
 * src/medium/heterogeneous.cpp with Woodcock tracking (the default 'method'): a float32 density
 * grid (src/volume/gridvolume.cpp, trilinear, the data AABB mapped onto [0, res-1]^3, zero outside),
 * density multiplier 'scale', constant albedo (constvolume) and a Henyey-Greenstein phase function
 * (src/phase/hg.cpp).  Densities must lie in [0, 1] (heterogeneous.cpp:236-239). */
enum { PG_MEDIUM_HETEROGENEOUS = 0 };
typedef struct pg_medium {
    uint32_t type;
    uint32_t res[3];
    const float *density;  /* res[0] * res[1] * res[2], x fastest; copied at upload */
    float aabb_min[3];
    float aabb_max[3];
    float scale;
    float albedo[3];
    float g;               /* HG mean cosine */
    uint32_t pad0;
} pg_medium;

/* Area emitter attached to a shape (src/emitters/area.cpp:158-183).  Sampling weight 1, so the
 * scene picks emitters uniformly (Scene::sampleEmitterDirect, src/librender/scene.cpp:871-895). */
typedef struct pg_emitter {
    uint32_t shape;
    uint32_t pad[3];
    float radiance[4];
} pg_emitter;

/* Environment emitter with Mitsuba 'envmap' semantics (src/emitters/envmap.cpp:100-677): a
 * latitude-longitude RGB image (x = phi, y = theta from +Y, texel (x, y) at rgb[3 * (y * width + x)]),
 * stored at half precision as the reference's MIP map does (SpectrumHalf, envmap.cpp:101-103;
 * negative texels are clamped, mipmap.h:232-240), bilinear lookups with repeat in x and clamp in y
 * (mipmap.h:503-596), importance sampling by the sin(theta)-weighted luminance CDFs of
 * EnvironmentMap::configure (envmap.cpp:260-329) with a tent-filtered in-pixel offset
 * (internalSampleDirection, :567-600).  to_world is the rotation part of the 'toWorld' transform,
 * row-major (world = R * local).  It is the last emitter of the uniform emitter pick
 * (Scene::sampleEmitterDirect, scene.cpp:871-895).  The volumetric integrator does not support it. */
typedef struct pg_envmap {
    uint32_t width;
    uint32_t height;
    const float *rgb;      /* width * height * 3, copied at upload */
    float to_world[9];
    float scale;           /* 'scale' (envmap.cpp:188) */
    uint32_t pad0;
    uint32_t pad1;
} pg_envmap;

/* Pinhole camera with Mitsuba 'perspective' semantics (src/sensors/perspective.cpp:271-298,
 * Transform::lookAt src/libcore/transform.cpp:191-214): fov along x, near/far clip. */
typedef struct pg_camera {
    float origin[3];
    float target[3];
    float up[3];
    float fov_x_deg;
    float near_clip;
    float far_clip;
    uint32_t width;
    uint32_t height;
} pg_camera;

/* Flattened scene (what a Mitsuba adapter extracts from Scene::getShapes()/getBSDFs()/emitters). */
typedef struct pg_scene_desc {
    uint32_t num_vertices;
    uint32_t num_triangles;
    uint32_t num_shapes;
    uint32_t num_materials;
    uint32_t num_emitters;
    uint32_t num_media;
    const float *positions;     /* 3 * num_vertices */
    const float *normals;       /* 3 * num_vertices, or NULL (face normals) */
    const uint32_t *indices;    /* 3 * num_triangles */
    const pg_shape *shapes;     /* shapes partition [0, num_triangles) */
    const pg_material *materials;
    const pg_emitter *emitters;
    pg_camera camera;
    const pg_medium *media;     /* num_media entries (may be NULL when 0) */
    int32_t camera_medium;      /* Sensor::getMedium, index into media or -1 */
    int32_t pad1;
    const pg_envmap *envmap;    /* Scene::getEnvironmentEmitter (scene.h), or NULL */
} pg_scene_desc;

/* Integrator parameters (MonteCarloIntegrator props: src/librender/integrator.cpp:195-230;
 * progressive: progressiveintegrator.cpp:296-300; useNee: progressive_path.cpp:117) plus the
 * SD-tree guiding parameters (Mueller et al. 2017) and the device/shard placement. */
typedef struct pg_config {
    int32_t device;               /* HIP device ordinal used by this context */
    int32_t max_depth;            /* -1 = unbounded (Mitsuba default) */
    int32_t rr_depth;             /* 5 */
    int32_t use_nee;              /* 1 */
    int32_t hide_emitters;        /* 0 */
    int32_t strict_normals;       /* 0 */
    float max_component_value;    /* +inf */
    uint32_t seed;                /* 1337 (deterministic.cpp salt) */
    int32_t guiding;              /* 0 = plain progressive path tracer, 1 = SD-tree guided */
    float bsdf_sampling_fraction; /* 0.5 */
    float s_tree_threshold;       /* 12000 */
    float d_tree_threshold;       /* 0.01 */
    int32_t d_tree_max_depth;     /* 20 */
    int32_t record_max_vertices;  /* 32: training-record vertices kept per path */
    int32_t rank;                 /* image-tile shard of this context */
    int32_t world_size;
    uint32_t tile_size;           /* 32 (Scene::setBlockSize default) */
    uint32_t max_paths_in_flight; /* paths per chunk; 0 = auto: 2^25, or four rounds of lanes (<= 2^27 paths a
                                     chunk) for a path-integrator pass of at least 3 x lanes x 2^26 paths; both
                                     capped to 70 % of the free device memory */
    int32_t gpu_depth_cap;        /* hard bounce cap on the device when max_depth < 0 (1024; the path integrator
                                     clamps it to 1098, and pg_create rejects a path-integrator max_depth above
                                     1097 with PG_ERR_INVALID; the volpath integrator honours both exactly) */
    int32_t path_lanes;           /* path chunks in flight on separate streams, 1..4 (0 = auto: 3) */
    int32_t integrator;           /* PG_INTEGRATOR_PATH (progressive_path) or _VOLPATH (progressive_volpath) */
    int32_t volume_majorant;      /* volpath free-flight / transmittance tracking: PG_MAJORANT_GRID (default:
                                     delta tracking against per-cell maxima of 8^3-voxel blocks, skipping empty
                                     cells) or PG_MAJORANT_GLOBAL (the reference's single majorant, scale * 1,
                                     heterogeneous.cpp:589-660).  Both sample the same distributions. */
    float distance_guiding;       /* volpath + guiding: mixing weight beta of guided free-flight sampling (weighted
                                     delta tracking toward the SD-tree's zero-variance collision probability,
                                     oracle/orc_volpath.h GuidedAccept); 0 = the reference's free flight. 0.25 */
    int32_t aovs;                 /* 1: accumulate the denoiser feature buffers (Denoiser::Sample albedo + normal,
                                     include/mitsuba/render/denoiser.h:12-16) of every camera sample's first hit;
                                     read with pg_read_aovs.  Path integrator only.  0 */
    int32_t bsdf_fraction_bound;  /* guided path integrator: how the one-sample-MIS BSDF fraction alpha of a vertex is
                                     chosen.  PG_FRACTION_FIXED: alpha = bsdf_sampling_fraction everywhere (Mueller et
                                     al. 2017).  PG_FRACTION_ALBEDO: alpha = max(bsdf_sampling_fraction, min(a, 0.95))
                                     with a = the max channel of BSDF::getAlbedo, which bounds the mixture weight
                                     f / (alpha p_bsdf + (1 - alpha) p_guide) <= (f / p_bsdf) / alpha by 1 for albedo
                                     bounded BSDF weights.  PG_FRACTION_THROUGHPUT: as ALBEDO with a scaled by the path
                                     throughput max(T), so a path may regain throughput it lost, but not grow past 1.
                                     PG_FRACTION_LEARNED: alpha per S-tree leaf, learned from the training records
                                     (after Mueller 2019: the candidate mixture in 0.05, 0.15 .. 0.95 with the largest
                                     estimated cross-entropy against f * L_i; bsdf_sampling_fraction
                                     until a leaf has 64 guided records).
                                     Any per-vertex choice independent of the sampled direction is unbiased.
                                     Default PG_FRACTION_FIXED (Mueller et al. 2017's fixed fraction). */
    int32_t kernel_timing;        /* 1: bracket every closest-hit, shading and shadow launch with HIP events and sum
                                     their device times into pg_stats trace_ms / shade_ms / shadow_ms.  Six event
                                     records per bounce cost ~2 % on C3, so 0 (the default) leaves
                                     those three statistics at 0. */
    int32_t volpath_exact_mis;    /* volpath: 0 (default) = the reference's MIS weight for an emitter reached through
                                     index-matched surfaces, whose emitter pdf uses the LAST segment's length
                                     (rayIntersectAndLookForEmitter + DirectSamplingRecord::setQuery,
                                     progressive_volpath.cpp:401-460, records.inl:170-178): biased, +34 % on
                                     data/tests/test_bidir_2.xml.  1 = the whole ray length: the MIS
                                     weights sum to one and the estimator is unbiased. */
    int32_t tail_paths;           /* path integrator: a chunk with at most this many live paths finishes in one launch
                                     (k_tail: each thread loops shade -> shadow -> closest hit) instead of one
                                     launch pair + count readback per bounce; bit-identical results.  0 = the
                                     default (131072, or the PG_TAIL_PATHS environment variable), < 0 = off. */
    int32_t glossy_prior;         /* guided path integrator: 1 = the BSDF's glossy sampling rate r
                                     (BSDF::getGlossySamplingRate, bsdf.h:365-381: 1 for roughconductor and
                                     roughdielectric, the glossy lobe's probability for roughplastic,
                                     roughplastic.cpp:323-345, 0 otherwise) raises the vertex's BSDF fraction
                                     to r + (1 - r) alpha; vertices with r = 1 are not guided, and only vertices
                                     with r = 0 feed the learned-fraction statistics.  0 = off (Mueller 2017). */
} pg_config;
enum { PG_FRACTION_FIXED = 0, PG_FRACTION_ALBEDO = 1, PG_FRACTION_THROUGHPUT = 2, PG_FRACTION_LEARNED = 3 };
enum { PG_INTEGRATOR_PATH = 0, PG_INTEGRATOR_VOLPATH = 1 };
enum { PG_MAJORANT_GRID = 0, PG_MAJORANT_GLOBAL = 1 };

/* Training record written per non-delta path vertex (SoA-free 32-byte AoS). */
typedef struct pg_record {
    float pos[3];
    uint32_t dir;      /* canonical (cos theta, phi) square coords as 2 x u16 */
    float radiance;    /* average incident radiance estimate along dir */
    float wo_pdf;      /* pdf the direction was sampled with (one-sample MIS) */
    float product;     /* guided vertex: f * L_i / wo_pdf, the BSDF-weighted contribution along dir divided
                          by the throughput before the vertex (channel average); 0 otherwise */
    float weight;      /* guided vertex: the D-tree pdf of dir (the mixture's p_guide); -1: not guided.
                          The learned fraction (PG_FRACTION_LEARNED) reads both in the splat. */
} pg_record;

typedef struct pg_stats {
    uint64_t paths;           /* camera paths traced since create */
    uint64_t segments;        /* path segments (extension rays) */
    uint64_t shadow_rays;
    uint64_t records;         /* training records written */
    double trace_ms;          /* device time of the closest-hit kernel (HIP events; lanes overlap; needs
                                 pg_config.kernel_timing) */
    double shade_ms;          /* device time of the shading kernels (all material classes) */
    double shadow_ms;
    double other_ms;
    uint64_t trace_launches;  /* closest-hit launches timed alone (the camera rays; every bounce with
                                 PG_NO_RAYS_FUSION) */
    uint64_t stree_nodes;
    uint64_t dtree_nodes;
    uint64_t shade_launches;  /* material-class shading launches */
    double volume_ms;         /* device time of the volumetric path kernel (integrator = volpath) */
    uint64_t volume_launches;
    uint64_t density_lookups; /* volpath: trilinear density-grid lookups (tentative collisions) */
    uint64_t escaped;         /* path integrator: segments whose ray left the scene (not shaded) */
    double rays_ms;           /* device time of the fused shadow + closest-hit launches (k_rays; kernel_timing) */
    uint64_t rays_launches;   /* k_rays launches (a bounce's shadow rays + the next bounce's closest hits) */
    uint64_t shadow_launches; /* unfused shadow-ray launches (PG_NO_RAYS_FUSION) */
    uint64_t tail_launches;   /* chunk tails finished in one launch (k_tail) */
    /* ABI 11: the volumetric wavefront's stages (integrator = volpath, PG_VOL_WAVEFRONT): device time
     * (HIP events; pg_config.kernel_timing), launches, items processed and density lookups made by the
     * free-flight launches (k_vflight) and the interaction launches (k_vvertex) */
    double vol_flight_ms;
    uint64_t vol_flight_launches;
    uint64_t vol_flights;
    uint64_t vol_flight_lookups;
    double vol_vertex_ms;
    uint64_t vol_vertex_launches; /* kernels: each interaction stage launches the medium and the surface kernel */
    uint64_t vol_vertices;
    uint64_t vol_vertex_lookups;
    /* ABI 12: the interactions' deferred transmittance walks (k_vnee: NEE shadow walks and emitter walks
     * through media, each on its own counter sub-stream): device time, launches, slots walked, lookups */
    double vol_nee_ms;
    uint64_t vol_nee_launches;
    uint64_t vol_nee_walks;
    uint64_t vol_nee_lookups;
} pg_stats;

/* ---- lifecycle ---------------------------------------------------------------------- */
pg_status pg_config_default(pg_config *cfg);
pg_status pg_create(const pg_config *cfg, void **ctx_out);
pg_status pg_destroy(void *ctx);
const char *pg_last_error(void *ctx);
int32_t pg_abi_version(void);
pg_status pg_cancel(void *ctx); /* thread-safe */

/* ---- scene ---------------------------------------------------------------------------- */
pg_status pg_upload_scene(void *ctx, const pg_scene_desc *scene);

/* ---- one progression (pass): spp samples per pixel of this rank's tiles,
 *      sample indices [sample_offset, sample_offset + spp).  record != 0 writes training
 *      records (only meaningful with guiding).  Accumulates into the film. ------------ */
pg_status pg_render_pass(void *ctx, uint32_t spp, uint32_t sample_offset, int32_t record);
/* Time-budget rendering (maxRenderTime; ProgressiveMonteCarloIntegrator::renderTime,
 * src/librender/progressiveintegrator.cpp:117-168,185,207-208): whole progressions of
 * spp_per_progression samples, sample indices from sample_offset on, until `seconds` of wall clock
 * have passed (checked after each batch of progressions) or max_spp samples are done (0 = no cap).
 * *spp_done = samples per pixel rendered (the reference's m_spp after renderTime).  No records. */
pg_status pg_render_time(void *ctx, double seconds, uint32_t spp_per_progression, uint32_t sample_offset,
                         uint32_t max_spp, uint32_t *spp_done);

/* ---- training records / SD-tree refit (the postprogression slot) ------------------------ */
pg_status pg_get_record_count(void *ctx, uint64_t *count);
/* Copy local records out: dst is host memory unless dst_is_device != 0. */
pg_status pg_get_records(void *ctx, void *dst, uint64_t max_records, int32_t dst_is_device, uint64_t *written);
/* Splat records (e.g. the all-gathered set of every rank) into the building SD-tree. */
pg_status pg_splat_records(void *ctx, const void *src, uint64_t count, int32_t src_is_device);
/* Splat this context's own records (single-GPU case). */
pg_status pg_splat_local_records(void *ctx);
/* Build sampling trees from the building trees, refine the S-tree for training iteration
 * `iteration`, reset the building trees; clears the local record buffer. */
pg_status pg_refit(void *ctx, uint32_t iteration);
/* Serialize / inject the SD-tree (golden-vector tests).  Query size with buf == NULL. */
pg_status pg_get_sdtree(void *ctx, void *buf, uint64_t capacity, uint64_t *size);
pg_status pg_put_sdtree(void *ctx, const void *buf, uint64_t size);
/* Evaluate / sample the sampling SD-tree on the device for host arrays (parity tests). */
pg_status pg_sdtree_pdf(void *ctx, const float *pos, const float *dir, uint64_t n, float *pdf_out);
pg_status pg_sdtree_sample(void *ctx, const float *pos, const float *u, uint64_t n, float *dir_out, float *pdf_out);

/* ---- film ------------------------------------------------------------------------------ */
/* rgbw: width*height*4 floats (sum r,g,b, sample count); sumsq: width*height*4 (sum r^2,g^2,b^2,0).
 * Pixels outside this rank's tiles are zero.  Either pointer may be NULL. */
pg_status pg_read_film(void *ctx, float *rgbw, float *sumsq);
pg_status pg_reset_film(void *ctx);
/* Denoiser feature buffers (pg_config.aovs = 1), the per-pixel inputs Denoiser::add averages
 * (src/librender/denoiser.cpp:138-144): albedo: width*height*4 floats (sum of BSDF::getAlbedo at the
 * first hit, r, g, b, sample count); normal: width*height*4 (sum of first-hit shading normals, world
 * space, 0).  A camera ray that escapes contributes Denoiser::Sample's defaults: albedo 0, normal
 * (0, 0, -1).  Cleared by pg_reset_film.  Either pointer may be NULL. */
pg_status pg_read_aovs(void *ctx, float *albedo, float *normal);
/* ---- filtered film: the reference's reconstruction filter (ImageBlock::put, imageblock.h:151-196) ----------
 * New entry points; pg_config, pg_stats and PG_ABI_VERSION are unchanged.  While no filter is set, nothing
 * below is allocated or launched and every other result is bit for bit what it was.
 *
 * pg_rfilter_table builds the reference's discretised table (ReconstructionFilter::configure,
 * rfilter.cpp:38-54; src/rfilters/{box,tent,gaussian}.cpp): values[i] = eval(radius * i / 31) for i < 31,
 * scaled by 1 / (sum * 2 * radius / 31), values[31] = 0.  PG_RFILTER_BOX: radius 0.5; PG_RFILTER_TENT: radius 1;
 * PG_RFILTER_GAUSSIAN: param = stddev (0 = the default 0.5), radius 4 * stddev.  Needs no device or context. */
enum { PG_RFILTER_BOX = 0, PG_RFILTER_TENT = 1, PG_RFILTER_GAUSSIAN = 2 };
pg_status pg_rfilter_table(int32_t type, float param, float *radius_out, float *values_out /* [32] */);
/* Turn the filtered film on with an arbitrary 32-entry table (negative lobes allowed: Mitsuba's own table of
 * mitchell, catmullrom or lanczos works), 0 < radius <= 4, else PG_ERR_INVALID; values == NULL turns it off.
 * After pg_create and before the first render pass (PG_ERR_STATE afterwards); path and volpath integrators;
 * PG_ERR_INVALID with the banded camera map (PG_CAMERA_BANDS).  The box film, sumsq and the feature buffers
 * keep accumulating per pixel exactly as without a filter.
 *
 * Every sample the box film takes (after the max_component_value clamp; samples ImageBlock::put rejects are
 * dropped) is splatted with W = width, r = radius, (jx, jy) = the camera's jitter of the sample:
 *   pos_x = ((float)(pix % W) + jx) - 0.5f                                   (float32, no contraction; y alike)
 *   columns X = max(ceil(pos_x - r), 0) .. min(floor(pos_x + r), W - 1)      (clipped to the whole image)
 *   wx[X] = values[min((int)fabsf(((float)X - pos_x) * (31.0f / r)), 31)],   w = wx * wy  (float32)
 *   acc[Y][X][c] += llrint((double)w * (double)L_c * 2^28), c = r, g, b;     acc[Y][X][3] += llrint((double)w * 2^28)
 * Signed 64-bit sums in units of 2^-28 (~3.7e-9 per tap): exact, so the film does not depend on chunk sizes,
 * lanes, launch variants or the shard split.  Range: |sum| < 2^35 per pixel and channel.
 *
 * pg_read_film_filtered: raw = width*height*4 int64 (sum w r, sum w g, sum w b, sum w); rgbw = the same as
 * (float)((double)raw * 2^-28); either may be NULL.  A rank's buffer covers the whole image: its tiles plus the
 * border its samples reach (ceil(radius - 0.5) pixels).  The developed pixel is rgb / w (hdrfilm).
 * PG_ERR_STATE when no filter is set.  pg_reset_film clears it; pg_comm_reduce_film sums it (int64, exact). */
pg_status pg_set_rfilter(void *ctx, float radius, const float *values /* [32] or NULL */);
pg_status pg_read_film_filtered(void *ctx, float *rgbw, int64_t *raw);
/* ---- denoiser: the library's own filter over the film and the feature buffers ----------------------------------
 * New entry points; pg_config, pg_stats and PG_ABI_VERSION are unchanged.  While none of them is called, nothing
 * below is allocated or launched and every other result is bit for bit what it was.
 *
 * The reference hands colour, albedo and normal to OIDN (Denoiser::denoise, src/librender/denoiser.cpp); OIDN is a
 * neural network and stays with the Mitsuba adapter.  This is an edge-avoiding a-trous wavelet (Dammertz et al.
 * 2010) steered by the albedo and normal sums and by the per-pixel variance of the mean, as the spatial part of
 * SVGF is (Schied et al. 2017).  The reference has no such filter: what follows is its definition, restated in
 * float64 by tests/denoise_ref.py.  float32 on the device, no FP contraction.
 *
 * Per pixel: rgbw = (sum L, n), sumsq = (sum L^2, 0), albedo = (sum a, n), normal = (sum N, 0); n is rgbw's.
 * 1. A pixel with n = 0 is invalid: its output is 0 and it is no tap of any pixel.  Otherwise c = sum L / n,
 *    abar = sum a / n, N = sum N / n normalised (0 if its length is 0), mod = abar + 0.01 per channel, and the
 *    filtered quantity is e = c / mod.  Variance of the mean per channel: max(sum L^2 / n - c^2, 0) / n for n >= 2,
 *    c^2 for n < 2; V = lum(var / mod^2), lum = 0.2126 r + 0.7152 g + 0.0722 b.
 * 2. Level i = 0 .. levels - 1, step s = 2^i, from (e, V) to (e', V'), with the distances between pixels p and q
 *    d_n = max(0, 1 - N_p . N_q) / sigma_n and d_a = |abar_p - abar_q|^2 / sigma_a^2:
 *    (a) Vt_p = the 3 x 3 average of V at step 1 with weights (1/4, 1/2, 1/4)^2 over the taps inside the image,
 *        valid and with d_n + d_a <= 80, divided by the sum of the weights used; the centre always counts.
 *    (b) taps q = p + s (dx, dy), dx, dy = -2 .. 2, h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *        d = d_n + d_a + |lum(e_p) - lum(e_q)| / (sigma_l sqrt(Vt_p) + 1e-6); a tap outside the image, an invalid
 *        tap or one with d > 80 has weight 0 (a hard cut: a feature edge is impermeable), any other
 *        w = h(dx) h(dy) exp(-d), the centre h(0)^2 unconditionally; e'_p = sum w e_q / sum w (accumulated as
 *        e_p + sum w (e_q - e_p) / sum w), V'_p = sum w^2 V_q / (sum w)^2.
 * 3. Output (e mod).rgb and the last V; invalid pixels give four zeros.
 * No atomics and no order dependence: two runs give the same bits. */
typedef struct pg_denoise_params {
    int32_t levels;  /* 1..6; 5 */
    float sigma_l;   /* > 0; 4.0 */
    float sigma_n;   /* > 0; 0.1 */
    float sigma_a;   /* > 0; 0.1 */
} pg_denoise_params;
/* The defaults.  Needs no device or context. */
pg_status pg_denoise_default_params(pg_denoise_params *params);
/* Filters the context's own film, sumsq and feature buffers where they lie and copies width * height * 4 floats
 * out (r, g, b, V).  params == NULL: the defaults.  PG_ERR_STATE without a scene or with pg_config.aovs = 0;
 * PG_ERR_INVALID for parameters out of range or not finite.  The film, sumsq and feature buffers are left as they
 * are; the scratch (four rows of 16 bytes per pixel) is allocated by the first call and freed with the context.  On
 * the root rank after pg_comm_reduce_film this is the whole image; on any other rank, its own tiles. */
pg_status pg_denoise(void *ctx, const pg_denoise_params *params, float *out_rgbv);
/* The same kernels on host arrays of width x height pixels (1 <= width, height <= 65536, at most 2^28 pixels) in the
 * layouts above: combined or reloaded images.  Any context works, with or without a scene or feature buffers; nothing
 * of the context changes.  PG_ERR_INVALID: a null array, a zero or oversized image, parameters as above. */
pg_status pg_denoise_arrays(void *ctx, const pg_denoise_params *params, uint32_t width, uint32_t height,
                            const float *rgbw, const float *sumsq, const float *albedo, const float *normal,
                            float *out_rgbv);
/* Device time of the last pg_denoise / pg_denoise_arrays of this context in milliseconds, from events around its
 * kernel launches (no copies).  PG_ERR_STATE before the first. */
pg_status pg_denoise_time(void *ctx, float *ms_out);
/* ---- textures: a bitmap or a checkerboard as the diffuse reflectance of a material ------------------------------
 * New entry points; pg_config, pg_stats, pg_scene_desc, pg_material and PG_ABI_VERSION are unchanged.  While no
 * texture is bound, no texture buffer is allocated on the device, no kernel compiled for textures is launched and
 * every result is bit for bit what it was.  (What the feature costs every scene -- one more, empty, material-class
 * queue per lane, a ninth counter row per bounce and host copies of the triangle indices, material records and
 * triangle classes -- is listed in DESIGN.md section 3.)
 *
 * Only the lookup without ray differentials (Texture2D::eval(its, false), texture.cpp:112-121): the path integrator
 * has no uv partials after the first vertex, and for filterType nearest / bilinear the reference uses none at all.
 *   uv   = t0 * b.x + t1 * b.y + t2 * b.z, b = (1 - u - v, u, v) the hit's barycentrics (skdtree.h:355,398-405;
 *          float32, no contraction); without texcoords uv = (u, v)
 *   uv'  = (uv.x * uscale, uv.y * vscale) + (uoffset, voffset)
 *   PG_TEXTURE_BITMAP (bitmap.cpp:431-449, MIP level 0, mipmap.h:503-596), float32 RGB texels, texel (x, y) at
 *          rgb[3 * (y * width + x)]; a non-finite uv' gives 0.
 *          PG_TEXFILTER_NEAREST: texel(floor(u' W), floor(v' H)).
 *          PG_TEXFILTER_BILINEAR: u = u' W - 0.5, x = floor(u), dx1 = u - x, dx2 = 1 - dx1 (y alike):
 *          T(x, y) dx2 dy2 + T(x, y + 1) dx2 dy1 + T(x + 1, y) dx1 dy2 + T(x + 1, y + 1) dx1 dy1, summed left to right.
 *          texel() wraps x, then y (PG_TEXWRAP_*): repeat (positive modulo), clamp, mirror (x mod 2 W, then
 *          2 W - x - 1 when x >= W), zero, one.
 *   PG_TEXTURE_CHECKERBOARD (checkerboard.cpp:66-74): x = 2 mod((int)(u' 2), 2) - 1 (the conversion truncates toward
 *          zero), y alike; color0 where x y == 1, else color1.
 * The texel address is clamped into the image for every finite uv'; beyond |u' W| = 2^30 the colour is unspecified.
 * The looked-up value replaces diffuse.reflectance / plastic.diffuseReflectance / roughplastic.diffuseReflectance at
 * every vertex (BSDF value, sampling weight, albedo, the guide-fraction bound and the first-hit albedo of the
 * denoiser buffers).  plastic / roughplastic take their specular sampling weight from the texture's average
 * (Texture::getAverage, plastic.cpp:201-202): `average`, or where average[0] < 0 the mean of the texels / (color0 +
 * color1) / 2.  Deviations from the reference: filterType ewa and trilinear are to be passed as bilinear (the
 * reference filters camera-ray hits with the ray differentials; every later vertex is level-0 bilinear there too),
 * and the shading frame keeps dpdu = p1 - p0 (computeUVTangents only for normal-mapped materials, below). */
enum { PG_TEXTURE_BITMAP = 0, PG_TEXTURE_CHECKERBOARD = 1 };
enum { PG_TEXFILTER_NEAREST = 0, PG_TEXFILTER_BILINEAR = 1 };
enum { PG_TEXWRAP_REPEAT = 0, PG_TEXWRAP_CLAMP = 1, PG_TEXWRAP_MIRROR = 2, PG_TEXWRAP_ZERO = 3, PG_TEXWRAP_ONE = 4 };
typedef struct pg_texture {
    uint32_t type;         /* PG_TEXTURE_* */
    uint32_t width;        /* bitmap only */
    uint32_t height;
    uint32_t filter;       /* PG_TEXFILTER_* */
    const float *rgb;      /* width * height * 3, finite and >= 0; copied by pg_set_textures */
    uint32_t wrap_u;       /* PG_TEXWRAP_* */
    uint32_t wrap_v;
    float uscale, vscale;
    float uoffset, voffset;
    float color0[3];       /* checkerboard only */
    float color1[3];
    float average[3];      /* Texture::getAverage; average[0] < 0: computed here */
    uint32_t pad0;
} pg_texture;
typedef struct pg_texture_binding {
    uint32_t material;     /* its diffuse reflectance is the slot: diffuse, plastic or roughplastic */
    uint32_t texture;
} pg_texture_binding;
/* texcoords: 2 * num_vertices floats of the uploaded scene, or NULL (uv = the barycentrics).  After pg_upload_scene
 * and before the first render pass of that scene (PG_ERR_STATE otherwise); a later pg_upload_scene clears the
 * textures; n_bindings == 0 turns them off.  PG_ERR_INVALID: a zero-sized bitmap, a non-finite or negative texel or
 * colour, a non-finite scale or offset, an enum or index out of range, a material without a diffuse slot, a material
 * bound twice, the volumetric integrator. */
pg_status pg_set_textures(void *ctx, const pg_texture *textures, uint32_t n_textures,
                          const pg_texture_binding *bindings, uint32_t n_bindings, const float *texcoords);
/* Unit entry points (parity tests).  pg_texture_query: the device lookup of `texture` (not necessarily bound; needs
 * only a context) at n raw uv pairs, the uv transform included; out: n x 3.  pg_hit_uvs: the closest hit's
 * interpolated uv before any texture's transform (rays: n x 8 as pg_trace_rays; out: n x 2, (0, 0) for a miss), with
 * the texcoords of the last pg_set_textures, else the barycentrics. */
pg_status pg_texture_query(void *ctx, const pg_texture *texture, const float *uv, uint64_t n, float *out);
pg_status pg_hit_uvs(void *ctx, const float *rays, uint64_t n, float *out);
/* ---- normal maps: the normalmap BSDF adapter (normalmap.cpp) on the surface integrator ---------------------------
 * New entry points; no struct and not PG_ABI_VERSION change.  While no map is bound, no buffer of the feature is
 * allocated, no kernel instantiation is launched that was not launched before and every result is bit for bit what
 * it was.  All of the following is float32 in the order written, without contraction (#pragma clang fp
 * contract(off)).
 *   dpdu  of a triangle whose material carries a map is the tangent of TriMesh::computeUVTangents
 *         (trimesh.cpp:683-735), computed on the host per triangle: with dP1 = p1 - p0, dP2 = p2 - p0, dUV1 = t1 - t0,
 *         dUV2 = t2 - t0 and det = dUV1.x dUV2.y - dUV1.y dUV2.x,
 *             dpdu = (dUV2.y dP1 - dUV1.y dP2) * (1 / det);
 *         det == 0: the first vector of coordinateSystem(cross(dP1, dP2) / |cross(dP1, dP2)|) (util.cpp:594-603); a
 *         zero-area triangle, and every triangle without texcoords (uv = the barycentrics, det = 1), keeps p1 - p0.
 *         Triangles of every other material keep dpdu = p1 - p0 bit for bit.
 *   base  = computeShadingFrame(shN, dpdu) (skdtree.h:373-380,426): n = shN, s = normalize(dpdu - n dot(n, dpdu)),
 *         t = cross(n, s).
 *   c     = the map's value at the hit's uv: the lookup of pg_set_textures above (uv transform, filter, wrap modes).
 *   nl    = 2 c - 1,  n' = normalize(base.toWorld(nl)),  s' = normalize(dpdu - n' dot(n', dpdu)),  t' = cross(n', s')
 *         (NormalMap::getFrame, normalmap.cpp:141-158).  A texel of (0.5, 0.5, 0.5) has no direction: unspecified.
 * Every BSDF eval, pdf and sample of the vertex (next-event estimation, the BSDF sample, the guided branch's eval and
 * pdf of the D-tree direction, the glossy sampling rate) runs in (s', t', n') with wi = toLocal'(-d).  Hemisphere rule
 * (normalmap.cpp:215,233,258,280): a direction wo evaluates to zero, and a sampled one is rejected, when
 * dot(wo_world, shN) * wo'.z <= 0, shN the unperturbed shading normal.  On the unperturbed frame stay: the emitter
 * side test, the reference normal of the emitter sampling, both strict_normals tests (dot(-d, shN) and dot(wo, shN),
 * the reference's its.wi.z and bRec.wo.z), the emitter-hit MIS pdf, the training record and the denoiser buffers.
 * The map is the outermost adapter, normalmap{ [twosided{] bsdf [}] }: PG_MAT_TWOSIDED of the bound material flips in
 * the perturbed frame.  (twosided{normalmap{}} mirrors about the unperturbed tangent plane: not expressible here.)
 * Bound materials: diffuse, plastic, roughplastic, conductor, roughconductor; a material may carry a texture
 * (pg_set_textures) and a map.  Life cycle as pg_set_textures: after pg_upload_scene and before the first render pass
 * (PG_ERR_STATE otherwise), cleared by a later pg_upload_scene, n_bindings == 0 turns the maps off.  The texcoords
 * belong to the scene: where this call and pg_set_textures both pass them they must be equal, and where one passes
 * NULL it reads the other's.  PG_ERR_INVALID: as pg_set_textures for the records and indices, a dielectric,
 * roughdielectric or null material, a material bound twice, unequal texcoords, the volumetric integrator.
 * `average` is not read. */
pg_status pg_set_normal_maps(void *ctx, const pg_texture *maps, uint32_t n_maps, const pg_texture_binding *bindings,
                             uint32_t n_bindings, const float *texcoords);
/* Unit entry point beside pg_hit_records: the frame the closest hit's BSDF calls run in (rays: n x 8 as
 * pg_trace_rays).  out: n x 12, (n', s', t', wi'); the base frame with dpdu = p1 - p0 and its wi where the material
 * carries no map; zeros for a miss. */
pg_status pg_hit_frames(void *ctx, const float *rays, uint64_t n, float *out);
/* ---- thin-lens sensor: depth of field in both integrators ---------------------------------------------------------
 * New entry points; pg_config, pg_stats, pg_scene_desc, pg_camera and PG_ABI_VERSION are unchanged.  The camera of
 * pg_scene_desc is a pinhole (PerspectiveCamera::sampleRay, perspective.cpp:271-298); pg_set_lens puts the thin lens
 * of ThinLens::sampleRay (thinlens.cpp:293-322) in front of it.  With nearP = ((1 - 2 sx) tan_half,
 * (1 - 2 sy) / aspect tan_half, 1) the pinhole's local near-plane point of the sample (float32, no contraction):
 *   (a0, a1)  = draw (sample, dimension 0x40000000) of the pixel's counter stream.  The reference draws the aperture
 *               sample right after the pixel sample (progressiveintegrator.cpp:263-264); here it has a dimension no
 *               other draw uses (surface path: 0 and 8 depth + slot; volumetric path: 1, 2, ...; the transmittance
 *               walks use other keys), so every later draw of a path is the same with the lens on or off.
 *   tmp       = squareToUniformDiskConcentric(a0, a1) * aperture_radius   (warp.cpp:81-102)
 *   focusP    = nearP * focus_distance                                    (nearP.z = 1)
 *   dl        = normalize(focusP - (tmp.x, tmp.y, 0)),  invZ = 1 / dl.z
 *   origin    = camera origin + left tmp.x + up tmp.y
 *   direction = left dl.x + up dl.y + dir dl.z,  tmin = near_clip invZ,  tmax = far_clip invZ
 * aperture_radius == 0 turns the lens off (focus_distance is then ignored and read back as 0): the pinhole kernels
 * run and every result is bit for bit that of a context on which the call was never made.  This deviates from the
 * reference, which turns a zero radius into Epsilon (thinlens.cpp:134-137).  PG_ERR_INVALID, with the state left as
 * it was: a negative or non-finite radius, a non-finite focus distance, a focus distance <= 0 with a radius > 0.
 * Valid for both integrators and at any time; it takes effect at the next pass.  It does not touch the film, the
 * SD-tree or the shadow-blocker list: the caller resets the film as after any camera change (the trained tree stays
 * valid, the lens only moves the first hits).  pg_upload_scene turns the lens off, its camera being a pinhole. */
pg_status pg_set_lens(void *ctx, float aperture_radius, float focus_distance);
pg_status pg_get_lens(void *ctx, float *aperture_radius, float *focus_distance); /* either may be NULL */
/* Unit entry point (parity tests): the camera rays the integrators generate, by the device function they call, for
 * n (global pixel = y * width + x, sample index) pairs under the context's camera, seed and lens.
 * o_tmin: n x 4 floats (origin, tmin); d_tmax: n x 4 floats (direction, tmax). */
pg_status pg_camera_rays(void *ctx, const uint32_t *pixels, const uint32_t *samples, uint32_t n, float *o_tmin,
                         float *d_tmax);
/* ---- delta emitters: point, spot and directional lights in both integrators -----------------------------------------
 * New entry points; pg_config, pg_stats, pg_scene_desc, pg_emitter and PG_ABI_VERSION are unchanged.  While none is
 * set, no kernel compiled for them is launched by the path integrator and every result is bit for bit what it was.
 *
 * The emitters of a scene are picked uniformly (Scene::sampleEmitterDirect, scene.cpp:871-895):
 *   ei = min((uint32_t)(sx * ne), ne - 1),  ne = area + delta + (envmap ? 1 : 0)
 * area emitters first in their uploaded order, then the delta emitters in theirs, the environment emitter last.  The
 * 1 / ne of the emitter-hit MIS weight counts all of them (Scene::pdfEmitterDirect).  A delta emitter's sample is in
 * the discrete measure: its pdf is 1 / ne, its next-event contribution has MIS weight 1 (progressive_path.cpp:211,
 * progressive_volpath.cpp:153,277) and at a guided vertex no D-tree pdf of its direction enters the weight.  It can
 * never be hit.  With ref the shaded point (float32, no contraction):
 *   point (point.cpp:131-147):  d = position - ref, dist = |d|, inv = 1 / dist, d *= inv;  value = intensity (inv inv)
 *   spot (spot.cpp:105-125,184-200):  the point formula times the falloff of cosTheta = dot(-d, direction):
 *          0 where cosTheta <= cos(cutoff_angle), 1 where cosTheta >= cos(beam_width), else
 *          (cutoff_angle - acosf(cosTheta)) / (cutoff_angle - beam_width); the cosines and the reciprocal are computed
 *          once by pg_set_delta_emitters.  No projection texture.
 *   directional (directional.cpp:90-91,159-180):  with (centre, radius) the bounding sphere of the uploaded triangles'
 *          box (its centre, 1.1 x its half diagonal) and diskCentre = centre - direction radius:
 *          dist = dot(ref - diskCentre, direction), a failed sample where dist < 0;  d = -direction, value = intensity
 * The shadow ray is the area emitters': origin ref, to dist (1 - ShadowEpsilon). */
typedef enum { PG_EMITTER_POINT = 0, PG_EMITTER_SPOT = 1, PG_EMITTER_DIRECTIONAL = 2 } pg_delta_type;
typedef struct pg_delta_emitter {
    int32_t type;          /* pg_delta_type */
    float position[3];     /* point, spot: toWorld * (0,0,0) */
    float direction[3];    /* spot: the axis (toWorld * +z); directional: the direction the light travels; normalised
                              on upload */
    float intensity[3];    /* point, spot: W/sr (m_intensity); directional: irradiance on a surface normal to it
                              (m_normalIrradiance) */
    float cutoff_angle, beam_width;   /* spot, radians */
} pg_delta_emitter;
/* After pg_upload_scene and before the first render pass of that scene (PG_ERR_STATE otherwise); a later
 * pg_upload_scene clears the delta emitters; n == 0 removes them, and the context is then bit for bit one on which
 * the call was never made.  Both integrators.  The shadow-blocker list is emptied.  PG_ERR_INVALID, with the state
 * left as it was: an unknown type, a non-finite field, a negative intensity, a zero direction of a spot or a
 * directional light, a spot without 0 <= beam_width < cutoff_angle < pi, more than 65534 emitters in total. */
pg_status pg_set_delta_emitters(void *ctx, const pg_delta_emitter *emitters, uint32_t n);
/* Unit entry point (parity tests): the device function the shaders call for next-event estimation, over the scene's
 * whole emitter set (area, delta, environment), at ref (n x 3) with a zero reference normal and samples (n x 2).
 * out: n x 8 floats: d.xyz, dist, value / pdf (rgb, the emitter-pick probability included), measure (0 = the sample
 * failed, 1 = solid angle, 2 = discrete). */
pg_status pg_emitter_query(void *ctx, const float *ref, const float *samples, uint64_t n, float *out);
/* ---- homogeneous media: analytic free flight, chromatic extinction (volumetric integrator) --------------------------
 * New entry points; pg_config, pg_stats, pg_scene_desc, pg_medium and PG_ABI_VERSION are unchanged.  While no record
 * is set, no kernel compiled for them is launched and every result is bit for bit what it was.
 *
 * HomogeneousMedium with strategy = "balance" (homogeneous.cpp:266-352) as progressive_volpath.cpp:114-217 uses it,
 * in float32 in this order, with sigma_t = sigma_a + sigma_s, exp = (float)exp((double)x) (math::fastexp) and log the
 * tracking loops' logf:
 *   weight: the given value; with -1, max over the channels with sigma_t != 0 of sigma_s / sigma_t, raised to 0.5
 *           when that is > 0 (homogeneous.cpp:168-183)
 *   sampleDistance on a ray with dist = maxt - mint:
 *           rand = next1D;  if rand < weight: rand /= weight, channel = min((int)(next1D * 3), 2),
 *           sampled = -log(1 - rand) / sigma_t[channel];  else sampled = +inf and no second draw
 *           success = sampled < dist and o + d * (sampled + mint) != o;  where sampled >= dist, sampled = dist
 *           pdfFailure = (sum_c exp(-sigma_t[c] sampled)) / 3,  pdfSuccess = (sum_c sigma_t[c] exp(-sigma_t[c] sampled)) / 3
 *           pdfSuccess *= weight,  pdfFailure = weight pdfFailure + (1 - weight)
 *           transmittance[c] = exp(-sigma_t[c] sampled), all three 0 when their maximum is < 1e-20
 *   evalTransmittance: exp(sigma_t[c] (mint - maxt)) per channel, 1 where sigma_t[c] = 0; no draws
 * A medium interaction multiplies the throughput by sigma_s transmittance / pdfSuccess, a flight that reaches the
 * surface or escapes by transmittance / pdfFailure (a grid medium keeps its albedo).  The shadow walks of the
 * next-event estimation and the emitter walks are chromatic per channel wherever they cross a homogeneous segment;
 * such a segment consumes no draw of the walk's sub-stream and is not counted in pg_stats.density_lookups.  Direction
 * guiding at medium vertices and training records work as in a grid medium; pg_config.distance_guiding does not apply
 * inside a homogeneous medium: its flight is the analytic one above whatever beta is.  Not supported: the strategies
 * single, manual and maximum, `monochromatic`, the material presets. */
typedef struct pg_homogeneous_medium {
    uint32_t medium;      /* index into the uploaded scene's media: the entry this record replaces */
    float sigma_a[3];     /* after Medium::Medium's scale; >= 0 */
    float sigma_s[3];
    float g;              /* HG mean cosine, |g| < 1 */
    float medium_sampling_weight; /* -1: the reference's rule (max channel albedo, raised to 0.5 when > 0) */
    uint32_t pad0;
} pg_homogeneous_medium;
/* After pg_upload_scene and before the first render pass of that scene (PG_ERR_STATE otherwise); a later
 * pg_upload_scene clears the records; n == 0 removes them, and the context is then bit for bit one on which the call
 * was never made.  Each call replaces the whole set.  A replaced entry's grid, box, scale and albedo are ignored;
 * shapes and camera_medium keep referring to it by index, and grid and homogeneous media may be mixed in one scene.
 * PG_ERR_INVALID, with the state left as it was: the path integrator, an index out of range or named twice, a
 * non-finite or negative coefficient, sigma_t = 0 in all three channels, |g| >= 1, a weight outside [0, 1] that is
 * not -1.  pg_medium_query refuses a replaced entry (PG_ERR_INVALID); pg_phase_query answers with the record's g. */
pg_status pg_set_homogeneous_media(void *ctx, const pg_homogeneous_medium *media, uint32_t n);
/* Unit entry point (parity tests): the device functions the integrator calls, for the homogeneous medium `medium`.
 * rays: n x 8 floats as pg_trace_rays (o.xyz, mint, d.xyz, maxt); keys: n x 2 (rng key, sample), the draws being
 * dimensions 1, 2, ... of that counter stream as for pg_medium_query (not read by op 1).  out: n x 8 floats.
 * op 0 (sampleDistance): success 1/0, t (mint + sampled; maxt where sampled >= dist), transmittance rgb, pdfSuccess,
 *      pdfFailure, draws used.  op 1 (evalTransmittance): transmittance rgb, then zeros. */
pg_status pg_homogeneous_query(void *ctx, uint32_t medium, int32_t op, const float *rays, const uint32_t *keys, uint64_t n,
                               float *out);
pg_status pg_get_stats(void *ctx, pg_stats *stats);
/* Path integrator: segments (counted in pg_stats.segments, not in escaped) whose hit was culled by the
 * closest-hit kernels since create: the ray's next vertex had already lost its Russian roulette, or was past the
 * depth limit, when the ray was written, and it hit no emitter, so that vertex was never shaded.  0 with
 * PG_NO_PATH_CULL=1 in the environment.  A read-only entry point: pg_stats keeps its ABI 12 layout. */
pg_status pg_get_culled(void *ctx, uint64_t *count);
/* Path integrator: segments since create that an any-hit probe answered instead of the closest-hit walk (the doom
 * probe): the ray's next vertex was already lost, as for pg_get_culled, and the ray misses every padded box over
 * the emitter triangles, so only whether it hits anything was still wanted.  Each is counted in pg_stats.segments
 * and in pg_get_culled (it hit something) or pg_stats.escaped (it did not), as when it was traced.  0 with
 * PG_NO_DOOM_PROBE=1 or PG_NO_PATH_CULL=1 in the environment, and for scenes with an environment emitter.  A
 * read-only entry point like pg_get_culled: pg_stats keeps its ABI 12 layout. */
pg_status pg_get_probes(void *ctx, uint64_t *count);
/* Path integrator: next-event shadow rays since create that the shading kernels resolved as occluded against the
 * learned blocker list, before the ray was stored or queued.  The recording passes count, per triangle, the shadow
 * rays it blocked; after each of them up to 8 triangles that each blocked at least 1/64 of the counted rays are listed,
 * and a later shadow ray that certainly hits one of them (margins on its barycentrics and distance, so the any-hit
 * walk would agree) is dropped where it would have been written.  Each is still counted in pg_stats.shadow_rays.
 * Results do not depend on the list.  0 with PG_NO_SHADOW_CULL=1 in the environment, before the first recording
 * pass, after pg_upload_scene / pg_put_sdtree (the list is emptied) and for scenes with an environment emitter.
 * A read-only entry point like pg_get_culled: pg_stats keeps its ABI 12 layout. */
pg_status pg_get_shadow_culled(void *ctx, uint64_t *count);
/* The current blocker list: *count (<= 8) BVH-order triangle ids in tri_ids[8], most frequent first, and (orig_ids
 * not NULL) the same triangles' indices in the uploaded scene. */
pg_status pg_get_blockers(void *ctx, uint32_t *tri_ids, uint32_t *orig_ids, uint32_t *count);
/* Path integrator: doom probes since create (each counted in pg_get_probes, and in pg_get_culled as the hit it is)
 * that the tracing kernels answered against the learned occluder list instead of walking the tree.  The probe rows of
 * the recording passes count, per triangle, the probes whose walk ended on it; after each of them up to 16 triangles
 * that each took at least 1/64 of the counted probes are listed (kept only if together they took half), and a later
 * probe that certainly hits one of them anywhere along its ray (the blocker test's margins, so the walk would return
 * a hit too) skips its walk.  No counter or result depends on the list.  0 with PG_NO_PROBE_LIST=1 in the
 * environment, before the first recording pass, after pg_upload_scene / pg_put_sdtree (the list is emptied),
 * wherever pg_get_probes is 0, and for the probes of a chunk's tail launch (they always walk).  A read-only entry
 * point like pg_get_culled: pg_stats keeps its ABI 12 layout. */
pg_status pg_get_probes_resolved(void *ctx, uint64_t *count);
/* The current occluder list, as pg_get_blockers: *count (<= 16) ids in tri_ids[16] and (not NULL) orig_ids[16]. */
pg_status pg_get_occluders(void *ctx, uint32_t *tri_ids, uint32_t *orig_ids, uint32_t *count);
/* Number of pixels owned by this rank (tile shard). */
pg_status pg_local_pixel_count(void *ctx, uint64_t *count);

/* ---- unit-level device entry points used by the parity tests ---------------------------- */
/* rays: n x 8 floats (o.xyz, tmin, d.xyz, tmax).  hits: n x 4 (t, prim as float bits, u, v);
 * prim = 0xFFFFFFFF for a miss.  any_hit: hits[i*4] = 1 if occluded else 0. */
pg_status pg_trace_rays(void *ctx, const float *rays, uint64_t n, int32_t any_hit, float *hits);
/* The shading kernels' blocker test on given rays (n x 8 floats as pg_trace_rays) against the k <= 8 BVH-order
 * triangles tri_ids, installed as the list for this call only: out[i] = 1 where the test answers "certainly
 * occluded", else 0.  Wherever it answers 1, pg_trace_rays(any_hit = 1) answers occluded. */
pg_status pg_blocker_test(void *ctx, const float *rays, uint64_t n, const uint32_t *tri_ids, uint32_t k, uint32_t *out);
/* The tracing kernels' occluder test and the probe walk on given rays (n x 8 floats as pg_trace_rays; a probe has no
 * tmax, the eighth float is ignored) against the k <= 16 BVH-order triangles tri_ids, installed as the list for this
 * call only: out[2 i] = 1 where the test answers "the walk certainly returns a hit", out[2 i + 1] = 1 where the probe
 * walk (the any-hit form of the closest-hit walk) returns one.  out[2 i] = 1 implies out[2 i + 1] = 1. */
pg_status pg_occluder_test(void *ctx, const float *rays, uint64_t n, const uint32_t *tri_ids, uint32_t k, uint32_t *out);
/* The closest hit's full record as the shading kernels build it (fillIntersectionRecord<true>,
 * skdtree.h:343-430: barycentric position, face normal flipped to the shading normal's side, interpolated
 * shading normal, shading frame by computeShadingFrame(n, dpdu = p1 - p0), wi = toLocal(-d)); the unit KAT of
 * src/tests/test_dgeom.cpp:69-177.  rays: n x 8 as pg_trace_rays; out: n x 16 floats (p.xyz, t, geoN.xyz,
 * shN.xyz, shFrame.s.xyz, wi.xyz), all zero for a miss. */
pg_status pg_hit_records(void *ctx, const float *rays, uint64_t n, float *out);
/* BSDF queries on the device for material `material` of the uploaded scene.
 * wi: n x 3 local; u: n x 3 (2D sample + component sample); out per query 12 floats:
 * wo.xyz, pdf, weight.rgb, sampled_type, eval(wi,wo_given).rgb, pdf(wi,wo_given).
 * wo_given: n x 3 local directions for the eval/pdf part (may be NULL). */
pg_status pg_bsdf_query(void *ctx, uint32_t material, const float *wi, const float *u,
                        const float *wo_given, uint64_t n, float *out);
/* HG phase function of medium `medium` on the device (HGPhaseFunction::sample / eval, hg.cpp:74-106).
 * in: n x 5 (wi.xyz pointing back along the incident ray, 2D sample); out: n x 5 floats
 * wo.xyz, pdf, eval(wi, wo_given) (0 when wo_given is NULL). */
pg_status pg_phase_query(void *ctx, uint32_t medium, const float *in, const float *wo_given, uint64_t n, float *out);
/* Medium queries on the device for medium `medium` (heterogeneous.cpp:546-660, gridvolume.cpp:337-380).
 * op 0 (density): in n x 3 world points; out n floats = lookupFloat(p) (unscaled).
 * op 1 (free flight) / op 2 (transmittance): in n x 8 rays (o.xyz, mint, d.xyz, maxt) and keys n x 2
 * (rng key, sample): the draws are dimensions 1, 2, ... of that counter stream.  out n x 4:
 * op 1: (interaction 1/0, t, draws used, 0), op 2: (transmittance estimate, draws used, 0, 0).
 * op 3 / op 4: as op 1 / op 2 with PG_MAJORANT_GRID tracking (ops 1, 2 use the global majorant). */
pg_status pg_medium_query(void *ctx, uint32_t medium, int32_t op, const float *in, const uint32_t *keys, uint64_t n,
                          float *out);
/* Environment emitter of the uploaded scene on the device (envmap.cpp).
 * op 0 (EnvironmentMap::sampleDirect, :516-543, from the scene's bounding-sphere centre):
 *      in n x 2 samples; out n x 8 = d.xyz (world), pdf (solid angle), value / pdf (rgb), distance.
 *      pdf = 0 where the sample fails.
 * op 1 (pdfDirect, :545-556): in n x 3 world directions; out n floats (solid-angle pdf).
 * op 2 (evalEnvironment without ray differentials, :380-410): in n x 3 world ray directions;
 *      out n x 3 radiance. */
pg_status pg_envmap_query(void *ctx, int32_t op, const float *in, uint64_t n, float *out);

/* Rough dielectric transmittance slice of a roughplastic material, as RoughPlastic::configure
 * reduces it (roughplastic.cpp:283-299, src/bsdfs/rtrans.h setEta/setAlpha/evalDiffuse):
 * table[100] = transmittance at cos(theta) = (j/99)^4 (interpolated with Catmull-Rom in
 * cos^(1/4)), fdr_int = 1 - internal diffuse transmittance.  Computed on the host at scene upload
 * by quadrature instead of read from data/microfacet/ *.dat.  Needs no device or context. */
/* Building-tree statistics of the SD-tree, i.e. the additive state that splats produce: the u64
 * quadrant sums of every building node (4 per node, 2^-24 fixed point) followed by the record count
 * of every D-tree (u64), in the order of the serialized tree.  Summing these vectors over ranks
 * (an all-reduce) and putting the sum back equals splatting every rank's records into one tree,
 * bit for bit (replaces the record all-gather of postprogression).
 * dst == NULL: only *words is returned.  Between pg_refit calls the layout is fixed. */
pg_status pg_get_tree_stats(void *ctx, void *dst, uint64_t capacity_words, int32_t dst_is_device, uint64_t *words);
pg_status pg_put_tree_stats(void *ctx, const void *src, uint64_t words, int32_t src_is_device);

pg_status pg_rough_transmittance(uint32_t distribution, float alpha, float eta, float *table, float *fdr_int);

/* ---- multi-GPU inside the library: one RCCL communicator per context (RCCL over xGMI) --------
 * Replaces the reference's distributed rendering (the remote scheduler that ships work units and
 * merges image blocks, include/mitsuba/core/sched_remote.h:50-236) for one render job: one
 * process (or thread) per GPU, each with a context created with its rank / world_size (its tile
 * shard).  Rank 0 calls pg_comm_unique_id and hands the PG_COMM_ID_BYTES bytes to every rank by
 * any out-of-band channel (MPI_Bcast, a file, torch.distributed); then every rank calls
 * pg_comm_init.  The pg_comm_* calls below are collective: every rank makes them, in the same
 * order.  Postprogression slot: pg_splat_local_records; pg_comm_allreduce_tree_stats; pg_refit
 * (every rank then holds the tree one GPU builds from all records, bit for bit).  End of the
 * job: pg_comm_reduce_film(root), then the root's pg_read_film returns the whole image. */
#define PG_COMM_ID_BYTES 128
pg_status pg_comm_unique_id(void *id_out);
pg_status pg_comm_init(void *ctx, const void *id);
/* In-place sum over ranks of the building statistics (the pg_get_tree_stats vector) on the device. */
pg_status pg_comm_allreduce_tree_stats(void *ctx);
/* Sum of every rank's film (+ sums of squares, + feature buffers) into rank `root`'s film; the
 * shards are disjoint, so the root's film equals the single-GPU film bit for bit. */
pg_status pg_comm_reduce_film(void *ctx, int32_t root);
/* In-place sum over ranks of n host doubles (e.g. inverse-variance combination statistics). */
pg_status pg_comm_allreduce_f64(void *ctx, double *values, uint64_t n);
/* The record exchange SURVEY.md §5/§8e names (north_star: "RCCL all-gather of records"), the
 * alternative to pg_splat_local_records + pg_comm_allreduce_tree_stats in the postprogression slot:
 * every rank's record count (ncclAllGather of one u64), then every rank's records (ncclAllGather in
 * slices of at most 2^22 records per rank, padded to whole slices, into one reused buffer of
 * world_size slices), and every rank splats ALL records into its building tree, slice by slice in rank
 * order.  Integer splat sums commute, so every rank ends with the tree one GPU builds from all
 * records, bit for bit -- the same tree as the statistics all-reduce.  counts_out (may be NULL):
 * world_size record counts.  The local records stay until pg_refit. */
pg_status pg_comm_allgather_records(void *ctx, uint64_t *counts_out);

#ifdef __cplusplus
}
#endif
#endif /* PG_CAPI_H */
