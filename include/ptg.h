/* ptg.h - C ABI of the MI355X-native path tracer.
 *
 * Drop-in boundary for the reference's per-pixel hot path
 * (Kalache-abdesattar/Path-Tracing...but-on-the-LUMI-cluster @ v1):
 *   path_trace_pixel  path_tracer.hh:637-741
 *   tonemap_pixel     path_tracer.hh:753-771
 *   baseline_render   main.cc:12-46 (the loop that calls them)
 *   ray_query_*       ray_query.hh:111-290 (BVH traversal underneath)
 *
 * Plain C, plain pointers and sizes.  Every type below reproduces the byte
 * layout of the reference type it names (bvh.hh, mesh.hh, scene.hh, math.hh),
 * so a caller holding the reference's std::vectors passes .data() unchanged.
 * NOTE: ptg_float3 is 16 bytes (OpenCL layout, math.hh:36) - never pass HIP's
 * 12-byte float3.
 *
 * Error convention: every int-returning entry returns PTG_OK (0) or a
 * negative PTG_E_* code; ptg_last_error() gives the message.  Nothing calls
 * exit().  One host thread per context; calls on a context are not reentrant
 * (the reference's functions are pure, main.cc drives them from one thread
 * plus OpenMP workers - ptg_render replaces that whole loop).
 */
#ifndef PTG_H
#define PTG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define PTG_ALIGNAS(n) alignas(n)
extern "C" {
#else
#define PTG_ALIGNAS(n) _Alignas(n)
#endif

#define PTG_ABI_VERSION 1

/* ---- reference-layout types ------------------------------------------- */

/* math.hh:31-37 */
typedef struct { PTG_ALIGNAS(8) uint32_t x; uint32_t y; } ptg_uint2;
typedef struct { PTG_ALIGNAS(16) uint32_t x; uint32_t y, z, w; } ptg_uint4;
typedef struct { PTG_ALIGNAS(16) float x; float y, z; } ptg_float3;       /* 16 B */
typedef struct { PTG_ALIGNAS(16) float x; float y, z, w; } ptg_float4;
typedef struct { PTG_ALIGNAS(4) uint8_t x; uint8_t y, z, w; } ptg_uchar4;
/* math.hh:152-153: row vectors */
typedef struct { ptg_float3 r[3]; } ptg_mat3;                              /* 48 B */
typedef struct { ptg_float4 r[4]; } ptg_mat4;                              /* 64 B */

/* bvh.hh:35-39 */
typedef struct { uint32_t node_count, node_offset; } ptg_bvh;
/* bvh.hh:45-49 */
typedef struct { float min_x, min_y, min_z, max_x, max_y, max_z; } ptg_bvh_node;   /* 24 B */
/* bvh.hh:57-67: accept top bit = leaf, rest = payload */
typedef struct { uint32_t accept, cancel; } ptg_bvh_link;
/* mesh.hh:18-28 */
typedef struct { uint32_t vertex_count, triangle_count, index_offset, base_vertex_offset; } ptg_mesh;
/* bvh.hh:73-79 */
typedef struct { ptg_bvh blas; ptg_mesh m; ptg_mat4 transform; ptg_mat4 inv_transform; } ptg_tlas_instance; /* 160 B */
/* scene.hh:7-17 */
typedef struct {
    ptg_mat3 orientation;
    ptg_float3 position;
    float aspect_ratio;
    float inv_focal_length;
    float focal_distance;
    float aperture_angle;
    int32_t aperture_polygon;
    float aperture_radius;
} ptg_camera;                                                              /* 96 B */
/* scene.hh:19-24 */
typedef struct { ptg_float3 direction; ptg_float3 color; float cos_solid_angle; } ptg_directional_light; /* 48 B */
/* scene.hh:26-34 */
typedef struct { ptg_bvh tlas; ptg_camera cam; ptg_directional_light light; } ptg_subframe; /* 160 B */

/* ---- render configuration ---------------------------------------------
 * The reference bakes these in as macros (config.hh:5-29, and
 * path_tracer.hh:431/656/659/697); here they are runtime values.
 */
typedef struct {
    uint32_t width;                        /* IMAGE_WIDTH */
    uint32_t height;                       /* IMAGE_HEIGHT */
    uint32_t samples_per_pixel;            /* SAMPLES_PER_PIXEL */
    uint32_t max_bounces;                  /* MAX_BOUNCES (4 = TESTING preset) */
    uint32_t student_id;                   /* STUDENT_ID, 4th RNG seed word */
    uint32_t samples_per_motion_blur_step; /* SAMPLES_PER_MOTION_BLUR_STEP (8) */
} ptg_render_config;

/* Fill with the reference's shipped values: 640x360, 256 spp, 4 bounces,
 * student id 152121358, 8 samples per motion-blur step (config.hh:5-29). */
void ptg_render_config_default(ptg_render_config* cfg);

/* ---- errors ------------------------------------------------------------ */
#define PTG_OK 0
#define PTG_E_INVALID (-1)   /* bad argument / state */
#define PTG_E_IO (-2)        /* file could not be read or written */
#define PTG_E_NOMEM (-3)     /* host or device allocation failed */
#define PTG_E_HIP (-4)       /* HIP runtime error (message has the hipError_t) */
#define PTG_E_NODEVICE (-5)  /* no usable gfx950 device */
#define PTG_E_RANGE (-6)     /* index / size out of the supported range */

int ptg_abi_version(void);
/* Message of the last error raised on this host thread ("" if none). */
const char* ptg_last_error(void);
/* Host worker threads each of this process's pools (scene load, per-frame
 * TLAS builds, TLAS block packing) may use; 0 (default) = automatic: the CPUs
 * the process may run on (affinity, cgroup CPU quota) divided by the ranks of
 * the node (LOCAL_WORLD_SIZE).  Returns the value now in effect. */
int ptg_set_host_threads(int threads);

/* ---- host-side scene (restatement of scene.cc / bvh.cc / mesh.cc) -------
 * Produces exactly the arrays the reference's load_scene (scene.cc:135) and
 * setup_animation_frame (scene.cc:271) produce, in reference layout.
 */
typedef struct ptg_scene ptg_scene;

typedef struct {
    const ptg_bvh_node* nodes; size_t node_count;     /* bvh_buffers.nodes */
    const ptg_bvh_link* links;                        /* 8 * node_count entries */
    size_t static_node_count;                         /* nodes owned by BLASes (uploaded once) */
    const uint32_t* indices; size_t index_count;      /* mesh_buffers.indices */
    const ptg_float3* pos;                            /* mesh_buffers.pos, vertex_count entries */
    const ptg_float3* normal;
    const ptg_float4* albedo;
    const ptg_float4* material;
    size_t vertex_count;
    const ptg_tlas_instance* instances; size_t instance_count;
    size_t static_instance_count;
    const ptg_subframe* subframes; size_t subframe_count;
} ptg_scene_view;

/* load_scene(): assets_dir must contain data/<name>.obj|.mtl.  The scene
 * depends on the configuration through width/height (camera aspect,
 * scene.cc:284) and samples_per_pixel (subframe count, scene.cc:648-650). */
int ptg_scene_load(const char* assets_dir, const ptg_render_config* cfg, ptg_scene** out);
/* setup_animation_frame() */
int ptg_scene_setup_frame(ptg_scene* s, uint32_t frame_index);
/* Pointers stay valid until the next setup_frame/destroy. */
int ptg_scene_view_get(const ptg_scene* s, ptg_scene_view* out);
/* get_animation_frame_count() (scene.cc:720-724) */
uint32_t ptg_scene_frame_count(const ptg_scene* s);
/* BLAS handle of a named mesh (the scene.meshes map, scene.hh:52); -1 if absent */
int ptg_scene_mesh(const ptg_scene* s, const char* name, ptg_mesh* mesh, ptg_bvh* blas);
void ptg_scene_destroy(ptg_scene* s);

/* write_bmp (bmp.cc:7-63): 24-bit bottom-up BMP from bytes 0..2 of each
 * `stride`-byte pixel of a `pitch`-byte row (BGRA input -> BGR file). */
int ptg_write_bmp(const char* path, uint32_t w, uint32_t h, uint32_t stride, uint32_t pitch,
                  const uint8_t* color_data);

/* ---- GPU renderer -------------------------------------------------------- */
typedef struct ptg_context ptg_context;

/* One context per GPU (device ordinal as seen by HIP).  Fails loudly with
 * PTG_E_NODEVICE if the device is not a gfx950 part. */
int ptg_context_create(int device, ptg_context** out);
void ptg_context_destroy(ptg_context* ctx);
/* hipStream_t the context launches on (NULL = legacy default stream).  Work
 * already queued on the previous stream is ordered before anything queued on
 * the new one (an event recorded there, waited on by the new stream). */
int ptg_context_set_stream(ptg_context* ctx, void* hip_stream);
/* The hipStream_t the context launches on (*out; NULL = the legacy default
 * stream), so a caller can order its own work - e.g. an RCCL collective over
 * the rendered tiles (include/ptg_rccl.h) - after the context's. */
int ptg_context_get_stream(ptg_context* ctx, void** out);
/* The HIP device ordinal of the context (*out). */
int ptg_context_device(ptg_context* ctx, int* out);

/* Once per run: the static part of the arrays (everything load_scene
 * produced).  nodes/links hold node_count BVH nodes (links: 8 per node, the
 * bvh_buffers layout, bvh.cc:218-225).  Host pointers. */
int ptg_upload_scene(ptg_context* ctx,
                     const ptg_bvh_node* nodes, const ptg_bvh_link* links, size_t node_count,
                     const uint32_t* indices, size_t index_count,
                     const ptg_float3* pos, const ptg_float3* normal,
                     const ptg_float4* albedo, const ptg_float4* material, size_t vertex_count);

/* Once per frame: what setup_animation_frame changed.  frame_nodes/links are
 * the TLAS nodes appended after the static ones (node indices
 * first_node .. first_node+frame_node_count-1 of the reference's
 * bvh_buffers; first_node must equal the static node count).  instances is
 * the full instance array (static + this frame's dynamic ones).  Host
 * pointers, read before the call returns (the caller may overwrite them at
 * once); the device copies are queued on the context's stream behind any
 * render already queued there.  The call waits only for the copies of the
 * upload two calls back (its pinned staging is reused) or, when a device
 * buffer must grow, for the stream to drain. */
int ptg_upload_frame(ptg_context* ctx,
                     const ptg_subframe* subframes, size_t subframe_count,
                     const ptg_tlas_instance* instances, size_t instance_count,
                     const ptg_bvh_node* frame_nodes, const ptg_bvh_link* frame_links,
                     size_t first_node, size_t frame_node_count);

/* Convenience: upload_scene + upload_frame from a ptg_scene. */
int ptg_upload_from_scene(ptg_context* ctx, const ptg_scene* s, int include_static);

/* baseline_render() body for a rectangle of the image: for each pixel, sum
 * path_trace_pixel over sample indices [sample_begin, sample_end) in index
 * order in float32 (main.cc:24-39), divide by cfg->samples_per_pixel
 * (main.cc:42) and tonemap (main.cc:43).
 * out_accum (optional, DEVICE pointer, [h][w] ptg_float4): the averaged radiance.
 * out_bgra  (optional, DEVICE pointer, [h][w] ptg_uchar4): tonemap_pixel output.
 * Pixel (x0+i, y0+k) lands at row k, column i.  Asynchronous on the context's
 * stream. */
int ptg_render(ptg_context* ctx, const ptg_render_config* cfg,
               uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
               uint32_t sample_begin, uint32_t sample_end,
               ptg_float4* out_accum, ptg_uchar4* out_bgra);

/* Same for an interleaved set of tiles (multi-GPU sharding): tiles of
 * tile_w x tile_h pixels numbered row-major over the image; this call renders
 * tiles first_tile, first_tile + tile_stride, ... (tile_count of them) and
 * writes them densely, tile after tile, each tile row-major
 * (tile_w*tile_h pixels per tile; pixels outside the image are left 0). */
int ptg_render_tiles(ptg_context* ctx, const ptg_render_config* cfg,
                     uint32_t tile_w, uint32_t tile_h,
                     uint32_t first_tile, uint32_t tile_stride, uint32_t tile_count,
                     ptg_float4* out_accum, ptg_uchar4* out_bgra);

/* Scatter densely packed tiles (as written by ptg_render_tiles for one
 * first_tile/tile_stride set) into a full image; DEVICE pointers. */
int ptg_scatter_tiles(ptg_context* ctx, const ptg_render_config* cfg,
                      uint32_t tile_w, uint32_t tile_h,
                      uint32_t first_tile, uint32_t tile_stride, uint32_t tile_count,
                      const ptg_uchar4* tiles_bgra, ptg_uchar4* image_bgra);

/* path_trace_pixel (path_tracer.hh:637) for a batch of (pixel, sample_index)
 * pairs: out[i] = path_trace_pixel(xy[i], sample_index[i], ...) (w = 0).
 * HOST pointers; synchronous.  Used for per-sample parity. */
int ptg_path_trace_samples(ptg_context* ctx, const ptg_render_config* cfg, size_t n,
                           const ptg_uint2* xy, const int32_t* sample_index, ptg_float4* out);

/* tonemap_pixel (path_tracer.hh:753) on n colours. HOST pointers; synchronous. */
int ptg_tonemap(ptg_context* ctx, size_t n, const ptg_float4* color, ptg_uchar4* out);
/* The same on DEVICE pointers, asynchronous on the context's stream (the
 * sample-range shard tonemaps the reduced radiance with it). */
int ptg_tonemap_device(ptg_context* ctx, size_t n, const ptg_float4* color, ptg_uchar4* out);

/* Ray-level query through the uploaded scene with subframe `subframe`'s TLAS:
 * rays are 8 floats (origin.xyz, dir.xyz, tmin, tmax).  For each ray, hits
 * gets 8 words {bary.x, bary.y, bary.z, thit (f32), instance_id, primitive_id,
 * back_face, shadowed}: the closest hit of ray_query_proceed/confirm
 * (ray_query.hh:248-290) and the any-hit bool of a single proceed
 * (path_tracer.hh:415-427).  HOST pointers; synchronous.
 * Contract: every tmin is +0 or positive (or NaN / +inf, which no hit
 * passes), as the reference's queries are (0 and MIN_RAY_DIST); a ray with a
 * negative or -0 tmin is refused (PTG_E_INVALID, nothing traced).  Any tmax
 * is accepted. */
int ptg_trace_rays(ptg_context* ctx, uint32_t subframe, size_t n, const float* rays, uint32_t* hits);

/* The same query through the kernels a render walks with: the wavefront
 * pipeline's closest-hit and any-hit walk kernels, launched over the n rays as
 * the queue of bounce round `round` (below 255) of subframe `subframe`, with
 * the render's launch shape - or with grid_blocks workgroups (0: the
 * context's own grid; above it: refused).  rays are 6 floats (origin.xyz,
 * dir.xyz): tmin and tmax are the kernels' own for that round - closest hit:
 * tmin 0 in round 0, MIN_RAY_DIST (1e-4) after it, tmax 1e9; any hit:
 * MIN_RAY_DIST and MAX_RAY_DIST (1e9).  hits is ptg_trace_rays' record, except
 * that word 2 is always 0 (the walk stores two barycentrics) and that words
 * 0-2 are 0 on a miss.  A queue position that neither walk wrote fails the
 * call (PTG_E_RANGE, the message names the position).
 * counted != 0 runs the kernels' counting instantiations (same results) and
 * fills stats[k] for the closest-hit (k = 0) and the any-hit walk (k = 1):
 *   [0] walks started
 *   [1] walks whose stack outgrew its on-chip window (part of it went to HBM)
 *   [2] the largest stack size seen, in the stack's own units: 8-byte entries
 *       in the closest-hit walk, 4-byte slots (one per entry) in the any-hit
 *       walk; both windows hold 16 of them
 *   [3] any-hit walks that began with the occluder a neighbouring ray found
 * A counted run whose [2] is above what a walk lane's HBM area holds (the
 * frame's stack bound in entries, twice that in slots) fails with
 * PTG_E_RANGE.  stats may be null in a plain run, which zeroes it otherwise.  HOST pointers;
 * synchronous; waits for the context's queued work first and changes nothing
 * a render or ptg_last_* reports.  Used for ray-level parity of the walks. */
int ptg_walk_rays(ptg_context* ctx, uint32_t subframe, uint32_t round, uint32_t grid_blocks, int counted,
                  size_t n, const float* rays /* n x 6 */, uint32_t* hits /* n x 8 */, uint64_t stats[2][4]);

/* The first ray path_trace_pixel traces for each (pixel, sample_index) pair:
 * the seed, the film jitter and get_camera_ray (path_tracer.hh:659-671,
 * :429-450).  rays gets 8 floats per pair, the layout ptg_trace_rays takes:
 * {origin.xyz, dir.xyz, 0, MAX_RAY_DIST (1e9)}; subframe gets
 * sample_index / samples_per_motion_blur_step, the subframe whose camera and
 * TLAS the sample uses.  HOST pointers; synchronous. */
int ptg_camera_rays(ptg_context* ctx, const ptg_render_config* cfg, size_t n,
                    const ptg_uint2* xy, const int32_t* sample_index,
                    float* rays /* n x 8 */, uint32_t* subframe /* n */);

/* ---- first-hit feature buffers and the denoiser -------------------------
 * What the first ray of every sample saw, averaged like the radiance.  With
 * the rectangle and sample-range meaning of ptg_render: each sample j of
 * [sample_begin, sample_end) casts the camera ray of (pixel, j)
 * (ptg_camera_rays) and takes its closest hit in that sample's subframe.
 *   hit:  albedo = the interpolated vertex albedo (path_tracer.hh:373-392),
 *         coverage 1, normal = the unit world-space shading normal, flipped on
 *         a back face (the vector trace_ray builds its tangent space from),
 *         depth = the hit distance
 *   miss: albedo (1,1,1), coverage 0, normal (0,0,0), depth 0
 * out_albedo = (sum albedo.rgb, sum coverage), out_normal_depth =
 * (sum normal.xyz, sum depth): each component summed in float32 in sample
 * order starting from +0, then divided by cfg->samples_per_pixel.
 * DEVICE pointers, [h][w] ptg_float4 each; asynchronous on the context's
 * stream. */
int ptg_render_features(ptg_context* ctx, const ptg_render_config* cfg,
                        uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                        uint32_t sample_begin, uint32_t sample_end,
                        ptg_float4* out_albedo, ptg_float4* out_normal_depth);

/* Edge-avoiding a-trous wavelet denoiser over the radiance, guided by the two
 * feature buffers.  Every operation is one float32 rounding in a fixed order
 * and the weights' exp is glibc's double exp, so a CPU restatement reproduces
 * the output bit for bit (DESIGN.md has the definition; the package's
 * denoise.atrous_reference is that restatement).  A pixel with a non-finite
 * channel is never used as a tap and is itself replaced by the weighted mean
 * of its finite neighbours. */
typedef struct {
    uint32_t iterations;   /* 0..8 passes; pass k has taps 2^k pixels apart */
    float sigma_color;     /* demodulated-radiance distance scale (halved every pass) */
    float sigma_albedo;    /* albedo + coverage distance scale */
    float sigma_normal;    /* normal distance scale */
    float sigma_depth;     /* relative depth distance scale */
    float albedo_floor;    /* radiance is divided by max(albedo, albedo_floor) before filtering */
} ptg_denoise_params;
void ptg_denoise_params_default(ptg_denoise_params* params);
/* radiance, albedo, normal_depth: [h][w] ptg_float4 as written by ptg_render
 * (out_accum) and ptg_render_features.  out_radiance ([h][w], w component 0)
 * may be the same buffer as radiance; out_bgra (optional) is tonemap_pixel of
 * it.  The intermediate images belong to the context.  iterations > 8, or a
 * sigma or albedo_floor that is not positive and finite, is PTG_E_INVALID;
 * iterations == 0 copies the radiance bits unchanged.  DEVICE pointers;
 * asynchronous on the context's stream. */
int ptg_denoise(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_denoise_params* params,
                const ptg_float4* radiance, const ptg_float4* albedo,
                const ptg_float4* normal_depth,
                ptg_float4* out_radiance, ptg_uchar4* out_bgra);

/* ---- per-pixel sample moments and the variance-guided denoiser ----------
 * ptg_render with one more output: how noisy each pixel's samples were.
 * Rectangle, sample range, out_accum and out_bgra are ptg_render's, bit for
 * bit.  out_moments (required, DEVICE pointer, [h][w] ptg_float4) gets, per
 * pixel, over the samples j of [sample_begin, sample_end) in index order:
 *   L_j = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z of c = path_trace_pixel(xy, j),
 *   for the n samples whose three channels are finite (a non-finite sample
 *   stays in the radiance sum and is left out here);
 *   s1 = sum L_j, s2 = sum L_j*L_j, both float32 from +0 in index order;
 *   m1 = s1/n, m2 = s2/n, var = max(m2 - m1*m1, 0) (0 for a NaN),
 *   vm = var/(n - 1), the variance of the pixel's mean (0 when n < 2);
 *   out_moments = (m1, m2, vm, (float)n), all 0 when n == 0.
 * The moments are normalised by the n finite samples of the range rendered,
 * NOT by cfg->samples_per_pixel as out_accum is: a partial sample range gives
 * the moments of that range.  Every operation is one float32 rounding.  A
 * null out_moments is PTG_E_INVALID.  Asynchronous on the context's stream. */
int ptg_render_moments(ptg_context* ctx, const ptg_render_config* cfg,
                       uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                       uint32_t sample_begin, uint32_t sample_end,
                       ptg_float4* out_accum, ptg_uchar4* out_bgra, ptg_float4* out_moments);

/* Radiance, moments and first-hit features in one pass: as if
 * ptg_render_moments and ptg_render_features had been called with the same
 * rectangle and sample range.  out_accum, out_bgra and out_moments (each
 * optional) are ptg_render_moments' bits - with a null out_moments,
 * ptg_render's; out_albedo and out_normal_depth (both required) are
 * ptg_render_features' bits, the division by cfg->samples_per_pixel and the
 * miss contribution included.  No arithmetic of its own is defined.  On the
 * wavefront pipeline the features are taken from the render's own primary
 * rays, so no second walk is made; under ptg_set_pipeline(ctx, 1) the two
 * passes run one after the other.  A null feature output, or two outputs
 * that are the same buffer, is PTG_E_INVALID; rectangle, sample range and
 * configuration are checked as ptg_render checks them.  A rectangle only (the
 * tile set is ptg_render_tiles_packed).  DEVICE pointers; asynchronous on the
 * context's stream. */
int ptg_render_with_features(ptg_context* ctx, const ptg_render_config* cfg,
                             uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                             uint32_t sample_begin, uint32_t sample_end,
                             ptg_float4* out_accum, ptg_uchar4* out_bgra, ptg_float4* out_moments,
                             ptg_float4* out_albedo, ptg_float4* out_normal_depth);

/* ---- tile packs: the five planes of a tile shard in one buffer ----------
 *
 * A tile pack is what one rank of a tile shard sends to the rank that
 * assembles the frame: ptg_render_with_features' five planes of its tiles in
 * ONE contiguous DEVICE buffer, so that one gather ships them all.  For
 * pack_tiles tiles of tile_w x tile_h pixels, S = pack_tiles * tile_w * tile_h
 * slots and the planes start at these byte offsets of the pack:
 *
 *     accum         0       [S] ptg_float4
 *     moments       16 * S  [S] ptg_float4
 *     albedo        32 * S  [S] ptg_float4
 *     normal_depth  48 * S  [S] ptg_float4
 *     bgra          64 * S  [S] ptg_uchar4
 *
 * Slot k * tile_w * tile_h + q of every plane holds pixel q (row-major within
 * the tile) of the rank's k-th tile: ptg_render_tiles' slot order.
 *
 * ptg_tile_pack_bytes is the pack's size: 68 * S rounded up to a multiple of
 * 256, which is also the stride from one rank's pack to the next in a
 * gathered buffer.  68 * S alone need not be a multiple of 16 (one 5 x 3 tile:
 * 1020), and the float4 planes of the second pack would then be misaligned.
 * 0 for a zero dimension, or when S does not stay below 2^31. */
size_t ptg_tile_pack_bytes(uint32_t tile_w, uint32_t tile_h, uint32_t pack_tiles);

/* ptg_render_with_features over ptg_render_tiles' tile set and the whole
 * sample range [0, cfg->samples_per_pixel), written into a tile pack sized
 * for pack_tiles >= tile_count tiles (every rank of a shard sizes its pack
 * for the largest tile count, so that the packs gather).  Every plane value
 * of a pixel inside the image is the bit pattern ptg_render_with_features
 * writes for that pixel in a render of the full rectangle; no arithmetic of
 * its own is defined.  Every other byte of the pack - pixels outside the
 * image, the tiles from tile_count to pack_tiles, the padding - is 0: the
 * pack is cleared on the stream before the render.  Under
 * ptg_set_pipeline(ctx, 1) the two passes run one after the other, as in
 * ptg_render_with_features.  pack_tiles < tile_count, a null pack or one that
 * is not 16-byte aligned is PTG_E_INVALID; the tile set and the configuration
 * are checked as ptg_render_tiles checks them.  A refused call launches
 * nothing.  Asynchronous on the context's stream. */
int ptg_render_tiles_packed(ptg_context* ctx, const ptg_render_config* cfg,
                            uint32_t tile_w, uint32_t tile_h,
                            uint32_t first_tile, uint32_t tile_stride, uint32_t tile_count,
                            uint32_t pack_tiles, void* pack /* DEVICE, ptg_tile_pack_bytes */);

/* The frame from the gathered packs of a `world`-rank tile shard: tile t
 * (row-major over the image) was rendered by rank t % world as its tile
 * t / world (first_tile = rank, tile_stride = world), and pack r starts at
 * packs + r * ptg_tile_pack_bytes(tile_w, tile_h, pack_tiles).  ONE launch
 * copies every requested plane of the whole image: a work-item owns an image
 * pixel, finds its pack and slot, loads the pixel's value from each requested
 * plane and stores it at out_*[y * width + x] (each output optional,
 * [height][width]).  Every pixel has exactly one source, so the outputs need
 * no clearing, and the values are the packs' bits.  No output, two outputs
 * that are the same buffer, an output that overlaps `packs`, world == 0, a
 * null `packs` or a pointer that is not aligned for its elements (16 bytes;
 * out_bgra 4) is PTG_E_INVALID; pack_tiles below ceil(tiles / world) is
 * PTG_E_RANGE.  A refused call launches nothing.  Needs no scene.  DEVICE
 * pointers; asynchronous on the context's stream. */
int ptg_assemble_tile_packs(ptg_context* ctx, const ptg_render_config* cfg,
                            uint32_t tile_w, uint32_t tile_h, uint32_t world, uint32_t pack_tiles,
                            const void* packs /* world packs back to back */,
                            ptg_float4* out_accum, ptg_uchar4* out_bgra, ptg_float4* out_moments,
                            ptg_float4* out_albedo, ptg_float4* out_normal_depth);

/* ptg_denoise with the luminance range set per pixel by the variance of the
 * pixel's mean (moments.z of ptg_render_moments) instead of a fixed
 * sigma_color: each pass prefilters the variance over 3 x 3 pixels, weighs a
 * tap's luminance difference by sigma_luminance * sqrt(variance) +
 * variance_floor, and filters the variance along with the image (weights
 * squared), so later passes narrow by themselves.  The guide terms are
 * ptg_denoise's.  Defined to the bit in DESIGN.md;
 * denoise.atrous_guided_reference is the CPU restatement. */
typedef struct {
    uint32_t iterations;   /* 0..8 passes; pass k has taps 2^k pixels apart */
    float sigma_luminance; /* luminance distance scale, in standard deviations of the pixel's mean */
    float sigma_albedo;    /* albedo + coverage distance scale */
    float sigma_normal;    /* normal distance scale */
    float sigma_depth;     /* relative depth distance scale */
    float albedo_floor;    /* radiance is divided by max(albedo, albedo_floor) before filtering */
    float variance_floor;  /* added to the luminance scale, so a noiseless pixel still has a range */
} ptg_denoise_guided_params;
void ptg_denoise_guided_params_default(ptg_denoise_guided_params* params);
/* radiance, albedo, normal_depth, out_radiance, out_bgra as for ptg_denoise;
 * moments: [h][w] ptg_float4 as written by ptg_render_moments (only .z is
 * read; a negative or non-finite .z counts as 0).  iterations > 8, or a float
 * field that is not positive and finite, is PTG_E_INVALID; iterations == 0
 * copies the radiance bits unchanged.  DEVICE pointers; asynchronous on the
 * context's stream. */
int ptg_denoise_guided(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_denoise_guided_params* params,
                       const ptg_float4* radiance, const ptg_float4* albedo,
                       const ptg_float4* normal_depth, const ptg_float4* moments,
                       ptg_float4* out_radiance, ptg_uchar4* out_bgra);

/* ---- temporal accumulation -----------------------------------------------
 * Carries last frame's accumulated radiance and luminance moments into this
 * frame.  Per pixel: the first-hit point (the pixel's centre ray through
 * `cam`, at the mean first-hit distance normal_depth.w / albedo.w) is
 * projected into `hist_cam`; of the four bilinear taps around it, those that
 * lie inside the image, carry a finite radiance, a positive coverage and a
 * positive sample count, and show the same surface (depth, normal and albedo
 * within the tolerances below) give the history; it is blended with this
 * frame's pixel by sample counts, the history's capped at max_history:
 *   a = n / (min(n_hist, max_history) + n),  out = hist + a * (this - hist)
 * for the radiance and for the two moments.  A pixel without a valid tap
 * keeps this frame's bits; a pixel whose own radiance is not finite (or whose
 * moments hold no sample) and that has a history takes the history alone, so
 * it comes out finite.  Every operation is one float32 rounding in a fixed
 * order (DESIGN.md 4.13 is the definition; denoise.temporal_reference the CPU
 * restatement, bit for bit). */
typedef struct {
    float max_history;       /* cap on the history's effective sample count, in samples */
    float depth_tolerance;   /* relative: |z_hist - z_expected| <= tol * max(z_hist, z_expected) */
    float normal_tolerance;  /* squared distance of the two normal.xyz */
    float albedo_tolerance;  /* squared distance of the two (albedo.rgb, coverage) */
} ptg_temporal_params;
void ptg_temporal_params_default(ptg_temporal_params* params);
/* radiance, moments, albedo, normal_depth: this frame's [h][w] ptg_float4
 * images as ptg_render_moments (out_accum, out_moments) and
 * ptg_render_features write them; cam: the camera they were rendered with
 * (for a motion-blurred frame, one of its subframe cameras).  hist_radiance,
 * hist_moments: the previous call's out_radiance and out_moments;
 * hist_albedo, hist_normal_depth, hist_cam: the previous frame's guides and
 * camera.  The images are DEVICE pointers; the two cameras are HOST
 * pointers, read before the call returns.  hist_cam and the four hist_*
 * images are all null (first frame: the outputs are the inputs' bits, with
 * out_radiance.w = 0) or all set; a mix is PTG_E_INVALID.
 * out_radiance ([h][w], w component 0) and out_moments ([h][w], the layout
 * of ptg_render_moments: m1, m2, variance of the mean, sample count; it goes
 * into ptg_denoise_guided and back in as the next frame's hist_moments) may
 * be this frame's radiance and moments themselves, which are read only at the
 * pixel written; an output that is one of the hist_* images, which are
 * gathered from neighbours, is PTG_E_INVALID, as are out_radiance ==
 * out_moments and a parameter that is not positive and finite.  out_bgra
 * (optional) is tonemap_pixel of out_radiance.  w or h above 2^24 is
 * PTG_E_RANGE.  Asynchronous on the context's stream. */
int ptg_temporal_accumulate(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_temporal_params* params,
                            const ptg_camera* cam, const ptg_camera* hist_cam,
                            const ptg_float4* radiance, const ptg_float4* moments,
                            const ptg_float4* albedo, const ptg_float4* normal_depth,
                            const ptg_float4* hist_radiance, const ptg_float4* hist_moments,
                            const ptg_float4* hist_albedo, const ptg_float4* hist_normal_depth,
                            ptg_float4* out_radiance, ptg_float4* out_moments, ptg_uchar4* out_bgra);

/* ---- temporal accumulation: several cameras and a history clamp -----------
 * ptg_temporal_accumulate with two insertions, for a frame whose camera moves
 * (DESIGN.md 4.17 is the definition; denoise.temporal_clamped_reference the
 * CPU restatement, bit for bit).
 *  - The reprojection runs once per camera of `cams`, in order, with the
 *    same pixel, depth and hist_cam; every valid tap of every camera adds into
 *    the same sums, and a camera that fails a test adds nothing.  Passing the
 *    subframe cameras of a motion-blurred frame gathers the history along the
 *    blur.  n_cams == 1 is ptg_temporal_accumulate's reprojection exactly.
 *  - With clamp_radius r > 0, a pixel that found history has the history's
 *    colour clamped per channel to [mu - clamp_sigma * sd, mu + clamp_sigma *
 *    sd], mu and sd the mean and standard deviation of this frame's radiance
 *    over the (2r + 1)^2 window around the pixel (pixels outside the image or
 *    with a non-finite channel left out; an empty window does not clamp).
 *    Where a channel was clipped, the history's first luminance moment moves
 *    with the colour, the second keeps the variance, and the history's sample
 *    count is capped at clipped_history (before the max_history cap).
 * With n_cams == 1 and clamp_radius == 0 the outputs are
 * ptg_temporal_accumulate's bits. */
typedef struct {
    ptg_temporal_params base;   /* as for ptg_temporal_accumulate */
    uint32_t clamp_radius;      /* 0: no clamp; 1 or 2: window (2r+1)^2 of this frame's radiance */
    float clamp_sigma;          /* half-width of the colour box, in standard deviations of the window */
    float clipped_history;      /* cap on the history's sample count at a pixel whose history was clipped */
} ptg_temporal_clamp_params;
/* base: ptg_temporal_params_default's; clamp_radius 1, clamp_sigma 2,
 * clipped_history 32: the best row of the measured sweep. */
void ptg_temporal_clamp_params_default(ptg_temporal_clamp_params* params);
/* The image arguments, hist_cam and everything ptg_temporal_accumulate says
 * about them carry over: the all-or-nothing history, no output that is a
 * hist_* image, out_radiance != out_moments, PTG_E_RANGE above 2^24.  Beyond
 * that: cams is a HOST array of n_cams cameras, 1 <= n_cams <= 512, read
 * before the call returns (they travel through a buffer the context owns; a
 * call queued behind another does not disturb it); clamp_radius <= 2;
 * clamp_sigma and clipped_history positive and finite; anything else is
 * PTG_E_INVALID and launches nothing.  With clamp_radius > 0 the radiance is
 * gathered from neighbours, so out_radiance == radiance is PTG_E_INVALID;
 * with clamp_radius == 0 it stays allowed, and out_moments == moments is
 * allowed in both cases (the moments are read at the pixel alone).
 * out_flags (optional, DEVICE, [h][w] bytes): bit 0 the pixel found history,
 * bit 1 its history was clipped.  Asynchronous on the context's stream. */
int ptg_temporal_accumulate_clamped(ptg_context* ctx, uint32_t w, uint32_t h, const ptg_temporal_clamp_params* params,
                                    uint32_t n_cams, const ptg_camera* cams, const ptg_camera* hist_cam,
                                    const ptg_float4* radiance, const ptg_float4* moments,
                                    const ptg_float4* albedo, const ptg_float4* normal_depth,
                                    const ptg_float4* hist_radiance, const ptg_float4* hist_moments,
                                    const ptg_float4* hist_albedo, const ptg_float4* hist_normal_depth,
                                    ptg_float4* out_radiance, ptg_float4* out_moments, ptg_uchar4* out_bgra,
                                    uint8_t* out_flags);

/* ---- adaptive sampling ----------------------------------------------------
 * A render that stops sampling a pixel once its mean is known well enough.
 * cfg->samples_per_pixel = N is the budget (the frame is set up for it: N / m
 * subframes, m = samples_per_motion_blur_step), spent in `passes` passes of
 * N / passes samples.  Pass k owns the subframes k, k + passes, ...: its local
 * sample jj is sample ((jj / m) * passes + k) * m + jj % m of the frame, so
 * every pass covers the whole shutter.  A pixel adds the samples of the
 * passes it takes, in pass order and in jj order inside a pass, into the
 * running sums ptg_render_moments keeps (radiance sum; s1, s2, n over the
 * finite samples, all from +0).  After pass k, when min_passes <= k + 1 <
 * passes, every pixel of the rectangle is judged on its current sums:
 *   noisy = n < 2 || !(vm <= tol * tol),  tol = threshold * (m1 + luminance_floor),
 *   m1 = s1/n, m2 = s2/n, vm = max(m2 - m1*m1, 0) / (n - 1)
 * and a pixel takes pass k + 1 if any pixel of its (2 dilate + 1)^2 window,
 * clipped to the rectangle, is noisy.  The rule keeps no state: a pixel that
 * stopped is woken again by a neighbour that turns noisy.  Before min_passes
 * every pixel is active; when no pixel is, the render ends.  Every operation
 * is one float32 rounding (DESIGN.md 4.14 is the definition, the package's
 * adaptive.adaptive_reference the CPU restatement, bit for bit).
 * With passes = 1 the three image outputs are ptg_render_moments' bits. */
typedef struct {
    uint32_t passes;        /* 1..16; N must be a multiple of passes * samples_per_motion_blur_step */
    uint32_t min_passes;    /* 1..passes: passes every pixel takes before the first selection */
    uint32_t dilate;        /* 0..2: radius of the window a noisy pixel keeps awake */
    float threshold;        /* relative standard error of the mean luminance a pixel stops at */
    float luminance_floor;  /* added to the mean, so a dark pixel has a tolerance too */
} ptg_adaptive_params;
void ptg_adaptive_params_default(ptg_adaptive_params* params);
/* Rectangle as for ptg_render.  Outputs, DEVICE pointers, [h][w], each
 * optional but at least one given; with ns = (passes the pixel took) * N / passes:
 *   out_accum   = radiance sum / (float)ns per channel, w = 0 (the pixel's own
 *                 count, not N);  out_bgra = tonemap_pixel of it;
 *   out_moments = (m1, m2, vm, (float)n) in ptg_render_moments' layout, for
 *                 ptg_denoise_guided and ptg_temporal_accumulate as they are;
 *   out_samples = ns (uint32).
 * Runs on the wavefront pipeline at every ptg_set_concurrency level with the
 * same bits; under ptg_set_pipeline(ctx, 1), or with a parameter outside the
 * ranges above, a threshold or floor that is not positive and finite, or an
 * N that passes * samples_per_motion_blur_step does not divide, it is
 * PTG_E_INVALID and launches nothing.  The call WAITS on the context's
 * stream once per selection: the host reads the 4-byte length of the next
 * pass's pixel list (nothing else is read back); the last pass and the
 * outputs are queued asynchronously as ptg_render's are. */
int ptg_render_adaptive(ptg_context* ctx, const ptg_render_config* cfg,
                        uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                        const ptg_adaptive_params* params,
                        ptg_float4* out_accum, ptg_uchar4* out_bgra, ptg_float4* out_moments,
                        uint32_t* out_samples);
/* The last ptg_render_adaptive call of the context: the passes it ran and the
 * active pixel count of each (active[k] = 0 from passes_run on).  The samples
 * it took are the sum of active[k] * N / passes. */
int ptg_last_adaptive_stats(ptg_context* ctx, uint32_t* passes_run, uint64_t active[16]);

/* ---- progressive rendering: a resumable sample accumulator ----------------
 * ptg_render_with_features in steps.  The running per-pixel sums that the
 * render entries keep inside the context and divide on their last chunk are
 * here a DEVICE buffer the caller owns (`state`), described by a small HOST
 * header (ptg_accum): ptg_accum_add traces the next samples into it,
 * ptg_accum_resolve divides and tonemaps a copy at any time without ending the
 * accumulation, and the two together are a checkpoint: a state copied out,
 * kept in a file and put back, in this or another context or process,
 * continues to the bits of the one-shot render, because every sum goes on in
 * sample order from the very float32 values the one-shot render would hold at
 * that sample.
 *
 * State layout (the checkpoint format).  `planes` planes of [h][w] ptg_float4,
 * row-major over the rectangle (pixel (x0+i, y0+k) at row k, column i), one
 * after the other:
 *   plane 0                   the radiance sums (ax, ay, az, 0)
 *   with PTG_ACCUM_MOMENTS    one plane (s1, s2, n, 0): the luminance sums of
 *                             ptg_render_moments over the finite samples, n a
 *                             uint32 stored in the float's bits
 *   with PTG_ACCUM_FEATURES   two planes: (sum albedo.rgb, sum coverage), then
 *                             (sum normal.xyz, sum depth) of ptg_render_features
 * Every sum is float32, in sample order from +0; a fresh state is all-zero
 * bytes. */
#define PTG_ACCUM_MOMENTS  1u   /* keep the luminance moments (s1, s2, n) */
#define PTG_ACCUM_FEATURES 2u   /* keep the eight first-hit feature sums */
#define PTG_ACCUM_MAGIC    0x41475450u   /* 'PTGA' */
#define PTG_ACCUM_VERSION  1u
typedef struct {                /* 64 bytes, HOST; written by ptg_accum_begin / _add only */
    uint32_t magic, version;    /* PTG_ACCUM_MAGIC, PTG_ACCUM_VERSION */
    ptg_render_config cfg;      /* the configuration every add uses */
    uint32_t x0, y0, w, h;      /* rectangle (no tile set) */
    uint32_t flags;             /* PTG_ACCUM_* */
    uint32_t sample_begin, sample_next;   /* the state holds samples [sample_begin, sample_next) */
    uint32_t reserved;          /* 0 */
} ptg_accum;
#ifdef __cplusplus
static_assert(sizeof(ptg_accum) == 64, "ptg_accum is 16 words");
#else
_Static_assert(sizeof(ptg_accum) == 64, "ptg_accum is 16 words");
#endif
/* Bytes of a state: planes * w * h * 16, planes = 1 + (MOMENTS: 1) +
 * (FEATURES: 2); 0 for unknown flag bits. */
size_t ptg_accum_state_bytes(uint32_t w, uint32_t h, uint32_t flags);
/* Start an accumulation over a rectangle: the configuration and the rectangle
 * are checked as ptg_render checks them (a scene and a frame are uploaded),
 * unknown flag bits are PTG_E_INVALID.  Fills *acc (sample_next =
 * sample_begin) and zeroes `state` (ptg_accum_state_bytes bytes, DEVICE)
 * asynchronously on the context's stream. */
int ptg_accum_begin(ptg_context* ctx, const ptg_render_config* cfg,
                    uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                    uint32_t flags, uint32_t sample_begin, ptg_accum* acc, void* state /* DEVICE */);
/* Trace samples [acc->sample_next, sample_end) of the frame now uploaded and
 * add them to the state in sample order, then set acc->sample_next =
 * sample_end.  The pipeline, concurrency level, chunk size and counting mode
 * are the context's; for ptg_last_* and the timing record the call counts as
 * a ptg_render* call.  Asynchronous on the context's stream.
 * CONTRACT, not checked: the scene and the frame uploaded are the same at
 * every add of one accumulation, and `state` is the buffer of that header
 * (or a copy of its bytes).  Nothing ties a state to a frame.
 * A header with a bad magic or version, sample_end <= acc->sample_next, or
 * PTG_ACCUM_FEATURES under ptg_set_pipeline(ctx, 1) (the megakernel keeps no
 * per-sample features) is PTG_E_INVALID; a range the frame has too few
 * subframes for is ptg_render's PTG_E_RANGE.  A refused call launches nothing
 * and leaves header and state untouched.  Without PTG_ACCUM_FEATURES it runs
 * on both pipelines. */
int ptg_accum_add(ptg_context* ctx, ptg_accum* acc, void* state /* DEVICE */, uint32_t sample_end);
/* Read the state, change nothing in it, and write any subset of the five
 * outputs (at least one; DEVICE pointers, [h][w] each).
 * by_samples == 0: every sum is divided by (float)cfg.samples_per_pixel, so
 *   the outputs are the bits of ptg_render_with_features(cfg, rectangle,
 *   sample_begin, sample_next, ...) on the same frame - without
 *   PTG_ACCUM_MOMENTS, out_accum and out_bgra are ptg_render's.  No arithmetic
 *   of its own is defined.
 * by_samples != 0: the radiance and the eight feature sums are divided by
 *   (float)(sample_next - sample_begin) instead: a preview at the final
 *   brightness.  out_bgra is tonemap_pixel of the radiance written; the
 *   moments, normalised by n, are the same in both modes.
 * An empty state (sample_next == sample_begin), a bad header, out_moments
 * without PTG_ACCUM_MOMENTS, out_albedo or out_normal_depth without
 * PTG_ACCUM_FEATURES, two outputs that are the same buffer, or an output that
 * overlaps the state is PTG_E_INVALID and launches nothing.  Needs no scene.
 * Asynchronous on the context's stream. */
int ptg_accum_resolve(ptg_context* ctx, const ptg_accum* acc, const void* state /* DEVICE */, int by_samples,
                      ptg_float4* out_accum, ptg_uchar4* out_bgra, ptg_float4* out_moments,
                      ptg_float4* out_albedo, ptg_float4* out_normal_depth);

/* Work counters of the last ptg_render* call (filled only while counting is
 * on, ptg_counters_enable; counting uses a separate, slower build of the
 * kernels):
 * [0] samples, [1] node visits, [2] triangle tests, [3] BLAS entries,
 * [4] ray queries, [5] closest-hit shades, [6] TLAS node visits (part of [1]),
 * [7] walk-loop iterations of whole waves (diagnostics).  [5] counts shading
 * passes: a surface path the certified pass lists for the exact pass
 * (ptg_last_redo_stats out[0]) is counted twice. */
int ptg_counters_enable(ptg_context* ctx, int enable);
int ptg_last_counters(ptg_context* ctx, uint64_t out[8]);
/* Counters split by kernel kind (same kinds as ptg_last_kernel_times). */
int ptg_last_kernel_counters(ptg_context* ctx, uint64_t out[6][8]);
/* Wavefront walk statistics of the last counted ptg_render* call, for the
 * closest-hit walk (out[0]) and the any-hit walk (out[1]):
 * [0] node phases that loaded block rows (wave instructions of one row),
 * [1] lanes those phases served, [2] leaf phases that loaded a triangle or
 * instance record, [3] lanes they served, [4] refills that started rays,
 * [5] lanes they started, [6] walk-loop iterations, [7] lanes active in them.
 * A node phase issues 7 row loads and a leaf phase 4, each a wave
 * instruction whatever its EXEC mask: [1]/[0] and [3]/[2] are the lanes per
 * vector-memory instruction of the walk. */
int ptg_last_walk_stats(ptg_context* ctx, uint64_t out[2][8]);

/* The certified shading of the last ptg_render* call (counting builds, as
 * ptg_last_counters).  The wavefront pipeline's surface kernel evaluates
 * the path's double-precision exp / pow / sin / cos with the GPU library and
 * proves per evaluation that the float the path keeps is the one glibc's
 * double gives (device/ref_math.h, float_certain); a path with an evaluation
 * the proof does not cover is shaded again with the restated glibc
 * algorithms.  The sky kernel runs the restated glibc algorithms directly
 * and certifies nothing.  out[0]: surface paths shaded again; out[1]:
 * reserved (always 0); out[2..8]: per certificate site (acc_exp, exp_times, add_mul_pow,
 * div_mul_pow, times_cos, times_sin, times_one_minus_div_pow) the paths in
 * which it failed. */
int ptg_last_redo_stats(ptg_context* ctx, uint64_t out[9]);

/* The arithmetic environment the bit-exact results rest on: the known-answer
 * checks of ptg_device.h's ptg_device_selftest, compiled with this library's
 * own flags and run on the context's device, against this host's libm.
 * Returns the mask of failed checks (0: all passed; see ptg_device.h for the
 * bits: FP contraction, glibc exp / pow / sin / cos, tonemap, fmin's tie rule,
 * division), or a negative error code.  A nonzero mask means this host's
 * reference build would not give the bits the GPU gives (a libm other than
 * glibc 2.35's FMA variants), or the library was built with the wrong flags. */
int ptg_arith_selftest(ptg_context* ctx);

/* Per-launch device timing, measured with HIP events recorded around every
 * kernel launch on the context's stream.  Enabling (re)starts the record;
 * every ptg_render* call after that appends its launches, without blocking
 * the host, so host work (e.g. the next frame's setup) keeps overlapping the
 * GPU.  Reading the record (ptg_last_timing / ptg_last_kernel_times) waits
 * for the recorded launches, returns their summed device time and count, and
 * clears it.  ptg_last_timing sums all path-tracing kernels (all kinds but
 * accumulate). */
int ptg_timing_enable(ptg_context* ctx, int enable);
int ptg_last_timing(ptg_context* ctx, double* trace_ms, uint32_t* launches);
/* The same per kernel kind: [0] megakernel, [1] extend (closest-hit walk),
 * [2] shadow (any-hit walk), [3] shade (surface hits), [4] camera,
 * [5] accumulate, [6] sky (rays that left the scene), [7] classify. */
int ptg_last_kernel_times(ptg_context* ctx, double ms[8], uint32_t launches[8]);
/* The same record read as busy time: per kind, the UNION of the recorded
 * launches' [start, end) intervals on one device time axis (busy_ms), beside
 * their plain sum (ms) and count.  Launches of one kind that overlap (the two
 * chunk pipelines) are counted once, so busy_ms never exceeds the wall time
 * of the recorded renders.  Waits for them and clears the record. */
int ptg_last_kernel_busy(ptg_context* ctx, double busy_ms[8], double ms[8], uint32_t launches[8]);

/* Execution strategy of ptg_render*: 0 = wavefront pipeline (default:
 * camera / extend / shadow / shade kernels over compacted path queues),
 * 1 = megakernel (one work-item runs a whole path).  Both produce identical
 * bits. */
int ptg_set_pipeline(ptg_context* ctx, int pipeline);

/* Concurrency of the wavefront pipeline: 0 = every kernel on the context's
 * stream; 1 = the sky and shadow kernels on a second stream beside the walks;
 * 2 (default) = in addition two sample chunks in flight on their own stream
 * pairs, folded in sample order.  All levels produce identical bits. */
int ptg_set_concurrency(ptg_context* ctx, int level);

/* Device memory the wavefront path state may take: at most `percent` (5-70,
 * default 35) of the GPU's HBM per chunk pipeline, and never more than 85% of
 * what is free.  A smaller share means smaller sample chunks (more launches);
 * the bits do not change. */
int ptg_set_hbm_share(ptg_context* ctx, int percent);

/* Live paths per sample chunk and pipeline: at most 2^log2_paths (16-28,
 * default 27: 2^27 x 380 B = ~51 GB of path state per pipeline).  A renderer
 * that owns the GPU takes 28 with a 40% HBM share (4 chunks of 256 spp at
 * 1280x720x1024, ~71% of HBM); the bits do not change. */
int ptg_set_chunk_paths(ptg_context* ctx, int log2_paths);

/* Environment knobs read once by ptg_context_create (timing experiments;
 * no result bit depends on any of them; a malformed or out-of-range value is
 * ignored).  An embedding application that must not have its memory use or
 * launch shape changed from outside should leave them unset:
 *   PTG_CHUNK_LOG2              initial ptg_set_chunk_paths value (16-28)
 *   PTG_HBM_SHARE               initial ptg_set_hbm_share value (5-70)
 *   PTG_WALK_RESIDENT[_ANY]     closest-hit [any-hit] walk blocks resident per
 *                               CU (pads the blocks' LDS; 0-64)
 *   PTG_WALK_BLOCKS[_ANY]       closest-hit [any-hit] walk blocks launched per
 *                               CU (0-64)
 * The ptg_set_* calls after ptg_context_create override the first two. */

/* Synchronise the context's stream. */
int ptg_synchronize(ptg_context* ctx);

/* Device memory helpers for C callers without a device allocator. */
int ptg_device_alloc(ptg_context* ctx, size_t bytes, void** out);
int ptg_device_free(ptg_context* ctx, void* p);
int ptg_memcpy_d2h(ptg_context* ctx, void* dst, const void* src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTG_H */
