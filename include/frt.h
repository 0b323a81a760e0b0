/*
 * frt.h -- C-ABI of the MI355X path-tracing integrator (the drop-in boundary).
 *
 * Replaces, for one GPU, the work the reference enqueues in
 *   path::Render(Scene*, viewer*, tf::Taskflow&)         first_ray/path.cpp:118-148
 *   path::Li(ray, Scene*, depth, prev_hrec, pdf, sampler) first_ray/path.cpp:4-116
 * as driven by renderer<path>::Render                    first_ray/integrator.h:14-46
 * and writes the film that viewer::add_sample fills       first_ray/viewer.cpp:109-132.
 *
 * The caller flattens its Scene (Scene.h:10-26) once into an frt_scene_view
 * (plain host arrays, fp64 like the reference's Vector3f), uploads it, and
 * renders tiles of the frame.  No torch / HIP C++ types cross this boundary;
 * a hip stream is passed as an opaque pointer.  See INTEGRATION.md for the
 * reference-side `path_gpu` binding.
 *
 * Errors: every call returns 0 on success or a negative FRT_E* code;
 * frt_last_error(ctx) describes the last failure (the reference throws
 * std::runtime_error, e.g. triangle.cpp:34, image.h:102; the C++ host
 * wrapper include/frt_integrator.hpp converts codes back into exceptions).
 */
#ifndef FRT_H
#define FRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRT_ABI_VERSION 9

enum {
    FRT_OK = 0,
    FRT_E_INVALID = -1,      /* bad argument / malformed scene view        */
    FRT_E_HIP = -2,          /* HIP runtime failure (message in last_error) */
    FRT_E_NO_SCENE = -3,     /* frt_render before frt_upload_scene          */
    FRT_E_UNSUPPORTED = -4,  /* material/feature outside the hot path       */
    FRT_E_IO = -5,           /* file could not be read / written            */
    FRT_E_NO_DEVICE = -6     /* no gfx950 device / bad device index         */
};

enum { FRT_WORLD_BVH = 0, FRT_WORLD_LIST = 1 };          /* parallel_bvh_node | hitable_list */
enum { FRT_MAT_LAMBERTIAN = 0,      /* material.h:50-73                                  */
       FRT_MAT_DIFFUSE_LIGHT = 1,   /* material.h:179-192                                */
       FRT_MAT_MODIFIED_PHONG = 2,  /* material.h:75-108 + cosine_power_pdf (pdf.h:99)   */
       FRT_MAT_METAL = 3,           /* material.h:110-130 + constant_pdf (pdf.h:186)     */
       FRT_MAT_DIELECTRIC = 4,      /* material.h:133-177 + dielectric_pdf (pdf.h:138)   */
       FRT_MAT_ROUGH_CONDUCTOR = 5 };/* material.h:246-315 + roughconductor_pdf (pdf.h:231) */
enum { FRT_DIST_GGX = 0, FRT_DIST_BECKMANN = 1 };   /* microfacet_distributions (util.h:48-52) */
enum { FRT_INTEGRATOR_PATH = 0,     /* path::Li           path.h:8-18, path.cpp:4-116      */
       FRT_INTEGRATOR_PSSMLT = 1,   /* pssmlt             pssmlt.h:29-76                   */
       FRT_INTEGRATOR_AO = 2,       /* ao::Li             ao.h:8-43, ao.cpp:4-27           */
       FRT_INTEGRATOR_NORMALS = 3,  /* normals_renderer   debug_renderer.h:6-50            */
       FRT_INTEGRATOR_ALBEDO = 4,   /* first-hit reflectance (below)                       */
       FRT_INTEGRATOR_DEPTH = 5,    /* first-hit distance and coverage (below)             */
       FRT_INTEGRATOR_DENOISE = 6,  /* feature-guided filter of a finished film (below)    */
       /* 7: not assigned, FRT_E_INVALID */
       FRT_INTEGRATOR_ERROR = 8     /* variance film of the context's last render (below)  */ };
/* FRT_INTEGRATOR_ALBEDO (not in the reference): the auxiliary image a compositor or
 *   an external denoiser expects beside a low-sample render.  The film is the mean
 *   over the pixel's samples of the reflectance colour at the camera ray's hit:
 *   lambertian albedo (its checker or image texture applied at the hit, as path
 *   sees it); modified_phong min(1, diffuse_reflectance (textured) + specular) per
 *   channel; metal albedo; dielectric and rough_conductor specular (textured);
 *   (1, 1, 1) on a diffuse_light and on a miss -- emitted and environment radiance
 *   is not reflectance, and dividing by 1 leaves it alone.  Every value is in
 *   [0, 1] for materials whose colours are.
 * FRT_INTEGRATOR_DEPTH (not in the reference): per sample, t = the Euclidean
 *   distance from the ray's origin (the lens point) to the hit; the film is
 *   (mean of t hit, mean of t^2 hit, mean of hit) with hit = 1 / 0 -- mean depth
 *   times coverage, its second moment, and coverage (alpha).  A miss adds
 *   (0, 0, 0); coverage is exactly 1.0f where every sample hit, and the stored
 *   floats keep y k >= x^2, so a variance taken from one film is never negative.
 * Both: camera samples are path's (film and lens dimensions of the hash stream),
 *   one camera ray a sample, no other ray; stats as normals.  They run in fp32
 *   on the plans of normals, with sample_offset, shards, frt_render_multi and
 *   every plan flag.  FRT_FLAG_FP64, _ENV_SAMPLING, _ROULETTE and _SOBOL have no
 *   effect, max_depth is ignored, and neither reads the environment: a context
 *   with an environment image runs the same kernels and gives the same film.
 * FRT_INTEGRATOR_DENOISE: the film argument is input and output, the colour of
 *   the whole frame (from path with any flags, accumulated progressive passes or
 *   pssmlt): frt_render reads it in pixel order, frt_render_device in slot order
 *   (padding slots stay as they are).  The call renders the normals, albedo and
 *   depth films of the uploaded scene with spp samples each -- seed,
 *   sample_offset, tile_size and the plan flags as given, bit-identical to the
 *   public renders with the same parameters --, runs an edge-avoiding a-trous
 *   wavelet filter (Dammertz et al. 2010; weights and constants: DESIGN.md
 *   "Denoiser", csrc/frt_denoise.hpp) over the colour divided by the albedo,
 *   multiplies the albedo back and writes the result over the film.
 *   Ignored: max_depth, FRT_FLAG_ENV_SAMPLING / _ROULETTE / _SOBOL / _FP64.
 *   Refused with FRT_E_INVALID and a text in frt_last_error: shard_count != 1
 *   (the stencil crosses tiles); for frt_render a film value that is negative,
 *   NaN or infinite, before any GPU work (frt_render_device does not look at
 *   the contents); the per-pixel hooks frt_selftest_path_host[_env].
 *   frt_render_multi runs the whole call on ctxs[0].  frt_stats: the sums of the
 *   three feature passes, kernel_ms with the filter kernels, the plan fields of
 *   the albedo pass.
 * FRT_INTEGRATOR_ERROR (not in the reference): the per-pixel error estimate of the
 *   film that this context's last successful render produced.  frt_render,
 *   frt_render_device and frt_render_multi trace no ray: they reduce the partial
 *   sums that render left on the device.  A render of kind path, ao, normals,
 *   albedo or depth leaves them, on any plan, with any flags, in fp32 or fp64 (the
 *   sums are fp32 in both).  It cut the samples of a pixel into K disjoint chunks
 *   (samples_per_item samples each, the last one what is left; 0 = the library's
 *   choice); with chunk c holding n_c samples with sum S_c, N = sum n_c,
 *   m_c = S_c / n_c and m = sum S_c / N, the film is, per pixel and channel,
 *       V = sum_c n_c (m_c - m)^2 / ((K - 1) N),
 *   the batch-means estimate: for independent samples the unbiased estimate of
 *   the variance of the pixel's mean, its square root the standard error.  fp32,
 *   one pass, West's weighted incremental update (csrc/frt_error.hpp); every value
 *   is finite and >= 0, and exactly 0 where all chunk means are bit-equal.
 *   frt_render scatters V into pixel order (only this shard's pixels are written);
 *   frt_render_device writes slot order, padding slots exactly 0.
 *   nx, ny, spp, tile_size, shard_index and shard_count must equal the recorded
 *   render's; every other field is ignored.  frt_render_multi hands shard (i, n)
 *   to ctxs[i] as it does for renders, and each context reduces its own shard:
 *   call it with the contexts, in the order, of the render.
 *   Refused with FRT_E_INVALID and a text in frt_last_error: no recorded render,
 *   or other parameters; a recorded render with K = 1 (render with
 *   samples_per_item < spp); the per-pixel hooks frt_selftest_path_host[_env].
 *   The record: a pssmlt render, a DENOISE call and any render call that fails
 *   or is refused (one refused for a null pointer aside) clear it -- they reuse or
 *   do not fill the sums --; frt_upload_scene, frt_set_env_image and
 *   frt_trace_device do not; an ERROR call leaves it, so calls repeat bit for bit.
 *   frt_stats: the ray counters, samples and work_items 0, pixels as for a render,
 *   kernel_ms the reduce kernel's time.
 *   FRT_FLAG_SOBOL: the call is accepted when the recorded render used the flag,
 *   but the samples of a pixel are then one stratified net and not independent
 *   draws: V estimates the variance of the unstratified estimator, an upper
 *   estimate of the true error (render_until, include/frt_integrator.hpp, takes
 *   its error from independent replicates in that case).
 *   frt_shard_slot_count / frt_shard_slots: the geometry of path. */
enum { FRT_FLAG_NO_LDS_SCENE = 1,      /* render_params.flags: keep small scenes in HBM/L2 (A/B timing)  */
       FRT_FLAG_WAVES5 = 2,            /* register cap for 5 waves/SIMD (A/B timing)                     */
       FRT_FLAG_WAVES6 = 4,            /* register cap for 6 waves/SIMD (A/B timing)                     */
       FRT_FLAG_WAVES4 = 8,            /* the compiler's own allocation, ~4 waves/SIMD (A/B timing)      */
       FRT_FLAG_BVH2 = 16,             /* binary nodes for HBM-resident scenes (A/B timing, self-test)   */
       /* 32, 64, 128: retired A/B plans (4-wide nodes from LDS, lockstep brute force,
          speculative traversal), measured slower and removed in round 4; FRT_E_INVALID since round 5 */
       FRT_FLAG_NO_OCT = 256,          /* LDS binary plan without the per-octant node copies (A/B timing) */
       FRT_FLAG_FP64 = 512,            /* path: the fp64 kernel for this call (self-test: fp64 host replay) */
       FRT_FLAG_FP32 = 1024,           /* path: the fp32 kernels even where the precision picks fp64      */
       FRT_FLAG_ENV_SAMPLING = 2048,   /* path: next-event estimation toward the environment image, MIS with the bsdf sample */
       FRT_FLAG_ROULETTE = 4096,       /* path: Russian roulette from the fourth vertex on (below)        */
       FRT_FLAG_SOBOL = 8192 };        /* path: Owen-scrambled Sobol' sample points (below)               */

/* FRT_FLAG_ENV_SAMPLING (frt_render, frt_render_device, frt_render_multi and
 * frt_selftest_path_host_env; fp32 and fp64).  Not the reference's estimator --
 * its environment_map is only evaluated where a bsdf-sampled ray leaves the
 * scene -- but one with the same expectation and far less noise under images
 * that hold most of their energy in a few texels (a sun, a window).
 *   path, the context (or the replay call) holds an image: texels are drawn
 *     with probability proportional to Rec.709 luminance x the texel's solid
 *     angle, from tables built once per image on the host (at the first such
 *     render, kept until frt_set_env_image changes or clears the image).  At a
 *     lambertian or rough conductor vertex the image is sampled instead of an
 *     area light: always when the scene has no lights, else with probability
 *     1/2 (the light-pick sample decides; its remainder feeds the reference's
 *     pick and the area-light term is doubled).  One shadow ray per vertex as
 *     before, counted in shadow_rays; the sample and the bsdf-sampled ray that
 *     leaves the scene are combined with the power heuristic, as area lights
 *     are.  A lambertian vertex takes nothing from below its shading normal.
 *     Other vertices (modified_phong, metal, dielectric) are unchanged, and so
 *     is the environment seen by the camera or after them.
 *     The A/B register-cap flags (FRT_FLAG_WAVES4/5/6) do not apply: these
 *     kernels have one cap per plan.
 *   no image (constant env_color), or an image without luminance: no effect,
 *     the film is that of the same call without the flag.
 *   ao, normals: no effect.
 *   pssmlt: FRT_E_INVALID with a text in frt_last_error (its primary-sample
 *     layout is the reference's). */

/* FRT_FLAG_ROULETTE (frt_render, frt_render_device, frt_render_multi and
 * frt_selftest_path_host[_env]; fp32 and fp64).  Not in the reference, whose
 * path::Li follows every path until a light, the environment or max_depth ends
 * it; the estimator has the same expectation and traces fewer rays per sample.
 *   path: a scattering vertex at depth >= 3 (the camera ray's hit is depth 0;
 *     the first three vertices never play -- the constant kRouletteDepth of
 *     csrc/frt_path.hpp, not a parameter) lets the path go on with probability
 *     q = min(1, largest component of the throughput the next ray would carry)
 *     and divides that throughput by q; q == 1 changes nothing.  The decision
 *     reads one random number of its own per vertex (RNG dimension 4 + 8 depth
 *     + 2), so every other sample of the path is the one
 *     the same call draws without the flag.  A path that stops still traces the
 *     vertex's shadow ray and keeps its next-event term.  A zero bsdf pdf ends
 *     the path as before.  The MIS weights, next-event estimation and max_depth
 *     are unchanged; with max_depth <= 2 the film and the counters are those of
 *     the call without the flag.
 *     Works with constant environments, environment images and
 *     FRT_FLAG_ENV_SAMPLING, on every plan, with sample_offset and shards.
 *     The A/B register-cap flags (FRT_FLAG_WAVES4/5/6) do not apply: these
 *     kernels have one cap per plan.
 *   ao, normals: no effect, the film is that of the same call without the flag.
 *   pssmlt: FRT_E_INVALID with a text in frt_last_error (its primary-sample
 *     layout is the reference's). */

/* FRT_FLAG_SOBOL (frt_render, frt_render_device, frt_render_multi and
 * frt_selftest_path_host[_env]; fp32 and fp64).  Not in the reference, whose
 * samplers draw every dimension independently; the estimator and its
 * expectation are unchanged, only the sample points are.
 *   path: dimension d of the sample with global index s (sample_offset + the
 *     local index) of a pixel is component d & 1 of a 2-D Owen-scrambled Sobol'
 *     point: the point with index s of pair d >> 1, pairs padded in the manner
 *     of Burley 2020 -- each pair the first two Sobol' dimensions with its own
 *     shuffle of the index and its own two scrambles, hashed from (seed, pixel,
 *     pair); the exact construction is DESIGN.md section 4.  The dimension
 *     layout is the one without the flag, so film position, lens, light point,
 *     image texel and bsdf direction are each one stratified pair, and roulette
 *     and light pick share one.  Any 2^m consecutive samples of a pixel that
 *     start at a multiple of 2^m are a (0, m, 2)-net in every pair: progressive
 *     passes (sample_offset) of power-of-two length keep the property, and k
 *     passes of n samples are the one call of k n samples.  Different seeds give
 *     independent scrambles, so averages over seeds keep their standard error.
 *     Works with FRT_FLAG_ROULETTE, constant environments, environment images
 *     and FRT_FLAG_ENV_SAMPLING, on every plan, with sample_offset and shards.
 *     The A/B register-cap flags (FRT_FLAG_WAVES4/5/6) do not apply: these
 *     kernels have one cap per plan.
 *   ao, normals: no effect, the film is that of the same call without the flag.
 *   pssmlt: FRT_E_INVALID with a text in frt_last_error (its primary samples
 *     are the hash stream's, mutated as the reference does). */

/* Kernel precision (frt_set_precision).  The reference computes in fp64
 * (geometry.h:351).  FRT_PRECISION_AUTO: fp64 for list worlds (hitable_list,
 * e.g. veach_mis: a few primitives, and lights small enough -- r = 0.033 --
 * that fp32 rounding moves samples onto or off them), fp32 for BVH worlds.
 * FRT_PRECISION_FP64: every path render in fp64 (the binary tree from HBM:
 * the debugging build SURVEY 8(a) names).  FRT_PRECISION_FP32: fp32 only.
 * AO, normals and PSS-MLT always run in fp32. */
enum { FRT_PRECISION_AUTO = 0, FRT_PRECISION_FP32 = 1, FRT_PRECISION_FP64 = 2 };

/* primitive reference: triangle t -> t ; sphere k -> FRT_PRIM_SPHERE | k */
#define FRT_PRIM_SPHERE (1 << 30)

typedef struct frt_material {
    int32_t type;            /* FRT_MAT_*                                                 */
    int32_t distribution;    /* rough_conductor: FRT_DIST_GGX / FRT_DIST_BECKMANN         */
    double albedo[3];        /* lambertian albedo / modified_phong diffuse_reflectance /
                                metal albedo                                              */
    double emit[3];          /* diffuse_light: constant_texture colour                    */
    double specular[3];      /* modified_phong / dielectric / rough_conductor:
                                specular_reflectance (constant texture)                   */
    double exponent;         /* modified_phong: specular_exponent                         */
    double ior;              /* dielectric: ref_idx                                       */
    double alpha;            /* rough_conductor: roughness (alphaU = alphaV)              */
    double eta[3], k[3];     /* rough_conductor: complex IOR (fresnelConductorExact)      */
    /* The material's texture (lambertian albedo, modified_phong diffuse_reflectance,
     * dielectric / rough_conductor specular_reflectance): FRT_TEX_CONSTANT uses the
     * colour field above; FRT_TEX_CHECKER (checker_texture, texture.h:30-49) of two
     * constants -- that field as tex0 and tex_odd as tex1 -- at u_scale, v_scale,
     * looked up at the hit's uv (sphere: get_sphere_uv, hitable.h:15-21; triangle:
     * interpolated OBJ vt, triangle.h:105-107).  FRT_TEX_IMAGE (image_texture,
     * texture.h:51-95): the scene view's image `image`, nearest texel at (u nx, v ny)
     * with the reference's wrap / clamp. */
    int32_t texture;
    int32_t image;           /* FRT_TEX_IMAGE: index into frt_scene_view.images      */
    double tex_odd[3];
    double tex_scale[2];
} frt_material;
enum { FRT_TEX_CONSTANT = 0, FRT_TEX_CHECKER = 1, FRT_TEX_IMAGE = 2 };

/* A decoded image for image_texture (texture.h:51-95; the reference's `image`,
 * image.h, as stb_image returns it: rows top to bottom, 3 channels).
 * FRT_IMAGE_SRGB8: nx*ny*3 bytes, the texel is FromSrgb(byte / 255) (util.h:62-66);
 * FRT_IMAGE_F32: nx*ny*3 floats used as they are (the STBI_HDR branch). */
enum { FRT_IMAGE_SRGB8 = 0, FRT_IMAGE_F32 = 1 };
typedef struct frt_image {
    int32_t nx, ny;
    int32_t format;          /* FRT_IMAGE_*                                               */
    int32_t reserved;
    const void *data;
} frt_image;

typedef struct frt_scene_view {
    int32_t world_kind;                 /* FRT_WORLD_BVH or FRT_WORLD_LIST              */
    /* triangles (triangle.h:55-66, one entry per `triangle` object) */
    int32_t n_tris;
    const double *tri_v;                /* 9 per tri: v0, v1, v2                        */
    const double *tri_n;                /* 9 per tri: vertex normals, or NULL           */
    const int32_t *tri_material;        /* index into materials                         */
    const uint8_t *tri_geometry_normal; /* use_geometry_normals per tri, NULL = all 1   */
    const double *tri_inv_area;         /* 1/(0.5|e1 x e2| nTriangles_of_mesh)           */
    /* spheres (sphere.h:8-24) */
    int32_t n_spheres;
    const double *sphere;               /* 4 per sphere: centre, radius                 */
    const int32_t *sphere_material;
    /* materials */
    int32_t n_materials;
    const frt_material *materials;
    /* BVH world: the parallel_bvh_node tree (parallel_bvh.h:8-27) */
    int32_t n_nodes;
    int32_t root;                       /* node index, or ~prim_ref for a 1-prim world  */
    const double *node_box;             /* 6 per node: min, max                         */
    const int32_t *node_child;          /* 2 per node: left, right; >=0 node, <0 ~prim  */
    /* list world (hitable_list, hitable_list.cpp:4-21) */
    int32_t n_list;
    const int32_t *list;                /* prim refs in list order                      */
    /* Scene::lights (hitable_list of emitters) */
    int32_t n_lights;
    const int32_t *lights;              /* prim refs                                    */
    /* camera (camera.h:10-28), already constructed */
    double cam_origin[3], cam_lower_left[3], cam_horizontal[3], cam_vertical[3];
    double cam_u[3], cam_v[3];
    double cam_lens_radius;
    /* environment_map with a constant texture (material.h:206-232) */
    double env_color[3];
    /* camera w axis and half_height (camera.h:18-26): PSS-MLT's screen mapping
     * (pssmlt.cpp:134-138) needs them; half_height = 256 / camera::dist */
    double cam_w[3];
    double cam_half_height;
    /* texture coordinates: 6 per tri (uv of v0, v1, v2, the OBJ's vt), or NULL = 0 */
    const double *tri_uv;
    /* images of FRT_TEX_IMAGE materials (ABI 7) */
    int32_t n_images;
    const frt_image *images;
} frt_scene_view;

typedef struct frt_render_params {
    int32_t nx, ny;          /* film size (viewer nx, ny); nx * ny <= 2^31 - 1 (int32 pixel
                              * indices), larger frames fail with FRT_E_INVALID             */
    int32_t spp;             /* samples per pixel (viewer ns)                              */
    uint32_t seed;           /* frame seed of the counter RNG (DESIGN.md "RNG stream spec") */
    int32_t max_depth;       /* scatter while depth <= max_depth; reference: 33 (path.cpp:36) */
    int32_t integrator;      /* FRT_INTEGRATOR_*                                           */
    int32_t tile_size;       /* square tiles, multiple of 8; 0 = 32                        */
    int32_t shard_index;     /* this call renders tiles t with t % shard_count == index    */
    int32_t shard_count;     /* 1 = whole frame                                            */
    int32_t samples_per_item;/* work granule in samples; 0 = automatic                     */
    int32_t flags;           /* FRT_FLAG_* bits, 0 = defaults                              */
    /* PSS-MLT only: spp = mutations per pixel (total = spp*nx*ny, the reference's
     * ns), split over mlt_chains chains (chain c runs in shard c % shard_count);
     * mlt_bootstrap = paths for the normaliser b (pssmlt.h:12 N_Init = 10000). */
    int32_t mlt_chains;
    int32_t mlt_bootstrap;
    /* progressive rendering (path / AO / normals): this call renders samples
     * [sample_offset, sample_offset + spp) of every pixel -- the RNG streams
     * are keyed by the global sample index, so passes of 64 + 64 + ... samples
     * average to the film of one call with their total (frt_film_accumulate). */
    int32_t sample_offset;
} frt_render_params;

typedef struct frt_stats {
    uint64_t camera_rays;    /* top-level scene queries, path.cpp:10 at depth 0 */
    uint64_t extension_rays; /* path.cpp:10 at depth > 0                        */
    uint64_t shadow_rays;    /* path.cpp:50                                     */
    uint64_t samples;
    uint64_t pixels;
    uint64_t work_items;
    double kernel_ms;        /* path megakernel, HIP events on its stream       */
    double total_ms;         /* whole call                                      */
    /* launch configuration of the megakernel (measurement reporting) */
    uint32_t scene_in_lds;   /* 1: nodes/triangles/materials were read from LDS */
    uint32_t waves_cap;      /* register cap in waves/SIMD, 0 = compiler's own  */
    uint32_t stack_entries;  /* per-lane LDS traversal stack                    */
    uint32_t bvh_depth;      /* levels of the device BVH (after leaf collapse)  */
    uint64_t scene_bytes;    /* scene bytes the plan reads: its LDS copy when   */
                             /* scene_in_lds (the octant node copies on that    */
                             /* plan), else nodes + triangles + shading records */
                             /* + materials in HBM                              */
    uint32_t fp64;           /* 1: the fp64 kernel ran (ABI 8)                  */
    uint32_t reserved;
} frt_stats;

int frt_get_abi_version(void);

/* ---- context: one per GPU, not thread-safe ---- */
typedef struct frt_ctx frt_ctx;
int frt_create(int hip_device, frt_ctx **out);
int frt_destroy(frt_ctx *ctx);
const char *frt_last_error(const frt_ctx *ctx);
/* FRT_PRECISION_*; read by the next frt_upload_scene (fp64 records are
 * uploaded only when the precision can select the fp64 kernels for that
 * scene) and by every render.  Default FRT_PRECISION_AUTO. */
int frt_set_precision(frt_ctx *ctx, int precision);

/* Scene::env_map as environment_map(image_texture) (material.h:206-244): on a
 * miss every integrator returns the image's nearest texel in the ray's direction
 * d = normalize(rd): phi = atan2(d.x, -d.z) (+ 2 pi when negative), theta =
 * acos(d.y), (u, v) = (phi / 2 pi, theta / pi), then image_texture's index rule
 * (row 0 = +y pole; FRT_IMAGE_SRGB8 or FRT_IMAGE_F32, converted as scene
 * textures are).  The fp32 kernels clamp d.y to [-1, 1] first (normalize can
 * leave it an ulp outside, where acosf is NaN); the fp64 kernels do not.
 * State of the context like frt_set_precision: the texels are copied to the
 * device during the call, kept across frt_upload_scene and read by every later
 * render; NULL = back to the constant env_color of the uploaded view.  A context
 * with an image renders with the kernels compiled for textures, every other
 * context with the ones it used before.  FRT_E_INVALID (text in frt_last_error)
 * for nx / ny <= 0, null data, an unknown format and for a negative or
 * non-finite texel (PSS-MLT's splats need contributions >= 0).
 * frt_render_multi: set the same image on every context; contexts that
 * disagree fail with FRT_E_INVALID. */
int frt_set_env_image(frt_ctx *ctx, const frt_image *img);

/* Copy the scene to HBM (fp32 device layout, DESIGN.md "Data layout").  The
 * view's arrays are only read during the call. */
int frt_upload_scene(frt_ctx *ctx, const frt_scene_view *scene);

/* Shard geometry: number of output slots of a shard (tiles * tile_size^2) and,
 * per slot, the linear film index y*nx+x it holds (or -1 for padding). */
int64_t frt_shard_slot_count(const frt_render_params *p);
int frt_shard_slots(const frt_render_params *p, int32_t *slot_pixel);

/* Render this shard.  `film_rgb` is the caller's full film (nx*ny*3 floats,
 * index (y*nx+x)*3, y = 0 bottom row, as viewer::fout_image); only this
 * shard's pixels are written, with the mean radiance (viewer.cpp:111).
 * PSS-MLT: every chain splats anywhere, so the shard's splat film is ADDED to
 * film_rgb (zero it first; summing all shards gives the image,
 * AccumulatePathContribution pssmlt.cpp:19-38). */
int frt_render(frt_ctx *ctx, const frt_render_params *p, float *film_rgb, frt_stats *st);

/* One process, n GPUs: ctxs[i] (each with the scene uploaded) renders shard
 * (i, n) of the whole-frame request `p` (shard_index 0, shard_count 1) on its
 * own host thread; the full film lands in film_rgb (PSS-MLT: the shard films
 * summed in order 0..n-1, added to film_rgb).  Replaces the multi-worker
 * path::Render task graph (path.cpp:118-148) across devices. */
int frt_render_multi(frt_ctx **ctxs, int n, const frt_render_params *p, float *film_rgb, frt_stats *st);

/* Device variant: writes the shard's slots (frt_shard_slot_count * 3 floats,
 * slot order) into device memory `slots_rgb` on `hip_stream` (NULL = the
 * context's stream) and returns after the work has completed.  PSS-MLT: the
 * slots are the whole film (nx*ny, natural order) holding this shard's splats;
 * shards are combined with a sum (RCCL reduce / all-reduce). */
int frt_render_device(frt_ctx *ctx, const frt_render_params *p, float *slots_rgb, void *hip_stream,
                      frt_stats *st);

/* PSS-MLT chain states of this context's last PSS-MLT render (parity tests and
 * diagnostics; pssmlt.cpp:301-365 keeps them in TMarkovChain): its local chains
 * [first, first + n), local chain j = global chain shard_index + j *
 * shard_count.  u_out (n x 92 floats, or NULL): the chain's final primary
 * samples; fp_out (n x 2, or NULL): its trajectory fingerprint = (accepted
 * proposals, sum of the accepted mutations' 1-based step indices mod 2^32).
 * FRT_E_INVALID when the last render of the context was not PSS-MLT or the
 * range is outside its chains. */
int frt_mlt_chain_state(frt_ctx *ctx, uint64_t first, uint64_t n, float *u_out, uint32_t *fp_out);

/* Ray queries on the uploaded scene: Scene::world->hit (path.cpp:10, 50;
 * parallel_bvh_node::hit parallel_bvh.h:39-64, hitable_list::hit
 * hitable_list.cpp:4-21) for a batch of rays, with the world's own t_min
 * (EPSILON * max(1, |o|) for a BVH, EPSILON for a list).  Device memory:
 * rays = n x 8 floats (origin xyz, t_max, direction xyz, flags: bit 0 = any
 * hit, the shadow query of path.cpp:50), hits = n x 4 floats (t, u, v, prim
 * as int32 bits: the scene view's triangle index or FRT_PRIM_SPHERE | k, -1 =
 * miss; a miss leaves t = t_max).  flags: FRT_FLAG_NO_LDS_SCENE / _BVH2 /
 * _NO_OCT choose the plan as for frt_render.  Returns after the work has
 * completed on `hip_stream` (NULL = the context's stream); st: kernel_ms,
 * camera_rays = n, and the plan that ran (scene_in_lds, waves_cap,
 * stack_entries -- 0 for a list world --, bvh_depth, scene_bytes).
 * What a tree plan answers: for origins inside the scene's root box or at
 * camera distance from it, the closest hit of the list of the same primitives,
 * bit for bit in t (and in u, v with the same primitive; primitives at one t
 * tie by DFS order, not list order), except below the BVH's own t_min.  That
 * is tested inside the box and at the shipped cameras.  It is not guaranteed
 * beyond: the slab test's rounding grows with |origin|, so from far away hits
 * near silhouettes and edges can be lost, at a rate that grows with |origin| /
 * scene extent (measured: none of 20,000 rays at 50 scene
 * sizes, 0.3 to 3 % of the rays aimed at exact vertices at 500).
 * The ray queue has its own word in the context, apart from the render's, but
 * a context is still one stream's worth of state: calls on one context are
 * issued from one host thread, one at a time (each returns when its work is
 * done).  n plus a chunk of 256 rays per resident wave must stay below 2^32.
 * Input domain: finite origins, directions and t_max, directions not zero,
 * and |origin| and the scene's coordinates below 1e8 on every axis.  (A
 * direction component below 1e-30 is nudged to +-1e-30 for the slab test;
 * with both an origin and a box plane beyond ~3.4e8 on that axis the slab
 * distances would be inf - inf = NaN, and the NaN-propagating min / max of
 * the box test would then cull the box.)  The rays a render makes stay inside
 * this domain for every scene the reference builds. */
int frt_trace_device(frt_ctx *ctx, const float *rays, int64_t n, float *hits, int flags, void *hip_stream,
                     frt_stats *st);

/* ---- host-side scene pipeline (native C++; what main.cpp + mesh_loader +
 *      parallel_bvh_node::create_bvh do in the reference) ---- */
typedef struct frt_host_scene frt_host_scene;
typedef struct frt_host_scene_info {
    int32_t n_tris, n_spheres, n_materials, n_lights, n_nodes, world_kind, n_list, bvh_depth;
    double load_ms, build_ms;
} frt_host_scene_info;
/* kind: "cornell_box_obj" (main.cpp:222-252), "veach_mis" (main.cpp:281-314),
 *       "obj_geo" / "obj_smooth" (any OBJ, cornell camera, geometric / vertex normals)
 * FRT_E_IO: unreadable file.  FRT_E_INVALID, and no scene: unknown kind, or a face of
 * the file with a vertex or normal index that is no number, 0, outside [1, count]
 * (negative: below -count) or not representable -- the reference's importer fails on
 * such a file.  A texture index that is missing or out of range only means no uv for
 * its mesh. */
int frt_scene_create(const char *kind, const char *obj_path, double aspect, frt_host_scene **out);
int frt_scene_view_get(const frt_host_scene *s, frt_scene_view *view);

/* Incremental construction, what main.cpp's scene functions do (e.g.
 * veach_ajar main.cpp:318-412, glass_of_water :414-480): OBJ files through
 * create_triangle_mesh(file, toWorld, bsdf, lights, use_geometry_normals)
 * (triangle.cpp:26-60), spheres, the camera, then parallel_bvh_node::create_bvh
 * or a hitable_list over the world prims in insertion order.
 *   frt_scene_new -> frt_scene_add_obj / _add_sphere ... -> frt_scene_set_camera
 *   -> frt_scene_finish -> frt_scene_view_get
 * add_obj: to_world16 = row-major Matrix4x4 or NULL (identity); bsdf = the one
 * material every mesh of the file takes, or NULL for the file's MTL materials
 * (mesh_loader.cpp:59-112); meshes whose material is a diffuse_light join
 * Scene::lights.  Returns FRT_E_IO (unreadable file) or FRT_E_INVALID (singular
 * matrix, bad material, a face index the file does not have: frt_scene_create's
 * rule); a refused file adds nothing, the scene is what it was before the call. */
enum { FRT_SPHERE_WORLD = 1, FRT_SPHERE_LIGHTS = 2, FRT_SPHERE_BOTH = 3 };
int frt_scene_new(frt_host_scene **out);
int frt_scene_add_obj(frt_host_scene *s, const char *obj_path, const double *to_world16, const frt_material *bsdf,
                      int use_geometry_normals);
/* where: FRT_SPHERE_WORLD (the world list), FRT_SPHERE_LIGHTS (a separate
 * Scene::lights object, as veach_mis main.cpp:298-302 does), or both (one object) */
int frt_scene_add_sphere(frt_host_scene *s, const double *center, double radius, const frt_material *m, int where);
/* camera.h:10-28; the reference constructs every scene's camera this way */
int frt_scene_set_camera(frt_host_scene *s, const double *lookfrom, const double *lookat, const double *vup,
                         double vfov, double aspect, double aperture, double focus_dist);
/* environment_map with a constant texture (material.h:206-232) */
int frt_scene_set_env(frt_host_scene *s, const double *rgb);
/* a decoded image (copied) for FRT_TEX_IMAGE materials; *index = its frt_material.image */
int frt_scene_add_image(frt_host_scene *s, const frt_image *img, int *index);
/* image `index` (frt_scene_add_image) is the scene's environment; -1 = the
 * constant of frt_scene_set_env.  The scene view has no field for it (ABI 9):
 * frt_scene_env_image gives the image to hand to frt_set_env_image: the scene's
 * copy, valid until the scene is destroyed; it returns 1 with *out
 * filled, or 0 and leaves *out alone when there is none. */
int frt_scene_set_env_image(frt_host_scene *s, int index);
int frt_scene_env_image(const frt_host_scene *s, frt_image *out);
/* world_kind FRT_WORLD_BVH (create_bvh) or FRT_WORLD_LIST */
int frt_scene_finish(frt_host_scene *s, int world_kind);
/* GPU BVH builders: replace the finished scene's world
 * (BVH or list) with a BVH over the same world prims built on ctx's device
 * (csrc/frt_lbvh.hip), in place of parallel_bvh_node::create_bvh's SAH sweep:
 *   FRT_GPU_BVH_PLOC  Morton codes, radix sort, then PLOC clustering (mutual
 *                     nearest neighbours by union surface area within 16
 *                     clusters in Morton order);
 *   FRT_GPU_BVH_LBVH  Morton codes, radix sort, Karras hierarchy, atomic refit;
 *   FRT_GPU_BVH_SAH   top-down binned SAH, one tree level per launch, one
 *                     workgroup per node (32 centroid bins per axis in LDS,
 *                     cost N_L A_L + N_R A_R: frt_scene_build_bvh_sah's rule).
 * frt_scene_build_bvh_gpu = the binned SAH builder.  Finish with FRT_WORLD_LIST to
 * skip the host build.  The topology differs from the reference's, so exact-t
 * ties between primitives may resolve differently.  device_ms (optional) =
 * device time of the build passes. */
enum { FRT_GPU_BVH_PLOC = 0, FRT_GPU_BVH_LBVH = 1, FRT_GPU_BVH_SAH = 2 };
int frt_scene_build_bvh_gpu(frt_host_scene *s, frt_ctx *ctx, double *device_ms);
int frt_scene_build_bvh_gpu_algo(frt_host_scene *s, frt_ctx *ctx, int algo, double *device_ms);
/* Binned SAH tree (32 centroid bins per axis, host threads) over the same
 * world prims: better traversal than the reference's sweep on large meshes
 * (same tie caveat as the GPU tree). */
int frt_scene_build_bvh_sah(frt_host_scene *s);
int frt_scene_info(const frt_host_scene *s, frt_host_scene_info *info);
void frt_scene_destroy(frt_host_scene *s);

/* cornell_1m generator: every non-emissive quad of `src_obj` bilinearly
 * tessellated into k x k cells, written as OBJ + MTL.
 * FRT_E_IO: a file cannot be read or written.  FRT_E_INVALID: k < 1, or a face
 * with a vertex index that frt_scene_create refuses (a token that is no number
 * included); what dst_obj then holds is unspecified.  A face keeps its first 64
 * corners, as in the importer. */
int frt_write_tessellated_obj(const char *src_obj, int k, const char *dst_obj);

/* Radiance RGBE (.hdr) reader: what stbi_loadf gives the reference's
 * image(file, STBI_HDR) (image.cpp:16): rows top to bottom, 3 floats per texel,
 * value = mantissa * 2^(e - 136), e == 0 -> 0; flat and new-style RLE scanlines,
 * "-Y h +X w" orientation only (anything else: FRT_E_UNSUPPORTED).  rgb == NULL:
 * sizes only; otherwise nx * ny * 3 floats.  FRT_E_IO: unreadable or truncated
 * file; FRT_E_INVALID: not a Radiance file, bad header or bad scanline data. */
int frt_read_hdr(const char *path, int32_t *nx, int32_t *ny, float *rgb);

/* image_pfm::save_image layout (image.h:89-118), path used as given. */
int frt_write_pfm(const char *path, int nx, int ny, const float *rgb);

/* ---- film / output side (viewer.cpp:109-132, image.cpp:24-58) ---- */
/* Progressive accumulation: acc = (acc * acc_spp + pass * pass_spp) / (acc_spp + pass_spp),
 * per element (n floats), so a film accumulated over passes is the mean over all of
 * their samples (viewer.cpp:111 divides by the total ns). */
int frt_film_accumulate(float *acc, int64_t acc_spp, const float *pass, int64_t pass_spp, int64_t n);
/* viewer::add_sample's display mapping (viewer.cpp:115-117): per channel
 * int(pow(1 - exp(-x), 1/2.2) * 255 + 0.5), stored as a byte, for a mean film
 * (nx*ny*3 floats, y = 0 bottom row) -> u8 rgb in the same layout. */
int frt_tonemap_u8(const float *rgb, int nx, int ny, uint8_t *out_u8);
/* image::save_image (image.cpp:24-58): u8 rgb (y = 0 bottom row) flipped to
 * top-down rows (stbi_flip_vertically_on_write) and written as PNG or BMP.  The
 * extension is appended when missing, as the reference does.  The reference's
 * switch writes BMP bytes for STBI_JPG and JPEG for STBI_BMP (image.cpp:40-52);
 * FRT_IMAGE_JPG reproduces the first, and JPEG encoding is not provided. */
enum { FRT_IMAGE_PNG = 0, FRT_IMAGE_BMP = 1, FRT_IMAGE_JPG = 2 };
int frt_write_image(const char *path, int nx, int ny, const uint8_t *rgb_u8, int format);

/* ---- self-test hook for CPU-only unit tests: runs the megakernel's per-lane
 *      path code (frt_path.hpp) on the host over the flattened fp32 scene for
 *      the listed pixels (linear y*nx+x); out_rgb = per-pixel means.  Not a
 *      render path: frt_render / frt_render_device never use it. ---- */
int frt_selftest_path_host(const frt_scene_view *scene, const frt_render_params *p, const int32_t *pixels,
                           int npix, float *out_rgb, frt_stats *st);
/* ... with an environment image (NULL = none), validated and converted as
 * frt_set_env_image does and read as a render reads it */
int frt_selftest_path_host_env(const frt_scene_view *scene, const frt_render_params *p, const int32_t *pixels,
                               int npix, const frt_image *env, float *out_rgb, frt_stats *st);
/* Same for PSS-MLT: n bootstrap-stream eye paths (frt_mlt.hpp) on the host;
 * out6 per path = film x, film y, r, g, b, scalar contribution. */
int frt_selftest_mlt_paths_host(const frt_scene_view *scene, int nx, int ny, uint32_t seed, int n, float *out6);
/* ---- frtx_*: further self-test hooks, added after the entry-point list of the
 *      frt_* C-ABI was fixed (tests/abi_symbols.txt); the same calling rules,
 *      a prefix of their own, no part of the drop-in boundary ---- */
/* The counting hook of the tree refinement pass (FRT_TREE_REFINE, README): the
 * scene is flattened without (out[0], nodes_off) and with (out[1], nodes_on)
 * the pass, whatever the environment says, and both binary trees are priced on
 * the pass's validation rays by the kernels' visit rule: v node visits and t
 * primitive tests per ray, j = v + w t.  depth counts levels of interior
 * nodes.  applies = 0: the tree is not LDS-resident, the pass does not run and
 * nothing is priced (n_rays = 0).  nodes_*: n_nodes x 16 floats, the flattened
 * node records (child 0 box lo hi, child 1 box lo hi, the two child refs as
 * int32 bits, two unused); NULL to skip.  FRT_E_INVALID when n_nodes exceeds
 * max_nodes. */
typedef struct frt_tree_cost {
    double v, t, j, w;
    int32_t depth, n_nodes, n_rays, applies;
} frt_tree_cost;
int frtx_selftest_tree_refine(const frt_scene_view *scene, frt_tree_cost out[2], float *nodes_off, float *nodes_on,
                             int32_t max_nodes);
/* The counting hook of the shadow-tree pass (FRT_SHADOW_TREE, README): the scene is flattened with
 * the pass on, whatever the environment says.  why: 0 the pass ran, 1 switched off, 2 no lights,
 * 3 coordinates too large for the proof, 4 a material other than lambertian / diffuse_light, 5 the
 * binary tree is not LDS-resident, 6 nothing to drop, 7 the extra nodes would change the launch plan.
 * With why = 0: the primitives kept and dropped (by the half-space rule, by the lights'-plane rule),
 * the main tree's nodes, the nodes appended and the main nodes the shadow tree shares, its root
 * (node index, or ~leaf) and whether it is empty; v_* / t_*: node visits and primitive tests per
 * area-light shadow ray of the refinement pass's validation rays (n_rays of them) started at the
 * main root and at the shadow root, root_stops_*: how many miss that root's box (the kernels test
 * no box at the shadow root: there such a ray costs the one visit that v_shadow counts).  segments > 0:
 * that many segments from those rays' origins to seeded points on the lights are put to the fp32
 * tri_intersect of every dropped triangle over (t_min, 1 - shadow_eps]; segment_hits counts the
 * hits, which the proof says is 0.  dropped: n_tris bytes per scene-view triangle, nodes: the
 * flattened node records as frtx_selftest_tree_refine gives them (NULL to skip either). */
typedef struct frt_shadow_tree_info {
    int32_t why, kept_prims, dropped_prims, rule_a, rule_b;
    int32_t nodes_main, nodes_added, nodes_shared, root, empty;
    int32_t n_rays, root_stops_main, root_stops_shadow, n_nodes;
    double v_main, t_main, v_shadow, t_shadow;
    int64_t segments, segment_hits;
} frt_shadow_tree_info;
int frtx_selftest_shadow_tree(const frt_scene_view *scene, frt_shadow_tree_info *out, uint8_t *dropped, float *nodes,
                              int32_t max_nodes, int64_t segments, uint32_t seed);
/* The counting hook of the exit-tree pass (FRT_EXIT_TREE, README): the scene is flattened without
 * the pass and with it as `mode` says (-1 the environment, 0 off, 1 on).  why: 0 the pass ran,
 * 1 switched off, 2 a material other than lambertian / diffuse_light, 3 the binary tree is not
 * LDS-resident, 4 coordinates too large for the proof, 5 no drop set with a gain, 6 the extra nodes
 * would change the launch plan.  classes: distinct drop sets found; taken: those given a tree, six
 * int32 each in `taken` (the dropped subtree as a node index or ~leaf, the exit root, origin
 * triangles, dropped triangles, nodes appended, main-tree nodes shared); budget_refused: one with
 * a gain was left out for the LDS budget.  roots: per scene-view triangle the node its extension
 * rays start at, 0 = the main root; view_of: per device triangle (the ids the leaves name) its
 * scene-view triangle.  nodes_off / nodes_on: the flattened node records of the two
 * flattens (frtx_selftest_tree_refine's layout; NULL to skip).  lds_bytes(_oct) against
 * lds_cap(_oct): what the residency rule compares (oct: 0 without octant copies).  v / t / j_all:
 * node visits, primitive tests and J per ray of the refinement pass's validation replay, every ray
 * started where the kernels start it, with the exit roots ignored [0] and used [1]; v / t_ext: the
 * same per extension ray (n_ext of the n_rays) over those alone. */
typedef struct frt_exit_tree_info {
    int32_t why, classes, taken, budget_refused;
    int32_t nodes_off, n_nodes, nodes_added, depth_off, depth_on, n_rays, n_ext, reserved;
    int64_t lds_bytes, lds_bytes_oct, lds_cap, lds_cap_oct;
    double v_all[2], t_all[2], j_all[2], v_ext[2], t_ext[2];
} frt_exit_tree_info;
int frtx_selftest_exit_tree(const frt_scene_view *scene, int32_t mode, frt_exit_tree_info *out, int32_t *roots,
                            int32_t *view_of, int32_t *taken, int32_t max_taken, float *nodes_off, float *nodes_on,
                            int32_t max_nodes);
/* frt_trace_device's queries through the same code on the host (host memory,
 * the same ray and hit layout), over the scene flattened as an upload would
 * flatten it (FRT_TREE_REFINE and FRT_LEAF_SIZE are read) */
int frtx_selftest_trace_host(const frt_scene_view *scene, const float *rays, int64_t n, float *hits);
/* FRT_INTEGRATOR_ERROR's arithmetic (csrc/frt_error.hpp, the code the kernel runs per element) on
 * host memory: partial = n_chunks x n_slots x 3 chunk sums in the device layout (slot s of chunk c
 * at 3 (c n_slots + s)), chunks of spi samples, the last one spp - (n_chunks - 1) spi (1 .. spi);
 * every slot is valid; out = n_slots x 3.  FRT_E_INVALID for n_chunks < 2 or counts that do not
 * describe such a cut. */
int frtx_selftest_chunk_variance(const float *partial, int n_chunks, int64_t n_slots, int spp, int spi, float *out);
/* The launch plan of a call, without a device: which kernel a render (kind 0: integrator, flags;
 * FRT_INTEGRATOR_PSSMLT answers with its two kernels) or a ray query (kind 1: flags) would launch
 * on a context whose uploaded scene has the properties in the query -- the fields the dispatch
 * reads, nothing else.  env_sampling: the context's image has sampling tables (a render builds
 * them on the device; the dispatch reads only that they exist).  The answer holds the dispatch's
 * return code, the plan's fields and the kernel as the offset of its host-side handle from the
 * library's load address: the value of that handle's symbol in the library's symbol table, whose
 * name is the kernel's (0: no kernel).  The hook itself returns FRT_E_INVALID for a NULL
 * argument, else FRT_OK. */
typedef struct frt_plan_query {
    int32_t kind, integrator, flags;
    int32_t world_kind, stack_needed, has_bvh4, depth4;
    int32_t mats, has_spec_mats, env_image, env_sampling, has_f64, precision;
    int64_t scene_lds_bytes, scene_lds_bytes_oct;
} frt_plan_query;
typedef struct frt_plan_answer {
    int32_t rc, stack, waves, lds_scene, wide, f64;
    int64_t lds, scene_lds;
    int64_t lds_boot;              /* PSS-MLT: the bootstrap launch's LDS bytes (lds: the chain launch's) */
    uint64_t kernel, kernel_boot;  /* kernel_boot: PSS-MLT's bootstrap kernel (kernel: its chain kernel) */
} frt_plan_answer;
int frtx_selftest_plan(const frt_plan_query *q, frt_plan_answer *a);
/* Render a list of pixels (not in the reference; the adaptive drivers' later passes).  Entry i
 * of `pixels` is a linear pixel y * nx + x of the nx x ny frame of `p`; out_rgb[3i .. 3i + 2] is
 * the mean radiance of its samples [sample_offset, sample_offset + spp): the samples frt_render
 * draws for that pixel with the same seed, max_depth, flags and environment, so the value is the
 * full render's up to fp32 summation order.  out_var (NULL to skip): the batch-means estimate V
 * of FRT_INTEGRATOR_ERROR for that entry, over chunks of samples_per_item samples (0: the library
 * takes max(1, spp / 16)); with out_var and fewer than 2 chunks the call is FRT_E_INVALID (the
 * text names samples_per_item).  Integrators: FRT_INTEGRATOR_PATH and _AO (normals, albedo,
 * depth: FRT_E_UNSUPPORTED; pssmlt, denoise, error: FRT_E_INVALID).  Precision as in frt_render
 * (the context's, FRT_FLAG_FP64 / _FP32); FRT_FLAG_ENV_SAMPLING, _ROULETTE and _SOBOL as in
 * frt_render; FRT_FLAG_BVH2 selects the binary tree; the other plan flags do nothing -- a kernel
 * of its own reads the scene from HBM -- and tile_size is ignored.  shard_count must be 1.  A
 * pixel outside [0, nx * ny) is FRT_E_INVALID before any kernel runs.  Duplicates are allowed,
 * each entry is rendered on its own; npix = 0 returns FRT_OK and writes nothing.  The call uses
 * buffers of its own: the chunk sums of the context's last frt_render stay, and a
 * FRT_INTEGRATOR_ERROR call after it still describes that render.  st: the three ray counters,
 * samples = npix * spp, pixels = npix, work_items, kernel_ms (both kernels), stack_entries,
 * bvh_depth, fp64; scene_in_lds = 0.
 * frtx_render_pixels: list and outputs in host memory.  frtx_render_pixels_device: all three in
 * device memory, launched on hip_stream (NULL: the context's); returns when the work is done. */
int frtx_render_pixels(frt_ctx *ctx, const frt_render_params *p, const int32_t *pixels, int64_t npix,
                       float *out_rgb, float *out_var, frt_stats *st);
int frtx_render_pixels_device(frt_ctx *ctx, const frt_render_params *p, const int32_t *pixels, int64_t npix,
                              float *out_rgb, float *out_var, void *hip_stream, frt_stats *st);
/* Radiance along caller-supplied first rays (not in the reference): this library's integrator --
 * NEE + MIS, every material, the environment and its sampling, roulette, Sobol' points, fp64 --
 * behind a first ray of the caller's instead of the thin-lens camera's: other cameras, light
 * probes, baking at surface points, non-raster sampling.  frt_trace_device is the counterpart for
 * callers with an integrator of their own.
 * The ray record is frt_trace_device's, 8 floats: words 0-2 the origin, word 3 t_max of the first
 * segment, words 4-6 the direction (any length, as the camera's), word 7 the entry's RNG stream id
 * as uint32 bits -- it is never read as a float.  out_rgb[3i .. 3i + 2] is the mean of Li along ray
 * i over samples [sample_offset, sample_offset + spp); every sample traces the same first ray.
 * Sample s of entry i draws from the stream keyed (seed, stream id, s) as a pixel render keys
 * (seed, pixel, s) (with FRT_FLAG_SOBOL: that sampler's key); dimensions 0-3 (film, lens) are not
 * read, every bounce reads the dimensions it reads in a render.  ENTRIES WITH EQUAL STREAM IDS SHARE
 * THEIR RANDOM NUMBERS: give independent estimates distinct ids (0 .. n - 1, say), and pass the
 * same id to correlate on purpose.  The first ray is a camera ray in every respect: depth 0, a
 * light it hits adds its full one-sided emission (no MIS), a miss -- or a first segment cut short
 * by t_max -- adds the environment.  The mean is sum / spp, correctly rounded.
 * out_var (NULL to skip): frtx_render_pixels' V under its chunk rule (samples_per_item, 0 =
 * max(1, spp / 16)); with out_var and fewer than 2 chunks the call is FRT_E_INVALID.
 * Integrators, precision and flags as in frtx_render_pixels (path and ao; _FP64 / _FP32,
 * _ENV_SAMPLING, _ROULETTE, _SOBOL, _BVH2; the other plan flags do nothing); nx, ny and tile_size
 * are ignored; shard_count must be 1.  Input domain, checked on the host before any kernel runs
 * (the device variant reads the list back first): origins and directions finite, the direction
 * not zero, t_max finite and > 0, |origin| < 1e8 (frt_trace_device's domain); a bad entry is
 * FRT_E_INVALID with its index in the text.  n = 0 returns FRT_OK and writes nothing.  The call
 * uses the pixel list's buffers, not the render's chunk sums: a FRT_INTEGRATOR_ERROR call after it
 * still describes the last frt_render.  st: as frtx_render_pixels, camera_rays = samples = n spp,
 * pixels = n.  A refusal made before the context is looked at is also kept, per thread, as the
 * text of frt_last_error(NULL).
 * frtx_radiance_rays: list and outputs in host memory.  frtx_radiance_rays_device: all three in
 * device memory, launched on hip_stream (NULL: the context's); returns when the work is done. */
int frtx_radiance_rays(frt_ctx *ctx, const frt_render_params *p, const float *rays, int64_t n,
                       float *out_rgb, float *out_var, frt_stats *st);
int frtx_radiance_rays_device(frt_ctx *ctx, const frt_render_params *p, const float *rays, int64_t n,
                              float *out_rgb, float *out_var, void *hip_stream, frt_stats *st);
/* The scene camera's own first rays as such records, to start from and perturb: entry i is the ray
 * a render makes for pixel pixels[i] of the nx x ny frame at sample p->sample_offset (the film and
 * lens points of seed, pixel and that sample; FRT_FLAG_SOBOL selects that sampler), always in fp32;
 * word 3 is the kernels' t_max (FLT_MAX), word 7 the pixel.  frtx_radiance_rays of these records
 * at spp = 1 and the same sample_offset is frtx_render_pixels of the pixels, bit for bit, where
 * the render is fp32.  pixels and rays_out (npix x 8 floats) are device memory; the list is
 * validated as frtx_render_pixels validates it.  Returns when the work is done. */
int frtx_camera_rays_device(frt_ctx *ctx, const frt_render_params *p, const int32_t *pixels, int64_t npix,
                            float *rays_out, void *hip_stream);
/* The two calls through the same per-lane code on the host (host memory; the scene flattened as
 * an upload flattens it, the material sets collapsed as frt_selftest_path_host_env collapses
 * them; env: an environment image or NULL; FRT_FLAG_FP64 selects fp64).  The radiance hook
 * refuses what frtx_radiance_rays refuses, with the text in frt_last_error(NULL). */
int frtx_selftest_radiance_host(const frt_scene_view *scene, const frt_render_params *p, const float *rays, int64_t n,
                                const frt_image *env, float *out_rgb, frt_stats *st);
int frtx_selftest_camera_rays_host(const frt_scene_view *scene, const frt_render_params *p, const int32_t *pixels,
                                   int64_t npix, float *rays_out);

/* ---- precomputed radiance transfer (the reference's path_prt integrator, path_prt.cpp, prt.h;
 *      DESIGN.md 5f).  Diffuse PRT after Sloan et al. 2002: a scene is baked once into per-corner
 *      transfer vectors and can then be relit under any environment at the cost of one first-hit
 *      query and a 25-term dot product per ray.  Not the reference's arithmetic: its frames are
 *      inconsistent and its interreflection estimator converges to nothing meaningful (DESIGN.md 5f
 *      lists the deviations).
 * Basis: 5 bands, 25 real SH coefficients, index k = l (l + 1) + m, K and P with the Condon-Shortley
 *   phase as prt.h EstimateSH has them.  One convention throughout, frt_set_env_image's: for a unit
 *   direction d, theta = acos(d.y), phi = atan2(d.x, -d.z) (+ 2 pi when negative), Y_k(d) =
 *   EstimateSH(l, m, theta, phi).
 * Corner records: one per (triangle t of the scene view, corner i), index 3 t + i, in fp64 rounded to
 *   fp32.  Normal n: tri_n where the view has vertex normals and tri_geometry_normal[t] is 0, else
 *   the normalised e1 x e2.  Origin o = v + 1e-4 n.  Albedo rho: a lambertian triangle's texture at
 *   the corner's uv (constant, checker or image, by the kernels' index rules in fp64); 0 for every
 *   other material.  Spheres have no corners, they only occlude.
 * Directions: n_dirs unit vectors, 3 floats each.  Nothing is normalised; a direction that is not
 *   finite or whose length is off 1 by more than 1e-3 is FRT_E_INVALID with its index in the text.
 *   Y_k of every direction is taken in fp64 and rounded to fp32 once (frtx_prt_basis gives that table).
 * Transfer T[3 t + i][k][ch], n_tris x 3 x 25 x 3 floats, = sum over bounces b = 0 .. B of T^b:
 *   T^0[c][k][ch] = rho[c][ch] (4 / n_dirs) sum_j [cos_j > 0 and ray j unoccluded] cos_j Y_k(d_j),
 *     cos_j = dot(n_c, d_j) in fp32, ray j = (o_c, d_j, t_max = FLT_MAX) answered as frt_trace_device
 *     answers that record with the any-hit flag; FRTX_PRT_UNSHADOWED traces nothing;
 *   T^b, b >= 1: the same directions with a closest-hit query; a ray that hits triangle q at (u, v)
 *     on its front side (dot(q's shading normal at the hit, -d) > 0) gathers (1 - u - v) T^(b-1)[q, 0]
 *     + u T^(b-1)[q, 1] + v T^(b-1)[q, 2], weighted rho[c][ch] (4 / n_dirs) cos_j; a miss, a sphere
 *     or a back side gathers 0.
 *   Order of the sums (part of the contract): the directions are cut into chunks of 64; a corner's
 *   terms of a chunk are added in ascending j into fp32 accumulators, the chunk sums in ascending
 *   chunk order, rho and 4 / n_dirs (fp32) are applied last as (rho * scale) * sum.  The result does
 *   not depend on how the work was scheduled or batched.
 * Environment Li[k][ch] (frtx_sh_project_image, fp64): sum over texels of value Y_k(theta_y, phi_x)
 *   sin(theta_y) (2 pi / nx) (pi / ny), theta_y = pi (y + 1/2) / ny, phi_x = 2 pi (x + 1/2) / nx, row
 *   0 at the +y pole, value = the fp32 texel image_texture's lookup returns.  img = NULL: the
 *   constant colour, Li[0] = E sqrt(4 pi), the rest 0.
 * Vertices at junctions: a corner's transfer is taken at the vertex itself.  A vertex that lies in the
 *   plane of a neighbouring wall (every vertex of the Cornell box) starts half of its rays in that
 *   plane and misses it, so it sees the environment through the junction, and gathers carry that light
 *   on (the reference's vertices do the same).  On such meshes PRT is brighter near junctions than the
 *   path integrator; the two agree on scenes without junctions (tests/test_prt_host.py).
 * Shading a ray (frtx_prt_rays): the closest hit comes from frt_trace_device.  On a lambertian
 *   triangle rgb[ch] = sum_k (ascending) Li[k][ch] interp(T[q, .][k][ch]); on a diffuse_light its
 *   emit (shown, but PRT lighting is the environment only); on any other material or a sphere 0; on
 *   a miss the context's environment in the ray's direction as every integrator looks it up. */
#define FRTX_PRT_UNSHADOWED (1 << 16)   /* frtx_prt_transfer flags: bounce 0 without visibility rays */
/* host only: Y[n][25] of n directions (checked as above) */
int frtx_prt_basis(const float *dirs, int64_t n, float *Y);
/* host only: li[25][3] of an image (frt_set_env_image's formats and refusals) or of env_color */
int frtx_sh_project_image(const frt_image *img_or_null, const double env_color[3], double li[75]);
/* host only: sqrt_n^2 jittered strata, uniform on the sphere, jitter from the counter hash keyed by
 * (seed, stratum), in the convention above; dirs = sqrt_n^2 x 3 floats; sqrt_n in [1, 4096] */
int frtx_prt_sample_dirs(int sqrt_n, uint32_t seed, float *dirs);
/* host only: the corner records; origin_normal = n_tris x 3 x 8 floats (o, 0, n, 0), albedo x 3 */
int frtx_prt_corners(const frt_scene_view *scene, float *origin_normal, float *albedo);
/* The transfer of the uploaded scene.  `scene` is the view that was uploaded: the corner records
 * are taken from its fp64 arrays, of which an upload keeps none (a view with another triangle
 * count is FRT_E_INVALID; one with the same count and other vertices bakes that view's corners
 * against the uploaded scene: passing the uploaded view is the caller's part of the contract).  flags: FRTX_PRT_UNSHADOWED, and FRT_FLAG_BVH2 to select the binary tree
 * (_NO_LDS_SCENE and _NO_OCT do nothing: the kernels read the scene from HBM).  T is written only
 * when the call succeeds; n_tris = 0 returns FRT_OK and writes nothing.  FRT_E_NO_SCENE before an
 * upload; FRT_E_INVALID with a text for n_dirs < 1, bounces outside [0, 16], a bad direction, unknown
 * flags.  st: kernel_ms (transfer and reduce kernels), shadow_rays = the visibility rays of bounce 0,
 * extension_rays = the gather rays, work_items, and the plan as frt_trace_device fills it.
 * frtx_prt_transfer: T in host memory.  frtx_prt_transfer_device: T in device memory, the work on
 * hip_stream (NULL: the context's); returns when it is done.  dirs is host memory in both. */
int frtx_prt_transfer(frt_ctx *ctx, const frt_scene_view *scene, const float *dirs, int64_t n_dirs, int bounces, int flags,
                      float *T, frt_stats *st);
int frtx_prt_transfer_device(frt_ctx *ctx, const frt_scene_view *scene, const float *dirs, int64_t n_dirs, int bounces, int flags,
                             float *T, void *hip_stream, frt_stats *st);
/* rgb[3 i ..] of ray i (frt_trace_device's record, checked as frtx_radiance_rays checks it; word 7
 * is not read).  li = 75 floats in host memory.  st: camera_rays = n, kernel_ms (the ray query and
 * the shade kernel), the ray query's plan.  frtx_prt_rays: T, rays and rgb in host memory;
 * frtx_prt_rays_device: in device memory, on hip_stream (NULL: the context's). */
int frtx_prt_rays(frt_ctx *ctx, const float *T, const float *li, const float *rays, int64_t n, float *rgb, frt_stats *st);
int frtx_prt_rays_device(frt_ctx *ctx, const float *T, const float *li, const float *rays, int64_t n, float *rgb,
                         void *hip_stream, frt_stats *st);
/* A PRT frame through the scene's own camera: film = nx x ny x 3 floats in host memory (index
 * (y nx + x) 3, y = 0 the bottom row, as frt_render's).  Per sample s of p->spp the first rays a
 * render makes for every pixel at sample p->sample_offset + s (frtx_camera_rays_device: seed,
 * FRT_FLAG_SOBOL) are shaded as frtx_prt_rays shades them, and the samples are averaged by
 * frt_film_accumulate's rule.  T and li in host memory.  st: camera_rays = samples = nx ny spp,
 * kernel_ms over the samples, the ray query's plan. */
int frtx_prt_render(frt_ctx *ctx, const frt_render_params *p, const float *T, const float *li, float *film, frt_stats *st);
/* Test hook: the bytes of chunk sums one batch of corners may take in frtx_prt_transfer and in its
 * replay (0: the default, 256 MiB).  The result of a transfer never depends on it. */
int frtx_selftest_prt_budget(int64_t bytes);
/* The two calls through the same code on the host (csrc/frt_prt.hpp over the host traversal of
 * frtx_selftest_trace_host), refusing what they refuse with the text in frt_last_error(NULL);
 * env: an environment image or NULL (the view's env_color). */
int frtx_selftest_prt_transfer_host(const frt_scene_view *scene, const float *dirs, int64_t n_dirs, int bounces, int flags,
                                    float *T);
int frtx_selftest_prt_rays_host(const frt_scene_view *scene, const frt_image *env, const float *T, const float *li,
                                const float *rays, int64_t n, float *rgb);

#ifdef __cplusplus
}
#endif
#endif /* FRT_H */
