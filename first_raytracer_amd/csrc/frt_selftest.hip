// frt_selftest.hip -- the host self-test hooks of the C-ABI (CPU-only unit
// tests): frt_path.hpp / frt_mlt.hpp, the code the kernels run per lane, on the
// host over the flattened scene.  No kernel.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "frt_ctx.hpp"
#include "frt_flatten.hpp"
#include "frt_prt.hpp"
#include "frt_rays.hpp"
#include "frt_tree_passes.hpp"
#include "host/envdist.hpp"
#include "host/prt.hpp"

using namespace frt;

constexpr int kSelftestStack = 8;   // small, so the host self-test exercises the overflow entries

// the self-test's per-pixel loop in precision R (fp64: the binary tree or the list); with `rays`
// the entries are first rays (frtx_selftest_radiance_host: ray_begin in path_begin's place)
template <typename R, int MATS = kMatsAll>
static void selftest_pixels(const DevScene &S, const FlatScene &F, const frt_render_params *p, const int32_t *pixels,
                            int npix, bool wide, std::vector<int> &stack, float *out_rgb, uint64_t cnt[3],
                            const float *rays = nullptr)
{
    uint32_t n_ext = 0, n_sh = 0;
    for (int i = 0; i < npix; ++i) {
        const int pix = rays ? 0 : pixels[i];
        const int px = pix % p->nx, py = pix / p->nx;
        float4 ray[2];
        if (rays) memcpy(ray, rays + 8 * (size_t)i, sizeof(ray));
        V3<R> acc = zero3<R>();
        for (int smp = 0; smp < p->spp; ++smp) {
            PathState<R> P;
            if (rays) ray_begin<MATS>(P, ray[0], ray[1], p->seed, (uint32_t)(smp + p->sample_offset));
            else path_begin<MATS>(P, S, px, py, p->nx, p->ny, p->seed, (uint32_t)pix, (uint32_t)(smp + p->sample_offset));
            ++cnt[0];
            for (;;) {
                Hit<R> h;
                const bool occl = p->integrator != FRT_INTEGRATOR_AO && light_shadow_ray(P);   // starts at the shadow root
                // an extension ray of the path integrator starts at its vertex's exit root (binary tree; 0 = the main root)
                const int xroot = p->integrator == FRT_INTEGRATOR_PATH && !P.shadow ? exit_root(P) : 0;
                if (S.world_kind == FRT_WORLD_LIST) {
                    h = trace<FRT_WORLD_LIST, 1>(S, P.ro, P.rd, P.rtmax, P.shadow, stack.data());
                } else if constexpr (!kIsF64<R>) {
                    h = wide ? trace<kWorldBvh4, 1, kSelftestStack>(S, P.ro, P.rd, P.rtmax, P.shadow, stack.data())
                        : xroot ? trace_bvh_from<1>(S, xroot, P.ro, P.rd, P.rtmax, stack.data())
                             : trace<FRT_WORLD_BVH, 1>(S, P.ro, P.rd, P.rtmax, P.shadow, stack.data(), occl);
                } else {
                    h = xroot ? trace_bvh_from<1>(S, xroot, P.ro, P.rd, P.rtmax, stack.data())
                              : trace<FRT_WORLD_BVH, 1>(S, P.ro, P.rd, P.rtmax, P.shadow, stack.data(), occl);
                }
                n_ext = n_sh = 0;
                const bool done = p->integrator == FRT_INTEGRATOR_AO ? ao_shade<MATS>(P, S, h, n_sh)
                                  : p->integrator == FRT_INTEGRATOR_NORMALS ? normals_shade<MATS>(P, S, h)
                                  : p->integrator == FRT_INTEGRATOR_ALBEDO ? albedo_shade(P, S, h)
                                  : p->integrator == FRT_INTEGRATOR_DEPTH ? depth_shade(P, S, h)
                                  : path_shade<MATS, true>(P, S, h, p->max_depth, n_ext, n_sh);
                cnt[1] += n_ext; cnt[2] += n_sh;
                if (done) break;
            }
            acc = acc + P.L;
        }
        if (p->integrator == FRT_INTEGRATOR_ALBEDO || p->integrator == FRT_INTEGRATOR_DEPTH) {   // film_reduce_mean
            const R n = (R)p->spp;
            out_rgb[3 * i] = (float)(acc.x / n); out_rgb[3 * i + 1] = (float)(acc.y / n); out_rgb[3 * i + 2] = (float)(acc.z / n);
            if (p->integrator == FRT_INTEGRATOR_DEPTH)
                out_rgb[3 * i + 1] = depth_moment_floor(out_rgb[3 * i], out_rgb[3 * i + 1], out_rgb[3 * i + 2]);
            continue;
        }
        if (rays) {   // the ray lists divide (sparse_reduce): exact where the sum is
            const R n = (R)p->spp;
            out_rgb[3 * i] = (float)(acc.x / n); out_rgb[3 * i + 1] = (float)(acc.y / n); out_rgb[3 * i + 2] = (float)(acc.z / n);
            continue;
        }
        const R k = R(1) / (R)p->spp;
        out_rgb[3 * i] = (float)(acc.x * k); out_rgb[3 * i + 1] = (float)(acc.y * k); out_rgb[3 * i + 2] = (float)(acc.z * k);
    }
}

// Self-test hook (CPU-only unit tests): runs frt_path.hpp -- the code the
// megakernel runs per lane -- on the host over the flattened scene, in fp32 or
// (FRT_FLAG_FP64) in fp64.  Not a render path: frt_render / frt_render_device
// never call it.
extern "C" int frt_selftest_path_host(const frt_scene_view *sv, const frt_render_params *p, const int32_t *pixels,
                                      int npix, float *out_rgb, frt_stats *st)
{
    return frt_selftest_path_host_env(sv, p, pixels, npix, nullptr, out_rgb, st);
}
// ... with an environment image (frt_set_env_image's validation and conversion; NULL = none)
static int selftest_replay(const frt_scene_view *sv, const frt_render_params *p, const int32_t *pixels, const float *rays,
                           int npix, const frt_image *env, float *out_rgb, frt_stats *st);
extern "C" int frt_selftest_path_host_env(const frt_scene_view *sv, const frt_render_params *p, const int32_t *pixels,
                                          int npix, const frt_image *env, float *out_rgb, frt_stats *st)
{
    if (!sv || !p || !pixels || !out_rgb || npix < 0 || p->spp <= 0 || p->nx <= 0 || p->ny <= 0) return FRT_E_INVALID;
    for (int i = 0; i < npix; ++i)
        if (pixels[i] < 0 || pixels[i] >= p->nx * p->ny) return FRT_E_INVALID;
    return selftest_replay(sv, p, pixels, nullptr, npix, env, out_rgb, st);
}
// the replay of a checked list: pixels, or (rays) first rays
static int selftest_replay(const frt_scene_view *sv, const frt_render_params *p, const int32_t *pixels, const float *rays,
                           int npix, const frt_image *env, float *out_rgb, frt_stats *st)
{
    if (p->integrator == FRT_INTEGRATOR_DENOISE) return FRT_E_INVALID;   // a filter over a frame: no per-pixel code
    if (p->integrator == FRT_INTEGRATOR_ERROR) return FRT_E_INVALID;     // a reduction of a context's chunk sums: no per-pixel code
    // albedo, depth: fp32 and the hash stream whatever the flags say, and no environment
    const bool feature = p->integrator == FRT_INTEGRATOR_ALBEDO || p->integrator == FRT_INTEGRATOR_DEPTH;
    if (feature) env = nullptr;
    const bool f64 = (p->flags & FRT_FLAG_FP64) != 0 && !feature;
    FlatScene F;
    std::string err;
    const int rc = flatten_scene(sv, F, err, f64);
    if (rc != FRT_OK) return rc;
    if (p->integrator == FRT_INTEGRATOR_AO)
        for (int i = 0; i < sv->n_materials; ++i)
            if (sv->materials[i].type == FRT_MAT_METAL) return FRT_E_UNSUPPORTED;
    DevScene S = host_scene(F);
    std::vector<float4> env_tex;
    bool env_sampling = false;
    if (env) {
        const int erc = env_texels_of(env, env_tex, err);
        if (erc != FRT_OK) return erc;
        // FRT_FLAG_ENV_SAMPLING: the tables behind the texels, as on a context
        if ((p->flags & FRT_FLAG_ENV_SAMPLING) && p->integrator != FRT_INTEGRATOR_AO &&
            p->integrator != FRT_INTEGRATOR_NORMALS) {
            std::vector<float> tab;
            env_sampling = env_tables_of(&env_tex[0].x, env->nx, env->ny, tab);
            const size_t n = env_tex.size();
            env_tex.resize(n + tab.size() / 4);
            memcpy(reinterpret_cast<float *>(env_tex.data() + n), tab.data(), tab.size() * sizeof(float));
        }
        S.env_texels = env_tex.data(); S.env_nx = env->nx; S.env_ny = env->ny;
    }
    std::vector<int> stack(std::max(F.depth + 1, kSelftestStack));
    const bool wide = !f64 && S.world_kind == FRT_WORLD_BVH && F.has4 && !(p->flags & FRT_FLAG_BVH2) &&
                      bvh4_stack_fits(F.depth4, kSelftestStack);
    uint64_t cnt[3] = {0, 0, 0};   // camera, extension, shadow
    constexpr int kEnvAll = kMatsAll | kMatsEnv;   // with an image: the code of the kMatsEnv kernels
    constexpr int kEnvNee = kEnvAll | kMatsEnvNee;   // ... and of the kernels that sample it
    // FRT_FLAG_ROULETTE, FRT_FLAG_SOBOL (path): the code of the kMatsRoulette / kMatsSobol kernels
    const bool path = p->integrator == FRT_INTEGRATOR_PATH;
    const bool roulette = (p->flags & FRT_FLAG_ROULETTE) && path, sobol = (p->flags & FRT_FLAG_SOBOL) && path;
    auto run_set = [&](auto extra) {                    // the material set, then the precision
        constexpr int X = decltype(extra)::value;
        auto run = [&](auto mats) {
            constexpr int M = decltype(mats)::value;
            if (f64) selftest_pixels<double, M | X>(S, F, p, pixels, npix, wide, stack, out_rgb, cnt, rays);
            else selftest_pixels<float, M | X>(S, F, p, pixels, npix, wide, stack, out_rgb, cnt, rays);
        };
        if (env_sampling) run(std::integral_constant<int, kEnvNee>{});
        else if (env) run(std::integral_constant<int, kEnvAll>{});
        else run(std::integral_constant<int, kMatsAll>{});
    };
    if (sobol && roulette) run_set(std::integral_constant<int, kMatsSobol | kMatsRoulette>{});
    else if (sobol) run_set(std::integral_constant<int, kMatsSobol>{});
    else if (roulette) run_set(std::integral_constant<int, kMatsRoulette>{});
    else run_set(std::integral_constant<int, 0>{});
    if (st) {
        memset(st, 0, sizeof(*st));
        st->camera_rays = cnt[0]; st->extension_rays = cnt[1]; st->shadow_rays = cnt[2];
        st->samples = cnt[0]; st->pixels = (uint64_t)npix;
        st->stack_entries = wide ? (uint32_t)kSelftestStack : (uint32_t)stack.size();
        st->bvh_depth = (uint32_t)(wide ? F.depth4 : F.depth);   // which tree was traversed
        st->fp64 = f64 ? 1u : 0u;
    }
    return FRT_OK;
}

// frtx_radiance_rays on the host: the request and the list refused as the entry point refuses
// them (the text in frt_last_error(NULL)), then ray_begin and the replay's loop per entry
extern "C" int frtx_selftest_radiance_host(const frt_scene_view *sv, const frt_render_params *p, const float *rays, int64_t n,
                                           const frt_image *env, float *out_rgb, frt_stats *st)
{
    auto fail = [](int code, const std::string &m) { frt::null_ctx_err() = m; return code; };
    if (!sv || !p || n < 0 || n > INT32_MAX || (n > 0 && (!rays || !out_rgb))) return fail(FRT_E_INVALID, "radiance_rays: bad arguments");
    const int k = p->integrator;
    if (k == FRT_INTEGRATOR_NORMALS || k == FRT_INTEGRATOR_ALBEDO || k == FRT_INTEGRATOR_DEPTH)
        return fail(FRT_E_UNSUPPORTED, "radiance_rays: path and ao only (normals, albedo and depth have no sparse kernel)");
    if (k != FRT_INTEGRATOR_PATH && k != FRT_INTEGRATOR_AO)
        return fail(FRT_E_INVALID, "radiance_rays: path and ao only (pssmlt is no per-pixel estimator; denoise and error are "
                                   "films of a whole frame)");
    if (p->shard_count != 1) return fail(FRT_E_INVALID, "radiance_rays: shard_count must be 1 (split the list instead)");
    if (p->spp <= 0 || p->sample_offset < 0) return fail(FRT_E_INVALID, "bad render params");
    std::string why;
    if (frt::rays_first_bad(rays, n, why) >= 0) return fail(FRT_E_INVALID, "radiance_rays: " + why);
    if (st) memset(st, 0, sizeof(*st));
    if (n == 0) return FRT_OK;
    frt_render_params q = *p;
    q.nx = q.ny = 1;   // ignored
    return selftest_replay(sv, &q, nullptr, rays, (int)n, env, out_rgb, st);
}

// frtx_camera_rays_device on the host: path_begin<MATS, float> over the scene flattened as an upload flattens it
extern "C" int frtx_selftest_camera_rays_host(const frt_scene_view *sv, const frt_render_params *p, const int32_t *pixels,
                                              int64_t npix, float *rays_out)
{
    if (!sv || !p || npix < 0 || (npix > 0 && (!pixels || !rays_out)) || p->nx <= 0 || p->ny <= 0 || p->sample_offset < 0 ||
        (int64_t)p->nx * p->ny > (int64_t)INT32_MAX)
        return FRT_E_INVALID;
    for (int64_t i = 0; i < npix; ++i)
        if (pixels[i] < 0 || pixels[i] >= p->nx * p->ny) return FRT_E_INVALID;
    FlatScene F;
    std::string err;
    const int rc = flatten_scene(sv, F, err, false);
    if (rc != FRT_OK) return rc;
    const DevScene S = host_scene(F);
    for (int64_t i = 0; i < npix; ++i) {
        const int pix = pixels[i];
        PathState<float> P;
        if (p->flags & FRT_FLAG_SOBOL)
            path_begin<kMatsSobol>(P, S, pix % p->nx, pix / p->nx, p->nx, p->ny, p->seed, (uint32_t)pix, (uint32_t)p->sample_offset);
        else
            path_begin<kMatsNone>(P, S, pix % p->nx, pix / p->nx, p->nx, p->ny, p->seed, (uint32_t)pix, (uint32_t)p->sample_offset);
        const float rec[8] = {P.ro.x, P.ro.y, P.ro.z, P.rtmax, P.rd.x, P.rd.y, P.rd.z, i2f(pix)};
        memcpy(rays_out + 8 * i, rec, sizeof(rec));
    }
    return FRT_OK;
}

// Self-test hook: n PSS-MLT bootstrap eye paths (fresh primary samples from the
// bootstrap stream) through frt_mlt.hpp on the host; out6[i] = x, y, r, g, b, sc.
extern "C" int frt_selftest_mlt_paths_host(const frt_scene_view *sv, int nx, int ny, uint32_t seed, int n,
                                           float *out6)
{
    if (!sv || !out6 || n < 0 || nx <= 0 || ny <= 0) return FRT_E_INVALID;
    FlatScene F;
    std::string err;
    const int rc = flatten_scene(sv, F, err, false);
    if (rc != FRT_OK) return rc;
    const DevScene S = host_scene(F);
    std::vector<int> stack(std::max(F.depth + 1, 1));
    for (int i = 0; i < n; ++i) {
        PrndSource src{nullptr, 0, 0, rng_key(seed ^ kMltBootSalt, (uint32_t)i, 0u), 0u, true, 0.0f, 0.0f};
        MltPath M;
        mlt_begin(M, S, src, nx, ny);
        uint32_t ne = 0, ns = 0;
        for (;;) {
            if (mlt_beyond(M)) { M.P.L = M.P.L + M.P.beta * env_of<float>(S); break; }
            const Hit<float> h = (S.world_kind == FRT_WORLD_LIST)
                              ? trace<FRT_WORLD_LIST, 1>(S, M.P.ro, M.P.rd, M.P.rtmax, M.P.shadow, stack.data())
                              : trace<FRT_WORLD_BVH, 1>(S, M.P.ro, M.P.rd, M.P.rtmax, M.P.shadow, stack.data(), M.P.shadow);
            if (mlt_shade(M, S, h, src, ne, ns)) break;
        }
        const f3 L = M.P.L;
        float *o = &out6[6 * (size_t)i];
        o[0] = M.x; o[1] = M.y; o[2] = L.x; o[3] = L.y; o[4] = L.z; o[5] = fmaxf(fmaxf(L.x, L.y), L.z);
    }
    return FRT_OK;
}

// Counting hook of the tree refinement pass (frt_tree_passes.hip refine_tree): the
// scene flattened without and with the pass, both trees priced on the pass's
// validation rays, and the flattened node records for structure checks.
extern "C" int frtx_selftest_tree_refine(const frt_scene_view *sv, frt_tree_cost out[2], float *nodes_off,
                                        float *nodes_on, int32_t max_nodes)
{
    if (!sv || !out) return FRT_E_INVALID;
    float *dst[2] = {nodes_off, nodes_on};
    for (int on = 0; on < 2; ++on) {
        FlatScene F;
        std::string err;
        const int rc = flatten_scene(sv, F, err, false, on, 0, 0);   // the main tree alone: no shadow-tree or exit-tree nodes behind it
        if (rc != FRT_OK) return rc;
        TreeCost c;
        const bool applies = tree_cost_host(F, c);
        const int nn = (int)(F.nodes.size() / 4);
        out[on] = frt_tree_cost{c.V, c.T, c.J, c.w, c.depth, nn, c.n_rays, applies ? 1 : 0};
        if (dst[on]) {
            if (nn > max_nodes) return FRT_E_INVALID;
            memcpy(dst[on], F.nodes.data(), F.nodes.size() * sizeof(float4));
        }
    }
    return FRT_OK;
}

// Counting hook of the shadow-tree pass (frt_tree_passes.hip shadow_tree): what it dropped and built,
// the traversal cost of the area-light shadow rays from either root, and the segment property test
extern "C" int frtx_selftest_shadow_tree(const frt_scene_view *sv, frt_shadow_tree_info *out, uint8_t *dropped,
                                         float *nodes, int32_t max_nodes, int64_t segments, uint32_t seed)
{
    if (!sv || !out || segments < 0) return FRT_E_INVALID;
    FlatScene F;
    std::string err;
    const int rc = flatten_scene(sv, F, err, false, -1, 1, 0);   // no exit-tree nodes behind the shadow tree's
    if (rc != FRT_OK) return rc;
    const auto &I = F.shadow;
    memset(out, 0, sizeof(*out));
    out->why = I.why;
    out->n_nodes = (int)(F.nodes.size() / 4);
    out->nodes_main = I.nodes_main;
    out->root = F.meta.sroot;
    if (nodes) {
        if (out->n_nodes > max_nodes) return FRT_E_INVALID;
        memcpy(nodes, F.nodes.data(), F.nodes.size() * sizeof(float4));
    }
    if (dropped) memset(dropped, 0, (size_t)std::max(sv->n_tris, 0));
    if (I.why != FlatScene::kShadowRan) return FRT_OK;
    out->dropped_prims = I.n_dropped;
    out->kept_prims = sv->n_tris + sv->n_spheres - I.n_dropped;
    out->rule_a = I.rule_a; out->rule_b = I.rule_b;
    out->nodes_added = I.added; out->nodes_shared = I.shared; out->empty = I.empty ? 1 : 0;
    if (dropped)
        for (int d = 0; d < sv->n_tris; ++d) dropped[F.tri_view[d]] = I.dropped[d];
    ShadowCost c;
    shadow_cost_host(F, c);
    out->n_rays = c.n_rays;
    out->v_main = c.V[0]; out->t_main = c.T[0]; out->v_shadow = c.V[1]; out->t_shadow = c.T[1];
    out->root_stops_main = c.stops[0]; out->root_stops_shadow = c.stops[1];
    if (segments > 0) {
        std::vector<float> org;
        shadow_origins_host(F, org);
        const DevScene S = host_scene(F);
        const int64_t no = (int64_t)(org.size() / 3);
        for (int64_t i = 0; i < segments && no > 0 && S.n_lights > 0; ++i) {
            const RngKey key = rng_key(seed, (uint32_t)i, (uint32_t)(i >> 32));
            const float *q = &org[3 * (size_t)(i % no)];
            const f3 o = mk3(q[0], q[1], q[2]);
            int idx = (int)(rng_u(key, 0) * (float)S.n_lights);
            if (idx == S.n_lights) idx -= 1;
            f3 ln;
            int lmat;
            const f3 d = prim_sample(S, S.lights[idx], o, rng_u(key, 1), rng_u(key, 2), ln, lmat);
            ++out->segments;
            for (int t = 0; t < S.n_tris; ++t) {
                if (!I.dropped[t]) continue;
                float u, v;
                if (prim_t(S, t, o, d, bvh_tmin(o), 1.0f - Cst<float>::shadow_eps, u, v) > 0.0f) ++out->segment_hits;
            }
        }
    }
    return FRT_OK;
}

// Counting hook of the exit-tree pass (frt_tree_passes.hip exit_tree): the scene flattened without the
// pass and with it (mode: -1 as FRT_EXIT_TREE says, 0 off, 1 on), what the pass took, the root of
// every triangle, and the traversal cost of the validation rays with the roots ignored and used
extern "C" int frtx_selftest_exit_tree(const frt_scene_view *sv, int32_t mode, frt_exit_tree_info *out, int32_t *roots,
                                       int32_t *view_of, int32_t *taken, int32_t max_taken, float *nodes_off,
                                       float *nodes_on, int32_t max_nodes)
{
    if (!sv || !out || mode < -1 || mode > 1 || max_taken < 0) return FRT_E_INVALID;
    memset(out, 0, sizeof(*out));
    FlatScene F0, F;
    std::string err;
    int rc = flatten_scene(sv, F0, err, false, -1, -1, 0);
    if (rc == FRT_OK) rc = flatten_scene(sv, F, err, false, -1, -1, mode);
    if (rc != FRT_OK) return rc;
    const auto &I = F.exit;
    out->why = I.why;
    out->classes = I.classes;
    out->taken = (int32_t)I.taken.size();
    out->nodes_off = (int32_t)(F0.nodes.size() / 4);
    out->n_nodes = (int32_t)(F.nodes.size() / 4);
    out->nodes_added = I.added;
    out->budget_refused = I.budget_refused ? 1 : 0;
    out->depth_off = F0.depth; out->depth_on = F.depth;
    out->lds_bytes = (int64_t)lds_planar_bytes(out->n_nodes, lds_rest(F));
    out->lds_bytes_oct = F.nodes_oct.empty() ? 0 : (int64_t)lds_octant_bytes(out->n_nodes, lds_rest(F));
    out->lds_cap = (int64_t)kLdsSceneBytes; out->lds_cap_oct = (int64_t)kLdsOctBytes;
    if (out->nodes_off > max_nodes || out->n_nodes > max_nodes) return FRT_E_INVALID;
    if (nodes_off) memcpy(nodes_off, F0.nodes.data(), F0.nodes.size() * sizeof(float4));
    if (nodes_on) memcpy(nodes_on, F.nodes.data(), F.nodes.size() * sizeof(float4));
    if (roots)
        for (int d = 0; d < sv->n_tris; ++d) {
            const int r = f2i(F.tshade[2 * (size_t)d + 1].z);
            if (r != (d < (int)I.root.size() ? I.root[d] : 0)) return FRT_E_UNSUPPORTED;   // the record and the meta disagree
            roots[F.tri_view[d]] = r;
        }
    if (view_of)
        for (int d = 0; d < sv->n_tris; ++d) view_of[d] = F.tri_view[d];
    if (taken)
        for (int k = 0; k < out->taken && k < max_taken; ++k) {
            const auto &c = I.taken[k];
            const int32_t rec[6] = {c.sub, c.root, c.members, c.dropped, c.added, c.shared};
            memcpy(taken + 6 * k, rec, sizeof(rec));
        }
    ExitCost c;
    if (exit_cost_host(F, c)) {
        out->n_rays = c.n_rays; out->n_ext = c.n_ext;
        for (int on = 0; on < 2; ++on) {
            out->v_all[on] = c.V_all[on]; out->t_all[on] = c.T_all[on]; out->j_all[on] = c.J_all[on];
            out->v_ext[on] = c.V_ext[on]; out->t_ext[on] = c.T_ext[on];
        }
    }
    return FRT_OK;
}

// frt_trace_device's queries on the host: trace_bvh / trace_list over the scene flattened as an upload would
extern "C" int frtx_selftest_trace_host(const frt_scene_view *sv, const float *rays, int64_t n, float *hits)
{
    if (!sv || n < 0 || (n > 0 && (!rays || !hits))) return FRT_E_INVALID;
    FlatScene F;
    std::string err;
    const int rc = flatten_scene(sv, F, err, false);
    if (rc != FRT_OK) return rc;
    const DevScene S = host_scene(F);
    std::vector<int> stack(std::max(F.depth + 1, 1));
    for (int64_t i = 0; i < n; ++i) {
        const float *q = rays + 8 * i;
        const f3 o = mk3(q[0], q[1], q[2]), d = mk3(q[4], q[5], q[6]);
        const bool anyhit = (f2i(q[7]) & 1) != 0;
        const Hit<float> h = S.world_kind == FRT_WORLD_LIST ? trace<FRT_WORLD_LIST, 1>(S, o, d, q[3], anyhit, stack.data())
                                                            : trace<FRT_WORLD_BVH, 1>(S, o, d, q[3], anyhit, stack.data());
        const int ref = (h.prim < 0 || (h.prim & FRT_PRIM_SPHERE)) ? h.prim : F.tri_view[h.prim];
        float *r = hits + 4 * i;
        r[0] = h.t; r[1] = h.u; r[2] = h.v;
        const float refbits = i2f(ref);
        memcpy(&r[3], &refbits, sizeof(float));
    }
    return FRT_OK;
}

// ---- precomputed radiance transfer on the host (frt.h): frt_prt.hpp, the code the
// kernels of frt_prt.hip run per lane, over the host traversal of frtx_selftest_trace_host ----

// one ray of a corner, as frt_trace_device answers its record
static Hit<float> prt_trace_host(const DevScene &S, f3 o, f3 d, bool anyhit, int *stack)
{
    return S.world_kind == FRT_WORLD_LIST ? trace<FRT_WORLD_LIST, 1>(S, o, d, kPrtTmax, anyhit, stack)
                                          : trace<FRT_WORLD_BVH, 1>(S, o, d, kPrtTmax, anyhit, stack);
}

// one bounce over every corner, batched and reduced as transfer_impl (frt_prt.hip) does
template <bool GATHER>
static void prt_bounce_host(const DevScene &S, std::vector<int> &stack, const std::vector<float> &on, const std::vector<float> &rho,
                            const float *dirs, const std::vector<float> &Y, int n_dirs, bool unshadowed, size_t budget,
                            const float *Tprev, float *Tcur, float *Tout)
{
    constexpr int NACC = GATHER ? kPrtT : kPrtCoef;
    const size_t nc = rho.size() / 3;
    const int n_chunks = (n_dirs + kPrtChunk - 1) / kPrtChunk;
    const float scale = 4.0f / (float)n_dirs;
    const size_t nb_max = prt_batch_corners(budget, n_chunks, NACC, nc);
    std::vector<float> partial;
    for (size_t c0 = 0; c0 < nc; c0 += nb_max) {
        const size_t nb = std::min(nb_max, nc - c0);
        partial.assign((size_t)n_chunks * nb * NACC, 0.0f);
        for (size_t ci = 0; ci < nb; ++ci) {
            const float *q = &on[8 * (c0 + ci)];
            const f3 o = mk3(q[0], q[1], q[2]), n = mk3(q[4], q[5], q[6]);
            for (int chunk = 0; chunk < n_chunks; ++chunk) {
                float acc[NACC] = {};
                const int j0 = chunk * kPrtChunk, jn = std::min(kPrtChunk, n_dirs - j0);
                for (int j = j0; j < j0 + jn; ++j) {
                    const f3 d = mk3(dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2]);
                    const float cj = prt_cos(n, d);
                    if (!(cj > 0.0f)) continue;
                    if constexpr (!GATHER) {
                        if (unshadowed || prt_trace_host(S, o, d, true, stack.data()).prim < 0) prt_add(acc, cj, &Y[(size_t)kPrtCoef * j]);
                    } else {
                        const Hit<float> h = prt_trace_host(S, o, d, false, stack.data());
                        if (h.prim >= 0 && !(h.prim & FRT_PRIM_SPHERE)) {
                            float u, v;
                            prt_bary(S, h.prim, o, d, u, v);
                            if (prt_front(S, h.prim, o, d, u, v))
                                prt_gather(acc, cj, u, v, Tprev + (size_t)S.tri_view[h.prim] * (3 * kPrtT));
                        }
                    }
                }
                memcpy(&partial[((size_t)chunk * nb + ci) * NACC], acc, sizeof(acc));
            }
        }
        for (size_t ci = 0; ci < nb; ++ci)
            for (int k = 0; k < kPrtCoef; ++k)
                for (int ch = 0; ch < 3; ++ch) {
                    const size_t at = (c0 + ci) * kPrtT + 3 * k + ch;
                    const float *p = GATHER ? &partial[ci * kPrtT + 3 * k + ch] : &partial[ci * kPrtCoef + k];
                    const float v = prt_final(rho[3 * (c0 + ci) + ch], scale, prt_chunk_sum(p, n_chunks, nb * NACC));
                    if (Tcur) Tcur[at] = v;
                    Tout[at] = GATHER ? Tout[at] + v : v;
                }
    }
}

// frtx_prt_transfer on the host: the request refused as the entry point refuses it (the text in
// frt_last_error(NULL)), then the corners, the Y table and the bounces, in the entry point's batches
// (frt_prt::batch_budget; frtx_selftest_prt_budget sets it for both).
extern "C" int frtx_selftest_prt_transfer_host(const frt_scene_view *sv, const float *dirs, int64_t n_dirs, int bounces, int flags,
                                               float *T)
{
    auto fail = [](int code, const std::string &m) { frt::null_ctx_err() = m; return code; };
    if (!sv) return fail(FRT_E_INVALID, "prt_transfer: bad arguments");
    const std::string refused = frt_prt::transfer_request_bad(dirs, n_dirs, bounces, flags);   // the entry point's validator
    if (!refused.empty()) return fail(FRT_E_INVALID, refused);
    if (sv->n_tris == 0) return FRT_OK;
    if (!T) return fail(FRT_E_INVALID, "prt_transfer: bad arguments");
    FlatScene F;
    std::string err;
    const int rc = flatten_scene(sv, F, err, false);
    if (rc != FRT_OK) return fail(rc, err);
    const DevScene S = host_scene(F);
    const size_t nc = (size_t)sv->n_tris * 3;
    std::vector<float> on(nc * 8), rho(nc * 3), Y((size_t)n_dirs * kPrtCoef);
    const std::string bad = frt_prt::corners(sv, on.data(), rho.data());
    if (!bad.empty()) return fail(FRT_E_INVALID, bad);
    frt_prt::y_table(dirs, n_dirs, Y.data());
    const size_t budget = frt_prt::batch_budget();
    std::vector<int> stack(std::max(F.depth + 1, 1));
    std::vector<float> a(bounces > 0 ? nc * kPrtT : 0), b(a.size()), out(nc * kPrtT);
    float *cur = bounces > 0 ? a.data() : nullptr, *prev = b.data();
    for (int k = 0; k <= bounces; ++k) {
        if (k == 0) prt_bounce_host<false>(S, stack, on, rho, dirs, Y, (int)n_dirs, (flags & FRTX_PRT_UNSHADOWED) != 0, budget, prev, cur, out.data());
        else prt_bounce_host<true>(S, stack, on, rho, dirs, Y, (int)n_dirs, false, budget, prev, cur, out.data());
        std::swap(cur, prev);
    }
    memcpy(T, out.data(), out.size() * sizeof(float));
    return FRT_OK;
}

// frtx_prt_rays on the host: the closest hit of every ray as frtx_selftest_trace_host takes it,
// then prt_shade; env: an environment image or NULL (the view's constant colour)
extern "C" int frtx_selftest_prt_rays_host(const frt_scene_view *sv, const frt_image *env, const float *T, const float *li,
                                           const float *rays, int64_t n, float *rgb)
{
    auto fail = [](int code, const std::string &m) { frt::null_ctx_err() = m; return code; };
    if (!sv || !li || n < 0 || (n > 0 && (!rays || !rgb)) || (sv->n_tris > 0 && !T)) return fail(FRT_E_INVALID, "prt_rays: bad arguments");
    for (int k = 0; k < kPrtT; ++k)
        if (!std::isfinite(li[k])) return fail(FRT_E_INVALID, "prt_rays: li[" + std::to_string(k) + "] is not finite");
    std::string why;
    if (frt::rays_first_bad(rays, n, why) >= 0) return fail(FRT_E_INVALID, "prt_rays: " + why);
    FlatScene F;
    std::string err;
    const int rc = flatten_scene(sv, F, err, false);
    if (rc != FRT_OK) return fail(rc, err);
    DevScene S = host_scene(F);
    std::vector<float4> env_tex;
    if (env) {
        const int erc = env_texels_of(env, env_tex, err);
        if (erc != FRT_OK) return fail(erc, err);
        S.env_texels = env_tex.data(); S.env_nx = env->nx; S.env_ny = env->ny;
    }
    std::vector<int> inv(std::max(sv->n_tris, 1), 0);
    for (int d = 0; d < sv->n_tris; ++d) inv[F.tri_view[d]] = d;
    std::vector<int> stack(std::max(F.depth + 1, 1));
    for (int64_t i = 0; i < n; ++i) {
        const float *q = rays + 8 * i;
        const f3 o = mk3(q[0], q[1], q[2]), d = mk3(q[4], q[5], q[6]);
        const Hit<float> h = S.world_kind == FRT_WORLD_LIST ? trace<FRT_WORLD_LIST, 1>(S, o, d, q[3], false, stack.data())
                                                            : trace<FRT_WORLD_BVH, 1>(S, o, d, q[3], false, stack.data());
        const int ref = (h.prim < 0 || (h.prim & FRT_PRIM_SPHERE)) ? h.prim : F.tri_view[h.prim];
        const f3 c = prt_shade(S, inv.data(), T, li, o, d, make_float4(h.t, h.u, h.v, i2f(ref)));
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
    }
    return FRT_OK;
}
