// frt_integrator.hpp -- C++ host API over the C-ABI (include/frt.h) that keeps
// the reference's integrator concept, so code written against
//   template <class I> struct renderer : I { double Render(Scene*, viewer&); }  (integrator.h:11-47)
//   struct path { void Render(Scene*, viewer*, ...); using_custom_viewer; }      (path.h:8-18)
//   struct viewer { add_sample(...); save_and_destroy(...); }                     (viewer.h:9-26)
// reads the same against frt::renderer<frt::path_gpu>.  Errors become
// exceptions (frt::error), as the reference throws std::runtime_error.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "frt.h"

namespace frt {

struct error : std::runtime_error {
    int code;
    error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc, const char *what, const frt_ctx *ctx = nullptr)
{
    if (rc != FRT_OK)
        throw error(rc, std::string(what) + " failed (" + std::to_string(rc) + ")" +
                            (ctx ? std::string(": ") + frt_last_error(ctx) : std::string()));
}

// Scene (Scene.h:10-26): world + lights + camera + environment, built natively
// by the reference's scene constructors (main.cpp:222-252, 281-314).
class Scene {
public:
    Scene(const std::string &kind, const std::string &obj_path, double aspect)
    {
        frt_host_scene *s = nullptr;
        check(frt_scene_create(kind.c_str(), obj_path.c_str(), aspect, &s), "frt_scene_create");
        scene_.reset(s);
        check(frt_scene_info(s, &info_), "frt_scene_info");
    }
    static Scene cornell_box_obj(const std::string &obj, double aspect) { return Scene("cornell_box_obj", obj, aspect); }
    static Scene veach_mis(const std::string &obj, double aspect) { return Scene("veach_mis", obj, aspect); }

    frt_scene_view view() const
    {
        frt_scene_view v;
        check(frt_scene_view_get(scene_.get(), &v), "frt_scene_view_get");
        if (has_env_)
            for (int k = 0; k < 3; ++k) v.env_color[k] = env_[k];
        return v;
    }
    // Scene::env_map with another constant colour (material.h:206-232)
    void set_env(double r, double g, double b) { env_[0] = r; env_[1] = g; env_[2] = b; has_env_ = true; }
    // Scene::env_map as environment_map(image) (material.h:206-244; main.cpp's
    // open scenes load grace.hdr / ennis.hdr this way): a Radiance .hdr file, or a
    // decoded image (copied).  The *_gpu integrators hand it to their contexts
    // after the upload (frt_set_env_image).
    void set_env_map(const std::string &hdr_path)
    {
        int32_t nx = 0, ny = 0;
        check(frt_read_hdr(hdr_path.c_str(), &nx, &ny, nullptr), ("frt_read_hdr(" + hdr_path + ")").c_str());
        env_data_.assign((size_t)nx * ny * 3 * sizeof(float), 0);
        check(frt_read_hdr(hdr_path.c_str(), &nx, &ny, reinterpret_cast<float *>(env_data_.data())),
              ("frt_read_hdr(" + hdr_path + ")").c_str());
        env_image_ = frt_image{nx, ny, FRT_IMAGE_F32, 0, env_data_.data()};
        has_env_image_ = true;
    }
    void set_env_map(const frt_image &img)
    {
        if (img.nx <= 0 || img.ny <= 0 || !img.data || (img.format != FRT_IMAGE_SRGB8 && img.format != FRT_IMAGE_F32))
            throw error(FRT_E_INVALID, "set_env_map: bad image");
        const size_t n = (size_t)img.nx * img.ny * 3 * (img.format == FRT_IMAGE_F32 ? sizeof(float) : 1);
        const uint8_t *src = static_cast<const uint8_t *>(img.data);
        env_data_.assign(src, src + n);
        env_image_ = img;
        env_image_.data = env_data_.data();
        has_env_image_ = true;
    }
    // the environment image, or nullptr for the constant colour
    const frt_image *env_map() const { return has_env_image_ ? &env_image_ : nullptr; }
    // replace the reference-topology BVH: binned SAH on the host, or the GPU
    // linear BVH on ctx's device (frt_scene_build_bvh_sah / _gpu)
    void build_bvh_sah()
    {
        check(frt_scene_build_bvh_sah(scene_.get()), "frt_scene_build_bvh_sah");
        check(frt_scene_info(scene_.get(), &info_), "frt_scene_info");
    }
    void build_bvh_gpu(frt_ctx *ctx)
    {
        check(frt_scene_build_bvh_gpu(scene_.get(), ctx, nullptr), "frt_scene_build_bvh_gpu", ctx);
        check(frt_scene_info(scene_.get(), &info_), "frt_scene_info");
    }
    const frt_host_scene_info &info() const { return info_; }

private:
    double env_[3] = {0, 0, 0};
    bool has_env_ = false;
    std::vector<uint8_t> env_data_;
    frt_image env_image_{};
    bool has_env_image_ = false;
    struct del { void operator()(frt_host_scene *s) const { frt_scene_destroy(s); } };
    std::unique_ptr<frt_host_scene, del> scene_;
    frt_host_scene_info info_{};
};

// viewer (viewer.h:9-26, viewer.cpp:109-140) without the GL window: the linear
// film (fout_image, doubles) and the tonemapped u8 image (out_image).
struct viewer {
    viewer(int nx, int ny, uint64_t ns, int num_channels = 3)
        : nx(nx), ny(ny), ns(ns), num_channels(num_channels), out_image((size_t)nx * ny * num_channels, 0),
          fout_image((size_t)nx * ny * num_channels, 0.0)
    {
    }
    // add_sample(pixel, sum) (viewer.cpp:109-132): sum *= 1/ns, store linear + tonemapped
    void add_sample(int x, int y, double r, double g, double b)
    {
        const double k = 1.0 / double(ns);
        store_mean(x, y, r * k, g * k, b * k);
    }
    // the GPU already returns the per-pixel mean (sum * 1/ns)
    void store_mean(int x, int y, double fr, double fg, double fb)
    {
        const size_t idx = ((size_t)y * nx + x) * num_channels;
        out_image[idx] = (uint8_t)int(std::pow(1 - std::exp(-fr), 1 / 2.2) * 255 + .5);
        out_image[idx + 1] = (uint8_t)int(std::pow(1 - std::exp(-fg), 1 / 2.2) * 255 + .5);
        out_image[idx + 2] = (uint8_t)int(std::pow(1 - std::exp(-fb), 1 / 2.2) * 255 + .5);
        fout_image[idx] = fr;
        fout_image[idx + 1] = fg;
        fout_image[idx + 2] = fb;
    }
    // image_pfm::save_image layout (image.h:89-118); path used as given (no $HOME prefix)
    void save_pfm(const std::string &path) const
    {
        std::vector<float> f(fout_image.begin(), fout_image.end());
        check(frt_write_pfm(path.c_str(), nx, ny, f.data()), "frt_write_pfm");
    }
    // image::save_image of out_image (image.cpp:24-58): FRT_IMAGE_PNG / _BMP / _JPG (BMP bytes, as the
    // reference's switch writes); path used as given, extension appended when missing
    void save_image(const std::string &path, int format = FRT_IMAGE_PNG) const
    {
        check(frt_write_image(path.c_str(), nx, ny, out_image.data(), format), "frt_write_image");
    }
    // a whole mean film at once (the GPU path): linear film + display bytes (frt_tonemap_u8)
    void store_film(const float *rgb)
    {
        for (size_t i = 0; i < fout_image.size(); ++i) fout_image[i] = rgb[i];
        check(frt_tonemap_u8(rgb, nx, ny, out_image.data()), "frt_tonemap_u8");
    }
    const int nx, ny;
    const uint64_t ns;
    const int num_channels;
    bool to_exit = false;
    std::vector<uint8_t> out_image;
    std::vector<double> fout_image;
};

// One frt_ctx per listed device with the scene uploaded and the environment
// image (if any) set (uploads run in parallel, one host thread per device).
class device_set {
public:
    device_set(const std::vector<int> &devices, const frt_scene_view &view, const frt_image *env_map = nullptr)
        : ctx_(devices.size(), nullptr)
    {
        std::vector<std::string> errs(devices.size());
        auto up = [&](size_t i) {
            try {
                check(frt_create(devices[i], &ctx_[i]), "frt_create");
                check(frt_upload_scene(ctx_[i], &view), "frt_upload_scene", ctx_[i]);
                if (env_map) check(frt_set_env_image(ctx_[i], env_map), "frt_set_env_image", ctx_[i]);
            } catch (const std::exception &e) {
                errs[i] = e.what();
            }
        };
        std::vector<std::thread> th;
        for (size_t i = 1; i < devices.size(); ++i) th.emplace_back(up, i);
        if (!devices.empty()) up(0);
        for (auto &t : th) t.join();
        for (const std::string &e : errs)
            if (!e.empty()) { release(); throw frt::error(FRT_E_HIP, e); }
    }
    ~device_set() { release(); }
    device_set(const device_set &) = delete;
    device_set &operator=(const device_set &) = delete;
    frt_ctx **data() { return ctx_.data(); }
    int size() const { return (int)ctx_.size(); }
    // FRT_INTEGRATOR_DENOISE (frt.h) on the first context: filters the finished nx x ny colour
    // film (finite, >= 0; from path, accumulated passes or pssmlt) in place, guided by spp-sample
    // normals, albedo and depth renders of the uploaded scene.  Returns the call's stats.
    frt_stats denoise(float *film_rgb, int nx, int ny, int spp = 16, uint32_t seed = 0, int tile_size = 32,
                      int flags = 0)
    {
        if (ctx_.empty()) throw frt::error(FRT_E_INVALID, "denoise: no device");
        frt_render_params p{};
        p.nx = nx; p.ny = ny; p.spp = spp; p.seed = seed; p.tile_size = tile_size; p.flags = flags;
        p.integrator = FRT_INTEGRATOR_DENOISE; p.shard_index = 0; p.shard_count = 1;
        frt_stats st{};
        check(frt_render(ctx_[0], &p, film_rgb, &st), "frt_render(denoise)", ctx_[0]);
        return st;
    }
    // FRT_INTEGRATOR_ERROR (frt.h): the variance film V (nx x ny x 3, pixel order) of the film that
    // the last frt_render_multi of these contexts with `p` produced -- per pixel and channel the
    // batch-means estimate of the variance of the mean; sqrt(V) is the standard error.  No ray is
    // traced; each context reduces the chunk sums of its own shard.  Returns the call's stats.
    frt_stats error(frt_render_params p, float *v_rgb)
    {
        if (ctx_.empty()) throw frt::error(FRT_E_INVALID, "error: no device");
        p.integrator = FRT_INTEGRATOR_ERROR; p.shard_index = 0; p.shard_count = 1;
        frt_stats st{};
        check(frt_render_multi(ctx_.data(), size(), &p, v_rgb, &st), "frt_render_multi(error)", ctx_[0]);
        return st;
    }

private:
    void release()
    {
        for (frt_ctx *&c : ctx_)
            if (c) { frt_destroy(c); c = nullptr; }
    }
    std::vector<frt_ctx *> ctx_;
};

// tile_gpu<I>: the drop-ins for the per-pixel integrators -- path_gpu for
// `path` (path.h:8-18), ao_gpu for `ao` (ao.h:8-43), normals_gpu for
// `normals_renderer` (debug_renderer.h:6-50).  Render() renders the frame on
// the listed GPUs with frt_render_multi (tile t -> device t % n) and stores
// the per-pixel means in the viewer.
template <int INTEGRATOR>
struct tile_gpu {
    std::vector<int> devices{0};
    uint32_t seed = 0;
    int max_depth = 33;     // path.cpp:36
    int tile_size = 32;
    // path with an environment image (Scene::set_env_map): also sample the image at every
    // diffuse or rough vertex (FRT_FLAG_ENV_SAMPLING, frt.h) -- not the reference's estimator,
    // the same expectation with far less noise under a sun or a window; off by default
    bool env_sampling = false;
    // path: Russian roulette from the fourth vertex on (FRT_FLAG_ROULETTE, frt.h) -- not in the
    // reference; the same expectation with fewer rays per sample in closed scenes; off by
    // default, on every device of `devices` when set; ao and normals ignore it
    bool roulette = false;
    // path: Owen-scrambled Sobol' sample points instead of independent hashes (FRT_FLAG_SOBOL,
    // frt.h) -- not in the reference; the same expectation with less noise per sample; off by
    // default, on every device of `devices` when set; ao and normals ignore it
    bool sobol = false;
    // keep the contexts of the last Render() until the next one (off: they are released when
    // Render() returns, as before): error() needs the chunk sums they hold
    bool keep_devices = false;
    frt_stats last_stats{};
    static constexpr bool using_custom_viewer = false;

    // the whole-frame request of an nx x ny render with spp samples under this integrator's switches
    frt_render_params params(int nx, int ny, int spp) const
    {
        frt_render_params p{};
        p.nx = nx; p.ny = ny; p.spp = spp; p.seed = seed;
        p.max_depth = max_depth; p.integrator = INTEGRATOR; p.tile_size = tile_size;
        p.shard_index = 0; p.shard_count = 1;
        if (env_sampling) p.flags |= FRT_FLAG_ENV_SAMPLING;
        if (roulette) p.flags |= FRT_FLAG_ROULETTE;
        if (sobol) p.flags |= FRT_FLAG_SOBOL;
        return p;
    }

    void Render(Scene *scene, viewer *film)
    {
        kept_.reset();
        std::unique_ptr<device_set> owned(new device_set(devices, scene->view(), scene->env_map()));
        device_set &gpus = *owned;
        const frt_render_params p = params(film->nx, film->ny, (int)film->ns);
        std::vector<float> rgb((size_t)film->nx * film->ny * 3, 0.0f);
        check(frt_render_multi(gpus.data(), gpus.size(), &p, rgb.data(), &last_stats), "frt_render_multi",
              gpus.data()[0]);
        if (keep_devices) { kept_ = std::move(owned); kept_params_ = p; }
        for (int y = 0; y < film->ny; ++y)
            for (int x = 0; x < film->nx; ++x) {
                const float *px = &rgb[3 * ((size_t)y * film->nx + x)];
                film->store_mean(x, y, px[0], px[1], px[2]);
            }
    }
    // The variance film of the last Render() (FRT_INTEGRATOR_ERROR, device_set::error): nx x ny x 3
    // floats in the film's order.  Needs keep_devices = true before that Render().
    std::vector<float> error()
    {
        if (!kept_) throw frt::error(FRT_E_INVALID, "error(): set keep_devices before Render()");
        std::vector<float> v((size_t)kept_params_.nx * kept_params_.ny * 3, 0.0f);
        kept_->error(kept_params_, v.data());
        return v;
    }

private:
    std::unique_ptr<device_set> kept_;
    frt_render_params kept_params_{};
};

using path_gpu = tile_gpu<FRT_INTEGRATOR_PATH>;
using ao_gpu = tile_gpu<FRT_INTEGRATOR_AO>;
using normals_gpu = tile_gpu<FRT_INTEGRATOR_NORMALS>;
// the first-hit feature images (not in the reference; frt.h): reflectance colour, and
// (depth x coverage, its second moment, coverage); max_depth and the estimator switches do nothing
using albedo_gpu = tile_gpu<FRT_INTEGRATOR_ALBEDO>;
using depth_gpu = tile_gpu<FRT_INTEGRATOR_DEPTH>;

// pssmlt_gpu: the drop-in for `pssmlt` (pssmlt.h:20-76) -- Kelemen PSS-MLT with
// film->ns mutations per pixel over `chains` GPU chains (chain c -> device
// c % n).  The splat film is the image (AccumulatePathContribution).
struct pssmlt_gpu {
    std::vector<int> devices{0};
    uint32_t seed = 0;
    int chains = 1 << 18;
    int bootstrap = 10000;  // pssmlt.cpp:303
    frt_stats last_stats{};
    static constexpr bool using_custom_viewer = false;

    void Render(Scene *scene, viewer *film)
    {
        device_set gpus(devices, scene->view(), scene->env_map());
        frt_render_params p{};
        p.nx = film->nx; p.ny = film->ny; p.spp = (int)film->ns; p.seed = seed;
        p.max_depth = 10; p.integrator = FRT_INTEGRATOR_PSSMLT; p.tile_size = 32;
        p.shard_index = 0; p.shard_count = 1; p.mlt_chains = chains; p.mlt_bootstrap = bootstrap;
        std::vector<float> rgb((size_t)film->nx * film->ny * 3, 0.0f);
        check(frt_render_multi(gpus.data(), gpus.size(), &p, rgb.data(), &last_stats), "frt_render_multi",
              gpus.data()[0]);
        for (int y = 0; y < film->ny; ++y)
            for (int x = 0; x < film->nx; ++x) {
                const float *px = &rgb[3 * ((size_t)y * film->nx + x)];
                film->store_mean(x, y, px[0], px[1], px[2]);
            }
    }
};

// ---- render until converged (not in the reference, whose ns is a compile-time guess) ----
// The frame figure e = sqrt(mean V) / mean film, both means over all n = 3 nx ny values: the
// predicted RMSE of the film over its mean.  (The binding's frame_error adds the same values in
// numpy's pairwise order: the two agree to rounding, not bit for bit; the films do.)
inline double frame_error(const float *film, const float *v, size_t n)
{
    double sf = 0.0, sv = 0.0;
    for (size_t i = 0; i < n; ++i) { sf += (double)film[i]; sv += (double)v[i]; }
    return std::sqrt(sv / (double)n) / (sf / (double)n);
}
// V of the mean of a + b samples from the V of the first a (in place) and of the other b, the
// passes independent: (a^2 Va + b^2 Vb) / (a + b)^2 in double, stored as float
inline void combine_variance(float *v, long a, const float *vp, long b, size_t n)
{
    const double da = (double)a, db = (double)b;
    const double wa = da * da, wb = db * db, tot = (da + db) * (da + db);
    for (size_t i = 0; i < n; ++i) v[i] = (float)((wa * (double)v[i] + wb * (double)vp[i]) / tot);
}
// four replicate films -> their mean (through frt_film_accumulate, one replicate at a time) and
// V = the sample variance of the four replicate means / 4
inline void replicate_variance(const std::vector<float> r[4], std::vector<float> &mean, std::vector<float> &v)
{
    const size_t n = r[0].size();
    mean = r[0];
    for (int k = 1; k < 4; ++k) check(frt_film_accumulate(mean.data(), k, r[k].data(), 1, (int64_t)n), "frt_film_accumulate");
    v.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const double a = r[0][i], b = r[1][i], c = r[2][i], d = r[3][i];
        const double m = (((a + b) + c) + d) * 0.25;
        v[i] = (float)(((((a - m) * (a - m) + (b - m) * (b - m)) + (c - m) * (c - m)) + (d - m) * (d - m)) / 12.0);
    }
}

struct until_pass {
    long long samples = 0;   // over the frame, after the pass
    double e = 0.0, ms = 0.0;
    long sampled = 0;        // pixels the pass sampled
    bool sparse = false;     // through frtx_render_pixels
};
struct until_result {
    std::vector<float> film, variance;   // nx x ny x 3 each, the film's order
    long spp_used = 0;                   // adaptive: the largest count of a pixel
    double e = 0.0;
    bool converged = false;
    std::vector<int32_t> counts;         // adaptive: samples per pixel, nx x ny
    std::vector<until_pass> passes;      // adaptive
};

// frtx_render_pixels (frt.h) on one context: the listed pixels' means and, with `variance`, their V
inline frt_stats render_pixels(frt_ctx *ctx, const frt_render_params &p, const std::vector<int32_t> &pixels,
                               std::vector<float> &rgb, std::vector<float> *variance = nullptr)
{
    rgb.assign(pixels.size() * 3, 0.0f);
    if (variance) variance->assign(pixels.size() * 3, 0.0f);
    frt_stats st{};
    check(frtx_render_pixels(ctx, &p, pixels.data(), (int64_t)pixels.size(), rgb.data(), variance ? variance->data() : nullptr, &st),
          "frtx_render_pixels", ctx);
    return st;
}

// frtx_radiance_rays (frt.h) on one context: the mean radiance along each of the n first rays
// (records of 8 floats: origin, t_max, direction, RNG stream id as uint32 bits; host memory) through
// the library's path or ao integrator, and with `var` their V.  rgb, var: n x 3 floats.
inline frt_stats radiance_rays(frt_ctx *ctx, const frt_render_params &p, const float *rays, int64_t n, float *rgb,
                               float *var = nullptr)
{
    frt_stats st{};
    check(frtx_radiance_rays(ctx, &p, rays, n, rgb, var, &st), "frtx_radiance_rays", ctx);
    return st;
}
// frtx_camera_rays_device (frt.h): the scene camera's first rays of the listed pixels at sample
// p.sample_offset, as records for radiance_rays.  pixels and rays_out (npix x 8 floats) are device
// memory; hip_stream NULL: the context's.
inline void camera_rays(frt_ctx *ctx, const frt_render_params &p, const int32_t *pixels, int64_t npix, float *rays_out,
                        void *hip_stream = nullptr)
{
    check(frtx_camera_rays_device(ctx, &p, pixels, npix, rays_out, hip_stream), "frtx_camera_rays_device", ctx);
}
// Ray records of a lat-long probe around `origin` in the environment image's convention
// (frt_set_env_image: phi = atan2(d.x, -d.z), theta = acos(d.y), row 0 = the +y pole), nx x ny texels
// in row-major order, each ray through (jx, jy) in [0, 1)^2 of its texel (0.5, 0.5: the centre);
// streams 0 .. nx ny - 1.  The binding's cameras.latlong.
inline std::vector<float> latlong_rays(const double origin[3], int nx, int ny, double jx = 0.5, double jy = 0.5)
{
    std::vector<float> rays((size_t)nx * ny * 8);
    const double pi = 3.14159265358979323846;
    for (int r = 0; r < ny; ++r)
        for (int c = 0; c < nx; ++c) {
            const double phi = 2.0 * pi * (c + jx) / nx, theta = pi * (r + jy) / ny, st = std::sin(theta);
            const uint32_t id = (uint32_t)(r * nx + c);
            float *q = &rays[8 * (size_t)id];
            q[0] = (float)origin[0]; q[1] = (float)origin[1]; q[2] = (float)origin[2]; q[3] = 3.40282347e+38f;
            q[4] = (float)(st * std::sin(phi)); q[5] = (float)std::cos(theta); q[6] = (float)(-st * std::cos(phi));
            std::memcpy(&q[7], &id, sizeof(id));
        }
    return rays;
}

// Precomputed radiance transfer (frt.h "precomputed radiance transfer"; the reference's path_prt).
// sh_project: li[25][3] of an environment image, or (img NULL) of a constant colour.
inline std::vector<double> sh_project(const frt_image *img, const double env_color[3] = nullptr)
{
    std::vector<double> li(75);
    check(frtx_sh_project_image(img, env_color, li.data()), "frtx_sh_project_image");
    return li;
}
// sqrt_n^2 stratified unit directions (3 floats each) for prt_transfer
inline std::vector<float> prt_sample_dirs(int sqrt_n, uint32_t seed = 0)
{
    std::vector<float> dirs((size_t)(sqrt_n > 0 ? sqrt_n : 1) * (size_t)(sqrt_n > 0 ? sqrt_n : 1) * 3);
    check(frtx_prt_sample_dirs(sqrt_n, seed, dirs.data()), "frtx_prt_sample_dirs");
    return dirs;
}
// frtx_prt_transfer on one context: T[n_tris][3][25][3] of the uploaded scene, whose view is passed again
inline frt_stats prt_transfer(frt_ctx *ctx, const frt_scene_view &scene, const std::vector<float> &dirs, int bounces, int flags,
                              std::vector<float> &T)
{
    T.assign((size_t)scene.n_tris * 3 * 75, 0.0f);
    frt_stats st{};
    check(frtx_prt_transfer(ctx, &scene, dirs.data(), (int64_t)(dirs.size() / 3), bounces, flags, T.data(), &st), "frtx_prt_transfer", ctx);
    return st;
}
// frtx_prt_rays on one context: rgb (n x 3 floats) of n ray records (host memory) under li (sh_project)
inline frt_stats prt_rays(frt_ctx *ctx, const std::vector<float> &T, const std::vector<double> &li, const float *rays, int64_t n,
                          float *rgb)
{
    float l[75];
    for (int k = 0; k < 75; ++k) l[k] = (float)li.at((size_t)k);
    frt_stats st{};
    check(frtx_prt_rays(ctx, T.data(), l, rays, n, rgb, &st), "frtx_prt_rays", ctx);
    return st;
}

// frtx_prt_render on one context: the nx x ny frame of `p` through the scene's camera, p.spp samples
inline frt_stats prt_render(frt_ctx *ctx, const frt_render_params &p, const std::vector<float> &T, const std::vector<double> &li,
                            float *film)
{
    float l[75];
    for (int k = 0; k < 75; ++k) l[k] = (float)li.at((size_t)k);
    frt_stats st{};
    check(frtx_prt_render(ctx, &p, T.data(), l, film, &st), "frtx_prt_render", ctx);
    return st;
}

// The active share of the frame below which an adaptive pass goes through frtx_render_pixels: the
// full render's time over the sparse kernel's for the same pixels and samples, rounded down to one
// decimal (1080p, 64 spp, one MI355X: profiles/adaptive/switch.json).  The binding's ADAPTIVE_SWITCH.
constexpr double kAdaptiveSwitch = 0.5;
// The first pass of an adaptive run when the caller names none (first_spp = 0): the smallest power
// of two at which the run's sum of mean V stays inside the calibration window of the sum of the
// actual squared error (profiles/adaptive/calibration.json).  The binding's ADAPTIVE_FIRST_SPP.
constexpr int kAdaptiveFirstSpp = 128;

// Progressive render of the whole-frame request `p` (path or ao; spp and sample_offset are the
// driver's) on `gpus` until e <= target or the next pass would exceed max_spp.  Pass 0 renders
// first_spp samples (a power of two >= 2), each later pass as many as there are so far
// (sample_offset = the total so far); the film is accumulated with frt_film_accumulate and V, the
// ERROR film of each pass, with combine_variance.  A pass that the library cut into one chunk a
// pixel (work_items == the slot count; the granule depends on the device, so it is seen only
// after the render) is rendered again with samples_per_item = half the pass -- that pass is paid
// twice -- and every later pass asks for half-pass granules up front.
// FRT_FLAG_SOBOL: four replicates, seeds seed .. seed + 3, each extended by the same passes (so
// each stays a prefix net); film and V from replicate_variance, spp_used counts all four, and the
// ERROR integrator is not called.  on_pass(total spp, e, kernel ms of the pass) after every pass.
// The loop of the Python binding's Context.render_until, film for film.
//
// adaptive: after every pass tau = target x the film's mean (its values added one after the other
// in double), and a pixel is active while the mean of its three V exceeds tau^2.  A later pass
// gives every active pixel as many samples as it has (n for the most-sampled one), from the first
// sample index not yet handed out: through frtx_render_pixels on the first context when their share
// of the frame is below switch_share, else through the full render of n samples, after which
// every pixel holds the new samples.  Per pixel the
// film merges as frt_film_accumulate and V as combine_variance with that pixel's own count.  The
// loop ends when no pixel is active (then e <= target) or when the next pass would take an active
// pixel past max_spp.  Stopping a pixel on its own V biases it a little.
// FRT_FLAG_SOBOL is refused.  The binding's render_until(adaptive=True), film for film.
inline until_result render_until_adaptive(device_set &gpus, frt_render_params p, double target, long max_spp, int first_spp,
                                          double switch_share, const std::function<void(long, double, double)> &on_pass);
inline until_result render_until(device_set &gpus, frt_render_params p, double target, long max_spp, int first_spp = 0,
                                 const std::function<void(long, double, double)> &on_pass = nullptr, bool adaptive = false,
                                 double switch_share = kAdaptiveSwitch)
{
    if (first_spp == 0) first_spp = adaptive ? kAdaptiveFirstSpp : 16;
    if (first_spp < 2 || (first_spp & (first_spp - 1))) throw error(FRT_E_INVALID, "render_until: first_spp must be a power of two >= 2");
    if (p.integrator != FRT_INTEGRATOR_PATH && p.integrator != FRT_INTEGRATOR_AO)
        throw error(FRT_E_INVALID, "render_until: path and ao renders only (pssmlt has no error estimate, denoise is a filter)");
    if (!(target > 0.0)) throw error(FRT_E_INVALID, "render_until: target must be > 0");
    const bool sobol = (p.flags & FRT_FLAG_SOBOL) && p.integrator == FRT_INTEGRATOR_PATH;
    const int reps = sobol ? 4 : 1;
    if (max_spp < (long)reps * first_spp) throw error(FRT_E_INVALID, "render_until: max_spp is below the first pass");
    p.shard_index = 0; p.shard_count = 1;
    const int64_t slots = frt_shard_slot_count(&p);
    if (slots < 0) throw error(FRT_E_INVALID, "render_until: bad render params");
    if (adaptive) {
        if (sobol)
            throw error(FRT_E_INVALID, "render_until: adaptive with FRT_FLAG_SOBOL is refused -- V is an upper estimate under "
                                       "Sobol' points and the replicates give no per-pixel error; render without the flag");
        return render_until_adaptive(gpus, p, target, max_spp, first_spp, switch_share, on_pass);
    }
    const size_t n3 = (size_t)p.nx * p.ny * 3;
    std::vector<float> films[4], pass(n3), vp(n3);
    until_result R;
    long total = 0;
    bool halve = false;   // a pass came out as one chunk: the later ones ask for two
    for (;;) {
        const long n = total == 0 ? first_spp : total;
        double ms = 0.0;
        for (int k = 0; k < reps; ++k) {
            frt_render_params q = p;
            q.spp = (int)n; q.sample_offset = (int)total; q.seed = p.seed + (uint32_t)k;
            if (halve) q.samples_per_item = (int)(n / 2);
            frt_stats st{};
            check(frt_render_multi(gpus.data(), gpus.size(), &q, pass.data(), &st), "frt_render_multi", gpus.data()[0]);
            if (!sobol && st.work_items == (uint64_t)slots) {   // one chunk a pixel
                halve = true;
                q.samples_per_item = (int)(n / 2);
                check(frt_render_multi(gpus.data(), gpus.size(), &q, pass.data(), &st), "frt_render_multi", gpus.data()[0]);
            }
            ms += st.kernel_ms;
            if (!sobol) {
                gpus.error(q, vp.data());
                if (total == 0) R.variance = vp;
                else combine_variance(R.variance.data(), total, vp.data(), n, n3);
            }
            if (total == 0) films[k] = pass;
            else check(frt_film_accumulate(films[k].data(), total, pass.data(), n, (int64_t)n3), "frt_film_accumulate");
        }
        total += n;
        if (sobol) replicate_variance(films, R.film, R.variance);
        R.spp_used = reps * total;
        const std::vector<float> &film = sobol ? R.film : films[0];
        R.e = frame_error(film.data(), R.variance.data(), n3);
        if (on_pass) on_pass(R.spp_used, R.e, ms);
        R.converged = R.e <= target;
        if (R.converged || 2 * R.spp_used > max_spp) break;
    }
    if (!sobol) R.film = films[0];
    return R;
}

inline until_result render_until_adaptive(device_set &gpus, frt_render_params p, double target, long max_spp, int first_spp,
                                          double switch_share, const std::function<void(long, double, double)> &on_pass)
{
    const int64_t slots = frt_shard_slot_count(&p);
    const size_t npx = (size_t)p.nx * p.ny, n3 = npx * 3;
    until_result R;
    std::vector<float> pass(n3), vp(n3), rgb, var;
    std::vector<int64_t> counts(npx, first_spp);
    bool halve = false;
    auto full_pass = [&](long n, long offset) -> double {   // pass, vp <- the frame's n samples from `offset` and their V
        frt_render_params q = p;
        q.spp = (int)n; q.sample_offset = (int)offset;
        if (halve) q.samples_per_item = (int)(n / 2);
        frt_stats st{};
        check(frt_render_multi(gpus.data(), gpus.size(), &q, pass.data(), &st), "frt_render_multi", gpus.data()[0]);
        if (st.work_items == (uint64_t)slots) {   // one chunk a pixel
            halve = true;
            q.samples_per_item = (int)(n / 2);
            check(frt_render_multi(gpus.data(), gpus.size(), &q, pass.data(), &st), "frt_render_multi", gpus.data()[0]);
        }
        gpus.error(q, vp.data());
        return st.kernel_ms;
    };
    // pixel i of the film <- its count's mean with n more samples (3 values each)
    auto merge = [&](size_t i, const float *c3, const float *v3, long n) {
        check(frt_film_accumulate(&R.film[3 * i], counts[i], c3, n, 3), "frt_film_accumulate");
        combine_variance(&R.variance[3 * i], (long)counts[i], v3, n, 3);
        counts[i] += n;
    };
    double ms = full_pass(first_spp, 0);
    R.film = pass;
    R.variance = vp;
    long offset = first_spp;   // samples [0, offset) of a pixel's stream are handed out
    long sampled = (long)npx;
    bool sparse = false;
    std::vector<int32_t> active;
    for (;;) {
        double sf = 0.0;
        for (size_t i = 0; i < n3; ++i) sf += (double)R.film[i];
        const double tau = target * (sf / (double)n3);
        const double tau2 = tau * tau;
        active.clear();
        int64_t cmax = 0;
        long long total = 0;
        for (size_t i = 0; i < npx; ++i) {
            const double m = (((double)R.variance[3 * i] + (double)R.variance[3 * i + 1]) + (double)R.variance[3 * i + 2]) / 3.0;
            if (m > tau2) { active.push_back((int32_t)i); cmax = std::max(cmax, counts[i]); }
            total += counts[i];
        }
        R.e = frame_error(R.film.data(), R.variance.data(), n3);
        R.passes.push_back(until_pass{total, R.e, ms, sampled, sparse});
        R.spp_used = (long)*std::max_element(counts.begin(), counts.end());
        if (on_pass) on_pass(R.spp_used, R.e, ms);
        R.converged = active.empty();
        const long n = (long)cmax;   // the pass to come doubles the active pixels
        if (R.converged || 2 * n > max_spp) break;
        sparse = (double)active.size() < switch_share * (double)npx;
        if (sparse) {
            // one call per count among the active pixels (ascending), each doubling its group: after
            // sparse passes alone that is one call with sample_offset = spp = n
            std::vector<int64_t> before, cs;
            for (int32_t i : active) before.push_back(counts[(size_t)i]);
            cs = before;
            std::sort(cs.begin(), cs.end());
            cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
            ms = 0.0;
            std::vector<int32_t> group;
            for (int64_t c : cs) {
                group.clear();
                for (size_t k = 0; k < active.size(); ++k)
                    if (before[k] == c) group.push_back(active[k]);
                frt_render_params q = p;
                q.spp = (int)c; q.sample_offset = (int)offset; q.samples_per_item = 0;
                ms += render_pixels(gpus.data()[0], q, group, rgb, &var).kernel_ms;
                for (size_t k = 0; k < group.size(); ++k) merge((size_t)group[k], &rgb[3 * k], &var[3 * k], (long)c);
            }
            sampled = (long)active.size();
        } else {
            ms = full_pass(n, offset);
            for (size_t i = 0; i < npx; ++i) merge(i, &pass[3 * i], &vp[3 * i], n);
            sampled = (long)npx;
        }
        offset += n;
    }
    R.counts.assign(counts.begin(), counts.end());
    return R;
}

// renderer<I> (integrator.h:11-47): time I::Render, print the statistics the
// reference prints -- with true 64-bit ray counts instead of node visits.
template <typename integrator>
struct renderer : public integrator {
    double Render(Scene *scene, viewer &film)
    {
        const auto t1 = std::chrono::high_resolution_clock::now();
        integrator::Render(scene, &film);
        const auto t2 = std::chrono::high_resolution_clock::now();
        const double secs = std::chrono::duration<double>(t2 - t1).count();
        const frt_stats &s = integrator::last_stats;
        const double rays = double(s.camera_rays + s.extension_rays + s.shadow_rays);
        std::printf("\nIt took me %g seconds to render.\n", secs);
        std::printf(" Camera rays: %llu\n Extension rays: %llu\n Shadow rays: %llu\n",
                    (unsigned long long)s.camera_rays, (unsigned long long)s.extension_rays,
                    (unsigned long long)s.shadow_rays);
        std::printf(" Kernel time: %.3f ms\n Rays/second: %.1fM/sec (kernel %.1fM/sec)\n", s.kernel_ms,
                    rays / secs / 1e6, rays / (s.kernel_ms * 1e-3) / 1e6);
        return secs;
    }
};

}  // namespace frt
