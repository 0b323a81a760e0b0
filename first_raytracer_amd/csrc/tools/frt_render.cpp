// frt_render -- command-line renderer: the reference's main() (main.cpp:483-525)
// with the scene, resolution, spp, seed and GPU count as flags instead of
// compile-time choices.  Writes the linear film as PFM (image.h:89-118).
//
//   frt_render --scene cornell|veach|obj --obj FILE [--res 1920x1080] [--ns 512]
//              [--seed 0] [--gpus 1] [--integrator path|pssmlt|ao|normals|albedo|depth|prt] [--chains 262144]
//              [--prt-dirs 32] [--prt-bounces 1] [--prt-unshadowed]
//              [--denoise [--denoise-spp 16]]
//              [--error-out v.pfm] [--target-error E --max-spp N [--first-spp 16] [--adaptive [--switch S]]]
//              [--env r,g,b | --env-map file.hdr [--env-sampling]] [--roulette] [--sobol] [--out out.pfm] [--png out.png] [--bvh reference|sah]
//              [--camera latlong [--cam-origin x,y,z] [--cam-passes K]]
//
// --integrator pssmlt: renderer<pssmlt_gpu>, --ns = mutations per pixel.
// --integrator ao / normals: renderer<ao_gpu> / renderer<normals_gpu> (ao.h, debug_renderer.h).
// --integrator albedo / depth: the first-hit feature images (FRT_INTEGRATOR_ALBEDO / _DEPTH, frt.h):
//   reflectance colour; (depth x coverage, its second moment, coverage).
// --integrator prt: precomputed radiance transfer (frt.h) in one run on the first GPU: the
//   transfer of the scene over --prt-dirs^2 stratified directions (seeded by --seed) with --prt-bounces
//   interreflections (--prt-unshadowed: bounce 0 without visibility rays), the projection of the
//   environment (--env-map, or the constant --env / the scene's colour), then the frame through the
//   scene's camera with --ns samples a pixel; prints the precompute's kernel ms and rays.
// --denoise: after the last pass of a path or pssmlt render, filter the film (FRT_INTEGRATOR_DENOISE:
//   an a-trous wavelet filter guided by --denoise-spp samples of normals, albedo and depth, on the
//   first GPU) before --out / --png are written; prints the feature and filter times.
// --error-out: also the variance film V of the render just done (FRT_INTEGRATOR_ERROR, frt.h: per
//   pixel and channel the batch-means estimate of the variance of the mean), as PFM, and the frame
//   figure e = sqrt(mean V) / mean film, the predicted RMSE over the mean; path and ao.
// --target-error E --max-spp N: frt::render_until -- passes of --first-spp, then doubling, until
//   e <= E or the next pass would exceed N samples per pixel; --ns is ignored; one line per pass
//   with the total spp, e and the pass's kernel ms.  With --sobol four replicates give the error.
// --adaptive (with --target-error): later passes sample only the pixels whose own error is above the
//   target (frt::render_until's adaptive rule), through frtx_render_pixels on the first GPU when their
//   share of the frame is below --switch (default frt::kAdaptiveSwitch); --first-spp defaults to
//   frt::kAdaptiveFirstSpp there; one line per pass with the
//   samples over the frame, the pixels sampled and how; --counts-out writes the samples per pixel as
//   PFM.  Not with --sobol.
// --camera latlong: instead of the scene camera's frame, a lat-long light probe from that camera's
//   origin, or from --cam-origin (frtx_radiance_rays over frt::latlong_rays, on the first GPU; path or ao): --res texels,
//   --ns samples a texel and pass, written upright -- the +y pole is the top row as viewed -- so the
//   image read back row by row from the top is an environment image for --env-map's convention.
//   --cam-passes K: K passes at sample offsets k * ns, each through another point of the texels
//   (hashed from the seed and k; one pass: the centres), averaged by frt_film_accumulate's rule.
// --env: constant environment colour (the reference scenes' is black).
// --env-map: a Radiance .hdr lat-long image as the environment (Scene::env_map over an
//   image_texture, material.h:206-244); exclusive with --env.
// --env-sampling: path also samples that image at diffuse and rough vertices
//   (FRT_FLAG_ENV_SAMPLING: the same expectation, far less noise under a sun or a
//   window); needs --env-map, and the path integrator (ao / normals have no light
//   sampling, pssmlt keeps the reference's sample layout).
// --roulette: path plays Russian roulette from the fourth vertex on (FRT_FLAG_ROULETTE:
//   the same expectation, fewer rays per sample in closed scenes); the path integrator only.
// --sobol: path draws its sample points from Owen-scrambled Sobol' pairs (FRT_FLAG_SOBOL: the
//   same expectation, less noise per sample); the path integrator only.
// --png: also the tonemapped display image (viewer::add_sample bytes, image::save_image).
// --bvh sah: rebuild the scene's BVH with the binned SAH builder (faster traversal;
//   exact-t ties then follow that tree's order instead of create_bvh's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frt_integrator.hpp"

int main(int argc, char **argv)
{
    std::string scene = "cornell", obj, out = "out.pfm", integrator = "path", png, bvh = "reference", env_map;
    int nx = 512, ny = 512, gpus = 1, chains = 1 << 18;
    long ns = 100;
    unsigned seed = 0;
    double env[3] = {0, 0, 0};
    bool has_env = false, env_sampling = false, roulette = false, sobol = false, denoise = false;
    int denoise_spp = 16;
    std::string error_out;
    double target_error = 0.0;
    long max_spp = 0;
    int first_spp = 16;
    bool has_target = false, has_max_spp = false, has_first_spp = false, adaptive = false;
    double switch_share = frt::kAdaptiveSwitch;
    std::string counts_out, camera;
    int cam_passes = 1;
    double cam_origin[3] = {0, 0, 0};
    bool has_cam_origin = false;
    int prt_dirs = 32, prt_bounces = 1;
    bool prt_unshadowed = false, has_prt_flag = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); }
            return argv[++i];
        };
        if (a == "--scene") scene = next();
        else if (a == "--obj") obj = next();
        else if (a == "--res") { if (std::sscanf(next(), "%dx%d", &nx, &ny) != 2) return 2; }
        else if (a == "--ns") ns = std::atol(next());
        else if (a == "--seed") seed = (unsigned)std::strtoul(next(), nullptr, 10);
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--out") out = next();
        else if (a == "--png") png = next();
        else if (a == "--bvh") bvh = next();
        else if (a == "--integrator") integrator = next();
        else if (a == "--chains") chains = std::atoi(next());
        else if (a == "--env") {
            if (std::sscanf(next(), "%lf,%lf,%lf", &env[0], &env[1], &env[2]) != 3) return 2;
            has_env = true;
        }
        else if (a == "--env-map") env_map = next();
        else if (a == "--env-sampling") env_sampling = true;
        else if (a == "--roulette") roulette = true;
        else if (a == "--sobol") sobol = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-spp") denoise_spp = std::atoi(next());
        else if (a == "--error-out") error_out = next();
        else if (a == "--target-error") { target_error = std::atof(next()); has_target = true; }
        else if (a == "--max-spp") { max_spp = std::atol(next()); has_max_spp = true; }
        else if (a == "--first-spp") { first_spp = std::atoi(next()); has_first_spp = true; }
        else if (a == "--adaptive") adaptive = true;
        else if (a == "--switch") switch_share = std::atof(next());
        else if (a == "--counts-out") counts_out = next();
        else if (a == "--camera") camera = next();
        else if (a == "--cam-passes") cam_passes = std::atoi(next());
        else if (a == "--cam-origin") {
            if (std::sscanf(next(), "%lf,%lf,%lf", &cam_origin[0], &cam_origin[1], &cam_origin[2]) != 3) return 2;
            has_cam_origin = true;
        }
        else if (a == "--prt-dirs") { prt_dirs = std::atoi(next()); has_prt_flag = true; }
        else if (a == "--prt-bounces") { prt_bounces = std::atoi(next()); has_prt_flag = true; }
        else if (a == "--prt-unshadowed") { prt_unshadowed = has_prt_flag = true; }
        else { std::fprintf(stderr, "unknown flag %s\n", a.c_str()); return 2; }
    }
    if (obj.empty()) { std::fprintf(stderr, "--obj is required\n"); return 2; }
    if (has_env && !env_map.empty()) { std::fprintf(stderr, "--env and --env-map exclude each other\n"); return 2; }
    if (env_sampling && env_map.empty()) { std::fprintf(stderr, "--env-sampling needs --env-map\n"); return 2; }
    if (env_sampling && integrator != "path") {
        std::fprintf(stderr, "--env-sampling: only --integrator path samples the environment image\n");
        return 2;
    }
    if (roulette && integrator != "path") {
        std::fprintf(stderr, "--roulette: only --integrator path plays Russian roulette\n");
        return 2;
    }
    if (sobol && integrator != "path") {
        std::fprintf(stderr, "--sobol: only --integrator path draws Sobol' sample points\n");
        return 2;
    }
    if (denoise && integrator != "path" && integrator != "pssmlt") {
        std::fprintf(stderr, "--denoise: only a path or pssmlt film is filtered\n");
        return 2;
    }
    if (has_prt_flag && integrator != "prt") { std::fprintf(stderr, "--prt-dirs / --prt-bounces / --prt-unshadowed go with --integrator prt\n"); return 2; }
    if (integrator == "prt" && (prt_dirs < 1 || prt_dirs > 4096 || prt_bounces < 0 || prt_bounces > 16 || ns < 1 || gpus != 1 || denoise ||
                                !camera.empty())) {
        std::fprintf(stderr, "--integrator prt: --prt-dirs in [1, 4096], --prt-bounces in [0, 16], --ns >= 1, one GPU, "
                             "not with --denoise or --camera\n");
        return 2;
    }
    const bool until = has_target;
    if (until && !(target_error > 0.0)) { std::fprintf(stderr, "--target-error must be > 0\n"); return 2; }
    if (!until && (has_max_spp || has_first_spp)) {
        std::fprintf(stderr, "--max-spp / --first-spp go with --target-error\n");
        return 2;
    }
    if ((until || !error_out.empty()) && integrator != "path" && integrator != "ao") {
        std::fprintf(stderr, "--error-out / --target-error: only a path or ao render has an error film\n");
        return 2;
    }
    if (adaptive && !has_first_spp) first_spp = frt::kAdaptiveFirstSpp;
    if (adaptive && !until) { std::fprintf(stderr, "--adaptive goes with --target-error\n"); return 2; }
    if (!counts_out.empty() && !adaptive) { std::fprintf(stderr, "--counts-out goes with --adaptive\n"); return 2; }
    if (adaptive && sobol) {
        std::fprintf(stderr, "--adaptive and --sobol exclude each other (no per-pixel error under Sobol' points)\n");
        return 2;
    }
    if (until && max_spp <= 0) { std::fprintf(stderr, "--target-error needs --max-spp\n"); return 2; }
    if (until && denoise) { std::fprintf(stderr, "--target-error and --denoise exclude each other\n"); return 2; }
    if (!camera.empty() && camera != "latlong") { std::fprintf(stderr, "unknown --camera %s (latlong)\n", camera.c_str()); return 2; }
    if (camera.empty() && (cam_passes != 1 || has_cam_origin)) { std::fprintf(stderr, "--cam-passes / --cam-origin go with --camera\n"); return 2; }
    if (!camera.empty() && (cam_passes < 1 || (integrator != "path" && integrator != "ao") || until || denoise || !error_out.empty())) {
        std::fprintf(stderr, "--camera: a path or ao render of --ns samples and --cam-passes >= 1 passes "
                             "(not with --target-error, --error-out or --denoise)\n");
        return 2;
    }
    try {
        if (until) std::printf("Resolution: %dx%d\nRendering until e <= %g, at most %ld samples\n", nx, ny, target_error, max_spp);
        else std::printf("Resolution: %dx%d\nSetting number of samples to %ld\n", nx, ny, ns);
        const std::string kind = scene == "cornell" ? "cornell_box_obj" : scene == "veach" ? "veach_mis" : "obj_smooth";
        frt::Scene s(kind, obj, double(nx) / double(ny));
        if (has_env) s.set_env(env[0], env[1], env[2]);
        if (!env_map.empty()) s.set_env_map(env_map);
        if (bvh == "sah") s.build_bvh_sah();
        else if (bvh != "reference") { std::fprintf(stderr, "unknown --bvh %s\n", bvh.c_str()); return 2; }
        std::printf("BVH construction took me %g seconds (%d triangles, depth %d).\n", s.info().build_ms * 1e-3,
                    s.info().n_tris, s.info().bvh_depth);
        frt::viewer film(nx, ny, (uint64_t)ns);
        std::vector<float> variance;   // --error-out
        auto report_error = [&](const std::vector<float> &rgb) {
            std::printf("Error film: e = sqrt(mean V) / mean film = %.6g\n", frt::frame_error(rgb.data(), variance.data(), rgb.size()));
        };
        auto run = [&](auto &render) {
            render.devices.clear();
            for (int g = 0; g < gpus; ++g) render.devices.push_back(g);
            render.seed = seed;
            render.Render(&s, film);
        };
        // path, ao: ... with the error film, or until converged
        auto run_error = [&](auto &render) {
            render.devices.clear();
            for (int g = 0; g < gpus; ++g) render.devices.push_back(g);
            render.seed = seed;
            if (until) {
                frt::device_set set(render.devices, s.view(), s.env_map());
                const frt::until_result r = frt::render_until(set, render.params(nx, ny, first_spp), target_error, max_spp, first_spp,
                                                              [](long spp, double e, double ms) {
                                                                  std::printf("pass: %ld spp  e = %.6g  %.3f ms\n", spp, e, ms);
                                                              }, adaptive, switch_share);
                for (const frt::until_pass &ps : r.passes)
                    std::printf("adaptive pass: %lld samples  %ld pixels %s  e = %.6g  %.3f ms\n", ps.samples, ps.sampled,
                                ps.sparse ? "sparse" : "full", ps.e, ps.ms);
                if (!counts_out.empty()) {
                    std::vector<float> cf((size_t)nx * ny * 3);
                    for (size_t i = 0; i < r.counts.size(); ++i) cf[3 * i] = cf[3 * i + 1] = cf[3 * i + 2] = (float)r.counts[i];
                    frt::check(frt_write_pfm(counts_out.c_str(), nx, ny, cf.data()), "frt_write_pfm");
                    std::printf("Saved %s\n", counts_out.c_str());
                }
                std::printf("%s after %ld spp: e = %.6g (target %.6g)\n", r.converged ? "Converged" : "Not converged",
                            r.spp_used, r.e, target_error);
                film.store_film(r.film.data());
                variance = r.variance;
                return;
            }
            render.keep_devices = !error_out.empty();
            render.Render(&s, film);
            if (!error_out.empty()) {
                variance = render.error();
                report_error(std::vector<float>(film.fout_image.begin(), film.fout_image.end()));
            }
        };
        if (!camera.empty()) {   // a lat-long probe from the camera's origin, through frtx_radiance_rays
            frt_render_params p{};
            if (integrator == "path") {
                frt::renderer<frt::path_gpu> render;
                render.seed = seed; render.env_sampling = env_sampling; render.roulette = roulette; render.sobol = sobol;
                p = render.params(nx, ny, (int)ns);
            } else {
                frt::renderer<frt::ao_gpu> render;
                render.seed = seed;
                p = render.params(nx, ny, (int)ns);
            }
            const frt_scene_view view = s.view();
            frt::device_set gpu({0}, view, s.env_map());
            if (!has_cam_origin) std::memcpy(cam_origin, view.cam_origin, sizeof(cam_origin));
            const size_t n = (size_t)nx * ny;
            std::vector<float> acc(n * 3), pass(n * 3);
            double ms = 0.0;
            unsigned long long rays = 0;
            for (int k = 0; k < cam_passes; ++k) {
                double jx = 0.5, jy = 0.5;
                if (cam_passes > 1) {   // a point of the texel hashed from (seed, k)
                    uint64_t h = ((uint64_t)seed << 32 | (uint32_t)k) + 0x9E3779B97F4A7C15ull;
                    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull; h = (h ^ (h >> 27)) * 0x94D049BB133111EBull; h ^= h >> 31;
                    jx = (double)(h >> 40) / (double)(1 << 24); jy = (double)((h >> 8) & 0xffffff) / (double)(1 << 24);
                }
                const std::vector<float> list = frt::latlong_rays(cam_origin, nx, ny, jx, jy);
                p.sample_offset = (int)(k * ns);
                const frt_stats st = frt::radiance_rays(gpu.data()[0], p, list.data(), (int64_t)n, k ? pass.data() : acc.data());
                if (k) frt::check(frt_film_accumulate(acc.data(), (int64_t)k * ns, pass.data(), ns, (int64_t)acc.size()), "frt_film_accumulate");
                ms += st.kernel_ms;
                rays += st.camera_rays + st.extension_rays + st.shadow_rays;
            }
            std::vector<float> up(n * 3);   // the film's row 0 is the bottom one: the probe's row 0 (+y) goes on top
            for (int r = 0; r < ny; ++r) std::memcpy(&up[(size_t)(ny - 1 - r) * nx * 3], &acc[(size_t)r * nx * 3], (size_t)nx * 3 * sizeof(float));
            film.store_film(up.data());
            std::printf("Lat-long probe from (%g, %g, %g): %d passes of %ld samples, %llu rays, %.3f ms on the GPU\n", cam_origin[0],
                        cam_origin[1], cam_origin[2], cam_passes, ns, rays, ms);
        } else if (integrator == "prt") {   // precompute + projection + render, on the first GPU
            frt::renderer<frt::path_gpu> render;
            render.seed = seed;
            const frt_render_params p = render.params(nx, ny, (int)ns);
            const frt_scene_view view = s.view();
            frt::device_set gpu({0}, view, s.env_map());
            std::vector<float> T;
            const frt_stats pre = frt::prt_transfer(gpu.data()[0], view, frt::prt_sample_dirs(prt_dirs, seed), prt_bounces,
                                                    prt_unshadowed ? FRTX_PRT_UNSHADOWED : 0, T);
            std::printf("PRT precompute: %d directions, %d bounces, %llu rays, %.3f ms on the GPU\n", prt_dirs * prt_dirs, prt_bounces,
                        (unsigned long long)(pre.shadow_rays + pre.extension_rays), pre.kernel_ms);
            const std::vector<double> li = frt::sh_project(s.env_map(), view.env_color);
            std::vector<float> rgb((size_t)nx * ny * 3);
            const frt_stats st = frt::prt_render(gpu.data()[0], p, T, li, rgb.data());
            film.store_film(rgb.data());
            std::printf("PRT render: %llu rays, %.3f ms on the GPU\n", (unsigned long long)st.camera_rays, st.kernel_ms);
        } else if (integrator == "pssmlt") {
            frt::renderer<frt::pssmlt_gpu> render;
            render.chains = chains;
            run(render);
        } else if (integrator == "path") {
            frt::renderer<frt::path_gpu> render;
            render.env_sampling = env_sampling;
            render.roulette = roulette;
            render.sobol = sobol;
            if (until || !error_out.empty()) run_error(render);
            else run(render);
        } else if (integrator == "ao") {
            frt::renderer<frt::ao_gpu> render;
            if (until || !error_out.empty()) run_error(render);
            else run(render);
        } else if (integrator == "normals") {
            frt::renderer<frt::normals_gpu> render;
            run(render);
        } else if (integrator == "albedo") {
            frt::renderer<frt::albedo_gpu> render;
            run(render);
        } else if (integrator == "depth") {
            frt::renderer<frt::depth_gpu> render;
            run(render);
        } else {
            std::fprintf(stderr, "unknown integrator %s\n", integrator.c_str());
            return 2;
        }
        if (denoise) {   // the finished film, on the first GPU
            std::vector<float> rgb(film.fout_image.begin(), film.fout_image.end());
            for (float &v : rgb) v = v < 0.0f ? 0.0f : v;   // path sums can end a few 1e-6 below 0; the filter refuses negatives
            frt::device_set gpu({0}, s.view(), s.env_map());
            const frt_stats st = gpu.denoise(rgb.data(), nx, ny, denoise_spp, seed);
            film.store_film(rgb.data());
            std::printf("Denoised: %d-spp normals, albedo and depth and the filter took %.3f ms on the GPU (%.3f ms in all)\n",
                        denoise_spp, st.kernel_ms, st.total_ms);
        }
        film.save_pfm(out);
        std::printf("Saved %s\n", out.c_str());
        if (!error_out.empty()) {
            frt::check(frt_write_pfm(error_out.c_str(), nx, ny, variance.data()), "frt_write_pfm");
            std::printf("Saved %s\n", error_out.c_str());
        }
        if (!png.empty()) {
            film.save_image(png, FRT_IMAGE_PNG);
            std::printf("Saved %s\n", png.c_str());
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "frt_render: %s\n", e.what());
        return 1;
    }
    return 0;
}
