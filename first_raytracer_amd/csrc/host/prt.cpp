// prt.cpp -- the host side of precomputed radiance transfer (prt.hpp) and the
// host-only entry points over it (frt.h): frtx_prt_basis, frtx_sh_project_image,
// frtx_prt_sample_dirs, frtx_prt_corners.  Plain C++, no device code.
#include "host/prt.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>

#include "frt_rays.hpp"
#include "host/abi_guard.hpp"

namespace frt_prt {

namespace {

const double kPi = 3.14159265358979323846;

double factorial(int n)
{
    double f = 1.0;
    for (int i = 2; i <= n; ++i) f *= (double)i;
    return f;
}
// the normalisation constant of Y_lm, m >= 0
double sh_k(int l, int m) { return std::sqrt(((2.0 * l + 1.0) * factorial(l - m)) / (4.0 * kPi * factorial(l + m))); }
// the associated Legendre function P_l^m(x), m >= 0, with the Condon-Shortley phase, by the
// standard upward recurrences in l from P_m^m = (-1)^m (2m - 1)!! (1 - x^2)^(m / 2)
double legendre(int l, int m, double x)
{
    double pmm = 1.0;
    if (m > 0) {
        const double s = std::sqrt((1.0 - x) * (1.0 + x));
        double odd = 1.0;
        for (int i = 1; i <= m; ++i) {
            pmm *= -odd * s;
            odd += 2.0;
        }
    }
    if (l == m) return pmm;
    double pm1 = x * (2.0 * m + 1.0) * pmm;
    if (l == m + 1) return pm1;
    double pl = 0.0;
    for (int k = m + 2; k <= l; ++k) {
        pl = ((2.0 * k - 1.0) * x * pm1 - (k + m - 1.0) * pmm) / (double)(k - m);
        pmm = pm1;
        pm1 = pl;
    }
    return pl;
}

// the project's counter hash (csrc/frt_device.hpp mix32, rng_key, rng_u; DESIGN.md "RNG stream
// spec"), restated for this plain C++ unit: the 24-bit uniform of dimension `dim` of (seed, id, 0)
uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
double hash_u(uint32_t seed, uint32_t id, uint32_t dim)
{
    const uint32_t a = mix32(seed ^ 0x2545F491U);
    const uint32_t k0 = mix32(mix32(a ^ id) + 0u * 0x9E3779B9U);
    const uint32_t k1 = mix32(mix32(a + id * 0x632BE5ABU) ^ (0u * 0x85157AF5U + 0x5851F42DU));
    const uint32_t h = mix32((k0 ^ (dim * 0x85EBCA77U + 0xC2B2AE3DU)) + k1);
    return (double)(h >> 8) * (1.0 / 16777216.0);
}

double from_srgb(double v) { return v <= 0.04045 ? v * (1.0 / 12.92) : std::pow((v + 0.055) * (1.0 / 1.055), 2.4); }
// the fp32 texel image_texture's lookup returns (csrc/frt_flatten.hip append_texels), as a double
double texel(const frt_image &im, size_t q, int ch)
{
    if (im.format == FRT_IMAGE_F32) return (double)static_cast<const float *>(im.data)[3 * q + ch];
    return (double)(float)from_srgb(static_cast<const uint8_t *>(im.data)[3 * q + ch] / 255.0);
}
// "" or why the image cannot be read (frt_set_env_image's rules)
std::string image_bad(const frt_image &im, const char *what)
{
    const std::string w = what;
    if (im.nx <= 0 || im.ny <= 0) return w + ": nx and ny must be positive";
    if (!im.data) return w + ": null data";
    if (im.format != FRT_IMAGE_SRGB8 && im.format != FRT_IMAGE_F32) return w + ": format must be FRT_IMAGE_SRGB8 or FRT_IMAGE_F32";
    return "";
}

// (int)x as the kernels' x86_trunc computes it, and the texture index rules of csrc/frt_path.hpp in fp64
int trunc_x86(double x)
{
    if (!(x > -2147483649.0 && x < 2147483648.0)) return (int)0x80000000;
    return (int)x;
}
int imod(int a, int b)
{
    const int r = a % b;
    return r < 0 ? r + b : r;
}
size_t image_index(int nx, int ny, double tu, double tv)
{
    int i = trunc_x86(tu * (double)nx), j = trunc_x86(tv * (double)ny);
    if (i < 0 || i > nx) i = imod(i, nx);
    if (j < 0 || j > ny) j = imod(j, ny);
    if (i == nx) i = nx - 1;
    if (j == ny) j = ny - 1;
    return (size_t)j * (size_t)nx + (size_t)i;
}

}  // namespace

double sh_eval(int l, int m, double theta, double phi)
{
    const double x = std::cos(theta);
    if (m == 0) return sh_k(l, 0) * legendre(l, 0, x);
    if (m > 0) return std::sqrt(2.0) * sh_k(l, m) * std::cos(m * phi) * legendre(l, m, x);
    return std::sqrt(2.0) * sh_k(l, -m) * std::sin(-m * phi) * legendre(l, -m, x);
}

void sh_all(double theta, double phi, double Y[kCoef])
{
    for (int l = 0; l < kBands; ++l)
        for (int m = -l; m <= l; ++m) Y[l * (l + 1) + m] = sh_eval(l, m, theta, phi);
}

void dir_angles(const float d[3], double &theta, double &phi)
{
    const double y = std::fmin(std::fmax((double)d[1], -1.0), 1.0);
    theta = std::acos(y);
    phi = std::atan2((double)d[0], -(double)d[2]);
    if (phi < 0.0) phi += 2.0 * kPi;
}

void y_table(const float *dirs, int64_t n, float *Y)
{
    for (int64_t j = 0; j < n; ++j) {
        double theta, phi, y[kCoef];
        dir_angles(dirs + 3 * j, theta, phi);
        sh_all(theta, phi, y);
        for (int k = 0; k < kCoef; ++k) Y[kCoef * j + k] = (float)y[k];
    }
}

int64_t dirs_first_bad(const float *dirs, int64_t n, std::string &why)
{
    for (int64_t j = 0; j < n; ++j) {
        const float *d = dirs + 3 * j;
        const char *bad = nullptr;
        if (!(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]))) {
            bad = "is not finite";
        } else {
            const double len = std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
            if (!(std::fabs(len - 1.0) <= 1e-3)) bad = "is no unit vector (its length is off 1 by more than 1e-3)";
        }
        if (bad) {
            why = "direction " + std::to_string(j) + " " + bad;
            return j;
        }
    }
    return -1;
}

std::string transfer_request_bad(const float *dirs, int64_t n_dirs, int bounces, int flags)
{
    if (n_dirs < 1 || n_dirs > (1 << 24)) return "prt_transfer: n_dirs must be in [1, 2^24]";
    if (bounces < 0 || bounces > 16) return "prt_transfer: bounces must be in [0, 16]";
    if (flags & ~(FRTX_PRT_UNSHADOWED | FRT_FLAG_NO_LDS_SCENE | FRT_FLAG_BVH2 | FRT_FLAG_NO_OCT)) return "prt_transfer: unknown flags";
    if (!dirs) return "prt_transfer: bad arguments";
    std::string why;
    if (dirs_first_bad(dirs, n_dirs, why) >= 0) return "prt_transfer: " + why;
    return "";
}

namespace {
constexpr size_t kBatchBudget = (size_t)256 << 20;
size_t g_batch_budget = kBatchBudget;
}  // namespace
size_t batch_budget() { return g_batch_budget; }

std::string corners(const frt_scene_view *sv, float *origin_normal, float *albedo)
{
    if (!sv || sv->n_tris < 0) return "prt_corners: bad arguments";
    if (sv->n_tris > 0 && (!sv->tri_v || !sv->tri_material || !sv->materials || !origin_normal || !albedo))
        return "prt_corners: bad arguments";
    for (int t = 0; t < sv->n_tris; ++t) {
        const double *v = sv->tri_v + 9 * (size_t)t;
        const int mi = sv->tri_material[t];
        if (mi < 0 || mi >= sv->n_materials) return "prt_corners: triangle " + std::to_string(t) + " names no material";
        const frt_material &m = sv->materials[mi];
        if (m.type == FRT_MAT_LAMBERTIAN && m.texture == FRT_TEX_IMAGE) {
            if (m.image < 0 || m.image >= sv->n_images || !sv->images) return "prt_corners: material " + std::to_string(mi) + " names no image";
            const std::string bad = image_bad(sv->images[m.image], "prt_corners: texture image");
            if (!bad.empty()) return bad;
        }
        const bool smooth = sv->tri_n && sv->tri_geometry_normal && sv->tri_geometry_normal[t] == 0;
        double ng[3] = {0.0, 0.0, 0.0};
        if (!smooth) {
            const double e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
            const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            for (int a = 0; a < 3; ++a) ng[a] = c[a] / len;
        }
        for (int i = 0; i < 3; ++i) {
            const size_t c = 3 * (size_t)t + i;
            const double *n = smooth ? sv->tri_n + 9 * (size_t)t + 3 * i : ng;
            float *on = origin_normal + 8 * c;
            for (int a = 0; a < 3; ++a) {
                on[a] = (float)(v[3 * i + a] + kCornerEps * n[a]);
                on[4 + a] = (float)n[a];
            }
            on[3] = on[7] = 0.0f;
            double rho[3] = {0.0, 0.0, 0.0};
            if (m.type == FRT_MAT_LAMBERTIAN) {
                const double tu = sv->tri_uv ? sv->tri_uv[6 * (size_t)t + 2 * i] : 0.0;
                const double tv = sv->tri_uv ? sv->tri_uv[6 * (size_t)t + 2 * i + 1] : 0.0;
                for (int a = 0; a < 3; ++a) rho[a] = m.albedo[a];
                if (m.texture == FRT_TEX_CHECKER) {   // checker_texture::value: tex1 where x * y == 1
                    const int x = 2 * imod(trunc_x86(tu * m.tex_scale[0] * 2.0), 2) - 1;
                    const int y = 2 * imod(trunc_x86(tv * m.tex_scale[1] * 2.0), 2) - 1;
                    if (x * y == 1)
                        for (int a = 0; a < 3; ++a) rho[a] = m.tex_odd[a];
                } else if (m.texture == FRT_TEX_IMAGE) {
                    const frt_image &im = sv->images[m.image];
                    const size_t q = image_index(im.nx, im.ny, tu, tv);
                    for (int a = 0; a < 3; ++a) rho[a] = texel(im, q, a);
                }
            }
            for (int a = 0; a < 3; ++a) albedo[3 * c + a] = (float)rho[a];
        }
    }
    return "";
}

std::string project(const frt_image *img, const double env[3], double li[3 * kCoef])
{
    if (!li || (!img && !env)) return "sh_project_image: bad arguments";
    for (int k = 0; k < 3 * kCoef; ++k) li[k] = 0.0;
    if (!img) {   // the constant colour: E times the integral of Y_00 = E sqrt(4 pi); the other bands integrate to 0
        for (int ch = 0; ch < 3; ++ch) li[ch] = env[ch] * std::sqrt(4.0 * kPi);
        return "";
    }
    const std::string bad = image_bad(*img, "sh_project_image");
    if (!bad.empty()) return bad;
    const double dw = (2.0 * kPi / img->nx) * (kPi / img->ny);
    for (int y = 0; y < img->ny; ++y) {
        const double theta = kPi * (y + 0.5) / img->ny, w = std::sin(theta) * dw;
        for (int x = 0; x < img->nx; ++x) {
            const double phi = 2.0 * kPi * (x + 0.5) / img->nx;
            double Y[kCoef];
            sh_all(theta, phi, Y);
            const size_t q = (size_t)y * img->nx + x;
            for (int ch = 0; ch < 3; ++ch) {
                const double v = texel(*img, q, ch);
                if (!(v >= 0.0 && v <= (double)FLT_MAX))
                    return "sh_project_image: texel (" + std::to_string(x) + ", " + std::to_string(y) + ") is negative or not finite";
                for (int k = 0; k < kCoef; ++k) li[3 * k + ch] += v * Y[k] * w;
            }
        }
    }
    return "";
}

void sample_dirs(int sqrt_n, uint32_t seed, float *dirs)
{
    const double inv = 1.0 / sqrt_n;
    for (int a = 0, i = 0; a < sqrt_n; ++a)
        for (int b = 0; b < sqrt_n; ++b, ++i) {
            const double x = (a + hash_u(seed, (uint32_t)i, 0)) * inv, y = (b + hash_u(seed, (uint32_t)i, 1)) * inv;
            const double ct = 1.0 - 2.0 * x, st = std::sqrt(std::fmax(0.0, 1.0 - ct * ct)), phi = 2.0 * kPi * y;
            // the inverse of dir_angles: phi = atan2(d.x, -d.z), theta = acos(d.y)
            dirs[3 * i] = (float)(st * std::sin(phi));
            dirs[3 * i + 1] = (float)ct;
            dirs[3 * i + 2] = (float)(-st * std::cos(phi));
        }
}

}  // namespace frt_prt

namespace {
int refuse(const std::string &m)
{
    frt::null_ctx_err() = m;
    return FRT_E_INVALID;
}
}  // namespace

#pragma GCC visibility push(default)
// test hook: the batch budget of frtx_prt_transfer and its replay in bytes (0: the default again)
extern "C" int frtx_selftest_prt_budget(int64_t bytes)
{
    if (bytes < 0) return FRT_E_INVALID;
    frt_prt::g_batch_budget = bytes ? (size_t)bytes : frt_prt::kBatchBudget;
    return FRT_OK;
}

extern "C" int frtx_prt_basis(const float *dirs, int64_t n, float *Y)
{
    return frt_guard([&]() -> int {
        if (n < 0 || (n > 0 && (!dirs || !Y))) return refuse("prt_basis: bad arguments");
        std::string why;
        if (frt_prt::dirs_first_bad(dirs, n, why) >= 0) return refuse("prt_basis: " + why);
        frt_prt::y_table(dirs, n, Y);
        return FRT_OK;
    });
}

extern "C" int frtx_sh_project_image(const frt_image *img, const double env_color[3], double li[75])
{
    return frt_guard([&]() -> int {
        const std::string bad = frt_prt::project(img, env_color, li);
        return bad.empty() ? FRT_OK : refuse(bad);
    });
}

extern "C" int frtx_prt_sample_dirs(int sqrt_n, uint32_t seed, float *dirs)
{
    return frt_guard([&]() -> int {
        if (sqrt_n < 1 || sqrt_n > 4096 || !dirs) return refuse("prt_sample_dirs: sqrt_n must be in [1, 4096]");
        frt_prt::sample_dirs(sqrt_n, seed, dirs);
        return FRT_OK;
    });
}

extern "C" int frtx_prt_corners(const frt_scene_view *sv, float *origin_normal, float *albedo)
{
    return frt_guard([&]() -> int {
        const std::string bad = frt_prt::corners(sv, origin_normal, albedo);
        return bad.empty() ? FRT_OK : refuse(bad);
    });
}
#pragma GCC visibility pop
