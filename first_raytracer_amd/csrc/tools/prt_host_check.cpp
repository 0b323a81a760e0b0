// prt_host_check.cpp -- the host side of precomputed radiance transfer (csrc/host/prt.cpp) under the
// address and undefined-behaviour sanitizers (Makefile prt_host_asan): the corner records of a
// 2-triangle scene, the basis' orthonormality over a 64^2 stratified set, and the projection of a
// 4 x 2 image.  Exit status 0 when every check holds; no device code.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "frt.h"
#include "frt_rays.hpp"
#include "host/prt.hpp"

// the per-thread refusal text of calls without a context (frt_render.hip defines the library's)
std::string &frt::null_ctx_err()
{
    static thread_local std::string e;
    return e;
}

static int fails = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            ++fails;                                               \
        }                                                          \
    } while (0)

static void check_corners()
{
    // an upward quad as two triangles: lambertian with a checker, and an emitter
    const double v[18] = {0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1};
    const double uv[12] = {0.1, 0.1, 0.1, 0.6, 0.6, 0.1, 0.6, 0.1, 0.1, 0.6, 0.6, 0.6};
    const int32_t mat[2] = {0, 1};
    frt_material m[2];
    memset(m, 0, sizeof(m));
    m[0].type = FRT_MAT_LAMBERTIAN;
    m[0].albedo[0] = 0.5; m[0].albedo[1] = 0.25; m[0].albedo[2] = 1.0;
    m[0].texture = FRT_TEX_CHECKER;
    m[0].tex_odd[0] = 0.125; m[0].tex_odd[1] = 0.0; m[0].tex_odd[2] = 0.75;
    m[0].tex_scale[0] = m[0].tex_scale[1] = 1.0;
    m[1].type = FRT_MAT_DIFFUSE_LIGHT;
    m[1].emit[0] = m[1].emit[1] = m[1].emit[2] = 5.0;
    frt_scene_view sv;
    memset(&sv, 0, sizeof(sv));
    sv.n_tris = 2; sv.tri_v = v; sv.tri_material = mat; sv.tri_uv = uv;
    sv.n_materials = 2; sv.materials = m;
    std::vector<float> on(2 * 3 * 8, -1.0f), rho(2 * 3 * 3, -1.0f);
    CHECK(frtx_prt_corners(&sv, on.data(), rho.data()) == FRT_OK);
    for (int c = 0; c < 6; ++c) {
        CHECK(on[8 * c + 4] == 0.0f && on[8 * c + 5] == 1.0f && on[8 * c + 6] == 0.0f);       // e1 x e2 = +y
        CHECK(on[8 * c + 1] == (float)1e-4);                                                  // lifted off the plane
        CHECK(on[8 * c] == (float)v[3 * c] && on[8 * c + 2] == (float)v[3 * c + 2]);
    }
    // cells (0, 0) and (1, 1) of the checker are tex1, (0, 1) and (1, 0) the albedo
    CHECK(rho[0] == 0.125f && rho[2] == 0.75f);
    CHECK(rho[3] == 0.5f && rho[4] == 0.25f && rho[5] == 1.0f);
    CHECK(rho[6] == 0.5f);
    for (int k = 9; k < 18; ++k) CHECK(rho[k] == 0.0f);   // the emitter's corners carry no transfer
    sv.tri_material = nullptr;
    CHECK(frtx_prt_corners(&sv, on.data(), rho.data()) == FRT_E_INVALID);
}

static void check_basis()
{
    const int sq = 64, n = sq * sq;
    std::vector<float> dirs(3 * (size_t)n), Y(25 * (size_t)n);
    CHECK(frtx_prt_sample_dirs(sq, 7u, dirs.data()) == FRT_OK);
    CHECK(frtx_prt_basis(dirs.data(), n, Y.data()) == FRT_OK);
    const double kPi = 3.14159265358979323846;
    double worst = 0.0;
    for (int a = 0; a < 25; ++a)
        for (int b = a; b < 25; ++b) {
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += (double)Y[25 * (size_t)j + a] * (double)Y[25 * (size_t)j + b];
            const double g = s * 4.0 * kPi / n - (a == b ? 1.0 : 0.0);
            worst = std::fmax(worst, std::fabs(g));
        }
    std::printf("basis: largest deviation of the Gram matrix from the identity %.4f over %d directions\n", worst, n);
    CHECK(worst < 0.05);   // stratified Monte Carlo over 4096 directions: a few times 1 / sqrt(n)
    float bad[3] = {0.0f, 2.0f, 0.0f};
    CHECK(frtx_prt_basis(bad, 1, Y.data()) == FRT_E_INVALID);
    CHECK(frt::null_ctx_err().find("direction 0") != std::string::npos);
}

static void check_projection()
{
    // a constant 4 x 2 image projects to E times the quadrature of Y_00 and of the other bands
    std::vector<float> texels(4 * 2 * 3);
    for (size_t q = 0; q < 8; ++q) { texels[3 * q] = 1.0f; texels[3 * q + 1] = 0.5f; texels[3 * q + 2] = 0.25f; }
    frt_image img{4, 2, FRT_IMAGE_F32, 0, texels.data()};
    double li[75];
    CHECK(frtx_sh_project_image(&img, nullptr, li) == FRT_OK);
    const double kPi = 3.14159265358979323846;
    // sum of sin(theta_y) (2 pi / 4) (pi / 2) over the 8 texels, times Y_00 = 1 / (2 sqrt(pi))
    const double area = 8.0 * std::sin(kPi / 4.0) * (2.0 * kPi / 4.0) * (kPi / 2.0), y00 = 0.5 / std::sqrt(kPi);
    CHECK(std::fabs(li[0] - area * y00) < 1e-12 && std::fabs(li[1] - 0.5 * area * y00) < 1e-12);
    for (int k = 1; k < 4; ++k) CHECK(std::fabs(li[3 * k]) < 1e-12);   // band 1 of a constant image: symmetric rows and columns cancel
    const double env[3] = {2.0, 1.0, 0.5};
    CHECK(frtx_sh_project_image(nullptr, env, li) == FRT_OK);
    CHECK(li[0] == 2.0 * std::sqrt(4.0 * kPi) && li[2] == 0.5 * std::sqrt(4.0 * kPi));
    for (int k = 3; k < 75; ++k) CHECK(li[k] == 0.0);
    const uint8_t bytes[6] = {0, 128, 255, 255, 0, 64};
    frt_image ldr{2, 1, FRT_IMAGE_SRGB8, 0, bytes};
    CHECK(frtx_sh_project_image(&ldr, nullptr, li) == FRT_OK && li[0] > 0.0);
    texels[5] = -1.0f;
    CHECK(frtx_sh_project_image(&img, nullptr, li) == FRT_E_INVALID);
    frt_image none{0, 2, FRT_IMAGE_F32, 0, texels.data()};
    CHECK(frtx_sh_project_image(&none, nullptr, li) == FRT_E_INVALID);
}

int main()
{
    check_corners();
    check_basis();
    check_projection();
    std::printf(fails ? "prt_host_check: %d checks failed\n" : "prt_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
