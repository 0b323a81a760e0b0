// denoise_probe -- the filter of FRT_INTEGRATOR_DENOISE (csrc/frt_denoise.hpp: denoise_pack,
// denoise_iterate, denoise_unpack -- the functions the kernels compile) as host code, for
// tests/test_denoise_host.py to compare with the numpy restatement.
//   denoise_probe NX NY colour.f32 normals.f32 albedo.f32 depth.f32 out.f32
// Each file holds NX * NY * 3 floats in pixel order; out gets the filtered film.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "frt_denoise.hpp"

static bool read_film(const char *path, std::vector<float> &v)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(v.data(), sizeof(float), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 8) return 2;
    const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]);
    if (nx <= 0 || ny <= 0) return 2;
    const size_t n = (size_t)nx * ny;
    std::vector<float> film[4];
    for (int k = 0; k < 4; ++k) {
        film[k].resize(3 * n);
        if (!read_film(argv[3 + k], film[k])) { std::fprintf(stderr, "cannot read %s\n", argv[3 + k]); return 1; }
    }
    auto at = [&](int k, size_t i) { return frt::f3{film[k][3 * i], film[k][3 * i + 1], film[k][3 * i + 2]}; };
    std::vector<float4> guides(n), a(n), b(n);
    for (size_t i = 0; i < n; ++i) {
        const frt::DenoisePixel P = frt::denoise_pack(at(0, i), at(1, i), at(2, i), at(3, i));
        guides[i] = P.g;
        a[i] = P.c;
    }
    for (int it = 0; it < frt::kDenoiseIterations; ++it) {
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x)
                b[(size_t)y * nx + x] = frt::denoise_iterate(x, y, nx, ny, 1 << it, frt::denoise_sigma_l(it), [&](int qx, int qy) {
                    const size_t q = (size_t)qy * nx + qx;
                    return frt::DenoisePixel{guides[q], a[q]};
                });
        std::swap(a, b);
    }
    std::vector<float> out(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const frt::f3 c = frt::denoise_unpack(a[i], at(2, i));
        out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
    }
    std::FILE *f = std::fopen(argv[7], "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 1;
    std::fclose(f);
    return 0;
}
