// envdist.cpp -- piecewise-constant distribution over the texels of a lat-long
// environment image, for next-event estimation toward it (FRT_FLAG_ENV_SAMPLING).
//
// Weight of texel (i, j): Rec.709 luminance x the exact solid angle of a texel
// of row j, (2 pi / nx) (cos(pi j / ny) - cos(pi (j + 1) / ny)); row 0 is the +y
// pole, as in env_eval.  Sums in fp64, tables stored in fp32: a marginal CDF over
// rows and a conditional CDF per row.  The probability of a texel is *defined*
// by the stored tables -- the differences of neighbouring entries -- so a texel
// whose fp32 entries coincide cannot be drawn and has probability 0 on both
// sides of the MIS weight (its energy stays with the bsdf sample).
// Deterministic host code: every context of a multi-GPU render and the host
// replay hold bit-identical tables.
#include "envdist.hpp"

#include <cmath>

bool env_tables_of(const float *rgba, int nx, int ny, std::vector<float> &tab)
{
    tab.assign(env_table_records(nx, ny) * 4, 0.0f);
    float *marg = tab.data(), *cond = tab.data() + (ny + 1);
    const double pi = 3.14159265358979323846;
    std::vector<double> row(ny), cum(nx + 1);
    double total = 0.0;
    for (int j = 0; j < ny; ++j) {
        // cos a - cos b as a product: no cancellation at the poles
        const double omega = (2.0 * pi / nx) * 2.0 * std::sin(pi * (2 * j + 1) / (2.0 * ny)) * std::sin(pi / (2.0 * ny));
        cum[0] = 0.0;
        for (int i = 0; i < nx; ++i) {
            const float *t = rgba + 4 * ((size_t)j * nx + i);
            cum[i + 1] = cum[i] + (0.2126 * t[0] + 0.7152 * t[1] + 0.0722 * t[2]) * omega;
        }
        row[j] = cum[nx];
        total += row[j];
        if (!(row[j] > 0.0)) continue;              // a dark row: never chosen, its conditional stays 0
        float *c = cond + (size_t)j * (nx + 1);
        for (int i = 1; i < nx; ++i) c[i] = (float)(cum[i] / row[j]);
        c[nx] = 1.0f;
    }
    if (!(total > 0.0) || !std::isfinite(total)) {
        tab.assign(tab.size(), 0.0f);
        return false;
    }
    double acc = 0.0;
    for (int j = 1; j < ny; ++j) {
        acc += row[j - 1];
        marg[j] = (float)(acc / total);
    }
    marg[ny] = 1.0f;
    return true;
}
