// sobol_probe -- prints the words of the FRT_FLAG_SOBOL sampler (csrc/frt_device.hpp:
// sobol_key, sobol_word, sobol_u) as host code, for tests/test_sobol_host.py to compare
// with the numpy restatement.  stdin: lines "seed pixel sample dim" (decimal);
// stdout: per line the 32-bit word and the 24-bit numerator of the uniform.
#include <cinttypes>
#include <cstdio>

#include "frt_device.hpp"

int main()
{
    unsigned long long seed, pixel, sample, dim;
    while (std::scanf("%llu %llu %llu %llu", &seed, &pixel, &sample, &dim) == 4) {
        const frt::RngKey k = frt::sobol_key((uint32_t)seed, (uint32_t)pixel, (uint32_t)sample);
        const uint32_t w = frt::sobol_word(k, (uint32_t)dim);
        const float u = frt::sobol_u(k, (uint32_t)dim);
        std::printf("%" PRIu32 " %" PRIu32 "\n", w, (uint32_t)(u * 16777216.0f));
    }
    return 0;
}
