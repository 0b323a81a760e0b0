// frt_error.hpp -- the arithmetic of FRT_INTEGRATOR_ERROR (frt.h): the
// batch-means estimate of the variance of a pixel's mean from the chunk sums a
// render leaves in the context's `partial`.  The kernel (frt_error.hip) and the
// host hook frtx_selftest_chunk_variance compile the same code.  DESIGN.md
// "Error film" states the estimator.
//
// Chunk c of an element (one channel of one slot) holds n_c samples with sum
// S_c; m_c = S_c / n_c, N = sum n_c, m = sum S_c / N, and
//   V = sum_c n_c (m_c - m)^2 / ((K - 1) N).
// One pass over the chunks with West's weighted incremental update (West 1979,
// the weighted form of Welford's): never sum x^2 - N m^2, whose two terms agree
// in all but the last bits at the spreads a converged pixel has.
//
// Every product and sum below is a statement of its own: -ffp-contract=on fuses
// within an expression only, so the device (which has the fused instruction)
// and the host (which may not) round alike.
#pragma once
#include "frt_device.hpp"

namespace frt {

struct ChunkVar {
    float mean = 0.0f;   // of the samples of the chunks so far
    float s = 0.0f;      // sum over those chunks of n_c (m_c - mean)^2
};

// samples of chunk c: spi, the last chunk what is left of spp
FRT_HD float chunk_samples(int c, int n_chunks, int spp, int spi)
{
    return (float)(c < n_chunks - 1 ? spi : spp - (n_chunks - 1) * spi);
}
// r_c = n_c / (n_0 + ... + n_c): the same for every element, so a lane divides once a chunk for
// all its elements.  r_0 = 1; the chunks before the last have equal n, so r_c <= 1/2 from c = 1 on.
FRT_HD float chunk_ratio(int c, int n_chunks, int spp, int spi)
{
    return chunk_samples(c, n_chunks, spp, spi) / (float)(c < n_chunks - 1 ? (c + 1) * spi : spp);
}

// one chunk: its sum, n = chunk_samples, r = chunk_ratio.  The first chunk (r = 1, mean = 0) sets
// mean = x exactly and adds n x 0 to s.  A chunk whose mean x is bit-equal to the running mean
// leaves mean and s as they are (d = 0), so equal chunk means give exactly 0.  With r <= 1/2 the
// new mean lies between the old one and x (rounding is monotone), d and x - mean share their sign,
// and s never decreases.
FRT_HD void chunk_var_add(ChunkVar &a, float sum, float n, float r)
{
    const float x = sum / n;
    const float d = x - a.mean;
    const float step = r * d;
    a.mean = a.mean + step;
    const float e = x - a.mean;
    const float nd = n * d;
    const float t = nd * e;
    a.s = a.s + t;
}

// V of n_chunks >= 2 chunks of spp samples in all
FRT_HD float chunk_var_result(const ChunkVar &a, int n_chunks, int spp)
{
    const float denom = (float)(n_chunks - 1) * (float)spp;
    return a.s / denom;
}

}  // namespace frt
