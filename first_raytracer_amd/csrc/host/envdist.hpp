// envdist.hpp -- the sampling distribution of an environment image
// (FRT_FLAG_ENV_SAMPLING): built on the host, read by env_sample / env_pdf
// (frt_path.hpp).  Internal to libfrt.so.
#pragma once
#include <cstddef>
#include <vector>

#pragma GCC visibility push(hidden)
// floats of the tables of an nx x ny image: the marginal CDF over rows (ny + 1),
// then one conditional CDF per row (nx + 1 each)
inline size_t env_table_floats(int nx, int ny) { return (size_t)(ny + 1) + (size_t)ny * (size_t)(nx + 1); }
// ... rounded up to whole 16-byte texel records (the tables follow the texels in their buffer)
inline size_t env_table_records(int nx, int ny) { return (env_table_floats(nx, ny) + 3) / 4; }
// Build the tables from the converted texels (rgba: 4 floats per texel, rows top
// to bottom, what env_eval reads).  False when no texel has luminance: the image
// cannot be sampled and the tables are all zero.
bool env_tables_of(const float *rgba, int nx, int ny, std::vector<float> &tab);
#pragma GCC visibility pop
