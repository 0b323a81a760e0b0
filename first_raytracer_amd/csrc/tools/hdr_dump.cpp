// hdr_dump -- stand-alone driver of the Radiance reader (csrc/host/hdr.cpp):
// prints, per file, the return code of frt_read_hdr and, on success, the size
// and a sum of the texels.  `make hdr_dump_asan` builds it with the address and
// undefined-behaviour sanitizers to run the reader over well-formed and
// malformed files (no GPU, no libfrt.so).
#include <cstdio>
#include <vector>

#include "frt.h"

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) {
        int32_t nx = 0, ny = 0;
        int rc = frt_read_hdr(argv[i], &nx, &ny, nullptr);
        if (rc != FRT_OK) { std::printf("%s: sizes rc %d\n", argv[i], rc); continue; }
        std::vector<float> rgb((size_t)nx * ny * 3);
        rc = frt_read_hdr(argv[i], &nx, &ny, rgb.data());
        double sum = 0;
        if (rc == FRT_OK)
            for (float v : rgb) sum += v;
        std::printf("%s: rc %d, %d x %d, sum %.9g\n", argv[i], rc, nx, ny, sum);
    }
    return 0;
}
