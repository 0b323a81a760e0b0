// Radiance RGBE (.hdr) reader: the floats stb_image's stbi_loadf hands the
// reference's image(file, STBI_HDR) (image.cpp:16) -- rows top to bottom, 3
// floats per texel, value = mantissa * 2^(e - 136), e == 0 -> 0.  Flat and
// new-style run-length-encoded scanlines, "-Y h +X w" orientation only.
// Plain host C++, no device code.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frt.h"

namespace {

struct Cursor {
    const unsigned char *p, *end;
    bool eof() const { return p >= end; }
    size_t left() const { return (size_t)(end - p); }
    // one header line without its newline; false at the end of the file
    bool line(std::string &out)
    {
        out.clear();
        if (eof()) return false;
        while (!eof() && *p != '\n') {
            if (out.size() < 1023) out.push_back((char)*p);
            ++p;
        }
        if (!eof()) ++p;
        return true;
    }
};

inline void rgbe_to_float(const unsigned char *in, float *out)
{
    if (in[3] != 0) {
        const float f = std::ldexp(1.0f, (int)in[3] - (128 + 8));
        out[0] = in[0] * f; out[1] = in[1] * f; out[2] = in[2] * f;
    } else {
        out[0] = out[1] = out[2] = 0.0f;
    }
}

// "-Y h +X w"; FRT_E_UNSUPPORTED for any other orientation
int parse_size(const std::string &t, int32_t &w, int32_t &h)
{
    if (t.size() < 3) return FRT_E_INVALID;
    const bool axis = (t[0] == '-' || t[0] == '+') && (t[1] == 'X' || t[1] == 'Y') && t[2] == ' ';
    if (!axis) return FRT_E_INVALID;
    if (t.compare(0, 3, "-Y ") != 0) return FRT_E_UNSUPPORTED;
    const char *s = t.c_str() + 3;
    char *e = nullptr;
    const long hh = std::strtol(s, &e, 10);
    if (e == s) return FRT_E_INVALID;
    while (*e == ' ') ++e;
    if (!((e[0] == '-' || e[0] == '+') && (e[1] == 'X' || e[1] == 'Y') && e[2] == ' ')) return FRT_E_INVALID;
    if (std::strncmp(e, "+X ", 3) != 0) return FRT_E_UNSUPPORTED;
    s = e + 3;
    const long ww = std::strtol(s, &e, 10);
    if (e == s) return FRT_E_INVALID;
    if (hh <= 0 || ww <= 0 || hh > (1 << 24) || ww > (1 << 24) || (long long)hh * ww > 0x7fffffffLL / 3) return FRT_E_INVALID;
    w = (int32_t)ww; h = (int32_t)hh;
    return FRT_OK;
}

int decode(Cursor c, int32_t w, int32_t h, float *rgb)
{
    const size_t n = (size_t)w * h;
    bool flat = w < 8 || w >= 32768;
    if (!flat) {   // a first scanline without the (2, 2, high bit clear) marker: the whole image is flat
        if (c.left() < 4) return FRT_E_IO;
        flat = c.p[0] != 2 || c.p[1] != 2 || (c.p[2] & 0x80);
    }
    if (flat) {
        if (c.left() < 4 * n) return FRT_E_IO;
        for (size_t q = 0; q < n; ++q) rgbe_to_float(c.p + 4 * q, rgb + 3 * q);
        return FRT_OK;
    }
    std::vector<unsigned char> scan(4 * (size_t)w);
    for (int32_t j = 0; j < h; ++j) {
        if (c.left() < 4) return FRT_E_IO;
        if (c.p[0] != 2 || c.p[1] != 2 || (c.p[2] & 0x80)) return FRT_E_INVALID;
        if (((int)c.p[2] << 8 | c.p[3]) != w) return FRT_E_INVALID;   // decoded scanline length
        c.p += 4;
        for (int k = 0; k < 4; ++k) {
            int32_t i = 0;
            while (i < w) {
                if (c.eof()) return FRT_E_IO;
                int count = *c.p++;
                if (count > 128) {                      // run
                    count -= 128;
                    if (count > w - i) return FRT_E_INVALID;
                    if (c.eof()) return FRT_E_IO;
                    const unsigned char v = *c.p++;
                    for (int z = 0; z < count; ++z) scan[4 * (size_t)(i++) + k] = v;
                } else {                                // literal
                    if (count == 0 || count > w - i) return FRT_E_INVALID;
                    if (c.left() < (size_t)count) return FRT_E_IO;
                    for (int z = 0; z < count; ++z) scan[4 * (size_t)(i++) + k] = *c.p++;
                }
            }
        }
        for (int32_t i = 0; i < w; ++i) rgbe_to_float(&scan[4 * (size_t)i], rgb + 3 * ((size_t)j * w + i));
    }
    return FRT_OK;
}

}  // namespace

extern "C" int frt_read_hdr(const char *path, int32_t *nx, int32_t *ny, float *rgb)
{
    if (!path || !nx || !ny) return FRT_E_INVALID;
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return FRT_E_IO;
    std::vector<unsigned char> buf;
    unsigned char chunk[65536];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) return FRT_E_IO;
    Cursor c{buf.data(), buf.data() + buf.size()};
    std::string t;
    if (!c.line(t)) return FRT_E_IO;
    if (t != "#?RADIANCE" && t != "#?RGBE") return FRT_E_INVALID;
    bool format = false;
    for (;;) {                                          // header lines up to the empty one
        if (!c.line(t)) return FRT_E_IO;
        if (t.empty()) break;
        if (t == "FORMAT=32-bit_rle_rgbe") format = true;
    }
    if (!format) return FRT_E_UNSUPPORTED;
    if (!c.line(t)) return FRT_E_IO;
    int32_t w = 0, h = 0;
    const int rc = parse_size(t, w, h);
    if (rc != FRT_OK) return rc;
    *nx = w; *ny = h;
    if (!rgb) return FRT_OK;
    return decode(c, w, h, rgb);
}
