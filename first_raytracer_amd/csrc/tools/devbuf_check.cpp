// devbuf_check.cpp -- the grow rule of csrc/frt_devbuf.hpp with a stand-alone main, for the address
// and undefined-behaviour sanitizers (make devbuf_asan): DevBuf over a counting allocator in host
// memory whose next call can be made to fail.  No device is touched.  Exit status 0: every check holds.
#include <cstdio>
#include <cstdlib>

#include "frt_devbuf.hpp"

namespace {

int g_allocs = 0, g_frees = 0, g_live = 0, g_bad = 0;
bool g_fail_next = false;
size_t g_last_bytes = 0;

hipError_t fake_alloc(void **p, size_t n)
{
    if (g_fail_next) return g_fail_next = false, hipErrorOutOfMemory;
    *p = std::malloc(n);   // the sanitizers see a write past n, a double free, a leak
    g_last_bytes = n;
    return ++g_allocs, ++g_live, hipSuccess;
}
hipError_t fake_free(void *p)
{
    std::free(p);
    return ++g_frees, --g_live, hipSuccess;
}

struct Ctx { std::string err; };   // what reserve asks of its context: set_err, as frt_ctx.hpp has it
int set_err(Ctx *c, int code, const std::string &m) { return c->err = m, code; }

#define CHECK(x) ((x) ? 0 : (std::printf("line %d: %s does not hold\n", __LINE__, #x), ++g_bad))

}  // namespace

int main()
{
    Ctx c;
    std::vector<DevBufAny *> owner;
    {
        DevBuf<unsigned char, fake_alloc, fake_free> a(owner), b(owner);
        CHECK(owner.size() == 2 && owner[0] == &a && owner[1] == &b && a.get() == nullptr && a.bytes == 0);
        // the 16-byte floor
        CHECK(a.reserve(&c, 0) == FRT_OK && a.bytes == 16 && g_last_bytes == 16 && a.get() != nullptr);
        a.get()[15] = 1;
        CHECK(a.reserve(&c, 16) == FRT_OK && g_allocs == 1);
        // growth: the old memory is freed, the capacity is what was asked
        CHECK(a.reserve(&c, 1000) == FRT_OK && a.bytes == 1000 && g_allocs == 2 && g_frees == 1 && g_live == 1);
        a.get()[999] = 1;
        // large enough: no reallocation, the same memory
        unsigned char *const before = a;
        CHECK(a.reserve(&c, 999) == FRT_OK && a.reserve(&c, 1) == FRT_OK && a.reserve(&c, 1000) == FRT_OK);
        CHECK(a.get() == before && a.bytes == 1000 && g_allocs == 2);
        // an allocation that fails: the context's error, an empty buffer of capacity 0, nothing live
        g_fail_next = true;
        CHECK(c.err.empty() && a.reserve(&c, 2000) == FRT_E_HIP && !c.err.empty());
        CHECK(a.get() == nullptr && a.bytes == 0 && g_live == 0 && g_frees == 2);
        // ... and the next call allocates again, even for a size the buffer once had
        CHECK(a.reserve(&c, 500) == FRT_OK && a.bytes == 500 && a.get() != nullptr && g_allocs == 3 && g_live == 1);
        a.get()[499] = 1;
        // a failure on an empty buffer frees nothing
        g_fail_next = true;
        CHECK(b.reserve(&c, 64) == FRT_E_HIP && b.get() == nullptr && b.bytes == 0 && g_frees == 2);
        CHECK(b.reserve(&c, 64) == FRT_OK && g_live == 2);
        // release: through the owner's list, as frt_destroy does, and once more
        for (DevBufAny *x : owner) x->release();
        CHECK(g_live == 0 && a.get() == nullptr && a.bytes == 0 && b.get() == nullptr && b.bytes == 0);
        const int frees = g_frees;
        a.release();
        b.release();
        CHECK(g_frees == frees);
        // a released buffer grows again
        CHECK(b.reserve(&c, 32) == FRT_OK && b.bytes == 32 && g_live == 1);
        b.release();
    }
    CHECK(g_live == 0 && g_allocs == g_frees);
    std::printf("devbuf_check: %d allocations, %d frees, %d live, %d checks failed\n", g_allocs, g_frees, g_live, g_bad);
    return g_bad ? 1 : 0;
}
