// frt_devbuf.hpp -- the context's grow-only device buffers: one grow rule (DevBuf::reserve), and
// one list of them on their context, so that frt_destroy frees every one in a loop.  Internal to
// libfrt.so.  The allocate and free calls are template parameters: csrc/tools/devbuf_check.cpp
// drives the rule with a counting allocator, without a device.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "frt.h"

// what the owner's list holds: the memory, its capacity in bytes, and how to free it; not copyable
struct DevBufAny {
    void *mem = nullptr;
    size_t bytes = 0;
    hipError_t (*const free_fn)(void *);
    DevBufAny(std::vector<DevBufAny *> &owner, hipError_t (*f)(void *)) : free_fn(f) { owner.push_back(this); }
    DevBufAny(const DevBufAny &) = delete;
    void release()
    {
        if (mem) (void)free_fn(mem);
        mem = nullptr;
        bytes = 0;
    }
};

template <typename T, hipError_t (*Alloc)(void **, size_t) = hipMalloc, hipError_t (*Free)(void *) = hipFree>
struct DevBuf : DevBufAny {
    explicit DevBuf(std::vector<DevBufAny *> &owner) : DevBufAny(owner, Free) {}
    T *get() const { return static_cast<T *>(mem); }
    operator T *() const { return get(); }
    // Room for at least `need` bytes (16 at the least); the contents are not kept when it grows.
    // A failed allocation sets the context's error (set_err, as HIPCHK does) and leaves the
    // buffer empty with capacity 0, so the next call allocates again.
    template <typename Ctx>
    int reserve(Ctx *c, size_t need)
    {
        need = std::max<size_t>(need, 16);
        if (need <= bytes) return FRT_OK;
        release();
        const hipError_t e = Alloc(&mem, need);
        if (e != hipSuccess) {
            mem = nullptr;
            return set_err(c, FRT_E_HIP, std::string("device buffer of ") + std::to_string(need) + " bytes: " + hipGetErrorString(e));
        }
        bytes = need;
        return FRT_OK;
    }
};
