// abi_guard.hpp -- the exception barrier of the host units' C entry points: the
// ABI has no out-of-memory code, so std::bad_alloc and anything else a body
// throws become FRT_E_INVALID (as frt_scene_new answers a failed allocation).
#pragma once
#include "frt.h"

template <class F>
int frt_guard(F &&body) noexcept
{
    try {
        return body();
    } catch (...) {
        return FRT_E_INVALID;
    }
}
