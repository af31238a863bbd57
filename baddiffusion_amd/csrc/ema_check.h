// Host-side argument check of the EMA entry points (bd_adam_clip_ema, bd_ema_update): plain C++, no HIP, so that it also
// compiles into a stand-alone program (ema_check_main.cpp) and runs under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>

namespace bd {

// [a, a + n) and [b, b + n) floats share an element.  Compared as integers: the pointers belong to different allocations.
static inline bool ranges_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = (uintptr_t)n * sizeof(float);
    return ua < ub ? ub - ua < bytes : ua - ub < bytes;
}

// 0: fine; 1: one_minus_decay is not a finite number in [0, 1]; 2: the shadow overlaps one of `others` over n floats.
static inline int ema_args_bad(const float* ema, const float* const* others, int n_others, int64_t n, float one_minus_decay) {
    if (!std::isfinite(one_minus_decay) || one_minus_decay < 0.f || one_minus_decay > 1.f) return 1;
    for (int k = 0; k < n_others; ++k)
        if (ranges_overlap(ema, others[k], n)) return 2;
    return 0;
}

}  // namespace bd
