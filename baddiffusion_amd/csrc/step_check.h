// Host-side buffer check of the dense vec4 entry points (bd_lincomb, bd_dpm_step, bd_unipc_step, bd_sigma_step, bd_scale_input): plain
// C++, no HIP, so that it also compiles into a stand-alone program (step_check_main.cpp) and runs under the host sanitizers.
#pragma once
#include "ema_check.h"

namespace bd {

struct StepBuf { const void* p; const char* name; };      // p may be null: an optional operand that is absent, skipped everywhere

enum StepBad { STEP_OK = 0, STEP_MISALIGNED, STEP_OUT_OUT, STEP_OUT_IN };
// a: the offending buffer -- the input's index, or n_in + the output's index, when misaligned; the output's index otherwise.
// b: what it overlaps -- an earlier output's index (STEP_OUT_OUT) or an input's index (STEP_OUT_IN).
struct StepViolation { StepBad code; int a, b; };

// Every buffer holds n floats and is read or written 16 bytes at a time.  An output may be an input's own buffer (same base: the
// kernels read each index before they write it); nothing else may overlap.  The first violation in this order: alignment of the
// inputs, then of the outputs; then per output, in order, the outputs before it and then the inputs.
static inline StepViolation step_buffers_bad(int64_t n, const StepBuf* in, int n_in, const StepBuf* out, int n_out) {
    auto f = [](const void* p) { return static_cast<const float*>(p); };
    for (int j = 0; j < n_in + n_out; ++j) {
        const void* p = j < n_in ? in[j].p : out[j - n_in].p;
        if (reinterpret_cast<uintptr_t>(p) & 15) return {STEP_MISALIGNED, j, -1};
    }
    for (int o = 0; o < n_out; ++o) {
        if (!out[o].p) continue;
        for (int p = 0; p < o; ++p)
            if (out[p].p && ranges_overlap(f(out[p].p), f(out[o].p), n)) return {STEP_OUT_OUT, o, p};
        for (int j = 0; j < n_in; ++j)
            if (in[j].p && in[j].p != out[o].p && ranges_overlap(f(in[j].p), f(out[o].p), n)) return {STEP_OUT_IN, o, j};
    }
    return {STEP_OK, -1, -1};
}

}  // namespace bd
