// Stand-alone driver of step_check.h for the host sanitizers (tests/test_step_exact_host.py builds it with -fsanitize=address,undefined).
// Not part of libbd_hip.so.  Exit status 0 = every case answered as expected.
#include "step_check.h"

#include <cstdio>
#include <vector>

int main() {
    using namespace bd;
    int fails = 0;
    auto expect = [&](const StepViolation& v, StepBad code, int a, int b, const char* what) {
        if (v.code != code || v.a != a || v.b != b) {
            std::printf("FAIL %s: got (%d, %d, %d), want (%d, %d, %d)\n", what, (int)v.code, v.a, v.b, (int)code, a, b);
            ++fails;
        }
    };
    // 16-byte aligned base; seven slots of 16 floats, never dereferenced by the check
    std::vector<float> buf(7 * 16 + 4);
    float* b = buf.data();
    while (reinterpret_cast<uintptr_t>(b) & 15) ++b;
    const int64_t n = 16;
    auto slot = [&](int k) { return static_cast<const void*>(b + 16 * k); };
    auto at = [&](int k, int off) { return static_cast<const void*>(b + 16 * k + off); };

    const StepBuf in3[3] = {{slot(0), "e"}, {slot(1), "x"}, {nullptr, "h"}};
    const StepBuf out2[2] = {{slot(2), "prev"}, {nullptr, "m0"}};
    expect(step_buffers_bad(n, in3, 3, out2, 2), STEP_OK, -1, -1, "null optional pointers are skipped");
    {   // an output on an input's base
        const StepBuf o[2] = {{slot(1), "prev"}, {slot(3), "m0"}};
        expect(step_buffers_bad(n, in3, 3, o, 2), STEP_OK, -1, -1, "same base");
    }
    for (int off : {4, -4}) {   // 16 bytes = 4 floats, either way
        const StepBuf o[2] = {{at(1, off), "prev"}, {slot(4), "m0"}};
        expect(step_buffers_bad(n, in3, 3, o, 2), STEP_OUT_IN, 0, off > 0 ? 1 : 0, "16-byte offset against an input");
    }
    {   // b == a + n and b + n == a
        const StepBuf i[2] = {{slot(1), "e"}, {slot(3), "x"}};
        const StepBuf o[1] = {{slot(2), "prev"}};
        expect(step_buffers_bad(n, i, 2, o, 1), STEP_OK, -1, -1, "touching ranges");
        const StepBuf o12[1] = {{at(2, -4), "prev"}};     // 12 floats of slot 2, the last 4 of slot 1
        expect(step_buffers_bad(12, i, 2, o12, 1), STEP_OK, -1, -1, "touching ranges, n = 12");
        expect(step_buffers_bad(13, i, 2, o12, 1), STEP_OUT_IN, 0, 0, "one float past touching");
    }
    {   // alignment: inputs first, then outputs; a is the index in the joined list
        const StepBuf i[2] = {{slot(0), "e"}, {at(1, 1), "x"}};
        const StepBuf o[2] = {{at(2, 2), "prev"}, {slot(3), "m0"}};
        expect(step_buffers_bad(n, i, 2, o, 2), STEP_MISALIGNED, 1, -1, "misaligned input");
        expect(step_buffers_bad(n, in3, 3, o, 2), STEP_MISALIGNED, 3, -1, "misaligned output");
        const StepBuf o3[2] = {{slot(2), "prev"}, {at(3, 3), "m0"}};
        expect(step_buffers_bad(n, in3, 3, o3, 2), STEP_MISALIGNED, 4, -1, "misaligned second output");
        const StepBuf ov[2] = {{at(0, 1), "prev"}, {slot(3), "m0"}};    // misaligned and overlapping: alignment is reported
        expect(step_buffers_bad(n, in3, 3, ov, 2), STEP_MISALIGNED, 3, -1, "alignment before overlap");
    }
    {   // out against out: equal, shifted, and before the same output's inputs
        const StepBuf same[2] = {{slot(2), "prev"}, {slot(2), "m0"}};
        expect(step_buffers_bad(n, in3, 3, same, 2), STEP_OUT_OUT, 1, 0, "two outputs on one base");
        const StepBuf sh[2] = {{slot(2), "prev"}, {at(2, 12), "m0"}};
        expect(step_buffers_bad(n, in3, 3, sh, 2), STEP_OUT_OUT, 1, 0, "two outputs 48 bytes apart");
        const StepBuf both[2] = {{slot(1), "prev"}, {slot(1), "m0"}};     // each is its input's base, but they are each other's too
        expect(step_buffers_bad(n, in3, 3, both, 2), STEP_OUT_OUT, 1, 0, "two outputs on one input's base");
        const StepBuf third[3] = {{slot(2), "prev"}, {slot(3), "m0"}, {at(3, 4), "xc"}};
        expect(step_buffers_bad(n, in3, 3, third, 3), STEP_OUT_OUT, 2, 1, "third output against the second");
        const StepBuf first[2] = {{at(0, 4), "prev"}, {at(0, 8), "m0"}};  // the first output's input comes before the second's output
        expect(step_buffers_bad(n, in3, 3, first, 2), STEP_OUT_IN, 0, 0, "outputs in order");
    }
    {   // n = 1: neighbours 16 bytes apart share nothing; the same address does
        const StepBuf i[1] = {{slot(0), "x"}};
        const StepBuf o[1] = {{at(0, 4), "out"}};
        expect(step_buffers_bad(1, i, 1, o, 1), STEP_OK, -1, -1, "n = 1, 16 bytes apart");
        expect(step_buffers_bad(4, i, 1, o, 1), STEP_OK, -1, -1, "n = 4, touching");
        expect(step_buffers_bad(5, i, 1, o, 1), STEP_OUT_IN, 0, 0, "n = 5, one float shared");
        const StepBuf o2[2] = {{slot(0), "out"}, {slot(0), "out2"}};
        expect(step_buffers_bad(1, i, 1, o2, 1), STEP_OK, -1, -1, "n = 1, same base");
        expect(step_buffers_bad(1, i, 1, o2, 2), STEP_OUT_OUT, 1, 0, "n = 1, out against out");
    }
    expect(step_buffers_bad(n, nullptr, 0, out2, 2), STEP_OK, -1, -1, "no inputs");
    expect(step_buffers_bad(n, in3, 3, nullptr, 0), STEP_OK, -1, -1, "no outputs");
    std::printf(fails ? "step_check: %d failure(s)\n" : "step_check: ok\n", fails);
    return fails ? 1 : 0;
}
