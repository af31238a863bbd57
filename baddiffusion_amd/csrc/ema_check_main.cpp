// Stand-alone driver of ema_check.h for the host sanitizers (tests/test_ema_host.py builds it with -fsanitize=address,undefined).
// Not part of libbd_hip.so.  Exit status 0 = every case answered as expected.
#include "ema_check.h"

#include <cstdio>
#include <limits>
#include <vector>

int main() {
    using bd::ema_args_bad;
    using bd::ranges_overlap;
    int fails = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) { std::printf("FAIL %s\n", what); ++fails; }
    };
    std::vector<float> buf(64);
    float* b = buf.data();
    const int64_t n = 16;
    expect(ranges_overlap(b, b, n), "same pointer");
    expect(ranges_overlap(b, b + 1, n) && ranges_overlap(b + 1, b, n), "shifted by one float");
    expect(ranges_overlap(b, b + n - 1, n) && ranges_overlap(b + n - 1, b, n), "last element shared");
    expect(!ranges_overlap(b, b + n, n) && !ranges_overlap(b + n, b, n), "adjacent ranges");
    expect(!ranges_overlap(b, b + 1, 1), "n = 1 neighbours");
    // the largest n an int64 holds must not overflow the byte count into a false negative for equal pointers
    expect(ranges_overlap(b, b, std::numeric_limits<int64_t>::max() / 8), "huge n, same pointer");
    const float* four[4] = {b + 16, b + 32, b + 48, b + 16};
    expect(ema_args_bad(b, four, 4, n, 0.f) == 0 && ema_args_bad(b, four, 4, n, 1.f) == 0 && ema_args_bad(b, four, 4, n, 1e-4f) == 0, "valid arguments");
    expect(ema_args_bad(b, four, 4, n, -0.1f) == 1 && ema_args_bad(b, four, 4, n, 1.5f) == 1, "one_minus_decay outside [0, 1]");
    expect(ema_args_bad(b, four, 4, n, std::numeric_limits<float>::quiet_NaN()) == 1, "one_minus_decay NaN");
    expect(ema_args_bad(b, four, 4, n, std::numeric_limits<float>::infinity()) == 1, "one_minus_decay inf");
    for (int k = 0; k < 4; ++k) {
        const float* o[4] = {b + 16, b + 32, b + 48, b + 16};
        o[k] = b + 15;
        expect(ema_args_bad(b + 16, o, 4, n, 0.5f) == 2, "overlap with one of the four");
    }
    const float* one[1] = {b + 8};
    expect(ema_args_bad(b, one, 1, n, 0.5f) == 2 && ema_args_bad(b, one, 1, 8, 0.5f) == 0, "single other range");
    expect(ema_args_bad(b, nullptr, 0, n, 0.5f) == 0, "no other range");
    std::printf(fails ? "ema_check: %d failure(s)\n" : "ema_check: ok\n", fails);
    return fails ? 1 : 0;
}
