// Host-only check of split_k() (csrc/common.h) against the three K-split bodies it replaced in conv_ps.hip, copied here verbatim.
//   hipcc -x hip --cuda-host-only -std=c++17 scripts/check_split_k.cpp -o check_split_k && ./check_split_k
// Sweeps slots {64 .. 512} x tiles 1..600 x nchunks 1..600 x mincps {4, 8}; ksplit and cps must agree everywhere.  Needs no device.
#include "../baddiffusion_amd/csrc/common.h"

using bd::cdiv;

// ps_small_split (mincps 4)
static void old_small(int slots, long long tiles, int nchunks, int mincps, int& ksplit, int& cps) {
    int ks = (int)(slots / tiles);
    if (ks < 1) ks = 1;
    if (ks > nchunks / mincps) ks = nchunks / mincps;
    if (ks < 1) ks = 1;
    cps = (int)cdiv(nchunks, ks);
    ksplit = (int)cdiv(nchunks, cps);
}
// ps_wgrad_split and ups_wgrad_split (mincps 8)
static void old_wgrad(int slots, long long tiles, int nchunks, int mincps, int& ksplit, int& cps) {
    int ks = (int)(slots / tiles);
    if (ks < 1) ks = 1;
    if (ks > nchunks / mincps) ks = nchunks / mincps > 0 ? nchunks / mincps : 1;
    cps = (int)cdiv(nchunks, ks);
    ksplit = (int)cdiv(nchunks, cps);
}

int main() {
    const int slots_set[] = {64, 96, 128, 192, 256, 304, 512};
    long long n = 0, bad = 0;
    for (int slots : slots_set)
        for (int mincps : {4, 8})
            for (long long tiles = 1; tiles <= 600; ++tiles)
                for (int nchunks = 1; nchunks <= 600; ++nchunks) {
                    int k0, c0, k1, c1, k2, c2;
                    bd::split_k(slots, tiles, nchunks, mincps, k0, c0);
                    old_small(slots, tiles, nchunks, mincps, k1, c1);
                    old_wgrad(slots, tiles, nchunks, mincps, k2, c2);
                    ++n;
                    if (k0 != k1 || c0 != c1 || k0 != k2 || c0 != c2) {
                        if (++bad <= 10) printf("MISMATCH slots %d tiles %lld nchunks %d mincps %d: new %d/%d small %d/%d wgrad %d/%d\n", slots, tiles, nchunks, mincps, k0, c0, k1, c1, k2, c2);
                    }
                }
    printf("split_k: %lld cases, %lld mismatches\n", n, bad);
    return bad ? 1 : 0;
}
