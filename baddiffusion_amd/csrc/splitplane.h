// The device vocabulary of the split-plane MFMA kernels (conv_ps.hip, conv_ph.hip, gemm_sp.hip, attn_sp.hip): operands are bf16 hi | lo
// planes in 128-byte rows (per row, every 32-element block is one line: 64 B of hi, 64 B of lo), DMA'd global -> LDS 16 bytes per lane
// into bank-swizzled slots and multiplied as lo*hi + hi*lo + hi*hi (or hi*hi alone) on v_mfma_f32_32x32x16_bf16.  What every one of
// those kernels does the same way lives here ONCE; tile shapes, rings and schedules stay with the kernels.
#pragma once
#include "common.h"

namespace bd {

typedef float sp_floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 sp_bf16x8 __attribute__((ext_vector_type(8)));
typedef short sp_short4 __attribute__((ext_vector_type(4)));
typedef short sp_short8 __attribute__((ext_vector_type(8)));
typedef unsigned sp_uint4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* sp_lds_ptr;
typedef const __attribute__((address_space(1))) void* sp_gbl_ptr;

// bank swizzle of the 16-byte slots of a 128-byte LDS row (row stride 128 B = half a 256-byte bank row): rows r and
// r^1 share a bank row, f spreads 16 consecutive rows over the 8 slots x 2 halves -> every ds_read_b128 lane group
// (16 lanes = 16 different rows, same logical slot) touches each bank once.
__device__ __forceinline__ int sp_swz(int row) { return (row >> 1) & 7; }

// (the DMA source of lanes whose filter tap falls outside the image is common.h's zero page, bd_zero16)
__device__ __forceinline__ void sp_dma16(const char* src, char* lds_dst) {
    __builtin_amdgcn_global_load_lds((sp_gbl_ptr)src, (sp_lds_ptr)lds_dst, 16, 0, 0);
}

// sp_wait<N>: until at most N of this wave's DMAs are outstanding AND all of its LDS reads have returned (N is an assembly-time
// literal).  sp_sync<N>: the same, then the workgroup barrier: behind it the chunk is visible to every wave and the stage read last
// may be refilled.  Raw s_barrier: a __syncthreads() would drain the DMAs in flight (vmcnt(0)).
template <int N>
__device__ __forceinline__ void sp_wait() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit count");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void sp_sync() {
    sp_wait<N>();
    __builtin_amdgcn_s_barrier();
}

// LDS reads as inline asm, address = LDS byte offset.  hipcc puts `s_waitcnt vmcnt(0)` in front of the intrinsic form
// whenever LDS-DMA loads are in flight (it cannot tell the stage being read from the stage being filled), so every chunk
// waited for the NEXT chunk's DMA before its first fragment read.  The asm form is opaque to that pass; the matching
// s_waitcnt lgkmcnt(0) is tied to the fragment registers by the caller so that no consumer can be scheduled above it.
template <int OFF>
__device__ __forceinline__ sp_short4 sp_read_tr(unsigned addr) {      // hardware transpose read of a K-major image
    sp_short4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <int OFF>
__device__ __forceinline__ sp_short8 sp_read128(unsigned addr) {      // one 16-byte slot of a K-contiguous image
    sp_short8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
__device__ __forceinline__ sp_bf16x8 sp_join(sp_short8 v) { return __builtin_bit_cast(sp_bf16x8, v); }
__device__ __forceinline__ sp_bf16x8 sp_join(sp_short4 v0, sp_short4 v1) {
    return sp_join(__builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- one K chunk (32 of K = two MFMA steps) of a wave's TM x 2 grid of 32 x 32 tiles, both operands K-contiguous -------------------
// fragment addresses: lane -> row li of a 32-row tile, k octet h; logical slot = plane*4 + step*2 + h
__device__ __forceinline__ void sp_frag_offsets(int (&foff)[2][2], int li, int h) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) foff[s][pl] = li * 128 + (((pl * 4 + s * 2 + h) ^ sp_swz(li)) << 4);
}
// a0 / b0: the wave's first A / B row in the LDS stage (32-row tiles 4096 bytes apart).  Within a K step all lo*hi, then all hi*lo,
// then all hi*hi; SP (BD_MODE_BF16): hi fragments only, one MFMA per product.
template <bool SP, int TM>
__device__ __forceinline__ void sp_mma_chunk(const char* a0, const char* b0, const int (&foff)[2][2], sp_floatx16 (&acc)[TM][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        sp_bf16x8 ah[TM], al[TM], bh[2], bl[2];
        if constexpr (TM == 1) {
            ah[0] = *reinterpret_cast<const sp_bf16x8*>(a0 + foff[s][0]);
            if constexpr (!SP) al[0] = *reinterpret_cast<const sp_bf16x8*>(a0 + foff[s][1]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (TM == 2) {
                ah[i] = *reinterpret_cast<const sp_bf16x8*>(a0 + i * 4096 + foff[s][0]);
                if constexpr (!SP) al[i] = *reinterpret_cast<const sp_bf16x8*>(a0 + i * 4096 + foff[s][1]);
            }
            bh[i] = *reinterpret_cast<const sp_bf16x8*>(b0 + i * 4096 + foff[s][0]);
            if constexpr (!SP) bl[i] = *reinterpret_cast<const sp_bf16x8*>(b0 + i * 4096 + foff[s][1]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) if constexpr (!SP) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[q], acc[i][q], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) if constexpr (!SP) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[q], acc[i][q], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[q], acc[i][q], 0, 0, 0);
    }
}

}  // namespace bd
