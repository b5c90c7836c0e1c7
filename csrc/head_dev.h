// Device code of the classifier-head backward that more than one kernel
// runs: head_bwd_fused_kernel (head.hip) and bwd_chain_kernel
// (bwd_chain.hip) both produce dz and dx of the head through these, so
// the two cannot drift apart in their bits.
//
// The two larger pieces are statement macros, not functions: as
// force-inlined functions they left head_bwd_fused_kernel with a
// different instruction schedule (the callee is simplified on its own
// before it is inlined); as macros the kernel compiles to the very
// instructions it had with the code written in place.
#pragma once

#include "common.h"

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.f;
    return z;
}

__device__ __forceinline__ ushort bf_bits(__bf16 v) {
    return *(const ushort*)&v;
}

// dz of one head element: bf16((p - t) / GB)
__device__ __forceinline__ __bf16 head_dz_elem(__bf16 pb, __bf16 tb,
                                               float inv_gb) {
    return f2bf((bf2f(pb) - bf2f(tb)) * inv_gb);
}

// W^T rows [k0, k0 + kc) of the head, zero-padded to 16 classes, into
// wts[KC][16] (LDS): thread k < KC stages row k, rows past kc as zeros.
#define HEAD_STAGE_WT(KC, wts, Wt, k0, kc, C, tid)                           \
    if (tid < KC) {                                                          \
        __bf16 w[16];                                                        \
        _Pragma("unroll") for (int c = 0; c < 16; ++c) {                     \
            w[c] = (__bf16)0.f;                                              \
            if (tid < kc && c < C) w[c] = Wt[(long)(k0 + tid) * C + c];      \
        }                                                                    \
        bf16x8 lo, hi;                                                       \
        _Pragma("unroll") for (int c = 0; c < 8; ++c) {                      \
            lo[c] = w[c];                                                    \
            hi[c] = w[c + 8];                                                \
        }                                                                    \
        *(bf16x8*)&wts[tid][0] = lo;                                         \
        *(bf16x8*)&wts[tid][8] = hi;                                         \
    }

// Declares f32x4 `acc`: one 16x16 dx fragment of the head, rows rg*16..
// of dz (dzs[.][16] in LDS, class index = k slot) against W^T rows
// ct*16.. (wts).  The accumulator starts at zero and takes ONE MFMA;
// lanes kch >= 2 hold k >= 16: zeros.
#define HEAD_DX_FRAG(acc, dzs, wts, rg, ct, lrow, kch)                       \
    bf16x8 af = zero8(), bfr = zero8();                                      \
    if (kch < 2) {                                                           \
        af = *(const bf16x8*)&dzs[rg * 16 + lrow][kch * 8];                  \
        bfr = *(const bf16x8*)&wts[ct * 16 + lrow][kch * 8];                 \
    }                                                                        \
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};                                        \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc, 0, 0, 0)
