// Device code of the classifier head that more than one kernel runs:
// head_bwd_fused_kernel (head.hip) and bwd_chain_kernel (bwd_chain.hip)
// both produce dz and dx of the head through these, and
// head_fwd_fused_kernel and fwd_chain_kernel (fwd_chain.hip) both
// produce probs through HEAD_FWD_EPILOGUE, so the pairs cannot drift
// apart in their bits.
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

// Register epilogue of the head forward, run by head_fwd_fused_kernel
// (head.hip) and fwd_chain_kernel (fwd_chain.hip): acc[FR] are the
// 16x16 logit fragments of rows row_base + f*16.. (lane (kch, lrow)
// holds rows kch*4 + r of column lrow; the 16 lanes of one kch hold one
// row).  Bias, the logit rounded to bf16 as the unfused path stores it,
// row max, __expf, the xor tree over the row's 16 lanes and the scaled
// store of probs[M][C]; cvalid = lrow < C.
#define HEAD_FWD_EPILOGUE(FR, acc, bias, probs, cvalid, lrow, kch,          \
                          row_base, M, C)                                    \
    const float bv = cvalid ? bf2f(bias[lrow]) : 0.f;                        \
    _Pragma("unroll") for (int f = 0; f < FR; ++f) {                         \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                      \
            float v = acc[f][r];                                             \
            v += bv;                                                         \
            v = bf2f(f2bf(v)); /* the logit as the unfused path stores it */ \
            float m = cvalid ? fmaxf(-1e30f, v) : -1e30f;                    \
            _Pragma("unroll") for (int off = 8; off > 0; off >>= 1)          \
                m = fmaxf(m, __shfl_xor(m, off, 64));                        \
            const float e = cvalid ? __expf(v - m) : 0.f;                    \
            float s = e;                                                     \
            _Pragma("unroll") for (int off = 8; off > 0; off >>= 1)          \
                s += __shfl_xor(s, off, 64);                                 \
            const float inv = 1.f / s;                                       \
            const int row = row_base + f * 16 + kch * 4 + r;                 \
            if (cvalid && row < M)                                           \
                probs[(long)row * C + lrow] = f2bf(e * inv);                 \
        }                                                                    \
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
