// Register-staged tile load of the gemm_nt kernels (gemm.hip).
#pragma once

#include "common.h"

// LDS row padding (+8 bf16 = 16 B) of the tiles StageReg writes:
// conflict-free ds_read_b128 fragment reads (Guideline 4)
#define LDS_PAD 8

// Staging is split into an ISSUE half (global -> registers, with
// bounds zero-fill and the optional fused >0 mask) and a WRITE half
// (registers -> padded LDS tile) so the HBM latency of tile t+1 hides
// under tile t's MFMA work (async-STAGE split, one barrier per K-step;
// cdna_hip_programming.md Guideline 15 / T14).
template <int TILE_ROWS, int KSTEP, int NT, bool HAS_MASK>
struct StageReg {
    static constexpr int EL = TILE_ROWS * KSTEP / NT;  // 4..32
    __bf16 v[EL];

    __device__ __forceinline__ void load(const __bf16* __restrict__ src,
                                         const __bf16* __restrict__ msk,
                                         int nrows, int K, int row0, int k0,
                                         int tid) {
        const int off = tid * EL;
        const int r = off / KSTEP, c = off % KSTEP;
        const int g = row0 + r, gk = k0 + c;
        if (g < nrows && gk + EL <= K) {
#pragma unroll
            for (int ch = 0; ch < EL; ch += (EL < 8 ? 4 : 8)) {
                if constexpr (EL >= 8) {
                    bf16x8 t = *(const bf16x8*)&src[(long)g * K + gk + ch];
                    if constexpr (HAS_MASK) {
                        bf16x8 mk =
                            *(const bf16x8*)&msk[(long)g * K + gk + ch];
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (!(bf2f(mk[i]) > 0.f)) t[i] = (__bf16)0.f;
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[ch + i] = t[i];
                } else {
                    bf16x4v t = *(const bf16x4v*)&src[(long)g * K + gk + ch];
                    if constexpr (HAS_MASK) {
                        bf16x4v mk =
                            *(const bf16x4v*)&msk[(long)g * K + gk + ch];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (!(bf2f(mk[i]) > 0.f)) t[i] = (__bf16)0.f;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[ch + i] = t[i];
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < EL; ++i) {
                __bf16 t = (__bf16)0.f;
                if (g < nrows && gk + i < K) {
                    t = src[(long)g * K + gk + i];
                    if constexpr (HAS_MASK) {
                        if (!(bf2f(msk[(long)g * K + gk + i]) > 0.f))
                            t = (__bf16)0.f;
                    }
                }
                v[i] = t;
            }
        }
    }

    __device__ __forceinline__ void write(
        ushort (*__restrict__ dst)[KSTEP + LDS_PAD], int tid) const {
        const int off = tid * EL;
        const int r = off / KSTEP, c = off % KSTEP;
#pragma unroll
        for (int ch = 0; ch < EL; ch += (EL < 8 ? 4 : 8)) {
            if constexpr (EL >= 8) {
                bf16x8 t;
#pragma unroll
                for (int i = 0; i < 8; ++i) t[i] = v[ch + i];
                *(bf16x8*)&dst[r][c + ch] = t;
            } else {
                bf16x4v t;
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = v[ch + i];
                *(bf16x4v*)&dst[r][c + ch] = t;
            }
        }
    }
};
