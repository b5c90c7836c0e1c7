// What the chain kernels share: fwd_chain_kernel (fwd_chain.hip) and
// bwd_chain_kernel (bwd_chain.hip) both keep an R x 256 tile in LDS from
// layer to layer and run a 256-wide layer as the same MFMA chain with B
// straight from L2, so both promise the bits of the unfused gemm_nt
// chain through ONE text of the geometry, the K-loop, the accumulator
// scatter and the piece loop; their launchers share the arm dispatch.
//
// The device pieces are statement macros and a loop-header macro, not
// functions, for head_dev.h's reason: as force-inlined function
// templates the K-loop and the piece loop changed the instructions of
// most instantiations; as macros every kernel compiles to the very
// instructions it had with the code written in place
// (profiles/r11_chain_shared.md, scripts/isa_diff.py).  They read the
// kernel's tid / lane split (tid, wave, lrow, kch) and the geometry
// constants by name.
#pragma once

#include "head_dev.h"

#include <type_traits>

// operands in the global address space: pointers that arrive inside the
// by-value argument block would otherwise compile to FLAT accesses,
// which count on lgkmcnt with the LDS reads
using gbf16 = __attribute__((address_space(1))) __bf16;
using gbf16x8 = __attribute__((address_space(1))) bf16x8;

// Tile geometry of a block of NW waves that owns R batch rows; wave w
// owns columns [w*256/NW, +256/NW) of every layer's output.
#define CHAIN_GEOMETRY(R, NW)                                                \
    constexpr int H = 256;                                                   \
    constexpr int NT = NW * 64;                                              \
    constexpr int LDT = H + 8;       /* padded tile row (bf16) */            \
    constexpr int PPR = H / 8;       /* 16-B pieces per tile row */          \
    constexpr int NP = R * PPR / NT; /* pieces per thread */                 \
    constexpr int FM = R / 16;       /* 16-row fragments per tile */         \
    constexpr int WN = H / NW;       /* columns per wave */                  \
    constexpr int FN = WN / 16;                                              \
    constexpr int NSTEP = H / 32;    /* K-steps of a 256-wide layer */       \
    /* K-steps per B load group: two where the accumulators leave room */    \
    constexpr int U = (FM * FN <= 8 && NW == 4) ? 2 : 1;                     \
    constexpr int UNR = NW == 4 ? NSTEP / U : 1; /* K-loop unroll count */   \
    static_assert(R * PPR % NT == 0, "piece mapping")

// Loop header over this thread's 16-B pieces of the tile: piece i is
// columns [col, col + 8) of tile row r.  Followed by the loop body.
#define CHAIN_FOR_PIECES(i, r, col)                                          \
    _Pragma("unroll") for (int i = 0; i < NP; ++i)                           \
        if (const int q_ = tid + i * NT, r = q_ / PPR,                       \
            col = (q_ % PPR) * 8; true)

// acc[FM][FN] += tile (A, LDS) · w^T for one 256-wide layer: w is
// [256][256] with K contiguous (gbf16*), 32-wide K-steps in increasing
// order.  B fragments of this wave's columns go straight from L2 to
// registers, U K-steps per load group, the next group in flight under
// the current group's MFMAs.  Fully unrolled with four waves; the
// eight-wave arms keep the loop rolled to stay inside their 128 VGPRs
// (they spilled otherwise).
#define CHAIN_LAYER_MMA(acc, tile, w)                                        \
    {                                                                        \
        const gbf16* const wp = w + (long)(wave * WN + lrow) * H + kch * 8;  \
        bf16x8 b[U][FN], bn[U][FN];                                          \
        auto load_b = [&](bf16x8(&bb)[U][FN], int t0) {                      \
            _Pragma("unroll") for (int u = 0; u < U; ++u)                    \
                _Pragma("unroll") for (int j = 0; j < FN; ++j)               \
                    bb[u][j] = *(const gbf16x8*)(wp + (long)j * 16 * H +     \
                                                 (t0 + u) * 32);             \
        };                                                                   \
        load_b(b, 0);                                                        \
        _Pragma("unroll UNR")                                                \
        for (int t0 = 0; t0 < NSTEP; t0 += U) {                              \
            if (t0 + U < NSTEP) load_b(bn, t0 + U);                          \
            _Pragma("unroll") for (int u = 0; u < U; ++u) {                  \
                bf16x8 a_frag[FM];                                           \
                _Pragma("unroll") for (int i = 0; i < FM; ++i)               \
                    a_frag[i] = *(const bf16x8*)&tile[i * 16 + lrow]         \
                                                    [(t0 + u) * 32 + kch * 8]; \
                _Pragma("unroll") for (int i = 0; i < FM; ++i)               \
                    _Pragma("unroll") for (int j = 0; j < FN; ++j)           \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16( \
                            a_frag[i], b[u][j], acc[i][j], 0, 0, 0);         \
            }                                                                \
            if (t0 + U < NSTEP) {                                            \
                _Pragma("unroll") for (int u = 0; u < U; ++u)                \
                    _Pragma("unroll") for (int j = 0; j < FN; ++j)           \
                        b[u][j] = bn[u][j];                                  \
            }                                                                \
        }                                                                    \
    }

// The same layer, same MFMAs in the same order, with the B fragments
// CHAIN_B_AHEAD K-steps ahead: a ring of CHAIN_B_AHEAD + 1 named register
// sets, the loop fully unrolled so that every set index is a constant
// and no set is ever copied into another.  Step t's MFMAs wait for set
// t alone; the loads of steps t+1 .. t+CHAIN_B_AHEAD stay in flight
// under them.  (CHAIN_LAYER_MMA hands bn over to b at the end of a step;
// that copy waits for the next step's loads, so its lookahead is one
// step in the source and none in the instructions.)  For the eight-wave
// arms of fwd_chain_kernel.
#define CHAIN_B_AHEAD 3
#define CHAIN_LAYER_MMA_AHEAD(acc, tile, w)                                  \
    {                                                                        \
        const gbf16* const wp = w + (long)(wave * WN + lrow) * H + kch * 8;  \
        bf16x8 bq[CHAIN_B_AHEAD + 1][FN];                                    \
        auto load_b = [&](bf16x8(&bb)[FN], int t) {                          \
            _Pragma("unroll") for (int j = 0; j < FN; ++j)                   \
                bb[j] = *(const gbf16x8*)(wp + (long)j * 16 * H + t * 32);   \
        };                                                                   \
        _Pragma("unroll") for (int t = 0; t < CHAIN_B_AHEAD; ++t)            \
            load_b(bq[t], t);                                                \
        _Pragma("unroll") for (int t = 0; t < NSTEP; ++t) {                  \
            if (t + CHAIN_B_AHEAD < NSTEP)                                   \
                load_b(bq[(t + CHAIN_B_AHEAD) % (CHAIN_B_AHEAD + 1)],        \
                       t + CHAIN_B_AHEAD);                                   \
            /* fences: left alone, the scheduler sinks the loads to just */  \
            /* above their first use */                                      \
            __builtin_amdgcn_sched_barrier(0);                               \
            bf16x8 a_frag[FM];                                               \
            _Pragma("unroll") for (int i = 0; i < FM; ++i)                   \
                a_frag[i] = *(const bf16x8*)&tile[i * 16 + lrow]             \
                                                [t * 32 + kch * 8];          \
            _Pragma("unroll") for (int i = 0; i < FM; ++i)                   \
                _Pragma("unroll") for (int j = 0; j < FN; ++j)               \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(     \
                        a_frag[i], bq[t % (CHAIN_B_AHEAD + 1)][j],           \
                        acc[i][j], 0, 0, 0);                                 \
            __builtin_amdgcn_sched_barrier(0);                               \
        }                                                                    \
    }

// acc[FM][FN] -> tile, each element rounded once by f2bf.  EPILOGUE is
// the caller's statement(s) on `float v` between the accumulator and the
// rounding (j is the column fragment, for a per-column operand), or
// empty.  The caller has made sure that no wave still reads the tile.
#define CHAIN_ACC_TO_TILE(acc, tile, EPILOGUE)                               \
    _Pragma("unroll") for (int i = 0; i < FM; ++i)                           \
        _Pragma("unroll") for (int j = 0; j < FN; ++j)                       \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                  \
                float v = acc[i][j][r];                                      \
                EPILOGUE;                                                    \
                tile[i * 16 + kch * 4 + r][wave * WN + j * 16 + lrow] =      \
                    bf_bits(f2bf(v));                                        \
            }

// ---------------------------------------------------------------- host

// The (rows, waves) arms both chains are built for.  Calls
// f(std::integral_constant<int, rows>{}, std::integral_constant<int,
// waves>{}), in the manner of with_bools, and returns true; false, with
// f not called, for any other pair.
template <class F>
inline bool with_chain_arm(int rows, int waves, F&& f) {
    using std::integral_constant;
    if (rows == 32 && waves == 4)
        f(integral_constant<int, 32>{}, integral_constant<int, 4>{});
    else if (rows == 32 && waves == 8)
        f(integral_constant<int, 32>{}, integral_constant<int, 8>{});
    else if (rows == 64 && waves == 4)
        f(integral_constant<int, 64>{}, integral_constant<int, 4>{});
    else if (rows == 64 && waves == 8)
        f(integral_constant<int, 64>{}, integral_constant<int, 8>{});
    else
        return false;
    return true;
}
