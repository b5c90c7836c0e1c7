// Persistent fused MLP forward for hidden widths 128 .. 1024 (serving
// path, gfx950 / MI355X): the wide sibling of fused_mlp.hip.
//
//   x [M][in_dim] -> H (ReLU) -> H (ReLU) x (nhidden - 1) -> cout
//
// One launch runs the whole chain.  A block of NW waves owns R batch rows
// and keeps them in ONE activation tile, tile[R][H + 8] bf16 in LDS,
// rewritten in place layer after layer (fused_mlp.hip's two buffers stop
// fitting at H = 512; at H = 1024, R = 64 the single tile is 132 KB of
// the CU's 160 KB):
//
//   * wave w holds ALL of its output columns [w * H/NW, +H/NW) of the
//     layer in f32 accumulators (FM x FN 16x16 fragments), so nothing of
//     the tile is overwritten before the block barrier that follows the K
//     loop; then bias + ReLU + one bf16 rounding go back into the tile;
//   * W never passes through LDS (little is left beside the tile): each
//     wave reads the B fragments of its own columns straight from L2 into
//     registers, three K-steps ahead where the registers allow it
//     (CHAIN_LAYER_MMA_AHEAD), one ahead otherwise (CHAIN_LAYER_MMA);
//   * the first layer streams x through two [R][KC + 8] chunk buffers that
//     ALIAS the tile, which holds nothing yet.  Rows past M, columns past
//     in_dim and rows that are not 16-B aligned (in_dim % 8 != 0) are
//     filled element by element, with zeros where there is no data;
//   * the head is one 16-column fragment per 16 rows: wave i < FM runs
//     rows [16 i, +16) over the whole K, adds the bias and takes the row
//     argmax over the 16 lanes that hold a row by an xor tree (lowest
//     index among equal maxima).  The logits that go out on request are
//     the very f32 values the argmax is taken over.
//
// Rounding points are those of the eager chain: every hidden activation
// is bf16(relu(acc + bias)), rounded once; accumulation is f32 MFMA with
// K in increasing order.  Layer pointers travel by value in the kernel
// arguments: no descriptor upload, legal under graph capture.
//
// The (R, NW) arms per width and the shipped choice: docs/KERNELS.md,
// "Fused serving forward, wide"; profiles/r19_fused_mlp_wide.md.

// This file's device code is built without packed f32 arithmetic (no
// v_pk_add/mul/fma_f32), as a per-file -target-feature -packed-fp32-ops
// would: the attribute must also reach the helpers of the headers below,
// or they could not be inlined into the kernel.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "chain_dev.h"
#include "launchers.h"

namespace {

// Hidden layers 0 .. nhidden-1, then the head at index nhidden.
struct FusedMlpLayers {
    const void* w[SS_FUSED_MLP_MAX + 1];  // [H][in_dim], [H][H].., [cout][H]
    const void* b[SS_FUSED_MLP_MAX + 1];  // bias of each
};

// Registers per lane that a block of NW waves leaves each of its waves
// when it has a CU to itself: the 512 of a SIMD over its NW / 4 waves.
constexpr int wide_reg_budget(int NW) { return NW <= 8 ? 256 : 2048 / NW; }

template <int HH, int R, int NW>
__global__ __launch_bounds__(NW * 64)
void fused_mlp_wide_kernel(
    const __bf16* __restrict__ x,  // [M][K0]
    const FusedMlpLayers L, int nhidden,
    int M, int K0, int C,
    int* __restrict__ amax,        // [M]
    float* __restrict__ logits) {  // [M][C] or null
    // the names CHAIN_LAYER_MMA* and CHAIN_ACC_TO_TILE read
    constexpr int H = HH;
    constexpr int NT = NW * 64;
    constexpr int LDT = H + 8;     // padded tile row (bf16)
    constexpr int FM = R / 16;     // 16-row fragments per tile
    constexpr int WN = H / NW;     // columns per wave
    constexpr int FN = WN / 16;
    constexpr int NSTEP = H / 32;  // K-steps of a hidden layer
    // K loop: B three steps ahead where accumulators + the ring of four B
    // sets + the A fragments leave some thirty registers for addresses
    constexpr bool AH =
        4 * FM * FN + 16 * FN + 4 * FM + 30 <= wide_reg_budget(NW);
    constexpr int U = 1;           // CHAIN_LAYER_MMA: one step per group,
    constexpr int UNR = 2;         // unrolled by two (four spills)
    static_assert(WN % 16 == 0 && FN >= 1 && R % 16 == 0, "fragment split");
    static_assert(FM <= NW, "one head fragment per wave");
    static_assert(NSTEP % UNR == 0 && NSTEP > CHAIN_B_AHEAD, "K loop");
    // first-layer stage: KC columns of x per chunk, two chunks in the tile
    constexpr int KC = H / 4 < 128 ? H / 4 : 128;
    constexpr int LDX = KC + 8;    // padded stage row (bf16)
    constexpr int XPR = KC / 8;    // 16-B pieces per stage row
    constexpr int XP = cdiv(R * XPR, NT);  // stage pieces per thread
    static_assert(2 * LDX <= LDT && KC % 32 == 0, "x stage inside the tile");

    __shared__ __attribute__((aligned(16))) ushort tile[R][LDT];
    // chunk buffer b = rows [b * R, +R) of xs
    ushort(*const xs)[LDX] = (ushort(*)[LDX]) & tile[0][0];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lrow = lane & 15;
    const int kch = lane >> 4;
    const int row0 = blockIdx.x * R;

    f32x4 acc[FM][FN];
    float bv[FN];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
    };
    auto load_bias = [&](int l) {
        const gbf16* const bias = (const gbf16*)L.b[l];
#pragma unroll
        for (int j = 0; j < FN; ++j)
            bv[j] = bf2f((__bf16)bias[wave * WN + j * 16 + lrow]);
    };

    // ---- layer 0 from x: chunk c sits in xs buffer c & 1; the loads of
    // chunk c + 1 are issued ahead of chunk c's MFMAs and written after
    // them; the barrier that ends a chunk frees the buffer that the next
    // one overwrites
    {
        const gbf16* const w = (const gbf16*)L.w[0];
        // 16-B pieces only where every row of x and W starts on one
        const bool vec = K0 % 8 == 0 && ((unsigned long)x & 15) == 0;
        const int nsteps = cdiv(K0, 32);
        const int nchunks = cdiv(K0, KC);
        bf16x8 xr[XP];
        auto xload = [&](int c) {
#pragma unroll
            for (int p = 0; p < XP; ++p) {
                const int q = tid + p * NT;
                const int r = q / XPR, k = c * KC + (q % XPR) * 8;
                xr[p] = zero8();
                if (q < R * XPR && row0 + r < M && k < K0) {
                    const __bf16* src = x + (long)(row0 + r) * K0 + k;
                    if (vec) {
                        xr[p] = *(const bf16x8*)src;
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (k + e < K0) xr[p][e] = src[e];
                    }
                }
            }
        };
        auto xwrite = [&](int buf) {
#pragma unroll
            for (int p = 0; p < XP; ++p) {
                const int q = tid + p * NT;
                if (q < R * XPR)
                    *(bf16x8*)&xs[buf * R + q / XPR][(q % XPR) * 8] = xr[p];
            }
        };
        // B fragments of K-step s: W rows of this wave's columns
        const gbf16* const wp = w + (long)(wave * WN + lrow) * K0 + kch * 8;
        auto load_b = [&](bf16x8(&bb)[FN], int s) {
            const int k = s * 32 + kch * 8;
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                bb[j] = zero8();
                if (k < K0) {
                    const gbf16* src = wp + (long)j * 16 * K0 + s * 32;
                    if (vec) {
                        bb[j] = *(const gbf16x8*)src;
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (k + e < K0) bb[j][e] = (__bf16)src[e];
                    }
                }
            }
        };
        auto mma_step = [&](const bf16x8(&bb)[FN], int buf, int kk) {
            bf16x8 a_frag[FM];
#pragma unroll
            for (int i = 0; i < FM; ++i)
                a_frag[i] = *(const bf16x8*)&xs[buf * R + i * 16 + lrow]
                                              [kk * 32 + kch * 8];
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_frag[i], bb[j], acc[i][j], 0, 0, 0);
        };
        bf16x8 b[FN], bn[FN];
        load_bias(0);
        xload(0);
        load_b(b, 0);
        xwrite(0);
        zero_acc();
        __syncthreads();
        for (int c = 0; c < nchunks; ++c) {
            if (c + 1 < nchunks) xload(c + 1);
            const int s0 = c * (KC / 32);
            const int ns = min(KC / 32, nsteps - s0);
            for (int kk = 0; kk < ns; ++kk) {
                if constexpr (AH) {
                    const bool more = s0 + kk + 1 < nsteps;
                    if (more) load_b(bn, s0 + kk + 1);
                    mma_step(b, c & 1, kk);
                    if (more) {
#pragma unroll
                        for (int j = 0; j < FN; ++j) b[j] = bn[j];
                    }
                } else {
                    // no room for a second B set beside 128 accumulator
                    // registers: each step loads its own (spilled otherwise)
                    if (c + kk > 0) load_b(b, s0 + kk);
                    mma_step(b, c & 1, kk);
                }
            }
            if (c + 1 < nchunks) xwrite((c + 1) & 1);
            __syncthreads();  // also: every wave has left the stage
        }
        CHAIN_ACC_TO_TILE(acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f)
        __syncthreads();
    }

    // ---- the H-wide layers, in place: the tile holds h_{l-1}
    for (int l = 1; l < nhidden; ++l) {
        const gbf16* const w = (const gbf16*)L.w[l];
        load_bias(l);
        zero_acc();
        if constexpr (AH) {
            CHAIN_LAYER_MMA_AHEAD(acc, tile, w)
        } else {
            CHAIN_LAYER_MMA(acc, tile, w)
        }
        __syncthreads();  // every wave has read the tile
        CHAIN_ACC_TO_TILE(acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f)
        __syncthreads();
    }

    // ---- head: wave i < FM takes rows [16 i, +16) of the tile against
    // the head's rows (rows >= C as zeros), K in order
    if (wave < FM) {
        const bool cvalid = lrow < C;
        const gbf16* const wp =
            (const gbf16*)L.w[nhidden] + (long)min(lrow, C - 1) * H + kch * 8;
        f32x4 hacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int t = 0; t < NSTEP; ++t) {
            const bf16x8 a =
                *(const bf16x8*)&tile[wave * 16 + lrow][t * 32 + kch * 8];
            bf16x8 bfrag = *(const gbf16x8*)(wp + t * 32);
            if (!cvalid) bfrag = zero8();
            hacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag, hacc, 0,
                                                           0, 0);
        }
        const float hb =
            cvalid ? bf2f((__bf16)((const gbf16*)L.b[nhidden])[lrow]) : 0.f;
        // lane (kch, lrow) holds rows kch * 4 + r of column lrow; the 16
        // lanes of one kch hold one row
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + wave * 16 + kch * 4 + r;
            const float v = hacc[r] + hb;
            if (logits && cvalid && row < M) logits[(long)row * C + lrow] = v;
            float best = cvalid ? v : -INFINITY;
            int bi = cvalid ? lrow : 16;
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) {
                const float ov = __shfl_xor(best, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (ov > best || (ov == best && oi < bi)) {
                    best = ov;
                    bi = oi;
                }
            }
            if (lrow == 0 && row < M) amax[row] = bi;
        }
    }
}

// The (rows, waves) arms built per width; f as with_chain_arm's.
template <int H, class F>
bool with_wide_arm(int rows, int waves, F&& f) {
    using std::integral_constant;
    auto arm = [&](auto r, auto nw) {
        if (rows != r.value || waves != nw.value) return false;
        f(integral_constant<int, H>{}, r, nw);
        return true;
    };
    using I32 = integral_constant<int, 32>;
    using I64 = integral_constant<int, 64>;
    using W4 = integral_constant<int, 4>;
    using W8 = integral_constant<int, 8>;
    using W16 = integral_constant<int, 16>;
    if constexpr (H == 128)
        return arm(I32{}, W4{}) || arm(I64{}, W4{});
    else if constexpr (H == 256)
        return arm(I32{}, W4{}) || arm(I64{}, W4{}) || arm(I64{}, W8{});
    else if constexpr (H == 512)
        return arm(I32{}, W8{}) || arm(I64{}, W8{}) || arm(I64{}, W16{});
    else
        return arm(I32{}, W8{}) || arm(I32{}, W16{}) || arm(I64{}, W8{});
}

}  // namespace

// rows / waves: 0 = the shipped choice, measured at M = 1024 and 16384
// (profiles/r19_fused_mlp_wide.md): where 64-row tiles would cover at most
// half of the 256 CUs (M <= 8192) 32 rows with 4 / 8 / 16 waves at
// H = 128 / 512 / 1024, above that 64 rows with 4 / 16 / 8 waves; H = 256
// takes 64 rows and 8 waves at every M.  Any other pair must be one of
// with_wide_arm's.
bool ss_fused_mlp_wide(const void* x, const void* const* w,
                       const void* const* b, int nhidden, const void* w_head,
                       const void* b_head, void* argmax, void* logits, int M,
                       int in_dim, int H, int cout, int rows, int waves,
                       hipStream_t stream) {
    if (M < 1 || M > INT32_MAX - 64 || in_dim < 1 || nhidden < 1 ||
        nhidden > SS_FUSED_MLP_MAX || cout < 1 || cout > 16)
        return false;
    if (H != 128 && H != 256 && H != 512 && H != 1024) return false;
    if (!x || !argmax || !aligned16(w_head) || !b_head) return false;
    FusedMlpLayers L = {};
    for (int l = 0; l < nhidden; ++l) {
        if (!aligned16(w[l]) || !b[l]) return false;
        L.w[l] = w[l];
        L.b[l] = b[l];
    }
    L.w[nhidden] = w_head;
    L.b[nhidden] = b_head;
    const bool few = cdiv(M, 64) <= 128;
    if (!rows) rows = few && H != 256 ? 32 : 64;
    if (!waves)
        waves = H == 128 ? 4 : H == 256 ? 8 : H == 512 ? (few ? 8 : 16)
                                                       : (few ? 16 : 8);
    auto launch = [&](auto h, auto r, auto nw) {
        constexpr int HH = h.value, R = r.value, NW = nw.value;
        hipLaunchKernelGGL((fused_mlp_wide_kernel<HH, R, NW>),
                           dim3(cdiv(M, R)), dim3(NW * 64), 0, stream,
                           (const __bf16*)x, L, nhidden, M, in_dim, cout,
                           (int*)argmax, (float*)logits);
    };
    switch (H) {
        case 128: return with_wide_arm<128>(rows, waves, launch);
        case 256: return with_wide_arm<256>(rows, waves, launch);
        case 512: return with_wide_arm<512>(rows, waves, launch);
        default: return with_wide_arm<1024>(rows, waves, launch);
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
