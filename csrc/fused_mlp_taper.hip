// Persistent fused MLP forward for hidden widths that change from layer
// to layer (serving path, gfx950 / MI355X): fused_mlp_wide.hip's sibling
// for models such as 784 -> 512 -> 256 -> 128 -> 10.
//
//   x [M][in_dim] -> N_0 (ReLU) -> N_1 (ReLU) .. -> N_{n-1} (ReLU) -> cout
//
// every N_l one of 128 / 256 / 512 / 1024, in any order, 1..8 of them.
// One launch runs the whole chain.  A block of NW waves owns R batch rows
// in ONE activation tile, tile[R][HMAX + 8] bf16 in LDS, HMAX the largest
// width of the model:
//
//   * the row stride is HMAX + 8 through the whole launch, whatever the
//     current layer's width: 16 rows of a ds_read_b128 A fragment land on
//     different banks in every layer.  Layer l reads columns [0, K_l) and
//     writes [0, N_l); columns at or past N_l keep what a wider earlier
//     layer left there, and the next layer's K loop ends before them;
//   * wave w holds ALL of its output columns [w * N_l/NW, +N_l/NW) in f32
//     accumulators, so nothing of the tile is overwritten before the block
//     barrier that follows the K loop (the in-place rule of the uniform
//     kernel).  The accumulator shape FM x N_l/NW/16 has to be a constant:
//     the layer body is a template on N_l, reached through a block-uniform
//     switch over the four widths, with K_l a run-time multiple of 128;
//   * W never passes through LDS: B fragments go from L2 to registers,
//     three K-steps ahead in a ring of four named register sets where the
//     registers of that N_l allow it.  K_l / 32 is a multiple of four, so
//     four steps make one turn of the ring and the unrolled unit; the
//     loads carry no guard (a step past the end reads the last step again
//     and is never used).  One step ahead otherwise;
//   * the first layer streams x through two [R][KC + 8] chunk buffers that
//     alias the still empty tile, exactly as the uniform kernel does, into
//     N_0 columns;
//   * the head is the uniform kernel's: one 16-column fragment per 16 rows
//     on waves < FM over K = N_{n-1}, bias, f32 logits on request, xor-tree
//     argmax, lowest index among equal maxima.
//
// Rounding points and order are the uniform kernel's: h_l = bf16(relu(acc
// + b_l)) rounded once, v_mfma_f32_16x16x32_bf16 from a zero accumulator
// with K increasing.  At equal widths this kernel gives that kernel's
// bits.  Pointers and widths travel by value in the kernel arguments.
//
// Arms, resources and measurements: docs/KERNELS.md, "Fused serving
// forward, mixed widths"; profiles/r21_fused_mlp_taper.md.

// Built without packed f32 arithmetic, for fused_mlp_wide.hip's reason:
// the attribute has to reach the helpers of the headers below too.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "chain_dev.h"
#include "launchers.h"

namespace {

// Hidden layers 0 .. nhidden-1, then the head at index nhidden.
struct TaperLayers {
    const void* w[SS_FUSED_MLP_MAX + 1];  // [N_0][in_dim], [N_l][N_{l-1}]..,
                                          // [cout][N_{n-1}]
    const void* b[SS_FUSED_MLP_MAX + 1];  // bias of each
    int n[SS_FUSED_MLP_MAX];              // N_l
};

// Registers per lane that a block of NW waves leaves each of its waves
// when it has a CU to itself.
constexpr int wide_reg_budget(int NW) { return NW <= 8 ? 256 : 2048 / NW; }

template <int HMAX, int R, int NW>
__global__ __launch_bounds__(NW * 64)
void fused_mlp_taper_kernel(
    const __bf16* __restrict__ x,  // [M][K0]
    const TaperLayers L, int nhidden,
    int M, int K0, int C,
    int* __restrict__ amax,        // [M]
    float* __restrict__ logits) {  // [M][C] or null
    constexpr int NT = NW * 64;
    constexpr int LDT = HMAX + 8;  // tile row (bf16), the same in every layer
    constexpr int FM = R / 16;     // 16-row fragments per tile
    static_assert(R % 16 == 0 && FM <= NW, "one head fragment per wave");
    // first-layer stage: KC columns of x per chunk, two chunks in the tile
    constexpr int KC = HMAX / 4 < 128 ? HMAX / 4 : 128;
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

    // f(integral_constant<N>) for the layer width n: block-uniform, and
    // only the widths this arm is built for (the launcher saw to that)
    auto with_width = [&](int n, auto&& f) {
        using std::integral_constant;
        switch (n) {
            case 128:
                if constexpr (128 / NW >= 16) f(integral_constant<int, 128>{});
                break;
            case 256:
                if constexpr (256 <= HMAX && 256 / NW >= 16)
                    f(integral_constant<int, 256>{});
                break;
            case 512:
                if constexpr (512 <= HMAX) f(integral_constant<int, 512>{});
                break;
            case 1024:
                if constexpr (1024 <= HMAX) f(integral_constant<int, 1024>{});
                break;
        }
    };

    // ---- layer 0 from x into N columns: chunk c sits in xs buffer c & 1;
    // the loads of chunk c + 1 are issued ahead of chunk c's MFMAs and
    // written after them; the barrier that ends a chunk frees the buffer
    // that the next one overwrites
    auto first_layer = [&](auto nc) {
        constexpr int N = nc.value;
        constexpr int WN = N / NW;  // columns per wave
        constexpr int FN = WN / 16;
        constexpr bool AH =
            4 * FM * FN + 16 * FN + 4 * FM + 30 <= wide_reg_budget(NW);
        const gbf16* const w = (const gbf16*)L.w[0];
        const gbf16* const bias = (const gbf16*)L.b[0];
        // 16-B pieces only where every row of x and W starts on one
        const bool vec = K0 % 8 == 0 && ((unsigned long)x & 15) == 0;
        const int nsteps = cdiv(K0, 32);
        const int nchunks = cdiv(K0, KC);
        f32x4 acc[FM][FN];
        float bv[FN];
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
#pragma unroll
        for (int j = 0; j < FN; ++j)
            bv[j] = bf2f((__bf16)bias[wave * WN + j * 16 + lrow]);
        xload(0);
        load_b(b, 0);
        xwrite(0);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
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
                    // no room for a second B set: each step loads its own
                    if (c + kk > 0) load_b(b, s0 + kk);
                    mma_step(b, c & 1, kk);
                }
            }
            if (c + 1 < nchunks) xwrite((c + 1) & 1);
            __syncthreads();  // also: every wave has left the stage
        }
        CHAIN_ACC_TO_TILE(acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f)
        __syncthreads();
    };

    // ---- layer l >= 1, in place: tile columns [0, K) hold h_{l-1}, K a
    // multiple of 128; columns [0, N) take h_l
    auto hidden_layer = [&](auto nc, int l, int K) {
        constexpr int N = nc.value;
        constexpr int WN = N / NW;
        constexpr int FN = WN / 16;
        constexpr bool AH =
            4 * FM * FN + 16 * FN + 4 * FM + 30 <= wide_reg_budget(NW);
        constexpr int NB = CHAIN_B_AHEAD + 1;
        const gbf16* const bias = (const gbf16*)L.b[l];
        const int nstep = K / 32;  // a multiple of NB
        // W_l is at most 2 MB: 32-bit element offsets from one base
        const gbf16* const w = (const gbf16*)L.w[l];
        const unsigned wo = (unsigned)(wave * WN + lrow) * K + kch * 8;
        // the loads carry no guard: a step past the end reads the last
        // step again, inside the row, and is never used
        auto load_b = [&](bf16x8(&bb)[FN], int t) {
            const unsigned off = wo + min(t, nstep - 1) * 32;
#pragma unroll
            for (int j = 0; j < FN; ++j)
                bb[j] = *(const gbf16x8*)(w + (off + (unsigned)(j * 16) * K));
        };
        f32x4 acc[FM][FN];
        float bv[FN];
#pragma unroll
        for (int j = 0; j < FN; ++j)
            bv[j] = bf2f((__bf16)bias[wave * WN + j * 16 + lrow]);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
        auto mma_step = [&](const bf16x8(&bb)[FN], int t) {
            bf16x8 a_frag[FM];
#pragma unroll
            for (int i = 0; i < FM; ++i)
                a_frag[i] =
                    *(const bf16x8*)&tile[i * 16 + lrow][t * 32 + kch * 8];
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_frag[i], bb[j], acc[i][j], 0, 0, 0);
        };
        if constexpr (AH) {
            // step kk of every turn reads set kk: no set is ever copied
            bf16x8 bq[NB][FN];
#pragma unroll
            for (int t = 0; t < CHAIN_B_AHEAD; ++t) load_b(bq[t], t);
            for (int t0 = 0; t0 < nstep; t0 += NB) {
#pragma unroll
                for (int kk = 0; kk < NB; ++kk) {
                    load_b(bq[(kk + CHAIN_B_AHEAD) % NB],
                           t0 + kk + CHAIN_B_AHEAD);
                    // fences: left alone, the scheduler sinks the loads to
                    // just above their first use
                    __builtin_amdgcn_sched_barrier(0);
                    mma_step(bq[kk], t0 + kk);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
            // two sets taking turns, no copies (nstep is even)
            bf16x8 b[FN], bn[FN];
            load_b(b, 0);
            for (int t = 0; t < nstep; t += 2) {
                load_b(bn, t + 1);
                mma_step(b, t);
                load_b(b, t + 2);
                mma_step(bn, t + 1);
            }
        }
        __syncthreads();  // every wave has read the tile
        CHAIN_ACC_TO_TILE(acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f)
        __syncthreads();
    };

    with_width(L.n[0], first_layer);
    for (int l = 1; l < nhidden; ++l)
        with_width(L.n[l], [&](auto nc) { hidden_layer(nc, l, L.n[l - 1]); });

    // ---- head: wave i < FM takes rows [16 i, +16) of the tile against
    // the head's rows (rows >= C as zeros), K in order
    if (wave < FM) {
        const int K = L.n[nhidden - 1];
        const int nstep = K / 32;
        const bool cvalid = lrow < C;
        const gbf16* const wp =
            (const gbf16*)L.w[nhidden] + (long)min(lrow, C - 1) * K + kch * 8;
        f32x4 hacc = {0.f, 0.f, 0.f, 0.f};
        for (int t0 = 0; t0 < nstep; t0 += 4) {  // nstep % 4 == 0
#pragma unroll
            for (int t = t0; t < t0 + 4; ++t) {
                const bf16x8 a =
                    *(const bf16x8*)&tile[wave * 16 + lrow][t * 32 + kch * 8];
                bf16x8 bfrag = *(const gbf16x8*)(wp + t * 32);
                if (!cvalid) bfrag = zero8();
                hacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag, hacc,
                                                               0, 0, 0);
            }
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

// The (rows, waves) arms built per largest width; f as with_chain_arm's.
template <int HMAX, class F>
bool with_taper_arm(int rows, int waves, F&& f) {
    using std::integral_constant;
    auto arm = [&](auto r, auto nw) {
        if (rows != r.value || waves != nw.value) return false;
        f(integral_constant<int, HMAX>{}, r, nw);
        return true;
    };
    using I32 = integral_constant<int, 32>;
    using I64 = integral_constant<int, 64>;
    using W4 = integral_constant<int, 4>;
    using W8 = integral_constant<int, 8>;
    using W16 = integral_constant<int, 16>;
    if constexpr (HMAX == 128)
        return arm(I32{}, W4{}) || arm(I64{}, W4{});
    else if constexpr (HMAX == 256)
        return arm(I32{}, W4{}) || arm(I64{}, W4{}) || arm(I64{}, W8{});
    else if constexpr (HMAX == 512)
        return arm(I32{}, W8{}) || arm(I64{}, W8{}) || arm(I64{}, W16{});
    else
        return arm(I32{}, W8{}) || arm(I32{}, W16{}) || arm(I64{}, W8{});
}

}  // namespace

// rows / waves: 0 = the shipped choice per (largest width, few / many
// tiles), measured at M = 1024 and 16384 on 784,512,256,128,10 and
// 784,1024,256,10 (profiles/r21_fused_mlp_taper.md); "few" is where
// 64-row tiles would cover at most half of the 256 CUs (M <= 8192).  Any
// other pair must be one of with_taper_arm's for the largest width, with
// at least 16 columns of the narrowest layer per wave.
bool ss_fused_mlp_taper(const void* x, const void* const* w,
                        const void* const* b, const int* widths, int nhidden,
                        const void* w_head, const void* b_head, void* argmax,
                        void* logits, int M, int in_dim, int cout, int rows,
                        int waves, hipStream_t stream) {
    if (M < 1 || M > INT32_MAX - 64 || in_dim < 1 || nhidden < 1 ||
        nhidden > SS_FUSED_MLP_MAX || cout < 1 || cout > 16)
        return false;
    if (!x || !argmax || !widths || !aligned16(w_head) || !b_head)
        return false;
    TaperLayers L = {};
    int hmax = 0, hmin = 1024;
    for (int l = 0; l < nhidden; ++l) {
        const int n = widths[l];
        if (n != 128 && n != 256 && n != 512 && n != 1024) return false;
        if (!aligned16(w[l]) || !b[l]) return false;
        L.w[l] = w[l];
        L.b[l] = b[l];
        L.n[l] = n;
        hmax = n > hmax ? n : hmax;
        hmin = n < hmin ? n : hmin;
    }
    L.w[nhidden] = w_head;
    L.b[nhidden] = b_head;
    const bool few = cdiv(M, 64) <= 128;
    if (!rows) rows = few && hmax != 256 ? 32 : 64;
    if (!waves) waves = hmax == 128 ? 4 : 8;
    if (hmin / waves < 16) return false;  // a wave owns >= 16 columns
    auto launch = [&](auto h, auto r, auto nw) {
        constexpr int HMAX = h.value, R = r.value, NW = nw.value;
        hipLaunchKernelGGL((fused_mlp_taper_kernel<HMAX, R, NW>),
                           dim3(cdiv(M, R)), dim3(NW * 64), 0, stream,
                           (const __bf16*)x, L, nhidden, M, in_dim, cout,
                           (int*)argmax, (float*)logits);
    };
    switch (hmax) {
        case 128: return with_taper_arm<128>(rows, waves, launch);
        case 256: return with_taper_arm<256>(rows, waves, launch);
        case 512: return with_taper_arm<512>(rows, waves, launch);
        default: return with_taper_arm<1024>(rows, waves, launch);
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
