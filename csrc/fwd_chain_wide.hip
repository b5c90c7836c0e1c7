// Training forward as ONE kernel at hidden widths 128 and 512 (gfx950 /
// MI355X): the wide sibling of fwd_chain.hip, which serves width 256.
//
//   per ReLU layer l, bottom to top (out = H):
//     h_l   = bf16(relu(h_{l-1} · W_l^T + b_l))              (stored)
//   probs   = softmax(bf16(h_top · W_head^T + b_head))       (stored)
//
// The split and the data movement are fused_mlp_wide.hip's: a block of
// NW waves owns R batch rows in ONE activation tile, tile[R][H + 8] bf16
// in LDS, rewritten in place layer after layer (two tiles stop fitting
// twice on a CU at H = 512):
//
//   * wave w holds ALL of its output columns [w * H/NW, +H/NW) of the
//     layer in FM x FN f32 accumulator fragments, so nothing of the tile
//     is overwritten before the block barrier that ends the K loop;
//   * W never passes through LDS: each wave reads the B fragments of its
//     own columns straight from L2 into registers, three K-steps ahead in
//     a ring of four named sets (CHAIN_LAYER_MMA_AHEAD);
//   * the first layer takes any in_dims % 8 == 0: x is streamed through
//     two [R][KC + 8] chunk buffers that ALIAS the still-empty tile, one
//     barrier per chunk, the loads of chunk c + 1 issued ahead of chunk
//     c's MFMAs.  Rows past M and columns past in_dims are zeros in both
//     operands.
//
// What training adds to the serving kernel: every h_l leaves the tile
// once, as 16-B row-contiguous stores, because the backward needs it (it
// is never read back), and the head ends in HEAD_FWD_EPILOGUE and writes
// bf16 probs.
//
// Bits: a layer is the v_mfma_f32_16x16x32_bf16 chain of gemm_nt_kernel,
// 32-wide K-steps in increasing order from a zero accumulator, followed
// by that kernel's epilogue, v = acc + bias; v = v > 0 ? v : 0; f2bf(v).
// The head is the MFMA chain and the register epilogue of
// head_fwd_fused_kernel (head_dev.h).  Every output equals the per-layer
// path bit for bit.
//
// Launch contract (the launcher returns false outside it): H 128 or 512,
// C <= 16, 1..8 layers, M >= 1, in_dims of the first layer a multiple of
// 8, every pointer 16-B aligned, (rows, waves) one of the built arms.
// Arms, resources and the shipped choice: docs/KERNELS.md, "Chain
// kernels, wide"; profiles/r20_chain_wide.md.

// This file's device code is built without packed f32 arithmetic (no
// v_pk_add/mul/fma_f32), as a per-file -target-feature -packed-fp32-ops
// would: the attribute must also reach the helpers of the headers below,
// or they could not be inlined into the kernel.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "chain_wide.h"

namespace {

// The layers of one launch, bottom first.  Passed BY VALUE: nothing to
// upload, nothing to keep alive, and legal under graph capture.
struct FwdWideLayers {
    const void* w[SS_FWD_CHAIN_MAX];  // W [H][in]
    const void* b[SS_FWD_CHAIN_MAX];  // bias [H]
    void* h[SS_FWD_CHAIN_MAX];        // post-ReLU output [M][H]
};

template <int HH, int R, int NW>
__global__ __launch_bounds__(NW * 64)
void fwd_chain_wide_kernel(
    const __bf16* __restrict__ x,       // [M][K0]: input of layer 0
    const FwdWideLayers L, int nlayers,
    const __bf16* __restrict__ W_head,  // [C][H]
    const __bf16* __restrict__ b_head,  // [C]
    __bf16* __restrict__ probs,         // [M][C]
    int M, int K0, int C) {
    // the names CHAIN_LAYER_MMA_AHEAD, CHAIN_ACC_TO_TILE and
    // CHAIN_FOR_PIECES read
    constexpr int H = HH;
    constexpr int NT = NW * 64;
    constexpr int LDT = H + 8;        // padded tile row (bf16)
    constexpr int PPR = H / 8;        // 16-B pieces per tile row
    constexpr int NP = R * PPR / NT;  // pieces per thread
    constexpr int FM = R / 16;        // 16-row fragments per tile
    constexpr int WN = H / NW;        // columns per wave
    constexpr int FN = WN / 16;
    constexpr int NSTEP = H / 32;     // K-steps of a hidden layer
    static_assert(WN % 16 == 0 && FN >= 1 && R % 16 == 0, "fragment split");
    static_assert(R * PPR % NT == 0 && NP >= 1, "piece mapping");
    static_assert(FM <= NW, "one head fragment per wave");
    static_assert(NSTEP > CHAIN_B_AHEAD, "K loop");
    // every built arm keeps B three K-steps ahead: accumulators + the ring
    // of four B sets + the A fragments leave some thirty registers for
    // addresses (no arm needs CHAIN_LAYER_MMA's one-step loop)
    static_assert(4 * FM * FN + 16 * FN + 4 * FM + 30 <= wide_reg_budget(NW),
                  "register budget of CHAIN_LAYER_MMA_AHEAD");
    // first-layer stage: KC columns of x per chunk, two chunks in the tile
    constexpr int KC = H / 4 < 128 ? H / 4 : 128;
    constexpr int LDX = KC + 8;       // padded stage row (bf16)
    constexpr int XPR = KC / 8;       // 16-B pieces per stage row
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
    // acc -> tile through the gemm_nt_kernel epilogue (bias, ReLU, one
    // rounding), then the tile -> h_l as 16-B row-contiguous stores.  The
    // caller has made sure that no wave still reads the tile; the barrier
    // in here makes the new tile whole for whatever reads it next.
    auto finish_layer = [&](int l) {
        CHAIN_ACC_TO_TILE(acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f)
        __syncthreads();
        gbf16* const ho = (gbf16*)L.h[l];
        CHAIN_FOR_PIECES(i, r, col) {
            if (row0 + r < M)
                *(gbf16x8*)&ho[(long)(row0 + r) * H + col] =
                    *(const bf16x8*)&tile[r][col];
        }
    };

    // ---- layer 0 from x: chunk c sits in xs buffer c & 1; the loads of
    // chunk c + 1 are issued ahead of chunk c's MFMAs and written after
    // them; the barrier that ends a chunk frees the buffer that the next
    // one overwrites
    {
        const gbf16* const w = (const gbf16*)L.w[0];
        const int nsteps = cdiv(K0, 32);
        const int nchunks = cdiv(K0, KC);
        bf16x8 xr[XP];
        auto xload = [&](int c) {
#pragma unroll
            for (int p = 0; p < XP; ++p) {
                const int q = tid + p * NT;
                const int r = q / XPR, k = c * KC + (q % XPR) * 8;
                xr[p] = zero8();
                if (q < R * XPR && row0 + r < M && k < K0)
                    xr[p] = *(const bf16x8*)&x[(long)(row0 + r) * K0 + k];
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
        // B fragments of K-step s: W rows of this wave's columns, the
        // 8-element pieces past K0 as zeros (K0 % 8 == 0)
        const gbf16* const wp = w + (long)(wave * WN + lrow) * K0 + kch * 8;
        auto load_b = [&](bf16x8(&bb)[FN], int s) {
            const bool in = s * 32 + kch * 8 < K0;
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                bb[j] = zero8();
                if (in)
                    bb[j] = *(const gbf16x8*)(wp + (long)j * 16 * K0 + s * 32);
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
                const bool more = s0 + kk + 1 < nsteps;
                if (more) load_b(bn, s0 + kk + 1);
                mma_step(b, c & 1, kk);
                if (more) {
#pragma unroll
                    for (int j = 0; j < FN; ++j) b[j] = bn[j];
                }
            }
            if (c + 1 < nchunks) xwrite((c + 1) & 1);
            __syncthreads();  // also: every wave has left the stage
        }
        finish_layer(0);
    }

    // ---- the H-wide layers, in place: the tile holds h_{l-1} (the h
    // store above only reads it, and so does the K loop)
    for (int l = 1; l < nlayers; ++l) {
        const gbf16* const w = (const gbf16*)L.w[l];
        load_bias(l);
        zero_acc();
        CHAIN_LAYER_MMA_AHEAD(acc, tile, w)
        __syncthreads();  // every wave has read the tile
        finish_layer(l);
    }

    // ---- head: wave i < FM takes rows [16 i, +16) of the tile (whole
    // since the barrier inside finish_layer; nothing writes it again)
    // against W_head's rows, rows >= C as zeros; K in order, as
    // head_fwd_fused_kernel
    if (wave < FM) {
        const bool cvalid = lrow < C;
        const __bf16* wp = W_head + (long)min(lrow, C - 1) * H + kch * 8;
        f32x4 hacc[1];
        hacc[0] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int t = 0; t < NSTEP; ++t) {
            const bf16x8 a =
                *(const bf16x8*)&tile[wave * 16 + lrow][t * 32 + kch * 8];
            bf16x8 bfrag = *(const bf16x8*)(wp + t * 32);
            if (!cvalid) bfrag = zero8();
            hacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag, hacc[0],
                                                              0, 0, 0);
        }
        const int row_base = row0 + wave * 16;
        HEAD_FWD_EPILOGUE(1, hacc, b_head, probs, cvalid, lrow, kch, row_base,
                          M, C)
    }
}

}  // namespace

bool ss_chain_wide_arm_built(int H, int rows, int waves) {
    if (H != 128 && H != 512) return false;
    chain_wide_shipped(H, 1, rows, waves);
    auto none = [](auto, auto, auto) {};
    return H == 128 ? with_chain_wide_arm<128>(rows, waves, none)
                    : with_chain_wide_arm<512>(rows, waves, none);
}

// rows / waves: 0 = the shipped choice (docs/KERNELS.md, "Chain kernels,
// wide"); any other pair must be one of with_chain_wide_arm's.
bool ss_fwd_chain_wide(const void* x, const void* const* w,
                       const void* const* b, void* const* h, int nlayers,
                       const void* W_head, const void* b_head, void* probs,
                       int M, int K0, int H, int C, int rows, int waves,
                       hipStream_t st) {
    if (M < 1 || M > INT32_MAX - 64 || (H != 128 && H != 512) || C < 1 ||
        C > 16 || nlayers < 1 || nlayers > SS_FWD_CHAIN_MAX || K0 < 8 ||
        K0 % 8 != 0)
        return false;
    if (!aligned16(x) || !aligned16(W_head) || !aligned16(b_head) ||
        !aligned16(probs))
        return false;
    FwdWideLayers L = {};
    for (int l = 0; l < nlayers; ++l) {
        if (!aligned16(w[l]) || !aligned16(b[l]) || !aligned16(h[l]))
            return false;
        L.w[l] = w[l];
        L.b[l] = b[l];
        L.h[l] = h[l];
    }
    chain_wide_shipped(H, M, rows, waves);
    auto launch = [&](auto hh, auto r, auto nw) {
        constexpr int HH = hh.value, R = r.value, NW = nw.value;
        hipLaunchKernelGGL((fwd_chain_wide_kernel<HH, R, NW>),
                           dim3(cdiv(M, R)), dim3(NW * 64), 0, st,
                           (const __bf16*)x, L, nlayers,
                           (const __bf16*)W_head, (const __bf16*)b_head,
                           (__bf16*)probs, M, K0, C);
    };
    return H == 128 ? with_chain_wide_arm<128>(rows, waves, launch)
                    : with_chain_wide_arm<512>(rows, waves, launch);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
