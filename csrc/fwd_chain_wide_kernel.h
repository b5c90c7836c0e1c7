// The text of the wide forward chain kernel and of its launch (see
// fwd_chain_wide.hip), compiled once per arm, each arm in a translation
// unit of its own, which defines
//
//   FWD_WIDE_KERNEL   the kernel's name
//   FWD_WIDE_LAUNCH   the name of the arm's (file-local) launch function
//   FWD_WIDE_DROP     (optional, default 0) the arm under dropout
//                     (fwd_chain_wide_drop.hip): a FwdChainDrop block
//                     follows the layers, and a layer whose bit is set in
//                     it masks its epilogue.
//                     2: the keep bits are drawn before the layer's K
//                        loop (shipped, as at width 256)
//                     1: in the epilogue (for an arm that cannot hold the
//                        bits through its K loop)
//   FWD_WIDE_HEAD     (optional, default 1) 0: the stage arm
//                     (fwd_chain_wide_stage.hip, .._stage_drop.hip), for a
//                     pipeline stage with no classifier head: no W_head /
//                     b_head / probs / C, the kernel ends with the h_top
//                     store, and layer 0 has a second start, from a
//                     stored H-wide activation (`tile0`, below)
//
// The arms share text through the preprocessor and not through a
// function template for fwd_chain_kernel.h's reason: this way the plain
// arm compiles to the instructions it has with its text written in
// place (scripts/isa_diff.py).  The including file pushes the
// no-packed-fp32-ops attribute around this header.

#include "chain_wide.h"

#ifndef FWD_WIDE_DROP
#define FWD_WIDE_DROP 0
#endif
#ifndef FWD_WIDE_HEAD
#define FWD_WIDE_HEAD 1
#endif
#if FWD_WIDE_DROP
#include "dropout_dev.h"
#endif

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
void FWD_WIDE_KERNEL(
    const __bf16* __restrict__ x,       // [M][K0]: input of layer 0
    const FwdWideLayers L, int nlayers,
#if FWD_WIDE_DROP
    const FwdChainDrop D,
#endif
#if FWD_WIDE_HEAD
    const __bf16* __restrict__ W_head,  // [C][H]
    const __bf16* __restrict__ b_head,  // [C]
    __bf16* __restrict__ probs,         // [M][C]
    int M, int K0, int C) {
#else
    // tile0 (block-uniform, K0 == H only): x goes straight into the tile
    // and layer 0 runs the in-place K loop of the later layers
    int M, int K0, int tile0) {
#endif
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
    // registers of a layer's keep bits: a nibble per fragment
    constexpr int NKB = FWD_WIDE_DROP ? (FM * FN + 7) / 8 : 0;
    static_assert(WN % 16 == 0 && FN >= 1 && R % 16 == 0, "fragment split");
    static_assert(R * PPR % NT == 0 && NP >= 1, "piece mapping");
#if FWD_WIDE_HEAD
    static_assert(FM <= NW, "one head fragment per wave");
#endif
    static_assert(NSTEP > CHAIN_B_AHEAD, "K loop");
    // every built arm keeps B three K-steps ahead: accumulators + the ring
    // of four B sets + the A fragments (+ the keep bits that stay live
    // through the loop) leave some thirty registers for addresses (no arm
    // needs CHAIN_LAYER_MMA's one-step loop)
    static_assert(4 * FM * FN + 16 * FN + 4 * FM + NKB + 30 <=
                      wide_reg_budget(NW),
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
#if FWD_WIDE_DROP
    // Keep bits of a layer: fragment (i, j) owns nibble i * FN + j, bit r
    // of it is row r of this lane's column (dropout_keep4_frag), so a
    // layer's mask lives in NKB registers: one, two at 64 rows on eight
    // waves.  One Philox call per fragment and lane: lane & 3 draws tile
    // row i * 16 + kch * 4 + (lane & 3) for the quad's column group.
    // Rows past M draw as well (the quad exchange needs every lane) and
    // are never stored.
    unsigned kb[NKB];
    auto draw_mask = [&](int l) {
        const DropoutArgs d = {D.key0,      D.key1,       D.layer[l], D.step,
                               D.row_first, D.row_stride, D.thr[l],   1.f};
        const int q = lane & 3;
#pragma unroll
        for (int n = 0; n < NKB; ++n) kb[n] = 0u;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
                kb[(i * FN + j) / 8] |=
                    dropout_keep4_frag(
                        d, dropout_sample(d, row0 + i * 16 + kch * 4 + q),
                        (unsigned)(wave * WN + j * 16 + lrow) >> 2, q)
                    << ((i * FN + j) % 8 * 4);
    };
    // block-uniform: whether layer l draws a mask at all
    auto drops = [&](int l) { return (D.on >> l) & 1u; };
#endif
    // acc -> tile through the gemm_nt_kernel epilogue (bias, ReLU, one
    // rounding; under dropout the mask and the scale ahead of the
    // rounding, as gemm_nt_kernel<.., DROPOUT>), then the tile -> h_l as
    // 16-B row-contiguous stores.  The caller has made sure that no wave
    // still reads the tile; the barrier in here makes the new tile whole
    // for whatever reads it next.
    auto finish_layer = [&](int l) {
#if FWD_WIDE_DROP
        if (drops(l)) {
#if FWD_WIDE_DROP == 1
            draw_mask(l);
#endif
            const float scale = D.scale[l];
            CHAIN_ACC_TO_TILE(
                acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f;
                v = (kb[(i * FN + j) / 8] >> ((i * FN + j) % 8 * 4 + r)) & 1u
                        ? v * scale
                        : 0.f)
        } else
#endif
        {
            CHAIN_ACC_TO_TILE(acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f)
        }
        __syncthreads();
        gbf16* const ho = (gbf16*)L.h[l];
        CHAIN_FOR_PIECES(i, r, col) {
            if (row0 + r < M)
                *(gbf16x8*)&ho[(long)(row0 + r) * H + col] =
                    *(const bf16x8*)&tile[r][col];
        }
    };

#if FWD_WIDE_HEAD
    constexpr int l0 = 1;
#else
    // ---- a middle stage: x is a stored H-wide activation and IS the
    // tile of layer 0, rows past M as zeros.  No x stage and no chunk
    // barriers: one barrier, then the loop below from l = 0, B three
    // K-steps ahead.  Same K order as the streamed start, so same bits.
    const int l0 = tile0 ? 0 : 1;
    if (tile0) {
        CHAIN_FOR_PIECES(i, r, col) {
            bf16x8 v = zero8();
            if (row0 + r < M)
                v = *(const bf16x8*)&x[(long)(row0 + r) * H + col];
            *(bf16x8*)&tile[r][col] = v;
        }
        __syncthreads();
    } else
#endif
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
#if FWD_WIDE_DROP == 2
        if (drops(0)) draw_mask(0);
#endif
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
    for (int l = l0; l < nlayers; ++l) {
        const gbf16* const w = (const gbf16*)L.w[l];
        load_bias(l);
#if FWD_WIDE_DROP == 2
        if (drops(l)) draw_mask(l);
#endif
        zero_acc();
        CHAIN_LAYER_MMA_AHEAD(acc, tile, w)
        __syncthreads();  // every wave has read the tile
        finish_layer(l);
    }

#if FWD_WIDE_HEAD
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
#endif
}

// This arm's launch.  rows / waves: 0 = the shipped choice (docs/KERNELS.md,
// "Chain kernels, wide"); any other pair must be one of
// with_chain_wide_arm's.  The arm under dropout takes its FwdChainDrop
// block and refuses one that masks no layer of the launch, names a layer
// past nlayers, carries a scale or threshold that no p in [0, 1) gives,
// or whose last row is no 32-bit sample id.  The stage arm takes `start`
// in place of the head: 0 = by K0 (the tile start at K0 == H), 1 = the
// streamed first layer, 2 = the tile start, refused unless K0 == H.
bool FWD_WIDE_LAUNCH(const void* x, const void* const* w,
                     const void* const* b, void* const* h, int nlayers,
#if FWD_WIDE_HEAD
                     const void* W_head, const void* b_head, void* probs,
                     int M, int K0, int H, int C, int rows, int waves,
#else
                     int M, int K0, int H, int rows, int waves, int start,
#endif
#if FWD_WIDE_DROP
                     const FwdChainDrop& D,
#endif
                     hipStream_t st) {
#if FWD_WIDE_HEAD
    if (M < 1 || M > INT32_MAX - 64 || (H != 128 && H != 512) || C < 1 ||
        C > 16 || nlayers < 1 || nlayers > SS_FWD_CHAIN_MAX || K0 < 8 ||
        K0 % 8 != 0)
        return false;
    if (!aligned16(x) || !aligned16(W_head) || !aligned16(b_head) ||
        !aligned16(probs))
        return false;
#else
    if (M < 1 || M > INT32_MAX - 64 || (H != 128 && H != 512) ||
        nlayers < 1 || nlayers > SS_FWD_CHAIN_MAX || K0 < 8 || K0 % 8 != 0 ||
        start < 0 || start > 2 || (start == 2 && K0 != H) || !aligned16(x))
        return false;
    const int tile0 = start == 2 || (start == 0 && K0 == H);
#endif
#if FWD_WIDE_DROP
    if (D.on == 0 || (D.on >> nlayers) != 0 ||
        (unsigned long)D.row_first +
                (unsigned long)(M - 1) * D.row_stride > UINT32_MAX)
        return false;
    for (int l = 0; l < nlayers; ++l)
        // p in (0, 1): a finite scale of at least 1, a threshold that keeps
        if (((D.on >> l) & 1u) &&
            !(D.scale[l] >= 1.f && D.scale[l] <= 3.4e38f && D.thr[l] > 0))
            return false;
#endif
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
        hipLaunchKernelGGL((FWD_WIDE_KERNEL<HH, R, NW>),
                           dim3(cdiv(M, R)), dim3(NW * 64), 0, st,
                           (const __bf16*)x, L, nlayers,
#if FWD_WIDE_DROP
                           D,
#endif
#if FWD_WIDE_HEAD
                           (const __bf16*)W_head, (const __bf16*)b_head,
                           (__bf16*)probs, M, K0, C);
#else
                           M, K0, tile0);
#endif
    };
    return H == 128 ? with_chain_wide_arm<128>(rows, waves, launch)
                    : with_chain_wide_arm<512>(rows, waves, launch);
}

}  // namespace
