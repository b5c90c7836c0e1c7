// The text of the wide backward chain kernel and of its launch (see
// bwd_chain_wide.hip), compiled once per loss, each loss in a
// translation unit of its own (bwd_chain_wide.hip: cross-entropy;
// bwd_chain_wide_mse.hip: squared error), which defines BWD_WIDE_KERNEL
// (the kernel's name), BWD_WIDE_LAUNCHER (the name of the arm's host
// launcher) and BWD_WIDE_MSE (0 / 1).  With 1 the head step computes the
// softmax-MSE dz, whose row sum every lane of the wave takes part in
// (head_dev.h: head_mse_dz_elem); nothing else differs.
//
// BWD_WIDE_HEAD (optional, default 1) 0 is the stage arm
// (bwd_chain_wide_stage.hip), for a pipeline stage with no classifier
// head: the chain is entered from dout [M][H], the received gradient of
// the top layer's output, in memory.  No head step, so no W_head^T and no
// dz_head in LDS: a thread takes its pieces of dout and of the top layer's
// mask source into registers, masks them there and writes dz_0 once to the
// tile and once to memory.  From the first K loop on the text is the
// headed kernel's.
//
// SCALED: the layers ran inverted dropout, so a kept dz element is
// bf16(dh · dz_scale) with dz_scale = 1/keep, one value for the launch
// (the stashed post-dropout h already is the mask: h > 0 ⇔ z > 0 ∧ kept).
// That is relu_bwd_scaled_kernel's value: the tile's bf16 dh, ONE f32
// multiply, a second rounding.  The multiply has nothing to fuse with,
// and the including files are built without packed f32 arithmetic, so it
// stays one v_mul_f32 per element (bwd_chain_stage.hip's chain_unpaired
// note is about a file built WITH packed f32).  SA is that float: an
// EMPTY pack when not SCALED, so those instantiations keep their kernel
// arguments and code.

#include "chain_wide.h"

#ifndef BWD_WIDE_HEAD
#define BWD_WIDE_HEAD 1
#endif

namespace {

// The layers of one launch, top first.  Passed BY VALUE: nothing to
// upload, nothing to keep alive, and legal under graph capture.
struct BwdWideLayers {
    const void* h[SS_BWD_CHAIN_MAX];   // post-ReLU output, the mask source
    const void* wt[SS_BWD_CHAIN_MAX];  // W^T [H][H], or null: chain ends
    void* dz[SS_BWD_CHAIN_MAX];        // masked gradient out
};

template <int HH, int R, int NW, bool SCALED = false, class... SA>
__global__ __launch_bounds__(NW * 64)
void BWD_WIDE_KERNEL(
#if BWD_WIDE_HEAD
    const __bf16* __restrict__ probs,    // [M][C]
    const __bf16* __restrict__ target,   // [M][C]
    const __bf16* __restrict__ Wt_head,  // [H][C]
    __bf16* __restrict__ dz_head,        // [M][C]
#else
    const __bf16* __restrict__ dout,     // [M][H]: dh of the top layer
#endif
    const BwdWideLayers L, int nlayers,
    __bf16* __restrict__ dx,             // [M][H] or null
#if BWD_WIDE_HEAD
    int M, int C, float inv_gb, SA... dz_scale) {
#else
    int M, SA... dz_scale) {
#endif
    static_assert(sizeof...(SA) == SCALED, "one dz_scale when SCALED");
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
    constexpr int NSTEP = H / 32;     // K-steps of a layer
#if BWD_WIDE_HEAD
    constexpr int HC = H < 256 ? H : 256;  // W_head^T rows per staged chunk
#endif
    static_assert(WN % 16 == 0 && FN >= 1 && R % 16 == 0, "fragment split");
    static_assert(R * PPR % NT == 0 && NP >= 1, "piece mapping");
#if BWD_WIDE_HEAD
    static_assert(NT >= HC && H % HC == 0, "one thread per W_head^T row");
#endif
    static_assert(NSTEP > CHAIN_B_AHEAD, "K loop");
    // every built arm keeps B three K-steps ahead: accumulators + the ring
    // of four B sets + the A fragments + the mask source that is in
    // flight under the K loop leave some thirty registers for addresses
    static_assert(4 * FM * FN + 16 * FN + 4 * FM + 4 * NP + 30 <=
                      wide_reg_budget(NW),
                  "register budget of CHAIN_LAYER_MMA_AHEAD");

    __shared__ __attribute__((aligned(16))) ushort tile[R][LDT];
#if BWD_WIDE_HEAD
    __shared__ __attribute__((aligned(16))) ushort wts[HC][16];
    __shared__ __attribute__((aligned(16))) ushort dzs[R][16];
#endif

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lrow = lane & 15;
    const int kch = lane >> 4;
    const int row0 = blockIdx.x * R;

    // mask source of the next mask pass, issued a phase ahead (rows past
    // M as zeros: they mask to zero and are never stored)
    bf16x8 hm[NP];
    auto load_mask = [&](int l) {
        const gbf16* h = (const gbf16*)L.h[l];
        CHAIN_FOR_PIECES(i, r, col) {
            hm[i] = zero8();
            if (row0 + r < M)
                hm[i] = *(const gbf16x8*)&h[(long)(row0 + r) * H + col];
        }
    };
    load_mask(0);

#if BWD_WIDE_HEAD
    // ---- head: dz_head of the tile, stored and kept as the MFMA A
    // operand (class index = k slot, k >= C zero)
    for (int e = tid; e < R * 16; e += NT) {
        const int r = e >> 4, c = e & 15;
        ushort bits = 0;
#if BWD_WIDE_MSE
        // whole waves per trip: the row sum is a cross-lane step, so the
        // guard stands around the loads and the store only
        static_assert(R * 16 % NT == 0, "whole waves per trip");
        const bool live = c < C && row0 + r < M;
        const long gi = (long)(row0 + r) * C + c;
        __bf16 pb = (__bf16)0.f, tb = (__bf16)0.f;
        if (live) {
            pb = probs[gi];
            tb = target[gi];
        }
        const __bf16 o = head_mse_dz_elem(pb, tb, inv_gb);
        if (live) {
            dz_head[gi] = o;
            bits = bf_bits(o);
        }
#else
        if (c < C && row0 + r < M) {
            const long gi = (long)(row0 + r) * C + c;
            const __bf16 o = head_dz_elem(probs[gi], target[gi], inv_gb);
            dz_head[gi] = o;
            bits = bf_bits(o);
        }
#endif
        dzs[r][c] = bits;
    }
    // dh of the top layer, HC columns per staged chunk of W_head^T
    for (int k0 = 0; k0 < H; k0 += HC) {
        if (k0 > 0) __syncthreads();  // every wave has read the last chunk
        HEAD_STAGE_WT(HC, wts, Wt_head, k0, HC, C, tid)
        __syncthreads();  // first chunk: dzs as well
        for (int idx = wave; idx < FM * (HC / 16); idx += NW) {
            const int rg = idx % FM, ct = idx / FM;
            HEAD_DX_FRAG(acc, dzs, wts, rg, ct, lrow, kch);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                tile[rg * 16 + kch * 4 + r][k0 + ct * 16 + lrow] =
                    bf_bits(f2bf(acc[r]));
        }
    }
    __syncthreads();
#else
    // ---- entry: dz_0 from dout and h_0, both in registers (rows past M
    // as zeros, never stored).  One LDS write per piece, no LDS read, and
    // no barrier ahead of it: a thread touches only its own pieces.  The
    // rule and the scaled product are the mask pass's below.
    {
        gbf16* const dzo = (gbf16*)L.dz[0];
        bf16x8 dv[NP];
        CHAIN_FOR_PIECES(i, r, col) {
            dv[i] = zero8();
            if (row0 + r < M)
                dv[i] = *(const bf16x8*)&dout[(long)(row0 + r) * H + col];
        }
        CHAIN_FOR_PIECES(i, r, col) {
            bf16x8 v = dv[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (!(bf2f(hm[i][e]) > 0.f)) v[e] = (__bf16)0.f;
                else if constexpr (SCALED)
                    v[e] = f2bf(bf2f(v[e]) * (dz_scale + ...));
            }
            *(bf16x8*)&tile[r][col] = v;
            if (row0 + r < M)
                *(gbf16x8*)&dzo[(long)(row0 + r) * H + col] = v;
        }
    }
#endif

    // ---- the ReLU layers: the tile holds dh of layer l
    for (int l = 0; l < nlayers; ++l) {
        // mask pass: dz_l replaces dh in the tile and goes out as 16-B
        // row-contiguous stores (a thread touches only its own pieces,
        // so no barrier inside the pass)
        gbf16* const dzo = (gbf16*)L.dz[l];
#if !BWD_WIDE_HEAD
        if (l > 0)  // the tile already holds dz_0
#endif
        CHAIN_FOR_PIECES(i, r, col) {
            bf16x8 v = *(const bf16x8*)&tile[r][col];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (!(bf2f(hm[i][e]) > 0.f)) v[e] = (__bf16)0.f;
                else if constexpr (SCALED)
                    v[e] = f2bf(bf2f(v[e]) * (dz_scale + ...));
            }
            *(bf16x8*)&tile[r][col] = v;
            if (row0 + r < M)
                *(gbf16x8*)&dzo[(long)(row0 + r) * H + col] = v;
        }
        const gbf16* const wt = (const gbf16*)L.wt[l];
        if (wt == nullptr) break;  // block-uniform: the chain ends
        if (l + 1 < nlayers) load_mask(l + 1);
        __syncthreads();

        // dh_{l-1} = dz_l · W_l, W^T straight from L2
        f32x4 acc[FM][FN];
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
        CHAIN_LAYER_MMA_AHEAD(acc, tile, wt)
        __syncthreads();  // every wave has read the dz tile
        CHAIN_ACC_TO_TILE(acc, tile, )
        __syncthreads();
    }

    // every layer's dgrad was in the chain: the tile is dx
    if (dx != nullptr) {
        CHAIN_FOR_PIECES(i, r, col) {
            if (row0 + r < M)
                *(bf16x8*)&dx[(long)(row0 + r) * H + col] =
                    *(const bf16x8*)&tile[r][col];
        }
    }
}

}  // namespace

// This loss's arm of ss_bwd_chain_wide (launchers.h), which selects it.
// rows / waves: 0 = the shipped choice (docs/KERNELS.md, "Chain kernels,
// wide"); any other pair must be one of with_chain_wide_arm's.
// dz_scale: 1.f runs the unscaled instantiations; any other value the
// scaled ones, built for every arm.
#if BWD_WIDE_HEAD
bool BWD_WIDE_LAUNCHER(const void* probs, const void* target,
                       const void* Wt_head, void* dz_head,
                       const void* const* h, const void* const* wt,
                       void* const* dz, int nlayers, void* dx, int M, int H,
                       int C, float inv_gb, int rows, int waves,
                       float dz_scale, hipStream_t st) {
    if (M < 1 || M > INT32_MAX - 64 || (H != 128 && H != 512) || C < 1 ||
        C > 16 || nlayers < 1 || nlayers > SS_BWD_CHAIN_MAX)
        return false;
    if (!aligned16(probs) || !aligned16(target) || !aligned16(Wt_head) ||
        !aligned16(dz_head))
        return false;
#else
bool BWD_WIDE_LAUNCHER(const void* dout, const void* const* h,
                       const void* const* wt, void* const* dz, int nlayers,
                       void* dx, int M, int H, int rows, int waves,
                       float dz_scale, hipStream_t st) {
    if (M < 1 || M > INT32_MAX - 64 || (H != 128 && H != 512) ||
        nlayers < 1 || nlayers > SS_BWD_CHAIN_MAX || !aligned16(dout))
        return false;
#endif
    BwdWideLayers L = {};
    for (int l = 0; l < nlayers; ++l) {
        const bool last = l + 1 == nlayers;
        if (!aligned16(h[l]) || !aligned16(dz[l])) return false;
        if (!last && !aligned16(wt[l])) return false;
        if (last && (wt[l] != nullptr) != (dx != nullptr)) return false;
        if (last && dx && !(aligned16(wt[l]) && aligned16(dx))) return false;
        L.h[l] = h[l];
        L.wt[l] = wt[l];
        L.dz[l] = dz[l];
    }
    chain_wide_shipped(H, M, rows, waves);
    auto launch = [&](auto hh, auto r, auto nw) {
        constexpr int HH = hh.value, R = r.value, NW = nw.value;
#if BWD_WIDE_HEAD
        if (dz_scale != 1.f)
            hipLaunchKernelGGL((BWD_WIDE_KERNEL<HH, R, NW, true, float>),
                               dim3(cdiv(M, R)), dim3(NW * 64), 0, st,
                               (const __bf16*)probs, (const __bf16*)target,
                               (const __bf16*)Wt_head, (__bf16*)dz_head, L,
                               nlayers, (__bf16*)dx, M, C, inv_gb, dz_scale);
        else
            hipLaunchKernelGGL((BWD_WIDE_KERNEL<HH, R, NW>),
                               dim3(cdiv(M, R)), dim3(NW * 64), 0, st,
                               (const __bf16*)probs, (const __bf16*)target,
                               (const __bf16*)Wt_head, (__bf16*)dz_head, L,
                               nlayers, (__bf16*)dx, M, C, inv_gb);
#else
        if (dz_scale != 1.f)
            hipLaunchKernelGGL((BWD_WIDE_KERNEL<HH, R, NW, true, float>),
                               dim3(cdiv(M, R)), dim3(NW * 64), 0, st,
                               (const __bf16*)dout, L, nlayers, (__bf16*)dx,
                               M, dz_scale);
        else
            hipLaunchKernelGGL((BWD_WIDE_KERNEL<HH, R, NW>),
                               dim3(cdiv(M, R)), dim3(NW * 64), 0, st,
                               (const __bf16*)dout, L, nlayers, (__bf16*)dx,
                               M);
#endif
    };
    return H == 128 ? with_chain_wide_arm<128>(rows, waves, launch)
                    : with_chain_wide_arm<512>(rows, waves, launch);
}
