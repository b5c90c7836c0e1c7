// Backward data path of the training step as ONE kernel (gfx950 /
// MI355X): the head backward and the ReLU-layer data gradients below it.
//
//   dz_head = bf16((probs − target)/GB)                      (stored)
//   dh      = bf16(dz_head · W_head)
//   per ReLU layer l, top to bottom (all 256 wide):
//     dz_l  = !(h_l > 0) ? +0 : dh                           (stored)
//     dh    = bf16(dz_l · W_l)          while the layer's dgrad is in
//                                       the chain; else the chain ends
//   dx      = dh of the last layer      (stored, when that dgrad is in)
//
// Replaces head_bwd_fused → gemm_nt<mask> → gemm_nt<mask> …: the chain
// is row-local, so a block that owns R batch rows keeps the dh tile in
// LDS from layer to layer instead of writing it to memory for the next
// launch to read back.  What goes to memory is dz_l, the MASKED
// gradient, in place of dh_l: the same bytes, and every weight-gradient
// kernel downstream then runs without a mask.
//
// Bits: dz_head and the head's dh come from the device code that
// head_bwd_fused_kernel runs (head_dev.h).  A layer's dh is the
// v_mfma_f32_16x16x32_bf16 chain of gemm_nt_kernel — A = dz rows, B =
// W^T rows ([in][out], K = out contiguous), 32-wide K-steps in
// increasing order from a zero accumulator, rounded once by f2bf — and
// the mask is StageReg's rule (a NaN or −0.0 in h masks to +0).  Every
// output equals the unfused chain bit for bit.
//
// W^T (128 KB per layer, L2-resident: every block reads all of it) goes
// L2 -> registers as the MFMA B operand, 16 B per lane and K-step, the
// next load group in flight under the current group's MFMAs, as in
// head_fwd_fused_kernel.  The A operand is the dz tile in LDS.
//
// Launch contract (the launcher returns false outside it): width 256,
// C <= 16, 1..8 layers, M >= 1 (rows past M are guarded), every layer
// but the last has its W^T, the last has it exactly when dx is wanted.

#include "chain_dev.h"
#include "launchers.h"

// The layers of one launch, top first.  Passed BY VALUE (24 pointers of
// kernel arguments): nothing to upload, nothing to keep alive, and
// legal under graph capture as it stands.
struct BwdChainLayers {
    const void* h[SS_BWD_CHAIN_MAX];   // post-ReLU output, the mask source
    const void* wt[SS_BWD_CHAIN_MAX];  // W^T [256][256], or null: chain ends
    void* dz[SS_BWD_CHAIN_MAX];        // masked gradient out
};

// R rows per tile, NW waves per block (CHAIN_GEOMETRY).  Second launch
// bound = waves per SIMD that two blocks on a CU need.  WLDS: W^T goes
// through LDS in 32-wide K-chunks (register-staged, double-buffered, one
// barrier per K-step, as gemm_nt_kernel stages B) instead of L2 ->
// registers; the measured alternative (85 KB of LDS: one block per CU).
// SCALED: the layers ran inverted dropout, so a kept dz element is
// bf16(dh · dz_scale) with dz_scale = 1/keep, one value for the launch
// (the stashed h already is the mask: h > 0 ⇔ z > 0 ∧ kept).  SA is that
// float: an EMPTY pack when not SCALED, so those instantiations keep
// their kernel arguments and code.
template <int R, int NW, bool WLDS, bool SCALED = false, class... SA>
__global__ __launch_bounds__(NW * 64, WLDS ? NW / 4 : NW / 2)
void bwd_chain_kernel(
    const __bf16* __restrict__ probs,    // [M][C]
    const __bf16* __restrict__ target,   // [M][C]
    const __bf16* __restrict__ Wt_head,  // [256][C]
    __bf16* __restrict__ dz_head,        // [M][C]
    const BwdChainLayers L, int nlayers,
    __bf16* __restrict__ dx,             // [M][256] or null
    int M, int C, float inv_gb, int ntiles, SA... dz_scale) {
    static_assert(sizeof...(SA) == SCALED, "one dz_scale when SCALED");
    CHAIN_GEOMETRY(R, NW);
    static_assert(NT >= H, "one thread per W_head^T row");

    __shared__ __attribute__((aligned(16))) ushort tile[R][LDT];
    __shared__ __attribute__((aligned(16))) ushort wts[H][16];
    __shared__ __attribute__((aligned(16))) ushort dzs[R][16];
    constexpr int LDW = 32 + 8;         // padded W^T chunk row (bf16)
    __shared__ __attribute__((aligned(16)))
    ushort ws[WLDS ? 2 : 1][WLDS ? H : 1][LDW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lrow = lane & 15;
    const int kch = lane >> 4;

    HEAD_STAGE_WT(H, wts, Wt_head, 0, H, C, tid)

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int row0 = t * R;

        // mask source of the next mask pass, issued a phase ahead (rows
        // past M as zeros: they mask to zero and are never stored)
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

        // ---- head: dz_head of the tile, stored and kept as the MFMA A
        // operand (class index = k slot, k >= C zero)
        for (int e = tid; e < R * 16; e += NT) {
            const int r = e >> 4, c = e & 15;
            ushort bits = 0;
            if (c < C && row0 + r < M) {
                const long gi = (long)(row0 + r) * C + c;
                const __bf16 o = head_dz_elem(probs[gi], target[gi], inv_gb);
                dz_head[gi] = o;
                bits = bf_bits(o);
            }
            dzs[r][c] = bits;
        }
        __syncthreads();
        for (int idx = wave; idx < FM * (H / 16); idx += NW) {
            const int rg = idx % FM, ct = idx / FM;
            HEAD_DX_FRAG(acc, dzs, wts, rg, ct, lrow, kch);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                tile[rg * 16 + kch * 4 + r][ct * 16 + lrow] =
                    bf_bits(f2bf(acc[r]));
        }
        __syncthreads();

        // ---- the ReLU layers: the tile holds dh of layer l
        for (int l = 0; l < nlayers; ++l) {
            // mask pass: dz_l replaces dh in the tile and goes out as
            // 16-B row-contiguous stores (a thread touches only its own
            // pieces, so no barrier inside the pass)
            gbf16* const dzo = (gbf16*)L.dz[l];
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

            f32x4 acc[FM][FN];
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (WLDS) {
                // dh_{l-1} = dz_l · W_l with W^T chunk t in ws[t & 1]:
                // the loads of chunk t+1 are issued ahead of chunk t's
                // MFMAs and written after them; the barrier that ends a
                // step frees the buffer the next step overwrites
                constexpr int WP = H * 4 / NT;  // 16-B pieces per thread
                bf16x8 wr[WP];
                auto wload = [&](int t) {
#pragma unroll
                    for (int p = 0; p < WP; ++p) {
                        const int q = tid + p * NT;
                        wr[p] = *(const gbf16x8*)&wt[(long)(q >> 2) * H +
                                                     t * 32 + (q & 3) * 8];
                    }
                };
                auto wwrite = [&](int buf) {
#pragma unroll
                    for (int p = 0; p < WP; ++p) {
                        const int q = tid + p * NT;
                        *(bf16x8*)&ws[buf][q >> 2][(q & 3) * 8] = wr[p];
                    }
                };
                wload(0);
                wwrite(0);
                __syncthreads();
                for (int t = 0; t < NSTEP; ++t) {
                    if (t + 1 < NSTEP) wload(t + 1);
                    bf16x8 a_frag[FM], b_frag[FN];
#pragma unroll
                    for (int i = 0; i < FM; ++i)
                        a_frag[i] = *(const bf16x8*)&tile[i * 16 + lrow]
                                                        [t * 32 + kch * 8];
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        b_frag[j] = *(const bf16x8*)&ws[t & 1]
                                                      [wave * WN + j * 16 +
                                                       lrow][kch * 8];
#pragma unroll
                    for (int i = 0; i < FM; ++i)
#pragma unroll
                        for (int j = 0; j < FN; ++j)
                            acc[i][j] =
                                __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                    a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
                    if (t + 1 < NSTEP) wwrite((t + 1) & 1);
                    __syncthreads();
                }
            } else {
                // dh_{l-1} = dz_l · W_l, W^T straight from L2
                CHAIN_LAYER_MMA(acc, tile, wt)
            }
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
        __syncthreads();  // LDS is rewritten by the next tile
    }
}

namespace {

// dz_scale: none, or the one float of the SCALED instantiation
template <int R, int NW, bool WLDS = false, class... SA>
void bwd_chain_launch(const void* probs, const void* target,
                      const void* Wt_head, void* dz_head,
                      const BwdChainLayers& L, int nlayers, void* dx, int M,
                      int C, float inv_gb, hipStream_t st, SA... dz_scale) {
    const int ntiles = cdiv(M, R);
    hipLaunchKernelGGL(
        (bwd_chain_kernel<R, NW, WLDS, sizeof...(SA) == 1, SA...>),
        dim3(ntiles), dim3(NW * 64), 0, st, (const __bf16*)probs,
        (const __bf16*)target, (const __bf16*)Wt_head, (__bf16*)dz_head, L,
        nlayers, (__bf16*)dx, M, C, inv_gb, ntiles, dz_scale...);
}

}  // namespace

// rows / waves: 0 = the shipped choice (64, 8); (32, 4), (32, 8),
// (64, 4) and (64, 8) are the measured arms (scripts/microbench_bwd_chain.py,
// docs/KERNELS.md).  w_lds: 0 = the shipped choice (W^T from L2 into
// registers), 1 = W^T through LDS, built for (64, 8) only.
// SS_BWD_CHAIN_ROWS / SS_BWD_CHAIN_WAVES / SS_BWD_CHAIN_WLDS (read once)
// override the shipped choice for tuning.
// dz_scale: 1.f runs the unscaled instantiations; any other value the
// scaled one, which only the shipped arm is built with.
bool ss_bwd_chain(const void* probs, const void* target, const void* Wt_head,
                  void* dz_head, const void* const* h, const void* const* wt,
                  void* const* dz, int nlayers, void* dx, int M, int H, int C,
                  float inv_gb, int rows, int waves, int w_lds,
                  float dz_scale, hipStream_t st) {
    if (M < 1 || H != 256 || C < 1 || C > 16 || nlayers < 1 ||
        nlayers > SS_BWD_CHAIN_MAX)
        return false;
    BwdChainLayers L = {};
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
    static const int env_rows = env_int("SS_BWD_CHAIN_ROWS", 0);
    static const int env_waves = env_int("SS_BWD_CHAIN_WAVES", 0);
    if (!rows) rows = env_rows ? env_rows : 64;
    if (!waves) waves = env_waves ? env_waves : 8;
    static const int env_wlds = env_int("SS_BWD_CHAIN_WLDS", 0);
    if (!w_lds) w_lds = env_wlds;
    if (dz_scale != 1.f) {
        if (rows != 64 || waves != 8 || w_lds != 0) return false;
        bwd_chain_launch<64, 8, false>(probs, target, Wt_head, dz_head, L,
                                       nlayers, dx, M, C, inv_gb, st,
                                       dz_scale);
        return true;
    }
    if (w_lds == 1) {
        if (rows != 64 || waves != 8) return false;
        bwd_chain_launch<64, 8, true>(probs, target, Wt_head, dz_head, L,
                                      nlayers, dx, M, C, inv_gb, st);
        return true;
    }
    return with_chain_arm(rows, waves, [&](auto r, auto nw) {
        bwd_chain_launch<r.value, nw.value>(probs, target, Wt_head, dz_head,
                                            L, nlayers, dx, M, C, inv_gb, st);
    });
}
