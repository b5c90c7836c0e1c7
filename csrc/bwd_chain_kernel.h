// The text of the backward chain kernel and of its launch (see
// bwd_chain.hip), compiled once per entry arm, each arm in a translation
// unit of its own (bwd_chain.hip, bwd_chain_stage.hip), which defines
// BWD_CHAIN_KERNEL (the kernel's name), BWD_CHAIN_HEAD (1: the chain
// starts at the classifier head, 0: the stage arm, from a stored dout)
// and BWD_CHAIN_SCALE(f) (the arm's text of f · dz_scale), for the
// reasons given in fwd_chain_kernel.h.  A headed arm also defines
// BWD_CHAIN_LAUNCHER (the name of its host launcher) and may define
// BWD_CHAIN_MSE 1 (bwd_chain_mse.hip): the head step then computes the
// softmax-MSE dz, whose row sum every lane of the wave takes part in
// (head_dev.h: head_mse_dz_elem); nothing else differs.

#ifndef BWD_CHAIN_MSE
#define BWD_CHAIN_MSE 0
#endif

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

// Mask pass of layer l: dz_l, made from this thread's dh pieces DH (a
// bf16x8 expression in i, r, col), replaces dh in the tile and goes out
// as 16-B row-contiguous stores (a thread touches only its own pieces,
// so no barrier inside the pass).  BWD_CHAIN_SCALE(f) is the arm's text
// of f · dz_scale.
#define BWD_CHAIN_MASK_PASS(l, DH)                                           \
    {                                                                        \
        gbf16* const dzo = (gbf16*)L.dz[l];                                  \
        CHAIN_FOR_PIECES(i, r, col) {                                        \
            bf16x8 v = DH;                                                   \
            _Pragma("unroll") for (int e = 0; e < 8; ++e) {                  \
                if (!(bf2f(hm[i][e]) > 0.f)) v[e] = (__bf16)0.f;             \
                else if constexpr (SCALED)                                   \
                    v[e] = f2bf(BWD_CHAIN_SCALE(bf2f(v[e])));                \
            }                                                                \
            *(bf16x8*)&tile[r][col] = v;                                     \
            if (row0 + r < M)                                                \
                *(gbf16x8*)&dzo[(long)(row0 + r) * H + col] = v;             \
        }                                                                    \
    }

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
//
// BWD_CHAIN_HEAD 0 is the stage arm: a pipeline stage with no classifier
// receives dh of its top layer as `dout` [M][256] in memory.  The arm has
// no W_head^T and no dz_head in LDS (10 KB less at R = 64) and no head
// section: the first mask pass takes its dh pieces from memory into
// registers, issued together with the mask source, masks them there and
// writes dz_0 once to the tile and once to memory — no LDS read and no
// barrier ahead of that pass.  From there on it is the same loop.

template <int R, int NW, bool WLDS, bool SCALED = false, class... SA>
__global__ __launch_bounds__(NW * 64, WLDS ? NW / 4 : NW / 2)
void BWD_CHAIN_KERNEL(
#if BWD_CHAIN_HEAD
    const __bf16* __restrict__ probs,    // [M][C]
    const __bf16* __restrict__ target,   // [M][C]
    const __bf16* __restrict__ Wt_head,  // [256][C]
    __bf16* __restrict__ dz_head,        // [M][C]
#else
    const __bf16* __restrict__ dout,     // [M][256]: dh of layer 0
#endif
    const BwdChainLayers L, int nlayers,
    __bf16* __restrict__ dx,             // [M][256] or null
#if BWD_CHAIN_HEAD
    int M, int C, float inv_gb, int ntiles, SA... dz_scale) {
#else
    int M, int ntiles, SA... dz_scale) {
#endif
    static_assert(sizeof...(SA) == SCALED, "one dz_scale when SCALED");
    CHAIN_GEOMETRY(R, NW);
#if BWD_CHAIN_HEAD
    static_assert(NT >= H, "one thread per W_head^T row");
#endif

    __shared__ __attribute__((aligned(16))) ushort tile[R][LDT];
#if BWD_CHAIN_HEAD
    __shared__ __attribute__((aligned(16))) ushort wts[H][16];
    __shared__ __attribute__((aligned(16))) ushort dzs[R][16];
#endif
    constexpr int LDW = 32 + 8;         // padded W^T chunk row (bf16)
    __shared__ __attribute__((aligned(16)))
    ushort ws[WLDS ? 2 : 1][WLDS ? H : 1][LDW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lrow = lane & 15;
    const int kch = lane >> 4;

#if BWD_CHAIN_HEAD
    HEAD_STAGE_WT(H, wts, Wt_head, 0, H, C, tid)
#endif

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

#if BWD_CHAIN_HEAD
        // ---- head: dz_head of the tile, stored and kept as the MFMA
        // A operand (class index = k slot, k >= C zero)
        for (int e = tid; e < R * 16; e += NT) {
            const int r = e >> 4, c = e & 15;
            ushort bits = 0;
#if BWD_CHAIN_MSE
            // whole waves per trip: the row sum is a cross-lane step, so
            // the guard stands around the loads and the store only
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
                const __bf16 o =
                    head_dz_elem(probs[gi], target[gi], inv_gb);
                dz_head[gi] = o;
                bits = bf_bits(o);
            }
#endif
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
#else
        // ---- entry from memory: the tile's dh pieces into registers,
        // in flight with the mask source, then the first mask pass
        bf16x8 dh0[NP];
        CHAIN_FOR_PIECES(i, r, col) {
            dh0[i] = zero8();
            if (row0 + r < M)
                dh0[i] = *(const bf16x8*)&dout[(long)(row0 + r) * H + col];
        }
        BWD_CHAIN_MASK_PASS(0, dh0[i])
#endif

        // ---- the ReLU layers: the tile holds dh of layer l (the stage
        // arm enters with dz_0 already made)
        for (int l = 0; l < nlayers; ++l) {
#if !BWD_CHAIN_HEAD
            if (l > 0)
#endif
                BWD_CHAIN_MASK_PASS(l, *(const bf16x8*)&tile[r][col])
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

// This arm's launch.  dz_scale: none, or the one float of the SCALED
// instantiation.
template <int R, int NW, bool WLDS = false, class... SA>
void bwd_chain_launch(
#if BWD_CHAIN_HEAD
    const void* probs, const void* target, const void* Wt_head,
    void* dz_head,
#else
    const void* dout,
#endif
    const BwdChainLayers& L, int nlayers, void* dx, int M,
#if BWD_CHAIN_HEAD
    int C, float inv_gb,
#endif
    hipStream_t st, SA... dz_scale) {
    const int ntiles = cdiv(M, R);
    hipLaunchKernelGGL(
        (BWD_CHAIN_KERNEL<R, NW, WLDS, sizeof...(SA) == 1, SA...>),
        dim3(ntiles), dim3(NW * 64), 0, st,
#if BWD_CHAIN_HEAD
        (const __bf16*)probs, (const __bf16*)target, (const __bf16*)Wt_head,
        (__bf16*)dz_head, L, nlayers, (__bf16*)dx, M, C, inv_gb, ntiles,
#else
        (const __bf16*)dout, L, nlayers, (__bf16*)dx, M, ntiles,
#endif
        dz_scale...);
}

// The layer table of a launch from the caller's arrays; false where a
// pointer is missing or misaligned, or the last W^T and dx disagree.
bool bwd_chain_layers(BwdChainLayers& L, const void* const* h,
                      const void* const* wt, void* const* dz, int nlayers,
                      void* dx) {
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
    return true;
}

// SS_BWD_CHAIN_ROWS / SS_BWD_CHAIN_WAVES / SS_BWD_CHAIN_WLDS (read once)
// in place of the arguments that ask for the shipped choice
void bwd_chain_env(int& rows, int& waves, int& w_lds) {
    static const int env_rows = env_int("SS_BWD_CHAIN_ROWS", 0);
    static const int env_waves = env_int("SS_BWD_CHAIN_WAVES", 0);
    static const int env_wlds = env_int("SS_BWD_CHAIN_WLDS", 0);
    if (!rows) rows = env_rows;
    if (!waves) waves = env_waves;
    if (!w_lds) w_lds = env_wlds;
}

}  // namespace

#if BWD_CHAIN_HEAD
// This loss's arm of ss_bwd_chain (launchers.h), which selects it.
// rows / waves: 0 = the shipped choice (64, 8); (32, 4), (32, 8),
// (64, 4) and (64, 8) are the measured arms (scripts/microbench_bwd_chain.py,
// docs/KERNELS.md).  w_lds: 0 = the shipped choice (W^T from L2 into
// registers), 1 = W^T through LDS, built for (64, 8) and cross-entropy
// only.
// SS_BWD_CHAIN_ROWS / SS_BWD_CHAIN_WAVES / SS_BWD_CHAIN_WLDS (read once)
// override the shipped choice for tuning.
// dz_scale: 1.f runs the unscaled instantiations; any other value the
// scaled one, which only the shipped arm is built with.
bool BWD_CHAIN_LAUNCHER(const void* probs, const void* target,
                        const void* Wt_head, void* dz_head,
                        const void* const* h, const void* const* wt,
                        void* const* dz, int nlayers, void* dx, int M, int H,
                        int C, float inv_gb, int rows, int waves, int w_lds,
                        float dz_scale, hipStream_t st) {
    if (M < 1 || H != 256 || C < 1 || C > 16 || nlayers < 1 ||
        nlayers > SS_BWD_CHAIN_MAX)
        return false;
    BwdChainLayers L = {};
    if (!bwd_chain_layers(L, h, wt, dz, nlayers, dx)) return false;
    bwd_chain_env(rows, waves, w_lds);
    if (!rows) rows = 64;
    if (!waves) waves = 8;
    if (dz_scale != 1.f) {
        if (rows != 64 || waves != 8 || w_lds != 0) return false;
        bwd_chain_launch<64, 8, false>(probs, target, Wt_head, dz_head, L,
                                       nlayers, dx, M, C, inv_gb, st,
                                       dz_scale);
        return true;
    }
    if (w_lds == 1) {
#if BWD_CHAIN_MSE
        return false;
#else
        if (rows != 64 || waves != 8) return false;
        bwd_chain_launch<64, 8, true>(probs, target, Wt_head, dz_head, L,
                                      nlayers, dx, M, C, inv_gb, st);
        return true;
#endif
    }
    return with_chain_arm(rows, waves, [&](auto r, auto nw) {
        bwd_chain_launch<r.value, nw.value>(probs, target, Wt_head, dz_head,
                                            L, nlayers, dx, M, C, inv_gb, st);
    });
}
#endif
