// Training forward as ONE kernel (gfx950 / MI355X): the 256-wide ReLU
// layers under the classifier head and the head itself.
//
//   per ReLU layer l, bottom to top (out = 256):
//     h_l   = bf16(relu(h_{l-1} · W_l^T + b_l))              (stored)
//   probs   = softmax(bf16(h_top · W_head^T + b_head))       (stored)
//
// Replaces gemm_nt<bias, relu> → … → head_fwd_fused: the forward is
// row-local, so a block that owns R batch rows keeps its activation
// tile in LDS from layer to layer.  Every h_l is written once, because
// the backward needs it, and never read back.
//
// Bits: a layer is the v_mfma_f32_16x16x32_bf16 chain of gemm_nt_kernel
// — A = activation rows, B = W rows ([out][in], K contiguous), 32-wide
// K-steps in increasing order from a zero accumulator, K past in_dims
// as zeros in both operands — followed by that kernel's epilogue,
// v = acc + bias; v = v > 0 ? v : 0; f2bf(v).  The head is the MFMA
// chain and the register epilogue of head_fwd_fused_kernel (head_dev.h).
// Every output equals the unfused chain bit for bit.
//
// W (128 KB per 256-wide layer, L2-resident: every block reads all of
// it) goes L2 -> registers as the MFMA B operand, 16 B per lane and
// K-step.  The A operand is the tile in LDS.  Two texts of the K loops
// (AH): B one load group ahead as in bwd_chain_kernel (CHAIN_LAYER_MMA),
// or three K-steps ahead in a ring of named register sets
// (CHAIN_LAYER_MMA_AHEAD), which the eight-wave arms ship: in the first
// text the hand-over of the next group's registers makes every K-step
// wait for the loads it has just issued.
//
// The launch can also zero a buffer for its caller (the step's flat
// gradient buffer, in place of a memset launch): stores at kernel entry
// that nothing in the kernel waits for.
//
// Two arms for where the chain starts.  L1 = false: the input is a
// stored 256-wide activation and the kernel's first action is to load
// its tile into LDS.  L1 = true: the first layer has any in_dims % 8 ==
// 0 (784 at the flagship); its A operand x is streamed from memory in
// KC-wide chunks through a register-staged, double-buffered LDS stage,
// one barrier per chunk, columns past in_dims as zeros.
//
// Launch contract (the launcher returns false outside it): width 256,
// C <= 16, 1..8 layers, M >= 1 (rows past M are guarded), in_dims of the
// first layer 256 (L1 = false) or a multiple of 8 (L1 = true), every
// pointer 16-B aligned.

#include "chain_dev.h"
#include "launchers.h"

// The layers of one launch, bottom first.  Passed BY VALUE: nothing to
// upload, nothing to keep alive, and legal under graph capture.
struct FwdChainLayers {
    const void* w[SS_FWD_CHAIN_MAX];  // W [256][in]
    const void* b[SS_FWD_CHAIN_MAX];  // bias [256]
    void* h[SS_FWD_CHAIN_MAX];        // post-ReLU output [M][256]
};

// R rows per tile, NW waves per block (CHAIN_GEOMETRY).  Second launch
// bound = waves per SIMD that two blocks on a CU need.
// AH = the K loops keep their B fragments CHAIN_B_AHEAD steps ahead
// (CHAIN_LAYER_MMA_AHEAD and its first-layer counterpart below).
template <int R, int NW, bool L1, bool AH>
__global__ __launch_bounds__(NW * 64, NW / 2)
void fwd_chain_kernel(
    const __bf16* __restrict__ x,       // [M][K0]: input of layer 0
    const FwdChainLayers L, int nlayers,
    const __bf16* __restrict__ W_head,  // [C][256]
    const __bf16* __restrict__ b_head,  // [C]
    __bf16* __restrict__ probs,         // [M][C]
    int M, int K0, int C,
    unsigned* __restrict__ zero_ptr,    // zero_bytes of zeros go here,
    long zero_bytes) {                  // or 0 (a multiple of 4)
    CHAIN_GEOMETRY(R, NW);
    // first-layer stage: KC columns of x per chunk
    constexpr int KC = 128;
    constexpr int LDX = KC + 8;         // padded stage row (bf16)
    constexpr int XPR = KC / 8;         // 16-B pieces per stage row
    constexpr int XP = R * XPR / NT;    // stage pieces per thread
    static_assert(R * XPR % NT == 0 && XP >= 1, "stage piece mapping");
    static_assert(FM <= NW, "one head fragment per wave");

    __shared__ __attribute__((aligned(16))) ushort tile[R][LDT];
    __shared__ __attribute__((aligned(16)))
    ushort xs[L1 ? 2 : 1][L1 ? R : 1][LDX];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lrow = lane & 15;
    const int kch = lane >> 4;
    const int row0 = blockIdx.x * R;

    // ---- zeros for the caller (the step's gradient buffer): stores
    // nobody in this launch waits for or reads, 16 B each where the
    // base allows it, the rest 4 B each
    if (zero_bytes > 0) {
        const long nthr = (long)gridDim.x * NT;
        const long gtid = (long)blockIdx.x * NT + tid;
        const long n16 = ((unsigned long)zero_ptr & 15) ? 0 : zero_bytes / 16;
        for (long i = gtid; i < n16; i += nthr)
            ((uint4*)zero_ptr)[i] = make_uint4(0u, 0u, 0u, 0u);
        for (long i = n16 * 4 + gtid; i < zero_bytes / 4; i += nthr)
            zero_ptr[i] = 0u;
    }

    f32x4 acc[FM][FN];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
    };
    // acc -> tile through the gemm_nt_kernel epilogue (bias, ReLU, one
    // rounding), then the tile -> h_l as 16-B row-contiguous stores.
    // The caller has made sure that no wave still reads the tile.
    auto finish_layer = [&](int l, const float (&bv)[FN]) {
        CHAIN_ACC_TO_TILE(acc, tile, v += bv[j]; v = v > 0.f ? v : 0.f)
        __syncthreads();
        gbf16* const ho = (gbf16*)L.h[l];
        CHAIN_FOR_PIECES(i, r, col) {
            if (row0 + r < M)
                *(gbf16x8*)&ho[(long)(row0 + r) * H + col] =
                    *(const bf16x8*)&tile[r][col];
        }
    };
    auto load_bias = [&](int l, float (&bv)[FN]) {
        const gbf16* const bias = (const gbf16*)L.b[l];
#pragma unroll
        for (int j = 0; j < FN; ++j)
            bv[j] = bf2f((__bf16)bias[wave * WN + j * 16 + lrow]);
    };

    int l = 0;
    if constexpr (L1) {
        // ---- layer 0 from x: chunk c of x sits in xs[c & 1]; the loads
        // of chunk c+1 are issued ahead of chunk c's MFMAs and written
        // after them; the barrier that ends a chunk frees the buffer the
        // next chunk overwrites
        const gbf16* const w = (const gbf16*)L.w[0];
        float bv[FN];
        load_bias(0, bv);
        const int nsteps = cdiv(K0, 32);
        const int nchunks = cdiv(K0, KC);
        bf16x8 xr[XP];
        auto xload = [&](int c) {
#pragma unroll
            for (int p = 0; p < XP; ++p) {
                const int q = tid + p * NT;
                const int r = q / XPR, k = c * KC + (q % XPR) * 8;
                xr[p] = zero8();
                if (row0 + r < M && k < K0)
                    xr[p] = *(const bf16x8*)&x[(long)(row0 + r) * K0 + k];
            }
        };
        auto xwrite = [&](int buf) {
#pragma unroll
            for (int p = 0; p < XP; ++p) {
                const int q = tid + p * NT;
                *(bf16x8*)&xs[buf][q / XPR][(q % XPR) * 8] = xr[p];
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
        // the MFMAs of K-step kk of the chunk in xs[buf]
        auto mma_step = [&](const bf16x8(&bb)[FN], int buf, int kk) {
            bf16x8 a_frag[FM];
#pragma unroll
            for (int i = 0; i < FM; ++i)
                a_frag[i] = *(const bf16x8*)&xs[buf][i * 16 + lrow]
                                              [kk * 32 + kch * 8];
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_frag[i], bb[j], acc[i][j], 0, 0, 0);
        };
        if constexpr (AH) {
            // B ring as in CHAIN_LAYER_MMA_AHEAD: a chunk is as many
            // K-steps as the ring has sets, so step kk of every chunk
            // reads set kk and the chunk body needs no copies.  Entering
            // a chunk, sets 0 .. AHEAD-1 hold (or await) its first steps.
            //
            // The loads carry no guard, so that no branch splits the
            // ring: a piece past K0 is read from the row's last piece
            // instead (K0 >= 8) and never used as it is.  Chunks whose
            // 128 columns all lie below K0 use their sets as loaded; the
            // one chunk that may follow them zeroes the pieces past K0
            // as it uses them.
            constexpr int NB = CHAIN_B_AHEAD + 1;
            static_assert(KC / 32 == NB, "one chunk = one turn of the B ring");
            bf16x8 bq[NB][FN];
            auto load_b_any = [&](bf16x8(&bb)[FN], int s) {
                const int off = min(s * 32, K0 - 8 - kch * 8);
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    bb[j] = *(const gbf16x8*)(wp + (long)j * 16 * K0 + off);
            };
            const int nfull = K0 / KC;
            xload(0);
#pragma unroll
            for (int s = 0; s < CHAIN_B_AHEAD; ++s) load_b_any(bq[s], s);
            xwrite(0);
            zero_acc();
            __syncthreads();
            for (int c = 0; c < nfull; ++c) {
                if (c + 1 < nchunks) xload(c + 1);
#pragma unroll
                for (int kk = 0; kk < NB; ++kk) {
                    // fences: left alone, the scheduler sinks these
                    // loads to just above their first use
                    load_b_any(bq[(kk + CHAIN_B_AHEAD) % NB],
                               c * NB + kk + CHAIN_B_AHEAD);
                    __builtin_amdgcn_sched_barrier(0);
                    mma_step(bq[kk], c & 1, kk);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (c + 1 < nchunks) xwrite((c + 1) & 1);
                __syncthreads();
            }
            if (nfull < nchunks) {
                const int s0 = nfull * NB;
                load_b_any(bq[NB - 1], s0 + NB - 1);
#pragma unroll
                for (int kk = 0; kk < NB; ++kk) {
                    if (s0 + kk < nsteps) {
                        const bool in = (s0 + kk) * 32 + kch * 8 < K0;
                        bf16x8 bz[FN];
#pragma unroll
                        for (int j = 0; j < FN; ++j)
                            bz[j] = in ? bq[kk][j] : zero8();
                        mma_step(bz, nfull & 1, kk);
                    }
                }
                __syncthreads();
            }
        } else {
            bf16x8 b[FN], bn[FN];
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
                __syncthreads();
            }
        }
        finish_layer(0, bv);  // nothing has read the tile yet
        l = 1;
    } else {
        // ---- the input tile (rows past M as zeros: never stored)
        CHAIN_FOR_PIECES(i, r, col) {
            bf16x8 v = zero8();
            if (row0 + r < M) v = *(const bf16x8*)&x[(long)(row0 + r) * H + col];
            *(bf16x8*)&tile[r][col] = v;
        }
    }
    __syncthreads();

    // ---- the 256-wide layers: the tile holds h_{l-1}
    for (; l < nlayers; ++l) {
        const gbf16* const w = (const gbf16*)L.w[l];
        float bv[FN];
        load_bias(l, bv);
        zero_acc();
        if constexpr (AH) {
            CHAIN_LAYER_MMA_AHEAD(acc, tile, w)
        } else {
            CHAIN_LAYER_MMA(acc, tile, w)
        }
        __syncthreads();  // every wave has read the tile
        finish_layer(l, bv);
    }

    // ---- head: one 16-row fragment per wave, A = the tile (the barrier
    // inside finish_layer made it whole), B = W_head rows, rows >= C as
    // zeros; K in order, as head_fwd_fused_kernel
    if (wave < FM) {
        const bool cvalid = lrow < C;
        const __bf16* wp = W_head + (long)min(lrow, C - 1) * H + kch * 8;
        bf16x8 hb[NSTEP];
#pragma unroll
        for (int t = 0; t < NSTEP; ++t)
            hb[t] = *(const bf16x8*)(wp + t * 32);
        f32x4 hacc[1];
        hacc[0] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NSTEP; ++t) {
            const bf16x8 a =
                *(const bf16x8*)&tile[wave * 16 + lrow][t * 32 + kch * 8];
            const bf16x8 bfrag = cvalid ? hb[t] : zero8();
            hacc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag, hacc[0],
                                                              0, 0, 0);
        }
        const int row_base = row0 + wave * 16;
        HEAD_FWD_EPILOGUE(1, hacc, b_head, probs, cvalid, lrow, kch, row_base,
                          M, C)
    }
}

// rows / waves: 0 = the shipped choice; (32, 4), (32, 8), (64, 4) and
// (64, 8) are the measured arms (scripts/microbench_fwd_chain.py,
// docs/KERNELS.md).  The shipped choice is eight waves on 64 rows, and on
// 32 rows where 64-row tiles would cover at most half of the 256 CUs
// (M <= 8192: measured at M = 4096, the flagship under gpipe with four
// micro-batches, 0.2438 against 0.2523 ms per step; 64 rows win at
// M = 16384, 0.1308 against 0.1382), as gemm_nt_dispatch picks its
// 32-row tier.
// l1: 1 = the input is a stored 256-wide activation, 2 = the first
// layer streams its input (any K0 % 8 == 0), 0 = the shipped choice:
// 1 where K0 == 256, else 2 unless SS_FWD_CHAIN_L1=0 switches the
// streamed first layer off (the launch is then refused).
// kloop: 1 = B fragments one step ahead (CHAIN_LAYER_MMA), 2 = three
// steps ahead in named sets (CHAIN_LAYER_MMA_AHEAD; built for the
// eight-wave arms, refused with four waves), 0 = the shipped choice:
// 2 with eight waves, 1 with four.
// SS_FWD_CHAIN_ROWS / SS_FWD_CHAIN_WAVES / SS_FWD_CHAIN_L1 /
// SS_FWD_CHAIN_KLOOP (read once) override the shipped choice for tuning.
// zero_ptr / zero_bytes: see launchers.h; the launch is refused when
// they are not 4-B granular.
bool ss_fwd_chain(const void* x, const void* const* w, const void* const* b,
                  void* const* h, int nlayers, const void* W_head,
                  const void* b_head, void* probs, int M, int K0, int H, int C,
                  int rows, int waves, int l1, int kloop, void* zero_ptr,
                  long zero_bytes, hipStream_t st) {
    if (M < 1 || M > INT32_MAX - 64 || H != 256 || C < 1 || C > 16 ||
        nlayers < 1 || nlayers > SS_FWD_CHAIN_MAX || K0 < 8 || K0 % 8 != 0)
        return false;
    if (zero_bytes < 0 || zero_bytes % 4 != 0 ||
        (zero_bytes > 0 && (!zero_ptr || ((uintptr_t)zero_ptr & 3))))
        return false;
    if (!aligned16(x) || !aligned16(W_head) || !aligned16(b_head) ||
        !aligned16(probs))
        return false;
    FwdChainLayers L = {};
    for (int l = 0; l < nlayers; ++l) {
        if (!aligned16(w[l]) || !aligned16(b[l]) || !aligned16(h[l]))
            return false;
        L.w[l] = w[l];
        L.b[l] = b[l];
        L.h[l] = h[l];
    }
    static const int env_rows = env_int("SS_FWD_CHAIN_ROWS", 0);
    static const int env_waves = env_int("SS_FWD_CHAIN_WAVES", 0);
    static const int env_l1 = env_int("SS_FWD_CHAIN_L1", 1);
    if (!rows) rows = env_rows ? env_rows : (cdiv(M, 64) <= 128 ? 32 : 64);
    if (!waves) waves = env_waves ? env_waves : 8;
    if (!l1) {
        if (K0 != H && !env_l1) return false;
        l1 = K0 != H ? 2 : 1;
    }
    if (l1 != 1 && l1 != 2) return false;
    if (l1 == 1 && K0 != H) return false;
    static const int env_kloop = env_int("SS_FWD_CHAIN_KLOOP", 0);
    if (!kloop) kloop = env_kloop ? env_kloop : (waves == 8 ? 2 : 1);
    if (kloop != 1 && kloop != 2) return false;
    if (kloop == 2 && waves != 8) return false;
    return with_chain_arm(rows, waves, [&](auto r, auto nw) {
        constexpr int R = r.value, NW = nw.value;
        with_bools(
            [&](auto streamed, auto ahead) {
                // no four-wave instantiation of the ahead loops
                constexpr bool AH = ahead.value && NW == 8;
                hipLaunchKernelGGL(
                    (fwd_chain_kernel<R, NW, streamed.value, AH>),
                    dim3(cdiv(M, R)), dim3(NW * 64), 0, st, (const __bf16*)x,
                    L, nlayers, (const __bf16*)W_head, (const __bf16*)b_head,
                    (__bf16*)probs, M, K0, C, (unsigned*)zero_ptr,
                    zero_bytes);
            },
            l1 == 2, kloop == 2);
    });
}
