// MFMA bf16 GEMM kernels for the MLP hot path (gfx950 / MI355X).
//
// Replaces the reference's NumPy BLAS calls (functional.py:13-21):
//   * gemm_nt:  C[M,N] = A[M,K] · B[N,K]^T (+bias) (+ReLU epilogue)
//               — forward (A=x, B=W) AND dgrad (A=dy, B=W^T copy),
//               with an optional fused ReLU-backward mask applied to A
//               while staging (mask = stashed post-ReLU output, same
//               shape as A).
//   * colsum:   gb[N] += Σ_rows (dY ⊙ mask) — bias grad.
// (wgrad_tn, the weight-gradient TN GEMM, lives in wgrad.hip.)
//
// Design notes (cdna_hip_programming.md):
//   * mfma_f32_16x16x32_bf16: per-wave 16×16 tile, K=32 per issue;
//     lane l holds A[l&15][(l>>4)*8 + j] / B-col[l&15], C row
//     (l>>4)*4+reg, col l&15 (verified on hardware by
//     tests/test_gpu_numerics.py::test_mfma_layout).
//   * LDS tiles padded +8 bf16 per row (16 B) → conflict-free
//     ds_read_b128 fragment reads (Guideline 4).
//   * These MLP shapes are small/memory-bound; the simple one-buffer
//     two-barrier structure is chosen for robustness at arbitrary
//     M/N/K (full bounds handling) — launch count, not MFMA peak, is
//     the budget here.

#include "dropout_dev.h"
#include "launchers.h"
#include "stage_reg.h"

// ---------------------------------------------------------------- gemm_nt

__device__ __forceinline__ const DropoutArgs& drop_args(const DropoutArgs& d) {
    return d;
}

// DROPOUT (valid only with HAS_BIAS && RELU && !HAS_MASK): the
// inverted-dropout mask of dropout_dev.h applied to the f32 value before
// its one rounding to bf16, v = keep ? relu(acc + b) * scale : +0.
// One Philox call per 16x16 fragment and lane: a call yields four
// consecutive columns of one sample; in the MFMA C layout those are the
// four lanes of a quad (lane & ~3 .. +3), each holding rows r = 0..3 of
// its column.  Lane q of the quad runs the call of row q, and the quad
// exchanges the four keep bits with DPP quad_perm broadcasts.  (A call
// per element, four per fragment and lane, measured 17.2 against 10.6 µs
// at the flagship hidden forward: profiles/r08_dropout.md.)
// DA is the DropoutArgs block: an EMPTY pack with DROPOUT off, so those
// instantiations keep their kernel arguments and code.
template <int BM, int BN, int KSTEP, int WAVES_M, int WAVES_N,
          bool HAS_BIAS, bool RELU, bool HAS_MASK, bool DROPOUT = false,
          class... DA>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64) void gemm_nt_kernel(
    const __bf16* __restrict__ A,     // [M][K]
    const __bf16* __restrict__ B,     // [N][K]
    const __bf16* __restrict__ bias,  // [N]
    const __bf16* __restrict__ mask,  // [M][K] (A-mask source, >0 keeps)
    __bf16* __restrict__ C,           // [M][N]
    int M, int N, int K, DA... da) {
    static_assert(sizeof...(DA) == DROPOUT, "one DropoutArgs block");
    static_assert(!DROPOUT || (HAS_BIAS && RELU && !HAS_MASK),
                  "dropout is an epilogue of the bias+ReLU forward");
    constexpr int WM = BM / WAVES_M;        // wave tile rows
    constexpr int WN = BN / WAVES_N;        // wave tile cols
    constexpr int FM = WM / 16;             // 16x16 frags per wave (M)
    constexpr int FN = WN / 16;
    constexpr int LDA = KSTEP + LDS_PAD;

    __shared__ ushort As[2][BM][LDA];
    __shared__ ushort Bs[2][BN][LDA];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WAVES_N;
    const int wn = wave % WAVES_N;
    // XCD-aware bijective remap (T1): decode the work id n-tile-fastest
    // so the blocks sharing an A (activation) m-slice run on ONE XCD
    // and hit its L2 instead of filling all eight.
    const int gx = gridDim.x, gy = gridDim.y;
    const int nwg = gx * gy;
    const int hw = blockIdx.x + gx * blockIdx.y;
    const int wid = xcd_remap(hw, nwg);
    const int m0 = ((wid / gy) % gx) * BM;
    const int n0 = (wid % gy) * BN;

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    const int lrow = lane & 15;
    const int kch = lane >> 4;  // 0..3 -> k offset kch*8

    StageReg<BM, KSTEP, WAVES_M * WAVES_N * 64, HAS_MASK> ra;
    StageReg<BN, KSTEP, WAVES_M * WAVES_N * 64, false> rb;
    ra.load(A, mask, M, K, m0, 0, tid);
    rb.load(B, nullptr, N, K, n0, 0, tid);
    ra.write(As[0], tid);
    rb.write(Bs[0], tid);
    __syncthreads();

    const int nsteps = (K + KSTEP - 1) / KSTEP;
    int cur = 0;
    for (int t = 0; t < nsteps; ++t) {
        // issue next tile's global loads early (latency hides under
        // this tile's MFMA)
        if (t + 1 < nsteps) {
            ra.load(A, mask, M, K, m0, (t + 1) * KSTEP, tid);
            rb.load(B, nullptr, N, K, n0, (t + 1) * KSTEP, tid);
        }

        // ---- MFMA on the current tile ----
#pragma unroll
        for (int kk = 0; kk < KSTEP / 32; ++kk) {
            bf16x8 a_frag[FM], b_frag[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i)
                a_frag[i] = *(const bf16x8*)&As[cur][wm * WM + i * 16 + lrow]
                                                   [kk * 32 + kch * 8];
#pragma unroll
            for (int j = 0; j < FN; ++j)
                b_frag[j] = *(const bf16x8*)&Bs[cur][wn * WN + j * 16 + lrow]
                                                   [kk * 32 + kch * 8];
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
        }

        if (t + 1 < nsteps) {
            ra.write(As[cur ^ 1], tid);
            rb.write(Bs[cur ^ 1], tid);
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: bias, ReLU, bf16 store ----
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int gcol = n0 + wn * WN + j * 16 + lrow;
            unsigned keep4 = 0;  // bit r: row r of this lane's column kept
            if constexpr (DROPOUT) {
                // before any lane leaves: the exchange needs the whole
                // quad.  The tile origins are multiples of 16, so the
                // quad shares gcol >> 2 and lane & 3 == gcol & 3.
                const DropoutArgs& d = drop_args(da...);
                const int q = lane & 3;
                const unsigned mine = dropout_keep4(
                    d, dropout_sample(d, m0 + wm * WM + i * 16 + kch * 4 + q),
                    (unsigned)gcol >> 2);
                const unsigned b0 = __builtin_amdgcn_update_dpp(
                    0, (int)mine, 0x00, 0xf, 0xf, true);
                const unsigned b1 = __builtin_amdgcn_update_dpp(
                    0, (int)mine, 0x55, 0xf, 0xf, true);
                const unsigned b2 = __builtin_amdgcn_update_dpp(
                    0, (int)mine, 0xaa, 0xf, 0xf, true);
                const unsigned b3 = __builtin_amdgcn_update_dpp(
                    0, (int)mine, 0xff, 0xf, 0xf, true);
                keep4 = ((b0 >> q) & 1) | (((b1 >> q) & 1) << 1) |
                        (((b2 >> q) & 1) << 2) | (((b3 >> q) & 1) << 3);
            }
            if (gcol >= N) continue;
            float bv = 0.f;
            if constexpr (HAS_BIAS) bv = bf2f(bias[gcol]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int grow = m0 + wm * WM + i * 16 + kch * 4 + r;
                if (grow >= M) continue;
                float v = acc[i][j][r];
                if constexpr (HAS_BIAS) v += bv;
                if constexpr (RELU) v = v > 0.f ? v : 0.f;
                if constexpr (DROPOUT)
                    v = (keep4 >> r) & 1 ? v * drop_args(da...).scale : 0.f;
                C[(long)grow * N + gcol] = f2bf(v);
            }
        }
    }
}

// ------------------------------------------------- gemm_nt (glds tier)

// Compute-bound tier (aligned ≥128-multiple shapes, no fused mask):
// stages tiles with gfx950 global_load_lds (direct HBM->LDS DMA, no
// VGPR round trip; the CDNA4 guide's ladder measures this as the
// dominant lever for the 128² structure).  LDS image is LANE-LINEAR
// (glds writes base+lane*16), so the bank-conflict fix is an XOR
// swizzle applied to BOTH the per-lane global SOURCE address and the
// fragment reads (rule 21): 16-B chunk c of row r lives at physical
// chunk c ^ ((r>>2)&3) — fragment-read banks become all-distinct.
template <bool HAS_BIAS, bool RELU>
__global__ __launch_bounds__(256) void gemm_nt_glds_kernel(
    const __bf16* __restrict__ A,     // [M][K], M%128==0, K%32==0
    const __bf16* __restrict__ B,     // [N][K], N%128==0
    const __bf16* __restrict__ bias,  // [N]
    __bf16* __restrict__ C,           // [M][N]
    int M, int N, int K) {
    constexpr int BM = 128, BN = 128, BKG = 32;

    __shared__ ushort As[2][BM * BKG];  // lane-linear [128][32] bf16
    __shared__ ushort Bs[2][BN * BKG];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1;  // 2x2 waves, wave tile 64x64
    const int wn = wave & 1;

    // XCD-aware bijective remap (see gemm_nt_kernel)
    const int gx = gridDim.x, gy = gridDim.y;
    const int nwg = gx * gy;
    const int hw = blockIdx.x + gx * blockIdx.y;
    const int wid = xcd_remap(hw, nwg);
    const int m0 = ((wid / gy) % gx) * BM;
    const int n0 = (wid % gy) * BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    // staging: glds is a WAVE instruction — each of the 4 waves gets
    // its own wave-uniform LDS base (16-row span); lane l covers
    // (row = l>>2 within the span, physical 16-B chunk p = l&3).  The
    // source chunk is PRE-SWIZZLED: c = p ^ ((row>>2)&3), matching
    // the fragment-read XOR (rule 21: both sides or neither).
    const int lrow4 = lane >> 2;  // 0..15 rows within the wave span
    const int p16 = lane & 3;     // physical chunk
    auto stage = [&](int buf, int k0) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int rA = half * 64 + wave * 16 + lrow4;
            const int cA = (p16 ^ ((rA >> 2) & 3)) * 8;
            __builtin_amdgcn_global_load_lds(
                (gptr_t)&A[(long)(m0 + rA) * K + k0 + cA],
                (lptr_t)&As[buf][(half * 64 + wave * 16) * BKG], 16, 0, 0);
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int rB = half * 64 + wave * 16 + lrow4;
            const int cB = (p16 ^ ((rB >> 2) & 3)) * 8;
            __builtin_amdgcn_global_load_lds(
                (gptr_t)&B[(long)(n0 + rB) * K + k0 + cB],
                (lptr_t)&Bs[buf][(half * 64 + wave * 16) * BKG], 16, 0, 0);
        }
    };

    const int lrow = lane & 15;
    const int kch = lane >> 4;

    stage(0, 0);
    __syncthreads();

    const int nsteps = K / BKG;
    int cur = 0;
    for (int t = 0; t < nsteps; ++t) {
        if (t + 1 < nsteps) stage(cur ^ 1, (t + 1) * BKG);

        bf16x8 a_frag[4], b_frag[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + i * 16 + lrow;
            a_frag[i] = *(const bf16x8*)
                &As[cur][row * BKG + (kch ^ ((row >> 2) & 3)) * 8];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = wn * 64 + j * 16 + lrow;
            b_frag[j] = *(const bf16x8*)
                &Bs[cur][row * BKG + (kch ^ ((row >> 2) & 3)) * 8];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
        // __syncthreads() drains the in-flight glds (hipcc emits the
        // vmcnt(0) inside the barrier when LDS-DMA is outstanding)
        __syncthreads();
        cur ^= 1;
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gcol = n0 + wn * 64 + j * 16 + lrow;
            float bv = 0.f;
            if constexpr (HAS_BIAS) bv = bf2f(bias[gcol]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int grow = m0 + wm * 64 + i * 16 + kch * 4 + r;
                float v = acc[i][j][r];
                if constexpr (HAS_BIAS) v += bv;
                if constexpr (RELU) v = v > 0.f ? v : 0.f;
                C[(long)grow * N + gcol] = f2bf(v);
            }
        }
    }
}

// ---------------------------------------------------------------- colsum

// 8-wide vectorized variant: each thread owns 8 contiguous columns
// (one bf16x8 load per row), 8x the bytes in flight per thread vs the
// scalar kernel (measured 195 us at 16384x4096 = 11x off roofline —
// latency-bound scalar loads).
template <bool HAS_MASK>
__global__ __launch_bounds__(256) void colsum8_kernel(
    const __bf16* __restrict__ dY,    // [M][N]
    const __bf16* __restrict__ mask,  // [M][N]
    float* __restrict__ gb,           // [N] (atomicAdd +=)
    int M, int N, int rows_per_block) {
    const int col0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    if (col0 >= N) return;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // 4-row unroll: four independent 16-B loads in flight per thread
    // per iteration (the single-row loop was latency-serialized —
    // measured 78 µs at 16384×4096 vs the ~17 µs traffic floor)
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
        bf16x8 v0 = *(const bf16x8*)(dY + (long)(r + 0) * N + col0);
        bf16x8 v1 = *(const bf16x8*)(dY + (long)(r + 1) * N + col0);
        bf16x8 v2 = *(const bf16x8*)(dY + (long)(r + 2) * N + col0);
        bf16x8 v3 = *(const bf16x8*)(dY + (long)(r + 3) * N + col0);
        if constexpr (HAS_MASK) {
            bf16x8 m0 = *(const bf16x8*)(mask + (long)(r + 0) * N + col0);
            bf16x8 m1 = *(const bf16x8*)(mask + (long)(r + 1) * N + col0);
            bf16x8 m2 = *(const bf16x8*)(mask + (long)(r + 2) * N + col0);
            bf16x8 m3 = *(const bf16x8*)(mask + (long)(r + 3) * N + col0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (bf2f(m0[e]) > 0.f) s[e] += bf2f(v0[e]);
                if (bf2f(m1[e]) > 0.f) s[e] += bf2f(v1[e]);
                if (bf2f(m2[e]) > 0.f) s[e] += bf2f(v2[e]);
                if (bf2f(m3[e]) > 0.f) s[e] += bf2f(v3[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                s[e] += bf2f(v0[e]) + bf2f(v1[e]) + bf2f(v2[e]) +
                        bf2f(v3[e]);
        }
    }
    for (; r < r1; ++r) {
        bf16x8 v = *(const bf16x8*)(dY + (long)r * N + col0);
        if constexpr (HAS_MASK) {
            bf16x8 m = *(const bf16x8*)(mask + (long)r * N + col0);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (bf2f(m[e]) > 0.f) s[e] += bf2f(v[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += bf2f(v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) atomicAdd(&gb[col0 + e], s[e]);
}

template <bool HAS_MASK>
__global__ __launch_bounds__(256) void colsum_kernel(
    const __bf16* __restrict__ dY,    // [M][N]
    const __bf16* __restrict__ mask,  // [M][N]
    float* __restrict__ gb,           // [N] (atomicAdd +=)
    int M, int N, int rows_per_block) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    if (col >= N) return;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) {
        float v = bf2f(dY[(long)r * N + col]);
        if constexpr (HAS_MASK) {
            if (!(bf2f(mask[(long)r * N + col]) > 0.f)) v = 0.f;
        }
        s += v;
    }
    atomicAdd(&gb[col], s);
}

// ---------------------------------------------------------------- launchers

// The tier ladder of every gemm_nt launch.  drop != null (bias + ReLU
// forward under dropout, no mask): the register-staged tiers run the
// mask in their epilogue and the function returns true; the 256-tile and glds tiers run as they are and
// it returns false — the caller owes the standalone pass.
static bool gemm_nt_dispatch(const void* A, const void* B, const void* bias,
                             const void* mask, void* C, int M, int N, int K,
                             bool relu, const DropoutArgs* drop,
                             hipStream_t stream) {
    const bool has_bias = bias != nullptr;
    const bool has_mask = mask != nullptr;

    // The register-staged kernel exists in five flavours, not eight:
    // bias excludes the mask and the mask excludes ReLU (a forward call
    // has bias/ReLU, a dgrad call has the mask), so the flags are
    // reduced to those five before they become template arguments.
    const bool use_mask = has_mask && !has_bias;
    const bool use_relu = relu && !use_mask;
    auto launch = [&](auto bm_tag) {
        constexpr int BM = decltype(bm_tag)::value;
        constexpr int BN = BM == 128 ? 128 : 64;
        constexpr int WAVES_M = BM == 32 ? 1 : 2;
        // 4 waves 2x2 everywhere ≥64: 8-wave 128² measured WORSE
        // (623 vs 720 TF @8k³) without the full 8-phase schedule —
        // exactly the guide's T3/T5 regime gate
        constexpr int WAVES_N = BM == 32 ? 4 : 2;
        dim3 block(WAVES_M * WAVES_N * 64);
        dim3 grid(cdiv(M, BM), cdiv(N, BN));
        if (drop) {
            hipLaunchKernelGGL(
                (gemm_nt_kernel<BM, BN, 32, WAVES_M, WAVES_N, true, true,
                                false, true, DropoutArgs>),
                grid, block, 0, stream, (const __bf16*)A, (const __bf16*)B,
                (const __bf16*)bias, (const __bf16*)nullptr, (__bf16*)C, M, N,
                K, *drop);
            return;
        }
        with_bools(
            [&](auto hb, auto rl, auto hm) {
                // Measured: KSTEP=64 is throughput-neutral at these
                // shapes (barrier savings offset by the occupancy drop
                // 7->4 blocks/CU), so every launch uses KSTEP=32; the
                // template keeps the deep K-step one constant away for
                // wider models.
                if constexpr (!(hm.value && (hb.value || rl.value)))
                    hipLaunchKernelGGL(
                        (gemm_nt_kernel<BM, BN, 32, WAVES_M, WAVES_N,
                                        hb.value, rl.value, hm.value>),
                        grid, block, 0, stream, (const __bf16*)A,
                        (const __bf16*)B, (const __bf16*)bias,
                        (const __bf16*)mask, (__bf16*)C, M, N, K);
            },
            has_bias, use_relu, use_mask);
    };
    using B128 = std::integral_constant<int, 128>;
    using B64 = std::integral_constant<int, 64>;
    using B32 = std::integral_constant<int, 32>;

    // widest tier first: 256-tile 8-phase kernel (gemm256.hip) for
    // aligned wide shapes — measured 1.3-1.6x the 128-glds tier
    // (1027-1293 TF vs 692-811 at 4096-16384 x 4096^2, zero LDS bank
    // conflicts; scripts/test_gemm256.py).  SS_GEMM256=0 disables.
    if (!has_mask && N >= 512 && (long)(M / 256) * (N / 256) >= 128) {
        static const int en256 = env_int("SS_GEMM256", 1);
        if (en256 && ss_gemm_nt_256(A, B, bias, C, M, N, K, relu, stream))
            return false;
    }
    // compute-bound tier: aligned shapes with no fused mask go to the
    // glds-staged kernel (direct HBM->LDS DMA)
    if (!has_mask && N >= 128 && M % 128 == 0 && N % 128 == 0 &&
        K % 32 == 0 && (long)(M / 128) * (N / 128) >= 512) {
        with_bools(
            [&](auto hb, auto rl) {
                hipLaunchKernelGGL(
                    (gemm_nt_glds_kernel<hb.value, rl.value>),
                    dim3(M / 128, N / 128), dim3(256), 0, stream,
                    (const __bf16*)A, (const __bf16*)B, (const __bf16*)bias,
                    (__bf16*)C, M, N, K);
            },
            has_bias, relu);
        return false;
    }
    // 128x128 only when the grid still covers the CUs with >=2
    // blocks each (1 block/CU = 4 waves starves latency hiding)
    if (N >= 128 && (long)cdiv(M, 128) * cdiv(N, 128) >= 512) {
        launch(B128{});
    } else if (M < 48 ||
               (long)cdiv(M, 64) * cdiv(N, 64) < 192) {
        // small-M / small-grid shapes: the 32-row config doubles the
        // block count (latency-bound regime — µbatched schedules)
        launch(B32{});
    } else {
        launch(B64{});
    }
    return drop != nullptr;
}

void ss_gemm_nt(const void* A, const void* B, const void* bias,
                const void* mask, void* C, int M, int N, int K,
                bool relu, hipStream_t stream) {
    gemm_nt_dispatch(A, B, bias, mask, C, M, N, K, relu, nullptr, stream);
}

bool ss_gemm_nt_dropout(const void* A, const void* B, const void* bias,
                        void* C, int M, int N, int K,
                        const DropoutArgs& drop, hipStream_t stream) {
    return gemm_nt_dispatch(A, B, bias, nullptr, C, M, N, K, true, &drop,
                            stream);
}

void ss_colsum(const void* dY, const void* mask, void* gb, int M, int N,
               hipStream_t stream) {
    // enough blocks to cover the CUs (256 CUs; Guideline 11)
    const bool vec8 = (N % 8 == 0) && N >= 2048;
    const int cols_per_block = vec8 ? 2048 : 256;
    int col_tiles = cdiv(N, cols_per_block);
    int splits = cdiv(512, col_tiles);
    if (splits > cdiv(M, 64)) splits = cdiv(M, 64);
    if (splits < 1) splits = 1;
    int rows_per_block = cdiv(M, splits);
    dim3 grid(col_tiles, splits);
    dim3 block(256);
    with_bools(
        [&](auto v8, auto hm) {
            if constexpr (v8.value)
                hipLaunchKernelGGL((colsum8_kernel<hm.value>), grid, block, 0,
                                   stream, (const __bf16*)dY,
                                   (const __bf16*)mask, (float*)gb, M, N,
                                   rows_per_block);
            else
                hipLaunchKernelGGL((colsum_kernel<hm.value>), grid, block, 0,
                                   stream, (const __bf16*)dY,
                                   (const __bf16*)mask, (float*)gb, M, N,
                                   rows_per_block);
        },
        vec8, mask != nullptr);
}
