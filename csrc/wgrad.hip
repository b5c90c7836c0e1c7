// Weight-gradient TN GEMM for the MLP hot path (gfx950 / MI355X).
//
//   wgrad_tn: gW[Mo,N] += (dY[Kb,Mo] ⊙ mask)^T · X[Kb,N]
//             gb[Mo]   += Σ_rows (dY ⊙ mask)          (fused bias grad)
//
// Split-K over the batch with f32 atomicAdd into gW — the atomic IS the
// gradient accumulation across µbatches / split-K slices (reference
// grad accumulation: layers.py:135-136).
//
// Global float atomics run at ONE chip-wide byte rate (~1.3 TB/s of
// added bytes) whatever the tiling, so every unit of K-parallelism that
// lives in a separate block costs a full output tile of atomic bytes.
// The kernel therefore carries K-parallelism INSIDE the block as well:
// KG wave groups (each the 2x2 arrangement of four waves on the same
// output tile, each with its own LDS image) take every KG-th 64-row
// K-step of the block's K-range; after the loop the groups' accumulator
// tiles are summed through LDS in a fixed group order and the block
// issues ONE set of atomics, row-contiguously (each wave-instruction
// covers 64 consecutive floats of one gW row = 256 contiguous bytes,
// the full-rate shape).  There is no inter-block protocol.

#include "common.h"
#include "launchers.h"

// operands in the global address space (see the kernel's pointer note)
using gbf16 = __attribute__((address_space(1))) __bf16;
using gbf16x8 = __attribute__((address_space(1))) bf16x8;

// Second launch bound = waves per SIMD the register allocation must
// leave room for: accumulators + the prefetch set + fragments stay
// inside the two-wave budget at 128-wide tiles, four waves at 64x64.
template <int BMT, int BNT, bool HAS_MASK, int KG>
__global__ __launch_bounds__(KG * 256, BMT* BNT > 64 * 64 ? 2 : 4)
void wgrad_tn_kernel(
    const __bf16* __restrict__ dY,    // [Kb][Mo]
    const __bf16* __restrict__ X,     // [Kb][N]
    const __bf16* __restrict__ mask,  // [Kb][Mo]
    float* __restrict__ gW,           // [Mo][N] (atomicAdd +=)
    float* __restrict__ gb,           // [Mo] or null: fused bias grad
    int Mo, int N, int Kb, int k_per_split,
    // optional CHUNK TABLE (deferred µbatch wgrad): int64 rows of
    // {dY*, X*, mask*}; grid.z covers chunks*split and each chunk is
    // an independent [Kb][*] pair accumulated into the same gW/gb —
    // ONE launch replaces num_µbatches launches per layer.
    const long* __restrict__ chunks, int nsplit) {
    // TN GEMM over the batch axis.  Tiles are staged in a BLOCKED
    // [rows/16][BKW/4][4][16] bf16 image so that
    //   * staging is plain 16-B vector writes (global rows are
    //     m/n-contiguous — no software transpose), and
    //   * MFMA A/B fragments come out of LDS through the gfx950
    //     HARDWARE transpose read ds_read_b64_tr_b16
    //     (__builtin_amdgcn_ds_read_tr16_b64_v4bf16): each 16-lane
    //     group hands the crossbar one [4][16] subtile and receives
    //     its column — semantics verified on hardware by
    //     scripts/probe_tr.hip.
    // The 128x128 instantiation halves both operands' L2 re-reads for
    // wide layers (traffic ∝ dY·(N/BNT) + X·(Mo/BMT)).
    constexpr int BKW = 64;        // K-step (batch rows per stage)
    constexpr int NMA = BMT / 16;  // 16-row blocks per A tile
    constexpr int NMB = BNT / 16;
    constexpr int FM = BMT / 32;   // 16x16 frags per wave (2x2 waves)
    constexpr int FN = BNT / 32;
    constexpr int NT = KG * 256;
    constexpr int A_EL = NMA * 16 * 64;     // bf16 per dY^T image
    constexpr int B_EL = NMB * 16 * 64;     // bf16 per X^T image
    constexpr int GRP_EL = A_EL + B_EL;     // one group's staging
    constexpr int STAGE_F = KG * GRP_EL / 2;  // staging space in floats
    // The summed f32 tile reuses the staging space; when the tile is
    // larger (KG=1 at 128 rows) it goes out in NPASS row bands.
    constexpr int NPASS = BMT * BNT <= STAGE_F       ? 1
                          : BMT * BNT <= 2 * STAGE_F ? 2
                                                     : 4;
    constexpr int RP = BMT / NPASS;  // tile rows per pass
    static_assert(RP % 16 == 0 && RP * BNT <= STAGE_F, "epilogue band");
    static_assert(KG * 256 <= STAGE_F, "bias partials fit the staging");

    // ALL LDS is this one array: per-group images in the loop, then
    // the bias partials, then the f32 tile of the reduction.
    __shared__ __attribute__((aligned(16))) ushort smem[KG * GRP_EL];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int gtid = tid & 255;  // thread within its K-group
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave = wv & 3;
    const int grp = wv >> 2;
    const int wm = wave >> 1;  // 2x2 waves
    const int wn = wave & 1;
    ushort* const At = smem + grp * GRP_EL;  // dY^T tile, blocked
    ushort* const Bt = At + A_EL;            // X^T tile, blocked
    // XCD-aware block remap (T1, bijective variant): the dispatcher
    // places hw block b on XCD b%8; remap so each XCD owns a
    // CONTIGUOUS run of work ids decoded n-tile-fastest — blocks that
    // share a dY m-slice then read it from ONE XCD's L2 instead of
    // filling all eight.
    const int gx = gridDim.x, gy = gridDim.y;
    const int nwg = gx * gy * gridDim.z;
    const int hw = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const int wid = xcd_remap(hw, nwg);
    const int bidy = wid % gy;
    const int bidx = (wid / gy) % gx;
    int bidz = wid / (gy * gx);
    if (chunks) {
        const long* row = chunks + (long)(bidz / nsplit) * 3;
        dY = (const __bf16*)row[0];
        X = (const __bf16*)row[1];
        mask = (const __bf16*)row[2];
        bidz = bidz % nsplit;
    }
    // Pointers read from the chunk table lose their address space and
    // would compile to FLAT loads, which count on lgkmcnt as well: the
    // LDS waits ahead of the MFMAs would then also wait for the
    // prefetch.  Name the global address space explicitly.
    const gbf16* const gdY = (const gbf16*)dY;
    const gbf16* const gX = (const gbf16*)X;
    const gbf16* const gmask = (const gbf16*)mask;
    const int m0 = bidx * BMT;
    const int n0 = bidy * BNT;
    const int kbeg = bidz * k_per_split;
    const int kend = min(Kb, kbeg + k_per_split);

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    // 16-row / 16-column fragments of this wave that reach into the
    // matrix (wave-uniform).  The N-remainder tile of a 784-wide layer
    // has 16 valid columns of 128: its waves skip the K-step's reads
    // and MFMAs or run the one-column form (see the K loop), and no
    // wave writes a fragment past the edge back.
    const int fmv = min(FM, max(0, (Mo - m0 - wm * (BMT / 2) + 15) / 16));
    const int fnv = min(FN, max(0, (N - n0 - wn * (BNT / 2) + 15) / 16));

    const bool do_db = (gb != nullptr) && (bidy == 0);
    float db_part = 0.f;

    // mblk-major image with the ksub bits 0,1 SWAPPED in the subtile
    // position (wgrad256.hip's placement): the four tr-read lane
    // groups (k-stride 2) then land on {row even|odd} x {phase 0|1}
    // of the 256-B bank rows — the optimal 2-clk pattern with NO
    // padding.
    auto swsub = [](int ksub) {
        return (ksub & ~3) | ((ksub & 1) << 1) | ((ksub >> 1) & 1);
    };
    auto baddr = [swsub](int k, int m) {
        return ((m >> 4) * 16 + swsub(k >> 2)) * 64 + (k & 3) * 16 + (m & 15);
    };

    // register staging: thread t of the group covers ELA contiguous
    // elems of one row of the [BKW][BMT] tile, as 8-element chunks.
    // Each chunk decides for itself: wholly in range -> one 16-B load,
    // wholly out of range -> zeros, straddling the edge (only when the
    // width is no multiple of 8) -> element by element.
    constexpr int ELA = BKW * BMT / 256;
    constexpr int ELB = BKW * BNT / 256;
    constexpr int CA = ELA / 8, CB = ELB / 8;
    const int ska = (gtid * ELA) / BMT, sma = (gtid * ELA) % BMT;
    const int skb = (gtid * ELB) / BNT, smb = (gtid * ELB) % BNT;
    bf16x8 ra[CA], rmk[CA], rb[CB];  // the ONE prefetch register set

    // `valid` = elements of the row left at this chunk.  A width that
    // is a multiple of 8 has no straddling chunk (chunk starts are
    // multiples of 8): that case is ONE unconditional 16-B load per
    // chunk, straight-line code.  A chunk out of range loads the
    // tensor's first 16 bytes instead (one shared cache line, the
    // value is dropped) and is zeroed in the WRITE half — zero-filling
    // or predicating the destination registers here made hipcc put a
    // vmcnt(0) between the dY and the X loads, i.e. ahead of the MFMAs
    // the prefetch is meant to run under.
    auto load_chunk = [](const gbf16* p, const gbf16* base, int valid,
                         auto width_mult8) {
        bf16x8 v;
        if constexpr (decltype(width_mult8)::value) {
            v = *(const gbf16x8*)(valid > 0 ? p : base);
            return v;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (__bf16)0.f;
        if (valid >= 8) {
            v = *(const gbf16x8*)p;
        } else if (valid > 0) {
            // straddling chunk: 8 loads in flight, element 0 (valid)
            // stands in for the ones past the edge
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const __bf16 t = p[i < valid ? i : 0];
                v[i] = i < valid ? t : (__bf16)0.f;
            }
        }
        return v;
    };
    const bool vecA = (Mo & 7) == 0, vecB = (N & 7) == 0;  // block-uniform
    // elements left in this thread's row at its first chunk; rows past
    // the K-range count as empty
    auto left_a = [&](int k0) {
        return k0 + ska < kend ? Mo - (m0 + sma) : 0;
    };
    auto left_b = [&](int k0) {
        return k0 + skb < kend ? N - (n0 + smb) : 0;
    };
    // ISSUE half: global -> registers for the K-step at k0
    auto stage_load = [&](int k0) {
        {
            const long off = (long)(k0 + ska) * Mo + m0 + sma;
            const int left = left_a(k0);
            auto rows = [&](auto w8) {
#pragma unroll
                for (int ch = 0; ch < CA; ++ch) {
                    ra[ch] = load_chunk(gdY + off + ch * 8, gdY,
                                        left - ch * 8, w8);
                    if constexpr (HAS_MASK)
                        rmk[ch] = load_chunk(gmask + off + ch * 8, gmask,
                                             left - ch * 8, w8);
                }
            };
            if (vecA) {
                rows(std::true_type{});
            } else {
                // the odd-width form drains its own loads: left
                // pending, its scratch registers make hipcc guard the
                // 16-B form's prefetch registers with a vmcnt(0) too
                rows(std::false_type{});
                __builtin_amdgcn_s_waitcnt(0x0F70);
            }
        }
        {
            const long off = (long)(k0 + skb) * N + n0 + smb;
            const int left = left_b(k0);
            auto rows = [&](auto w8) {
#pragma unroll
                for (int ch = 0; ch < CB; ++ch)
                    rb[ch] = load_chunk(gX + off + ch * 8, gX, left - ch * 8,
                                        w8);
            };
            if (vecB) {
                rows(std::true_type{});
            } else {
                rows(std::false_type{});
                __builtin_amdgcn_s_waitcnt(0x0F70);
            }
        }
    };
    // WRITE half: registers -> the group's image for the K-step at k0;
    // the mask and the zeros of out-of-range chunks are applied here
    auto stage_write = [&](int k0) {
        const int la = left_a(k0), lb = left_b(k0);
#pragma unroll
        for (int ch = 0; ch < CA; ++ch) {
            bf16x8 v = ra[ch];
            const bool in = la - ch * 8 > 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bool keep = in;
                if constexpr (HAS_MASK)
                    keep = keep && bf2f(rmk[ch][i]) > 0.f;
                if (!keep) v[i] = (__bf16)0.f;
            }
            *(bf16x8*)&At[baddr(ska, sma + ch * 8)] = v;
        }
#pragma unroll
        for (int ch = 0; ch < CB; ++ch) {
            bf16x8 v = rb[ch];
            if (!(lb - ch * 8 > 0)) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = (__bf16)0.f;
            }
            *(bf16x8*)&Bt[baddr(skb, smb + ch * 8)] = v;
        }
    };

    // glds staging (unmasked full tiles): a subtile of the unpadded
    // image is exactly 8 aligned 16-B pieces, so a per-lane SOURCE
    // scatter performs the transpose while the LDS dest stays
    // lane-linear; piece q -> position p = q/8 (mblk = p/16, ksub =
    // swsub(p&15)), r = q%8 -> global (k = ksub*4 + (r>>1), m =
    // mblk*16 + (r&1)*8).  The four waves of a group fill its image.
    auto glds_stage = [&](const gbf16* src, ushort* img,
                          int nmt, int ld, int base_col, int gk0) {
        const int total = nmt * 16 * 8;          // pieces
        const int per_wave = total / 4;          // 4 waves per group
        for (int i0 = 0; i0 < per_wave; i0 += 64) {
            const int q = wave * per_wave + i0 + lane;
            const int p = q >> 3, rr = q & 7;
            const int ksub = ((p & 15) & ~3) | (((p & 15) & 1) << 1) |
                             (((p & 15) >> 1) & 1);
            const int k = ksub * 4 + (rr >> 1);
            const int m = (p >> 4) * 16 + (rr & 1) * 8;
            __builtin_amdgcn_global_load_lds(
                (gptr_t)(src + (long)(gk0 + k) * ld + base_col + m),
                (lptr_t)(img + (long)(wave * per_wave + i0) * 8), 16, 0,
                0);
        }
    };
    auto full_tile = [&](int k0) {
        return !HAS_MASK && m0 + BMT <= Mo && n0 + BNT <= N &&
               k0 + BKW <= kend;
    };

    // ---- fragments via hardware transpose read, then MFMA ----
    const int lcol4 = (lane & 15) * 4;
    auto mma_step = [&](auto all_cols) {
        // all_cols false: only the first 16-column fragment (a wave
        // whose other fragments lie past N)
        constexpr int FNU = decltype(all_cols)::value ? FN : 1;
#pragma unroll
        for (int kk = 0; kk < BKW / 32; ++kk) {
            const int g2 = kk * 8 + (lane >> 4) * 2;  // k-subtile pair
            bf16x8 a_frag[FM], b_frag[FNU];
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int mblk = wm * FM + i;
                bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4p)&At[(mblk * 16 + swsub(g2)) * 64 + lcol4]);
                bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4p)&At[(mblk * 16 + swsub(g2 + 1)) * 64 + lcol4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a_frag[i][e] = lo[e];
                    a_frag[i][e + 4] = hi[e];
                }
            }
#pragma unroll
            for (int j = 0; j < FNU; ++j) {
                const int nblk = wn * FN + j;
                bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4p)&Bt[(nblk * 16 + swsub(g2)) * 64 + lcol4]);
                bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4p)&Bt[(nblk * 16 + swsub(g2 + 1)) * 64 + lcol4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    b_frag[j][e] = lo[e];
                    b_frag[j][e + 4] = hi[e];
                }
            }
#pragma unroll
            for (int i = 0; i < FM; ++i) {
#pragma unroll
                for (int j = 0; j < FNU; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
            }
        }
    };

    // K loop.  Group g owns K-steps g, g+KG, ... of the block's range;
    // every group runs the same trip count and reaches every barrier,
    // also when it has no step left (small Kb, the last split).
    // Register-staged steps are software-pipelined (async-STAGE split):
    // the loads of the group's next step are issued before this step's
    // MFMAs and written to LDS after the barrier that frees the image.
    const int nsteps = kend > kbeg ? (kend - kbeg + BKW - 1) / BKW : 0;
    const int niter = (nsteps + KG - 1) / KG;
    int k0 = kbeg + grp * BKW;
    if (k0 < kend && !full_tile(k0)) stage_load(k0);
    for (int it = 0; it < niter; ++it, k0 += KG * BKW) {
        const bool active = k0 < kend;
        // vmcnt(0) alone: the prefetch is due here anyway.  Stated on
        // every path, it keeps hipcc from guarding the prefetch
        // registers with a vmcnt(0) in the middle of the NEXT issue
        // half (seen in the .s between the dY and the X loads, where it
        // held the MFMAs back until the dY loads had landed).
        __builtin_amdgcn_s_waitcnt(0x0F70);
        if (active) {
            if (full_tile(k0)) {
                glds_stage(gdY, At, NMA, Mo, m0, k0);
                glds_stage(gX, Bt, NMB, N, n0, k0);
            } else {
                stage_write(k0);
            }
        }
        __syncthreads();  // also drains the LDS-DMA (vmcnt inside)

        const int kn = k0 + KG * BKW;
        if (kn < kend && !full_tile(kn)) stage_load(kn);

        if (active) {
            if (do_db) {
                constexpr int NKQ = 256 / BMT;  // threads stacked on k
                constexpr int KPT = BKW / NKQ;  // k values per thread
                const int m = gtid % BMT, kq = gtid / BMT;
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    const ushort u = At[baddr(kq * KPT + j, m)];
                    db_part += bf2f(*(const __bf16*)&u);
                }
            }
            // wave-uniform: a wave with no fragment inside the matrix
            // reads and multiplies nothing; one with a single column
            // fragment (the 16-column remainder of N = k·128 + 16)
            // takes the one-column form.  Run-time guards on every
            // fragment of one form compiled to +66 VGPRs of acc
            // copies (spills at KG = 2); this second form costs +28.
            if (fmv > 0 && fnv > 1)
                mma_step(std::true_type{});
            else if (fmv > 0 && fnv == 1)
                mma_step(std::false_type{});
        }
        __syncthreads();
    }

    // ---- epilogue: the staging space is free from here on ----
    float* const red = (float*)smem;

    if (do_db) {
        // KG*NKQ partials per row, summed in a fixed order
        constexpr int NQ = KG * (256 / BMT);
        red[tid] = db_part;  // [grp][kq][m] with m fastest
        __syncthreads();
        if (tid < BMT && m0 + tid < Mo) {
            float s = 0.f;
#pragma unroll
            for (int qq = 0; qq < NQ; ++qq) s += red[qq * BMT + tid];
            atomicAdd(&gb[m0 + tid], s);
        }
        __syncthreads();
    }

    const int lrow = lane & 15;
    const int kch = lane >> 4;
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        // sum the groups' accumulators into the f32 band, group 0
        // first, then 1, ... — a fixed order, so split_k == 1 stays
        // bitwise reproducible
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            if (grp == g) {
#pragma unroll
                for (int i = 0; i < FM; ++i) {
                    const int trow = wm * (BMT / 2) + i * 16;
                    if (trow / RP != p || i >= fmv) continue;
#pragma unroll
                    for (int j = 0; j < FN; ++j) {
                        if (j >= fnv) continue;
                        const int cc = wn * (BNT / 2) + j * 16 + lrow;
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            const int ix =
                                (trow - p * RP + kch * 4 + rr) * BNT + cc;
                            if (g == 0)
                                red[ix] = acc[i][j][rr];
                            else
                                red[ix] += acc[i][j][rr];
                        }
                    }
                }
            }
            __syncthreads();
        }
        // ONE set of atomics per block, row-contiguous: a wave
        // instruction covers 64 consecutive floats of one gW row
        for (int ix = tid; ix < RP * BNT; ix += NT) {
            const int grow = m0 + p * RP + ix / BNT;
            const int gcol = n0 + ix % BNT;
            if (grow < Mo && gcol < N)
                atomicAdd(&gW[(long)grow * N + gcol], red[ix]);
        }
        if (p + 1 < NPASS) __syncthreads();
    }
}

// ------------------------------------------------------------ dispatch

namespace {

// shipped K-groups per block, by tile regime (measured arms:
// docs/KERNELS.md, profiles/r03_wgrad_onchip_reduce.md)
constexpr int WGRAD_KG_128 = 2;  // 128x128 and 64x128 tiles (LDS caps it)
constexpr int WGRAD_KG_64 = 4;   // 64x64 tiles
// blocks the auto split aims for: one per CU
constexpr int WGRAD_TARGET_BLOCKS = 256;

// tile and K-group choice shared by the plain and the chunked launcher
struct WgradCfg {
    int bm, bn, kg;
};

WgradCfg wgrad_cfg(int Mo, int N, int split_k) {
    // big tiles only pay when both dims are wide enough that the
    // grid still covers the CUs AND operand re-reads dominate
    // (measured: at 256-wide layers the 64-config's block count wins)
    int tile = ((Mo >= 256 && N >= 512) || (Mo >= 512 && N >= 256)) ? 1 : 0;
    // debug/tuning overrides (read once): SS_WGRAD_BIG = 0 (64x64),
    // 1 (128x128), 2 (64x128); SS_WGRAD_KG = 1, 2, 4
    static const int env_big = env_int("SS_WGRAD_BIG", -1);
    static const int env_kg = env_int("SS_WGRAD_KG", -1);
    if (env_big >= 0) tile = env_big > 2 ? 1 : env_big;
    WgradCfg c;
    c.bm = tile == 1 ? 128 : 64;
    c.bn = tile == 0 ? 64 : 128;
    // K-groups per block: see docs/KERNELS.md for the measured arms
    c.kg = tile == 0 ? WGRAD_KG_64 : WGRAD_KG_128;
    if (env_kg == 1 || env_kg == 2 || env_kg == 4) c.kg = env_kg;
    if (tile != 0 && c.kg > 2) c.kg = 2;  // LDS: two blocks per CU
    // split_k == 1 is the single-owner deterministic path: one group,
    // one block per tile, K summed in order
    if (split_k == 1) c.kg = 1;
    return c;
}

// auto split: ~256 blocks, one per CU, each of KG groups of four waves
// (8 waves per CU at the 128 tiles, 16 at 64x64).  The atomic bytes of
// a launch are split_k·Mo·N·4 at one chip-wide rate, so K-parallelism
// beyond that block count belongs in the groups, not in the split:
// measured at 16384x256x784 masked, KG=2: split 8/16/32/64 = 56/38/48/68
// µs; at 16384x256x256, KG=4: split 8/16/32 = 22.6/15.5/21.1 µs.
// SS_WGRAD_BLOCKS overrides the target (read once).
int wgrad_auto_split(int tiles, int Kb, int kg) {
    static const int env_blocks = env_int("SS_WGRAD_BLOCKS", 0);
    const int target = env_blocks > 0 ? env_blocks : WGRAD_TARGET_BLOCKS;
    int split_k = cdiv(target, tiles);
    // round DOWN to a power of two (even k-slice boundaries;
    // measured best at 256×784)
    while (split_k & (split_k - 1)) split_k &= split_k - 1;
    const int max_split = cdiv(Kb, 64 * kg);  // a K-step per group
    if (split_k > max_split) split_k = max_split;
    return split_k;
}

}  // namespace

#define WGRAD_LAUNCH(BMT, BNT, HM, KGV, ...)                                \
    hipLaunchKernelGGL((wgrad_tn_kernel<BMT, BNT, HM, KGV>), grid,          \
                       dim3(KGV * 256), 0, stream, __VA_ARGS__)
#define WGRAD_BY_MASK(BMT, BNT, KGV, ...)                                   \
    do {                                                                    \
        if (has_mask) WGRAD_LAUNCH(BMT, BNT, true, KGV, __VA_ARGS__);       \
        else WGRAD_LAUNCH(BMT, BNT, false, KGV, __VA_ARGS__);               \
    } while (0)
#define WGRAD_DISPATCH(cfg, ...)                                            \
    do {                                                                    \
        if (cfg.bm == 128) {                                                \
            if (cfg.kg == 1) WGRAD_BY_MASK(128, 128, 1, __VA_ARGS__);       \
            else WGRAD_BY_MASK(128, 128, 2, __VA_ARGS__);                   \
        } else if (cfg.bn == 128) {                                         \
            if (cfg.kg == 1) WGRAD_BY_MASK(64, 128, 1, __VA_ARGS__);        \
            else WGRAD_BY_MASK(64, 128, 2, __VA_ARGS__);                    \
        } else {                                                            \
            if (cfg.kg == 1) WGRAD_BY_MASK(64, 64, 1, __VA_ARGS__);         \
            else if (cfg.kg == 2) WGRAD_BY_MASK(64, 64, 2, __VA_ARGS__);    \
            else WGRAD_BY_MASK(64, 64, 4, __VA_ARGS__);                     \
        }                                                                   \
    } while (0)

void ss_wgrad_tn(const void* dY, const void* X, const void* mask, void* gW,
                 void* gb, int Mo, int N, int Kb, int split_k,
                 hipStream_t stream) {
    // widest tier first: 8-phase 256-tile TN kernel for aligned wide
    // unmasked shapes (bias grad via the standalone colsum kernel).
    // SS_WGRAD256=0 disables.
    // >= 64 output tiles: below that the split-K short loops lose to
    // the 128-tile kernel (measured 440 vs 514 TF at 1024^2 x 16384)
    if (!mask && split_k <= 0 && Mo >= 512 && N >= 512 &&
        (long)(Mo / 256) * (N / 256) >= 64) {
        static const int en = env_int("SS_WGRAD256", 1);
        if (en && ss_wgrad_tn_256(dY, X, gW, Mo, N, Kb, stream)) {
            if (gb) ss_colsum(dY, nullptr, gb, Kb, Mo, stream);
            return;
        }
    }
    const WgradCfg cfg = wgrad_cfg(Mo, N, split_k);
    if (split_k <= 0)
        split_k = wgrad_auto_split(cdiv(Mo, cfg.bm) * cdiv(N, cfg.bn), Kb,
                                   cfg.kg);
    int k_per_split = cdiv(cdiv(Kb, split_k), 64) * 64;  // BKW=64
    split_k = cdiv(Kb, k_per_split);
    dim3 grid(cdiv(Mo, cfg.bm), cdiv(N, cfg.bn), split_k);
    const bool has_mask = mask != nullptr;
    WGRAD_DISPATCH(cfg, (const __bf16*)dY, (const __bf16*)X,
                   (const __bf16*)mask, (float*)gW, (float*)gb, Mo, N, Kb,
                   k_per_split, (const long*)nullptr, 1);
}

void ss_wgrad_tn_multi(const void* chunk_table, int nchunks, bool has_mask,
                       void* gW, void* gb, int Mo, int N, int Kb_chunk,
                       int split_k, hipStream_t stream) {
    const WgradCfg cfg = wgrad_cfg(Mo, N, split_k);
    if (split_k <= 0)
        split_k = wgrad_auto_split(
            cdiv(Mo, cfg.bm) * cdiv(N, cfg.bn) * nchunks, Kb_chunk, cfg.kg);
    int k_per_split = cdiv(cdiv(Kb_chunk, split_k), 64) * 64;
    split_k = cdiv(Kb_chunk, k_per_split);
    dim3 grid(cdiv(Mo, cfg.bm), cdiv(N, cfg.bn), split_k * nchunks);
    WGRAD_DISPATCH(cfg, (const __bf16*)nullptr, (const __bf16*)nullptr,
                   (const __bf16*)nullptr, (float*)gW, (float*)gb, Mo, N,
                   Kb_chunk, k_per_split, (const long*)chunk_table, split_k);
}
