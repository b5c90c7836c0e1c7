// Device body of the weight-gradient TN GEMM (see wgrad.hip for the
// algorithm): one output tile of one problem over one K-range, from the
// staging loop to the block's single set of atomics.
//
// The body is TEXT that a kernel includes inside its own function, not
// a function, for chain_dev.h's reason: as a force-inlined function
// template (with the block decode passed in as values, or as a callable
// run at the decode's old place) every shipped instantiation compiled
// to other instructions and another register allocation; as text each
// compiles to the very instructions it had with the code written in
// place (profiles/r13_wgrad_group.md, scripts/isa_diff.py).
//
//     #include "wgrad_dev.h"          // file scope: the declarations
//     ...
//     __global__ void kernel(...) {
//         __shared__ __attribute__((aligned(16)))
//         ushort smem[NSTAGE * wgrad_set_el<BMT, BNT, KG>()];
//     #define WGRAD_TILE_HERE
//     #include "wgrad_dev.h"          // the body, once per use
//     }
//
// The body reads by name: the constants BMT, BNT, HAS_MASK, KG, NSTAGE;
// smem (the kernel's ONE LDS array); float* gW, gb; int Mo, N; and the
// statement macro WGRAD_DECODE, which it expands after the wave ids and
// which declares what the block works on:
//     const gbf16 *gdY, *gX, *gmask;   operands [Kb][Mo], [Kb][N], [Kb][Mo]
//     int m0, n0;                       tile origin
//     bool db_owner;                    this block adds gb (n-tile 0)
//     int kbeg, kend;                   K-range
#ifndef SS_WGRAD_DEV_H
#define SS_WGRAD_DEV_H

#include "common.h"

// operands in the global address space (see the pointer note above
// WGRAD_DECODE in wgrad.hip)
using gbf16 = __attribute__((address_space(1))) __bf16;
using gbf16x8 = __attribute__((address_space(1))) bf16x8;

// bf16 elements of one staging set: per-group dY^T and X^T images
template <int BMT, int BNT, int KG>
constexpr int wgrad_set_el() {
    return KG * (BMT + BNT) * 64;
}

// One iteration's overlap of the two-set K loop: `issue` starts the
// LDS-DMA of the next step into `nxt`, `compute` reads the current step
// from `cur`.  The two sets never overlap, and saying so with restrict
// is what the overlap hangs on: inlining turns it into alias scopes on
// the DMA and on the LDS reads, and without them hipcc waits vmcnt(0)
// for EVERY pending LDS-DMA ahead of the first ds_read, i.e. it drains
// the prefetch before the MFMAs it was meant to run under.
template <class Issue, class Compute>
__device__ __forceinline__ void wgrad_two_sets(ushort* __restrict__ cur,
                                               ushort* __restrict__ nxt,
                                               Issue issue, Compute compute) {
    issue(nxt);
    compute(cur);
}

#endif  // SS_WGRAD_DEV_H

#ifdef WGRAD_TILE_HERE
#undef WGRAD_TILE_HERE
{
    // NSTAGE = 1: one staging set; a K-step is staged, drained at a
    // barrier, multiplied, and a second barrier frees the set.
    // NSTAGE = 2: two sets; step t+1 is staged into the other set while
    // step t is multiplied, and the one barrier at the top of an
    // iteration both publishes step t and frees the set of step t-1.
    // NSTAGE changes when loads are issued, never the order of sums.
    static_assert(NSTAGE == 1 || NSTAGE == 2, "staging depth");
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

    // ALL LDS is the caller's one array: per-group images in the loop,
    // then the bias partials, then the f32 tile of the reduction.
    static_assert(KG * GRP_EL == wgrad_set_el<BMT, BNT, KG>(), "set size");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int gtid = tid & 255;  // thread within its K-group
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave = wv & 3;
    const int grp = wv >> 2;
    const int wm = wave >> 1;  // 2x2 waves
    const int wn = wave & 1;
    // the group's images; with two sets, those of the current step
    using img_t = std::conditional_t<NSTAGE == 1, ushort* const, ushort*>;
    img_t At = smem + grp * GRP_EL;  // dY^T tile, blocked
    img_t Bt = At + A_EL;            // X^T tile, blocked
    WGRAD_DECODE

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

    const bool do_db = (gb != nullptr) && (WGRAD_DB_OWNER);
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
    // (Ai, Bi): the images to read with two sets; one set reads At, Bt
    auto mma_step = [&](auto all_cols, const ushort* Ai = nullptr,
                        const ushort* Bi = nullptr) {
        const ushort* const Ar = NSTAGE == 1 ? At : Ai;
        const ushort* const Br = NSTAGE == 1 ? Bt : Bi;
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
                    (lds_v4p)&Ar[(mblk * 16 + swsub(g2)) * 64 + lcol4]);
                bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4p)&Ar[(mblk * 16 + swsub(g2 + 1)) * 64 + lcol4]);
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
                    (lds_v4p)&Br[(nblk * 16 + swsub(g2)) * 64 + lcol4]);
                bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4p)&Br[(nblk * 16 + swsub(g2 + 1)) * 64 + lcol4]);
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
    if constexpr (NSTAGE == 1) {
        if (k0 < kend && !full_tile(k0)) stage_load(k0);
        for (int it = 0; it < niter; ++it, k0 += KG * BKW) {
            const bool active = k0 < kend;
            // vmcnt(0) alone: the prefetch is due here anyway.  Stated
            // on every path, it keeps hipcc from guarding the prefetch
            // registers with a vmcnt(0) in the middle of the NEXT issue
            // half (seen in the .s between the dY and the X loads,
            // where it held the MFMAs back until the dY loads had
            // landed).
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
                // wave-uniform: a wave with no fragment inside the
                // matrix reads and multiplies nothing; one with a
                // single column fragment (the 16-column remainder of
                // N = k·128 + 16) takes the one-column form.  Run-time
                // guards on every fragment of one form compiled to +66
                // VGPRs of acc copies (spills at KG = 2); this second
                // form costs +28.
                if (fmv > 0 && fnv > 1)
                    mma_step(std::true_type{});
                else if (fmv > 0 && fnv == 1)
                    mma_step(std::false_type{});
            }
            __syncthreads();
        }
    } else {
        // Two staging sets; (At, Bt) name the group's image in the set
        // of the CURRENT step.  The ISSUE of a step is its glds (full
        // tiles, straight into the step's set) or its register loads
        // (masked, remainder and tail tiles; written into the set at
        // the top of the step's own iteration).  Step t+1 is issued
        // right after the barrier of iteration t: every wave has then
        // finished the MFMAs of step t-1, the last readers of that set.
        constexpr int SET_EL = KG * GRP_EL;
        ushort* const A0 = At;  // the group's image in set 0
        auto issue = [&](int k, ushort* Ai) {
            if (full_tile(k)) {
                glds_stage(gdY, Ai, NMA, Mo, m0, k);
                glds_stage(gX, Ai + A_EL, NMB, N, n0, k);
            } else {
                stage_load(k);
            }
        };
        if (k0 < kend) issue(k0, A0);
        for (int it = 0; it < niter; ++it, k0 += KG * BKW) {
            const bool active = k0 < kend;
            At = A0 + (it & 1) * SET_EL;
            Bt = At + A_EL;
            // step t has landed: its LDS-DMA, or its register loads
            __builtin_amdgcn_s_waitcnt(0x0F70);
            if (active && !full_tile(k0)) stage_write(k0);
            __syncthreads();  // the ONE barrier of the iteration

            const int kn = k0 + KG * BKW;
            wgrad_two_sets(
                At, A0 + ((it & 1) ^ 1) * SET_EL,
                [&](ushort* An) {
                    if (kn < kend) issue(kn, An);
                },
                [&](const ushort* Ai) {  // as above, on the current set
                    if (!active) return;
                    if (do_db) {
                        constexpr int NKQ = 256 / BMT;
                        constexpr int KPT = BKW / NKQ;
                        const int m = gtid % BMT, kq = gtid / BMT;
#pragma unroll
                        for (int j = 0; j < KPT; ++j) {
                            const ushort u = Ai[baddr(kq * KPT + j, m)];
                            db_part += bf2f(*(const __bf16*)&u);
                        }
                    }
                    if (fmv > 0 && fnv > 1)
                        mma_step(std::true_type{}, Ai, Ai + A_EL);
                    else if (fmv > 0 && fnv == 1)
                        mma_step(std::false_type{}, Ai, Ai + A_EL);
                });
        }
        __syncthreads();  // the reduction reuses the staging space
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
#endif  // WGRAD_TILE_HERE
