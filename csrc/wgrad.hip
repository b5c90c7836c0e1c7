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
//
// The tile body (staging loop, MFMAs, reduction, atomics) is the text
// of wgrad_dev.h.  NSTAGE = 2 gives it two LDS staging sets, so the
// loads of K-step t+1 run under the MFMAs of step t.

#include "common.h"
#include "launchers.h"
#include "wgrad_dev.h"

// What a block of wgrad_tn_kernel works on (wgrad_dev.h expands this
// after the wave ids).
// XCD-aware block remap (T1, bijective variant): the dispatcher places
// hw block b on XCD b%8; remap so each XCD owns a CONTIGUOUS run of work
// ids decoded n-tile-fastest — blocks that share a dY m-slice then read
// it from ONE XCD's L2 instead of filling all eight.
// Pointers read from the chunk table lose their address space and would
// compile to FLAT loads, which count on lgkmcnt as well: the LDS waits
// ahead of the MFMAs would then also wait for the prefetch.  Name the
// global address space explicitly.
#define WGRAD_DECODE                                                        \
    const int gx = gridDim.x, gy = gridDim.y;                               \
    const int nwg = gx * gy * gridDim.z;                                    \
    const int hw = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);        \
    const int wid = xcd_remap(hw, nwg);                                     \
    const int bidy = wid % gy;                                              \
    const int bidx = (wid / gy) % gx;                                       \
    int bidz = wid / (gy * gx);                                             \
    if (chunks) {                                                           \
        const long* row = chunks + (long)(bidz / nsplit) * 3;               \
        dY = (const __bf16*)row[0];                                         \
        X = (const __bf16*)row[1];                                          \
        mask = (const __bf16*)row[2];                                       \
        bidz = bidz % nsplit;                                               \
    }                                                                       \
    const gbf16* const gdY = (const gbf16*)dY;                              \
    const gbf16* const gX = (const gbf16*)X;                                \
    const gbf16* const gmask = (const gbf16*)mask;                          \
    const int m0 = bidx * BMT;                                              \
    const int n0 = bidy * BNT;                                              \
    const int kbeg = bidz * k_per_split;                                    \
    const int kend = min(Kb, kbeg + k_per_split);
#define WGRAD_DB_OWNER bidy == 0

// Second launch bound = waves per SIMD the register allocation must
// leave room for: accumulators + the prefetch set + fragments stay
// inside the two-wave budget at 128-wide tiles, four waves at 64x64.
template <int BMT, int BNT, bool HAS_MASK, int KG, int NSTAGE>
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
    // ALL LDS is this one array (a second LDS object beside a glds
    // staging array can cost a vmcnt(0) per K-step).
    __shared__ __attribute__((aligned(16)))
    ushort smem[NSTAGE * wgrad_set_el<BMT, BNT, KG>()];
#define WGRAD_TILE_HERE
#include "wgrad_dev.h"
}
#undef WGRAD_DECODE
#undef WGRAD_DB_OWNER

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

// Staging depth of a launch: the caller's (1 or 2), else SS_WGRAD_STAGES
// (read once), else two sets where they measured faster: unmasked
// launches with K-groups whose grid has full tiles, which stage by glds
// (16384 x 256 x 784: 28.7 -> 25.5 µs, x 256 x 256: 14.5 -> 12.2 µs, the
// best split unchanged at 16; profiles/r13_wgrad_group.md).  The head
// (10 x 256, register-staged remainder tiles only) measured the same
// either way and keeps one set, as do masked launches and the
// single-owner path, which were not measured.
int wgrad_stages(const WgradCfg& cfg, int Mo, int N, bool has_mask,
                 int stages) {
    if (stages == 1 || stages == 2) return stages;
    static const int env_stages = env_int("SS_WGRAD_STAGES", 0);
    if (env_stages == 1 || env_stages == 2) return env_stages;
    return !has_mask && cfg.kg > 1 && Mo >= cfg.bm && N >= cfg.bn ? 2 : 1;
}

}  // namespace

#define WGRAD_LAUNCH(BMT, BNT, HM, KGV, ...)                                \
    do {                                                                    \
        if (stages == 2)                                                    \
            hipLaunchKernelGGL((wgrad_tn_kernel<BMT, BNT, HM, KGV, 2>),     \
                               grid, dim3(KGV * 256), 0, stream,            \
                               __VA_ARGS__);                                \
        else                                                                \
            hipLaunchKernelGGL((wgrad_tn_kernel<BMT, BNT, HM, KGV, 1>),     \
                               grid, dim3(KGV * 256), 0, stream,            \
                               __VA_ARGS__);                                \
    } while (0)
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
                 void* gb, int Mo, int N, int Kb, int split_k, int stages,
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
    stages = wgrad_stages(cfg, Mo, N, has_mask, stages);
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
    const int stages = 1;  // the deferred-µbatch path keeps one set
    WGRAD_DISPATCH(cfg, (const __bf16*)nullptr, (const __bf16*)nullptr,
                   (const __bf16*)nullptr, (float*)gW, (float*)gb, Mo, N,
                   Kb_chunk, k_per_split, (const long*)chunk_table, split_k);
}
