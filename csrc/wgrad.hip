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

#include <climits>
#include <vector>

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

// ------------------------------------------------------ grouped launch
//
// wgrad_group_kernel: up to SS_WGRAD_GROUP_MAX independent unmasked
// problems of ONE tile configuration in one launch, side by side.  Each
// problem owns a contiguous run of work ids (n-tile fastest, then
// m-tile, then K-slice, as in wgrad_tn_kernel), so after xcd_remap over
// the whole grid a K-slice's tiles still sit on one XCD.  The problems
// arrive BY VALUE in the kernel argument (no device table, nothing to
// upload, legal under graph capture), the way the backward chain takes
// its layers.
struct WgradGroupItem {
    const __bf16* dY;  // [Kb][Mo]
    const __bf16* X;   // [Kb][N]
    float* gW;         // [Mo][N] (atomicAdd +=)
    float* gb;         // [Mo] or null
    int Mo, N, Kb, k_per_split;
    int gx, gy;        // m-tiles, n-tiles
    int first;         // first work id; INT_MAX in unused slots
};
struct WgradGroupArgs {
    WgradGroupItem p[SS_WGRAD_GROUP_MAX];
};

using gf32 = __attribute__((address_space(1))) float;

// The block's problem is the last one whose first work id is <= wid.
// It is picked by a compare-and-select chain over CONSTANT indices: a
// dynamic index into the by-value array makes hipcc copy the whole
// block to scratch.  Everything here is block-uniform (scalar loads and
// selects).  The pointers go through the global address space for the
// reason given above wgrad_tn_kernel's decode; gW / gb come back as
// plain pointers for atomicAdd and keep the inferred address space.
#define WGRAD_DECODE                                                        \
    const int wid = xcd_remap((int)blockIdx.x, (int)gridDim.x);             \
    const gbf16* gdY = (const gbf16*)args.p[0].dY;                          \
    const gbf16* gX = (const gbf16*)args.p[0].X;                            \
    gf32* sgW = (gf32*)args.p[0].gW;                                        \
    gf32* sgb = (gf32*)args.p[0].gb;                                        \
    int Mo = args.p[0].Mo, N = args.p[0].N, Kb = args.p[0].Kb;              \
    int k_per_split = args.p[0].k_per_split;                                \
    int gx = args.p[0].gx, gy = args.p[0].gy, first = 0;                    \
    _Pragma("unroll") for (int i = 1; i < SS_WGRAD_GROUP_MAX; ++i) {        \
        const bool t = wid >= args.p[i].first;                              \
        gdY = t ? (const gbf16*)args.p[i].dY : gdY;                         \
        gX = t ? (const gbf16*)args.p[i].X : gX;                            \
        sgW = t ? (gf32*)args.p[i].gW : sgW;                                \
        sgb = t ? (gf32*)args.p[i].gb : sgb;                                \
        Mo = t ? args.p[i].Mo : Mo;                                         \
        N = t ? args.p[i].N : N;                                            \
        Kb = t ? args.p[i].Kb : Kb;                                         \
        k_per_split = t ? args.p[i].k_per_split : k_per_split;              \
        gx = t ? args.p[i].gx : gx;                                         \
        gy = t ? args.p[i].gy : gy;                                         \
        first = t ? args.p[i].first : first;                                \
    }                                                                       \
    float* const gW = (float*)sgW;                                          \
    float* const gb = (float*)sgb;                                          \
    const gbf16* const gmask = nullptr;                                     \
    const int lid = wid - first;                                            \
    const int bidy = lid % gy;                                              \
    const int bidx = (lid / gy) % gx;                                       \
    const int bidz = lid / (gy * gx);                                       \
    const int m0 = bidx * BMT;                                              \
    const int n0 = bidy * BNT;                                              \
    const int kbeg = bidz * k_per_split;                                    \
    const int kend = min(Kb, kbeg + k_per_split);
#define WGRAD_DB_OWNER bidy == 0

template <int BMT, int BNT, int KG, int NSTAGE>
__global__ __launch_bounds__(KG * 256, BMT* BNT > 64 * 64 ? 2 : 4)
void wgrad_group_kernel(const WgradGroupArgs args) {
    constexpr bool HAS_MASK = false;
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
int wgrad_target_blocks() {
    static const int env_blocks = env_int("SS_WGRAD_BLOCKS", 0);
    return env_blocks > 0 ? env_blocks : WGRAD_TARGET_BLOCKS;
}

int wgrad_auto_split(int tiles, int Kb, int kg) {
    const int target = wgrad_target_blocks();
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

// Shapes the widest tier (wgrad256.hip) is tried for first: unmasked,
// auto split, >= 64 output tiles of 256 x 256.  SS_WGRAD256=0 (read
// once) disables it.
bool wgrad_tier256(int Mo, int N, int split_k) {
    static const int en = env_int("SS_WGRAD256", 1);
    return en && split_k <= 0 && Mo >= 512 && N >= 512 &&
           (long)(Mo / 256) * (N / 256) >= 64;
}

// Configurations wgrad_group_kernel is built for: the shipped two-set
// forms with K-groups.
bool wgrad_groupable(const WgradCfg& c) {
    return (c.bm == 64 && c.bn == 64 && c.kg == 4) ||
           (c.bn == 128 && c.kg == 2);
}

// The split a launch really runs: K-slices are whole 64-row steps.
int wgrad_eff_split(int Kb, int split_k) {
    return cdiv(Kb, cdiv(cdiv(Kb, split_k), 64) * 64);
}

// Splits of the problems of ONE grouped launch.  split[i] comes in as
// the caller's value (0 = auto) and goes out as the split to run;
// tiles[i] are the problem's output tiles.
//
// A block of the two-set kernels holds 96-128 KB of LDS, one block per
// CU, so the launch is ONE wave only up to the target of 256 blocks and
// a block past it runs alone after the wave: at the flagship (head
// 10x256 + two 256x256, Kb 16384) 256 blocks take 21.9 us, 264 take
// 39.7 us, and the three launches back to back 32.5 us
// (profiles/r15_wgrad_concurrent.md).  The rule, for the auto problems:
//   1. every problem starts at wgrad_auto_split of an equal share of
//      the CUs, i.e. of tiles * n: for a group of one that IS
//      wgrad_auto_split (flagship: hidden 4, head 16; 192 blocks);
//   2. the blocks left under the target go, one split step at a time,
//      to the problem whose blocks have the longest K range (first in
//      the list on a tie), while the launch still fits (flagship:
//      hidden 4 -> 6, 256 blocks: the sweep's best cell).
// Explicit splits are kept and count against the target.
void wgrad_group_splits(int n, const int* tiles, const int* Kb, int kg,
                        int* split) {
    const int target = wgrad_target_blocks();
    bool autos[SS_WGRAD_GROUP_MAX];
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        autos[i] = split[i] == 0;
        if (autos[i]) split[i] = wgrad_auto_split(tiles[i] * n, Kb[i], kg);
        split[i] = wgrad_eff_split(Kb[i], split[i]);
        blocks += tiles[i] * split[i];
    }
    if (n < 2) return;
    for (;;) {
        int best = -1, best_s = 0;
        for (int i = 0; i < n; ++i) {
            if (!autos[i]) continue;
            // the next split that changes the grid, within a K-step per
            // group
            const int max_split = cdiv(Kb[i], 64 * kg);
            int s = split[i] + 1;
            while (s <= max_split && wgrad_eff_split(Kb[i], s) == split[i])
                ++s;
            if (s > max_split) continue;
            s = wgrad_eff_split(Kb[i], s);
            if (blocks + tiles[i] * (s - split[i]) > target) continue;
            if (best < 0 || cdiv(Kb[i], split[i]) >
                                cdiv(Kb[best], split[best])) {
                best = i;
                best_s = s;
            }
        }
        if (best < 0) return;
        blocks += tiles[best] * (best_s - split[best]);
        split[best] = best_s;
    }
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
    if (!mask && wgrad_tier256(Mo, N, split_k)) {
        if (ss_wgrad_tn_256(dY, X, gW, Mo, N, Kb, stream)) {
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

// ------------------------------------------------------ grouped launch

int ss_wgrad_group_plan(const WgradProblem* p, int n, const int* splits,
                        WgradGroupLaunch* out) {
    if (n < 0 || (n > 0 && (!p || !out))) return -1;
    for (int i = 0; i < n; ++i) {
        if (p[i].Mo < 1 || p[i].N < 1 || p[i].Kb < 1) return -1;
        if (splits && (splits[i] < 0 || splits[i] == 1)) return -1;
    }
    auto split_of = [&](int i) { return splits ? splits[i] : 0; };
    auto cfg_of = [&](int i) {
        return wgrad_cfg(p[i].Mo, p[i].N, split_of(i));
    };
    auto can_group = [&](int i) {
        return wgrad_groupable(cfg_of(i)) &&
               !wgrad_tier256(p[i].Mo, p[i].N, split_of(i));
    };
    int nl = 0;
    for (int i = 0; i < n;) {
        const WgradCfg cfg = cfg_of(i);
        int j = i + 1;
        if (can_group(i)) {
            for (; j < n && j - i < SS_WGRAD_GROUP_MAX && can_group(j); ++j) {
                const WgradCfg c = cfg_of(j);
                if (c.bm != cfg.bm || c.bn != cfg.bn || c.kg != cfg.kg) break;
            }
        }
        WgradGroupLaunch& L = out[nl++];
        L = WgradGroupLaunch{};
        L.first = i;
        L.count = j - i;
        auto tiles_of = [&](int k) {
            return cdiv(p[k].Mo, cfg.bm) * cdiv(p[k].N, cfg.bn);
        };
        if (L.count == 1 && wgrad_tier256(p[i].Mo, p[i].N, split_of(i))) {
            i = j;  // the 256-tile tier sizes its own grid: 0, 0
            continue;
        }
        int tiles[SS_WGRAD_GROUP_MAX], kb[SS_WGRAD_GROUP_MAX];
        for (int k = i; k < j; ++k) {
            tiles[k - i] = tiles_of(k);
            kb[k - i] = p[k].Kb;
            L.split[k - i] = split_of(k);
        }
        wgrad_group_splits(L.count, tiles, kb, cfg.kg, L.split);
        for (int k = i; k < j; ++k)
            L.blocks[k - i] = tiles[k - i] * L.split[k - i];
        i = j;
    }
    return nl;
}

bool ss_wgrad_tn_group(const WgradProblem* p, int n, const int* splits,
                       hipStream_t stream) {
    if (n == 0) return true;
    // every check first: a refused call launches nothing
    std::vector<WgradGroupLaunch> plan(n > 0 ? n : 0);
    const int nl = ss_wgrad_group_plan(p, n, splits, plan.data());
    if (nl < 0) return false;
    for (int i = 0; i < n; ++i)
        if (!aligned16(p[i].dY) || !aligned16(p[i].X) || !p[i].gW ||
            ((uintptr_t)p[i].gW & 3) || ((uintptr_t)p[i].gb & 3))
            return false;
    for (int l = 0; l < nl; ++l) {
        const WgradGroupLaunch& L = plan[l];
        const WgradProblem* q = p + L.first;
        if (L.count == 1) {
            ss_wgrad_tn(q->dY, q->X, nullptr, q->gW, q->gb, q->Mo, q->N,
                        q->Kb, splits ? splits[L.first] : 0, 0, stream);
            continue;
        }
        const WgradCfg cfg = wgrad_cfg(q->Mo, q->N, 0);
        WgradGroupArgs args;
        int nblocks = 0;
        for (int k = 0; k < SS_WGRAD_GROUP_MAX; ++k) {
            WgradGroupItem& it = args.p[k];
            it = WgradGroupItem{};
            it.first = INT_MAX;
            if (k >= L.count) continue;
            it.dY = (const __bf16*)q[k].dY;
            it.X = (const __bf16*)q[k].X;
            it.gW = (float*)q[k].gW;
            it.gb = (float*)q[k].gb;
            it.Mo = q[k].Mo;
            it.N = q[k].N;
            it.Kb = q[k].Kb;
            it.k_per_split = cdiv(cdiv(q[k].Kb, L.split[k]), 64) * 64;
            it.gx = cdiv(q[k].Mo, cfg.bm);
            it.gy = cdiv(q[k].N, cfg.bn);
            it.first = nblocks;
            nblocks += L.blocks[k];
        }
        const dim3 grid(nblocks);
        if (cfg.bm == 128)
            hipLaunchKernelGGL((wgrad_group_kernel<128, 128, 2, 2>), grid,
                               dim3(2 * 256), 0, stream, args);
        else if (cfg.bn == 128)
            hipLaunchKernelGGL((wgrad_group_kernel<64, 128, 2, 2>), grid,
                               dim3(2 * 256), 0, stream, args);
        else
            hipLaunchKernelGGL((wgrad_group_kernel<64, 64, 4, 2>), grid,
                               dim3(4 * 256), 0, stream, args);
    }
    return true;
}
