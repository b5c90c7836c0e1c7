// The text of the fused head backward kernel and of its launch (see
// head.hip), compiled once per loss, each loss in a translation unit of
// its own (head.hip: cross-entropy; head_mse.hip: squared error), which
// defines HEAD_BWD_KERNEL (the kernel's name), HEAD_BWD_LAUNCHER (the
// name of the arm's host launcher) and HEAD_BWD_MSE (0 / 1: which dz and
// which loss term step 2 computes).  Text, not a template parameter, so
// that the cross-entropy instantiations keep the very instructions they
// had with the code written in place, and a translation unit per loss so
// that neither set of instantiations is scheduled around the other's.
//
// Also here: the metric helpers that the kernel shares with
// head_metrics_kernel (head.hip) and the contract of the head launchers.

#include "head_dev.h"
#include "launchers.h"

#include <climits>
#include <cmath>

namespace {

constexpr float SS_FLT_MIN = 1.17549435e-38f;

__device__ __forceinline__ bool finite_f(float v) {
    return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
}

// -t * log(max(p, FLT_MIN)); a zero target contributes nothing, so a
// zero prob under it never makes 0 * log
__device__ __forceinline__ float xent_term(float p, float t) {
    return t == 0.f ? 0.f : -t * logf(fmaxf(p, SS_FLT_MIN));
}

// Sort key of a bf16 value in column c < 16: greater value first, then
// lower column, so a max over keys is argmax with the lowest index
// winning ties (-0 and +0 compare equal, as in a float compare).  Keys
// of real columns are > 0; 0 stands for "no column".
__device__ __forceinline__ unsigned argmax_key16(__bf16 v, int c) {
    unsigned u = bf_bits(v);
    if ((u & 0x7fffu) == 0) u = 0;
    u = (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
    return (u << 4) | (unsigned)(15 - c);
}

// The four totals of one block: the lanes that hold row results pass
// theirs in, the wave sums go through `part` (16 words of LDS), and
// after the caller's barrier head_metrics_commit adds them to the slot.
__device__ __forceinline__ void head_metrics_wave_sums(float loss, int correct,
                                                       int rows, int bad,
                                                       int* part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        loss += __shfl_xor(loss, off, 64);
        correct += __shfl_xor(correct, off, 64);
        rows += __shfl_xor(rows, off, 64);
        bad += __shfl_xor(bad, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        int* w = part + (threadIdx.x >> 6) * 4;
        w[0] = __float_as_int(loss);
        w[1] = correct;
        w[2] = rows;
        w[3] = bad;
    }
}

__device__ __forceinline__ void head_metrics_commit(const int* part,
                                                    int* metrics, int slots) {
    const int tid = threadIdx.x;
    if (tid >= 4) return;
    int* slot = metrics + (blockIdx.x & (slots - 1)) * 4;
    if (tid == 0) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += __int_as_float(part[w * 4]);
        atomicAdd((float*)slot, s);
    } else {
        int s = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += part[w * 4 + tid];
        atomicAdd(slot + tid, s);
    }
}

}  // namespace

// --------------------------------------------------------------- backward

// A block walks row tiles of RB rows (with gW the grid is <= 256, so at
// most 256 blocks add into any gradient element) and, for K > KC,
// column chunks of KC.  Per tile:
//   1. the x tile's global loads are issued (only when gW is wanted —
//      wgrad is the only reason this kernel reads x),
//   2. dz of the tile is computed, stored, and kept in LDS as bf16
//      (MFMA A operand, class index = k slot, k >= C zero) and as f32,
//   3. one MFMA per 16x16 dx fragment (B operand: W^T rows, staged once
//      per chunk), the tile goes through LDS and out as 16-B
//      row-contiguous stores,
//   4. the x tile replaces the dx tile in LDS; thread k sums
//      dz[r][c]·x[r][k] over the tile's rows into registers.
// The register sums are added to gW once per block and chunk, row-
// contiguously (a wave instruction covers 64 consecutive floats of one
// gW row).
//
// METRICS: step 2 of the first chunk already holds probs[r][c] and
// target[r][c] of a row in 16 adjacent lanes, so the row's loss term,
// argmax match and finiteness are a 4-step xor reduction there.  The
// lane of column 0 keeps the totals of its rows in registers over all
// tiles of the block; after the first chunk's tile loop the wave sums
// go to LDS, the barrier that ends every chunk carries them, and four
// threads add them to the block's slot.  Later chunks recompute dz and
// must not count again.
//
// HEAD_BWD_MSE: dz of step 2 is the softmax-MSE one, s·(g − Σ_c s·g)
// with g = −2(t − s)/GB (head_mse_dz_elem, head_dev.h).  The row sum is
// taken over the 16 lanes that hold the row, so every lane of a wave
// reaches it: the c < C, row < M guard stands around the loads and the
// store only, and the guarded-out lanes add +0.  RB·16 is a multiple of
// the 256 threads, so every trip of the e loop is entered by whole
// waves.  The loss term of the METRICS instantiations is (t − p)², what
// head_metrics_kernel<true> sums.  Everything from dzs / dzf on is the
// same text for both losses.
template <int RB, int KC, int C4, bool METRICS>
__global__ __launch_bounds__(256) void HEAD_BWD_KERNEL(
    const __bf16* __restrict__ probs,   // [M][C]
    const __bf16* __restrict__ target,  // [M][C]
    const __bf16* __restrict__ x,       // [M][K]
    const __bf16* __restrict__ Wt,      // [K][C]
    __bf16* __restrict__ dz,            // [M][C]
    __bf16* __restrict__ dx,            // [M][K]
    float* __restrict__ gW,             // [C][K] (atomicAdd +=) or null
    float* __restrict__ gb,             // [C]    (atomicAdd +=) or null
    int* __restrict__ metrics,          // [slots][4] (atomicAdd +=) or null
    int slots,                          // power of two
    int M, int K, int C, float inv_gb, int ntiles) {
    constexpr int LDT = KC + 8;              // padded tile row (bf16)
    constexpr int PPR = KC / 8;              // 16-B pieces per tile row
    constexpr int NP = RB * PPR / 256;       // pieces per thread
    constexpr int NRG = RB / 16;             // 16-row groups per tile
    static_assert(RB * PPR % 256 == 0, "piece mapping");

    __shared__ __attribute__((aligned(16))) ushort tile[RB][LDT];
    __shared__ __attribute__((aligned(16))) ushort wts[KC][16];
    __shared__ __attribute__((aligned(16))) ushort dzs[RB][16];
    __shared__ __attribute__((aligned(16))) float dzf[RB][16];
    __shared__ int mpart[METRICS ? 16 : 1];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lrow = lane & 15;
    const int kch = lane >> 4;
    const bool wg = gW != nullptr;  // block-uniform

    float gbacc = 0.f;
    float m_loss = 0.f;
    int m_correct = 0, m_rows = 0, m_bad = 0;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);  // multiple of 32
        const bool first = k0 == 0;

        // W^T rows of this chunk, zero-padded to 16 classes
        HEAD_STAGE_WT(KC, wts, Wt, k0, kc, C, tid)

        float gw[C4 * 4];
#pragma unroll
        for (int c = 0; c < C4 * 4; ++c) gw[c] = 0.f;

        for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
            const int row0 = t * RB;

            // 1. x tile -> registers (rows past M and columns past the
            //    chunk as zeros)
            bf16x8 xr[NP];
            if (wg) {
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const int q = tid + i * 256;
                    const int r = q / PPR, col = (q % PPR) * 8;
                    xr[i] = zero8();
                    if (row0 + r < M && col < kc)
                        xr[i] = *(const bf16x8*)&x[(long)(row0 + r) * K + k0 +
                                                    col];
                }
            }

            // 2. dz of the tile
            for (int e = tid; e < RB * 16; e += 256) {
                const int r = e >> 4, c = e & 15;
                float d = 0.f;
                ushort bits = 0;
                float term = 0.f;
                unsigned pkey = 0, tkey = 0;
                bool bad = false;
#if HEAD_BWD_MSE
                static_assert(RB * 16 % 256 == 0, "whole waves per trip");
                const bool live = c < C && row0 + r < M;
                const long gi = (long)(row0 + r) * C + c;
                __bf16 pb = (__bf16)0.f, tb = (__bf16)0.f;
                if (live) {
                    pb = probs[gi];
                    tb = target[gi];
                }
                // every lane: the row sum is a cross-lane step
                const __bf16 o = head_mse_dz_elem(pb, tb, inv_gb);
                if (live) {
                    if (first) dz[gi] = o;
                    d = bf2f(o);
                    bits = bf_bits(o);
                    if (METRICS && first) {
                        bad = !finite_f(bf2f(pb));
                        const float df = bf2f(tb) - bf2f(pb);
                        term = df * df;
                        pkey = argmax_key16(pb, c);
                        tkey = argmax_key16(tb, c);
                    }
                }
#else
                if (c < C && row0 + r < M) {
                    const long gi = (long)(row0 + r) * C + c;
                    const __bf16 pb = probs[gi], tb = target[gi];
                    const __bf16 o = head_dz_elem(pb, tb, inv_gb);
                    if (first) dz[gi] = o;
                    d = bf2f(o);
                    bits = bf_bits(o);
                    if (METRICS && first) {
                        bad = !finite_f(bf2f(pb));
                        term = xent_term(bf2f(pb), bf2f(tb));
                        pkey = argmax_key16(pb, c);
                        tkey = argmax_key16(tb, c);
                    }
                }
#endif
                dzs[r][c] = bits;
                dzf[r][c] = d;
                if (METRICS && first) {  // block-uniform
                    // the row's 16 lanes: e & 15 == lane & 15
                    const bool rowbad =
                        ((__ballot(bad) >> (lane & 48)) & 0xffffull) != 0;
#pragma unroll
                    for (int off = 8; off > 0; off >>= 1) {
                        term += __shfl_xor(term, off, 64);
                        pkey = max(pkey, (unsigned)__shfl_xor((int)pkey, off,
                                                              64));
                        tkey = max(tkey, (unsigned)__shfl_xor((int)tkey, off,
                                                              64));
                    }
                    if (c == 0 && row0 + r < M) {
                        m_rows += 1;
                        if (rowbad) {
                            m_bad += 1;
                        } else {
                            m_loss += term;
                            m_correct += (pkey & 15u) == (tkey & 15u);
                        }
                    }
                }
            }
            __syncthreads();

            // 3. dx fragments: acc starts at zero, ONE MFMA, k slot =
            //    class index (lanes kch >= 2 hold k >= 16: zeros)
            const int nfrag = NRG * (kc / 16);
            for (int idx = wave; idx < nfrag; idx += 4) {
                const int rg = idx % NRG, ct = idx / NRG;
                HEAD_DX_FRAG(acc, dzs, wts, rg, ct, lrow, kch);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    tile[rg * 16 + kch * 4 + r][ct * 16 + lrow] =
                        bf_bits(f2bf(acc[r]));
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int q = tid + i * 256;
                const int r = q / PPR, col = (q % PPR) * 8;
                if (row0 + r < M && col < kc)
                    *(bf16x8*)&dx[(long)(row0 + r) * K + k0 + col] =
                        *(const bf16x8*)&tile[r][col];
            }

            // 4. weight and bias gradient of the tile
            if (wg) {
                __syncthreads();
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const int q = tid + i * 256;
                    *(bf16x8*)&tile[q / PPR][(q % PPR) * 8] = xr[i];
                }
                __syncthreads();
                if (tid < kc) {
#pragma unroll 4
                    for (int r = 0; r < RB; ++r) {
                        const ushort u = tile[r][tid];
                        const float xv = bf2f(*(const __bf16*)&u);
#pragma unroll
                        for (int g = 0; g < C4; ++g) {
                            const float4 d = *(const float4*)&dzf[r][g * 4];
                            gw[g * 4 + 0] += d.x * xv;
                            gw[g * 4 + 1] += d.y * xv;
                            gw[g * 4 + 2] += d.z * xv;
                            gw[g * 4 + 3] += d.w * xv;
                        }
                    }
                }
                if (first && gb != nullptr && tid < 16) {
                    float s = 0.f;
                    for (int r = 0; r < RB; ++r) s += dzf[r][tid];
                    gbacc += s;
                }
            }
            __syncthreads();  // LDS is rewritten by the next tile
        }

        // ONE set of atomics per block and chunk
        if (wg && tid < kc) {
#pragma unroll
            for (int c = 0; c < C4 * 4; ++c)
                if (c < C) atomicAdd(&gW[(long)c * K + k0 + tid], gw[c]);
        }
        if (METRICS && first)
            head_metrics_wave_sums(m_loss, m_correct, m_rows, m_bad, mpart);
        __syncthreads();  // wts is rewritten by the next chunk
        if (METRICS && first) head_metrics_commit(mpart, metrics, slots);
    }
    if (wg && gb != nullptr && tid < C) atomicAdd(&gb[tid], gbacc);
}

// ---------------------------------------------------------------- launchers

namespace {

bool head_contract(int M, int K, int C) {
    return M >= 1 && C >= 1 && C <= 16 && K >= 32 && K % 32 == 0 && K <= 1024;
}

bool slots_ok(int slots) { return slots >= 1 && (slots & (slots - 1)) == 0; }

// most blocks that may add into one gradient element: one per CU
constexpr int HEAD_BWD_MAX_BLOCKS = 256;

template <int RB, int KC>
void head_bwd_launch(const void* probs, const void* target, const void* x,
                     const void* Wt, void* dz, void* dx, void* gW, void* gb,
                     void* metrics, int slots, int M, int K, int C,
                     float inv_gb, hipStream_t st) {
    const int ntiles = cdiv(M, RB);
    // the cap only matters where blocks add into gW / gb
    const dim3 grid(gW == nullptr || ntiles < HEAD_BWD_MAX_BLOCKS
                        ? ntiles
                        : HEAD_BWD_MAX_BLOCKS);
#define HEAD_BWD_K(C4V, MV)                                                  \
    hipLaunchKernelGGL((HEAD_BWD_KERNEL<RB, KC, C4V, MV>), grid,             \
                       dim3(256), 0, st, (const __bf16*)probs,               \
                       (const __bf16*)target, (const __bf16*)x,              \
                       (const __bf16*)Wt, (__bf16*)dz, (__bf16*)dx,          \
                       (float*)gW, (float*)gb, (int*)metrics, slots, M, K,   \
                       C, inv_gb, ntiles)
#define HEAD_BWD_C4(C4V)                                                     \
    do {                                                                     \
        if (metrics) HEAD_BWD_K(C4V, true);                                  \
        else HEAD_BWD_K(C4V, false);                                         \
    } while (0)
    switch ((C + 3) / 4) {
        case 1: HEAD_BWD_C4(1); break;
        case 2: HEAD_BWD_C4(2); break;
        case 3: HEAD_BWD_C4(3); break;
        default: HEAD_BWD_C4(4); break;
    }
#undef HEAD_BWD_C4
#undef HEAD_BWD_K
}

}  // namespace

// This loss's arm of ss_head_bwd_fused (launchers.h), which selects it.
bool HEAD_BWD_LAUNCHER(const void* probs, const void* target, const void* x,
                       const void* Wt, void* dz, void* dx, void* gW, void* gb,
                       int M, int K, int C, float inv_gb, int rows_per_block,
                       void* metrics, int slots, hipStream_t st) {
    if (!head_contract(M, K, C)) return false;
    if (metrics && !slots_ok(slots)) return false;
    // without gW the grid is not capped: 32-row tiles put two blocks on
    // a CU, whose load / MFMA / store phases then overlap
    // SS_HEAD_BWD_ROWS (read once) overrides the choice for tuning.
    static const int env_rows = env_int("SS_HEAD_BWD_ROWS", 0);
    if (!rows_per_block) rows_per_block = env_rows;
    const int rb = rows_per_block ? rows_per_block : (gW ? 64 : 32);
    // the 128-row arm halves the column chunk to stay inside 64 KB of LDS
    if (rb == 32)
        head_bwd_launch<32, 256>(probs, target, x, Wt, dz, dx, gW, gb, metrics,
                                 slots, M, K, C, inv_gb, st);
    else if (rb == 64)
        head_bwd_launch<64, 256>(probs, target, x, Wt, dz, dx, gW, gb, metrics,
                                 slots, M, K, C, inv_gb, st);
    else if (rb == 128)
        head_bwd_launch<128, 128>(probs, target, x, Wt, dz, dx, gW, gb, metrics,
                                  slots, M, K, C, inv_gb, st);
    else
        return false;
    return true;
}
