// Fused classifier head (gfx950 / MI355X): the last Linear (C <= 16
// classes) together with the softmax-cross-entropy head, as ONE forward
// and ONE backward kernel.
//
//   head_fwd_fused: probs = softmax(bf16(x · W^T + b))
//   head_bwd_fused: dz = bf16((probs − target)/GB)
//                   dx = bf16(dz · W)                 (B operand: W^T copy)
//                   gW += dz^T · x ; gb += colsum(dz)  (optional, f32)
//
// Replaces gemm_nt → softmax_fwd and head_xent_bwd → gemm_nt(dz, Wt) →
// wgrad_tn for this shape class.  Those kernels run far below any
// hardware limit here (a 64-wide N tile for 10 columns, one wave per
// softmax row with 10 live lanes, the logits and dz round-tripping
// through memory between launches).
//
// probs, dz and dx are BIT-IDENTICAL to the unfused chain: the same
// v_mfma_f32_16x16x32_bf16 with the same operand slots and K-step
// order, the same bf16 rounding points (logits are rounded to bf16 and
// widened again before the softmax), the same __expf / multiply, and
// the same xor tree over the 16 lanes that hold one row (the unfused
// tree's offsets 32 and 16 only add zeros for C <= 16).  gW / gb differ
// from wgrad_tn only in f32 summation order.
//
// Launch contract (both kernels): C <= 16, K % 32 == 0, K <= 1024,
// M >= 1.  The launchers return false outside it.
//
// Training metrics.  head_bwd_fused can also add the batch's loss sum,
// argmax matches, row count and non-finite-row count into a slotted
// accumulator (METRICS instantiations), and head_metrics_kernel does the
// same for any (M, C) probs / target pair, cross-entropy or squared
// error.  The accumulator is [S][4] 32-bit words, S a power of two:
// word 0 f32 loss_sum, words 1..3 int32 correct, rows, nonfinite.  A
// block adds its totals ONCE, into slot blockIdx.x % S, so that the
// same-address atomics of a launch spread over S addresses; the host
// folds the slots.  A row with a NaN or Inf prob counts in rows and
// nonfinite only.

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

// ---------------------------------------------------------------- forward

// One 16-column fragment per wave: wave w of a block owns FR fragments
// of 16 rows.  The MFMA A operand of row r, K-step t is 16 contiguous
// bytes of x per lane, so x goes global -> registers with 16-B loads
// and no LDS; W (C x K, <= 32 KB, L2-resident) is read the same way as
// the B operand, rows c >= C as zeros.  Up to 8 K-steps of loads are in
// flight per wave before the first MFMA, and the next group is issued
// ahead of the current group's MFMAs.  There is no barrier.
template <int WAVES, int FR>
__global__ __launch_bounds__(WAVES * 64) void head_fwd_fused_kernel(
    const __bf16* __restrict__ x,     // [M][K]
    const __bf16* __restrict__ W,     // [C][K]
    const __bf16* __restrict__ bias,  // [C]
    __bf16* __restrict__ probs,       // [M][C]
    int M, int K, int C) {
    constexpr int U = 8 / FR;  // K-steps per load group

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lrow = lane & 15;
    const int kch = lane >> 4;
    const int row_base = (blockIdx.x * WAVES + wave) * (16 * FR);
    if (row_base >= M) return;  // wave-uniform

    const bool cvalid = lrow < C;
    const __bf16* xp[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f)
        xp[f] = x + (long)min(row_base + f * 16 + lrow, M - 1) * K + kch * 8;
    const __bf16* wp = W + (long)min(lrow, C - 1) * K + kch * 8;

    const int nsteps = K / 32;
    bf16x8 a[FR][U], b[U], an[FR][U], bn[U];
    auto load = [&](bf16x8(&aa)[FR][U], bf16x8(&bb)[U], int t0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u < nsteps) {
#pragma unroll
                for (int f = 0; f < FR; ++f)
                    aa[f][u] = *(const bf16x8*)(xp[f] + (t0 + u) * 32);
                bb[u] = *(const bf16x8*)(wp + (t0 + u) * 32);
            }
        }
    };

    f32x4 acc[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) acc[f] = {0.f, 0.f, 0.f, 0.f};

    load(a, b, 0);
    for (int t0 = 0; t0 < nsteps; t0 += U) {
        const bool more = t0 + U < nsteps;
        if (more) load(an, bn, t0 + U);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u < nsteps) {
                const bf16x8 bv = cvalid ? b[u] : zero8();
#pragma unroll
                for (int f = 0; f < FR; ++f)
                    acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a[f][u], bv, acc[f], 0, 0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int f = 0; f < FR; ++f) a[f][u] = an[f][u];
                b[u] = bn[u];
            }
        }
    }

    // ---- epilogue in registers: lane (kch, lrow) holds rows
    // kch*4 + r of column lrow; the 16 lanes of one kch hold one row
    // (head_dev.h: the forward chain kernel runs the same code)
    HEAD_FWD_EPILOGUE(FR, acc, bias, probs, cvalid, lrow, kch, row_base, M, C)
}

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
template <int RB, int KC, int C4, bool METRICS>
__global__ __launch_bounds__(256) void head_bwd_fused_kernel(
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

// ---------------------------------------------------------------- metrics

// The metric totals of any (M, C) probs / target pair: one wave per row,
// four rows per block and pass, lanes strided over the columns like
// row_argmax_kernel, rows walked grid-stride.  MSE selects the squared
// error as the row loss, otherwise cross-entropy.  One atomic set per
// block, into slot blockIdx.x % slots.
template <bool MSE>
__global__ __launch_bounds__(256) void head_metrics_kernel(
    const __bf16* __restrict__ probs,   // [M][C]
    const __bf16* __restrict__ target,  // [M][C]
    int* __restrict__ metrics,          // [slots][4] (atomicAdd +=)
    int slots, int M, int C) {
    __shared__ int mpart[16];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    float m_loss = 0.f;
    int m_correct = 0, m_rows = 0, m_bad = 0;
    for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
        const __bf16* pr = probs + (long)row * C;
        const __bf16* tr = target + (long)row * C;
        float term = 0.f;
        float pbest = -INFINITY, tbest = -INFINITY;
        int pi = INT_MAX, ti = INT_MAX;
        bool bad = false;
        for (int c = lane; c < C; c += 64) {
            const float p = bf2f(pr[c]), t = bf2f(tr[c]);
            bad |= !finite_f(p);
            if (MSE) term += (t - p) * (t - p);
            else term += xent_term(p, t);
            if (p > pbest || pi == INT_MAX) {
                pbest = p;
                pi = c;
            }
            if (t > tbest || ti == INT_MAX) {
                tbest = t;
                ti = c;
            }
        }
        const bool rowbad = __ballot(bad) != 0;  // row is wave-uniform
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            term += __shfl_xor(term, off, 64);
            const float pv = __shfl_xor(pbest, off, 64);
            const int pj = __shfl_xor(pi, off, 64);
            if (pj != INT_MAX &&
                (pi == INT_MAX || pv > pbest || (pv == pbest && pj < pi))) {
                pbest = pv;
                pi = pj;
            }
            const float tv = __shfl_xor(tbest, off, 64);
            const int tj = __shfl_xor(ti, off, 64);
            if (tj != INT_MAX &&
                (ti == INT_MAX || tv > tbest || (tv == tbest && tj < ti))) {
                tbest = tv;
                ti = tj;
            }
        }
        if (lane == 0) {
            m_rows += 1;
            if (rowbad) {
                m_bad += 1;
            } else {
                m_loss += term;
                m_correct += pi == ti;
            }
        }
    }
    head_metrics_wave_sums(m_loss, m_correct, m_rows, m_bad, mpart);
    __syncthreads();
    head_metrics_commit(mpart, metrics, slots);
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
    hipLaunchKernelGGL((head_bwd_fused_kernel<RB, KC, C4V, MV>), grid,       \
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

// rows_per_block: 0 = the shipped choice; 32 / 64 / 128 select the
// measured arms (scripts/microbench_head.py, docs/KERNELS.md)
bool ss_head_fwd_fused(const void* x, const void* W, const void* bias,
                       void* probs, int M, int K, int C, int rows_per_block,
                       hipStream_t st) {
    if (!head_contract(M, K, C)) return false;
    const int rb = rows_per_block ? rows_per_block : 64;
#define HEAD_FWD(WV, FRV)                                                    \
    hipLaunchKernelGGL((head_fwd_fused_kernel<WV, FRV>),                     \
                       dim3(cdiv(M, WV * FRV * 16)), dim3(WV * 64), 0, st,   \
                       (const __bf16*)x, (const __bf16*)W,                   \
                       (const __bf16*)bias, (__bf16*)probs, M, K, C)
    if (rb == 32) HEAD_FWD(2, 1);
    else if (rb == 64) HEAD_FWD(4, 1);
    else if (rb == 128) HEAD_FWD(4, 2);
    else return false;
#undef HEAD_FWD
    return true;
}

bool ss_head_bwd_fused(const void* probs, const void* target, const void* x,
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

// kind: 0 = cross-entropy, 1 = squared error.  acc is [slots][4] words.
bool ss_head_metrics(const void* probs, const void* target, void* acc,
                     int slots, int M, int C, int kind, hipStream_t st) {
    if (M < 1 || C < 1 || !slots_ok(slots) || (kind != 0 && kind != 1))
        return false;
    // enough blocks to fill the chip; more would only add atomics
    const dim3 grid(min(cdiv(M, 4), 1024));
    if (kind == 1)
        hipLaunchKernelGGL(head_metrics_kernel<true>, grid, dim3(256), 0, st,
                           (const __bf16*)probs, (const __bf16*)target,
                           (int*)acc, slots, M, C);
    else
        hipLaunchKernelGGL(head_metrics_kernel<false>, grid, dim3(256), 0, st,
                           (const __bf16*)probs, (const __bf16*)target,
                           (int*)acc, slots, M, C);
    return true;
}
