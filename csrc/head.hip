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
//
// Squared error.  head_bwd_fused also serves the softmax-MSE head
// (loss = 1): dz = bf16(s · (g − Σ_c s·g)), g = −2(t − s)/GB, the bits of
// head_mse_bwd_kernel (head_dev.h: head_mse_dz_elem), the METRICS arm
// summing (t − p)².  Those instantiations are head_bwd_mse_kernel in
// head_mse.hip; the forward is the same for both losses.

// The backward kernel's text is head_bwd_kernel.h; this file compiles
// its cross-entropy arm.
#define HEAD_BWD_KERNEL head_bwd_fused_kernel
#define HEAD_BWD_LAUNCHER ss_head_bwd_fused_xent
#define HEAD_BWD_MSE 0
#include "head_bwd_kernel.h"

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

// loss: 0 = cross-entropy (this file's instantiations), 1 = squared
// error (head_mse.hip's).  Both arms check the same contract first.
bool ss_head_bwd_fused(const void* probs, const void* target, const void* x,
                       const void* Wt, void* dz, void* dx, void* gW, void* gb,
                       int M, int K, int C, float inv_gb, int rows_per_block,
                       void* metrics, int slots, int loss, hipStream_t st) {
    if (loss != 0 && loss != 1) return false;
    return (loss ? ss_head_bwd_fused_mse : ss_head_bwd_fused_xent)(
        probs, target, x, Wt, dz, dx, gW, gb, M, K, C, inv_gb, rows_per_block,
        metrics, slots, st);
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
