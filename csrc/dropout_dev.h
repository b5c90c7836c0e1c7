// Counter-based dropout mask: the one device definition (gfx950 / MI355X).
//
// The keep decision of element (sample, col) of layer `layer` at
// optimizer step `step` under a 64-bit seed is a pure function of those
// five values, so any DP x PP x micro-batch partition of a batch draws
// the bits the serial model draws:
//
//   words = Philox4x32-10(counter = (sample, col >> 2, layer, step),
//                         key     = (seed & 0xffffffff, seed >> 32))
//   keep  = words[col & 3] < thr,  thr = min(2^32 - 1, round((1 - p) 2^32))
//   y     = keep ? y * float32(1 / (1 - p)) : +0     (inverted dropout)
//
// One Philox call covers four consecutive columns of one sample.  The
// CPU twin is ops/functional.py:dropout_keep_mask (numpy uint64).
#pragma once

#include "common.h"
#include "launchers.h"  // DropoutArgs

__host__ __device__ __forceinline__ unsigned philox_mulhi(unsigned a,
                                                          unsigned b) {
    return (unsigned)(((unsigned long long)a * b) >> 32);
}

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by
// the Weyl constants between rounds.
__host__ __device__ __forceinline__ void philox4x32_10(
    unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
    unsigned k1, unsigned (&out)[4]) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    constexpr unsigned W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
        const unsigned hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// The four words of (sample, column group): columns 4*cgroup .. +3.
__host__ __device__ __forceinline__ void dropout_words(
    const DropoutArgs& d, unsigned sample, unsigned cgroup,
    unsigned (&w)[4]) {
    philox4x32_10(sample, cgroup, d.layer, d.step, d.key0, d.key1, w);
}

// Bit k set: column 4*cgroup + k of `sample` is kept.
__host__ __device__ __forceinline__ unsigned dropout_keep4(
    const DropoutArgs& d, unsigned sample, unsigned cgroup) {
    unsigned w[4];
    dropout_words(d, sample, cgroup, w);
    return (unsigned)(w[0] < d.thr) | ((unsigned)(w[1] < d.thr) << 1) |
           ((unsigned)(w[2] < d.thr) << 2) | ((unsigned)(w[3] < d.thr) << 3);
}

__host__ __device__ __forceinline__ unsigned dropout_sample(
    const DropoutArgs& d, unsigned row) {
    return d.row_first + row * d.row_stride;
}
