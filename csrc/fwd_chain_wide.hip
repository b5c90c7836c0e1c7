// Training forward as ONE kernel at hidden widths 128 and 512 (gfx950 /
// MI355X): the wide sibling of fwd_chain.hip, which serves width 256.
//
//   per ReLU layer l, bottom to top (out = H):
//     h_l   = bf16(relu(h_{l-1} · W_l^T + b_l))              (stored)
//   probs   = softmax(bf16(h_top · W_head^T + b_head))       (stored)
//
// The split and the data movement are fused_mlp_wide.hip's: a block of
// NW waves owns R batch rows in ONE activation tile, tile[R][H + 8] bf16
// in LDS, rewritten in place layer after layer (two tiles stop fitting
// twice on a CU at H = 512):
//
//   * wave w holds ALL of its output columns [w * H/NW, +H/NW) of the
//     layer in FM x FN f32 accumulator fragments, so nothing of the tile
//     is overwritten before the block barrier that ends the K loop;
//   * W never passes through LDS: each wave reads the B fragments of its
//     own columns straight from L2 into registers, three K-steps ahead in
//     a ring of four named sets (CHAIN_LAYER_MMA_AHEAD);
//   * the first layer takes any in_dims % 8 == 0: x is streamed through
//     two [R][KC + 8] chunk buffers that ALIAS the still-empty tile, one
//     barrier per chunk, the loads of chunk c + 1 issued ahead of chunk
//     c's MFMAs.  Rows past M and columns past in_dims are zeros in both
//     operands.
//
// What training adds to the serving kernel: every h_l leaves the tile
// once, as 16-B row-contiguous stores, because the backward needs it (it
// is never read back), and the head ends in HEAD_FWD_EPILOGUE and writes
// bf16 probs.
//
// Bits: a layer is the v_mfma_f32_16x16x32_bf16 chain of gemm_nt_kernel,
// 32-wide K-steps in increasing order from a zero accumulator, followed
// by that kernel's epilogue, v = acc + bias; v = v > 0 ? v : 0; f2bf(v).
// The head is the MFMA chain and the register epilogue of
// head_fwd_fused_kernel (head_dev.h).  Every output equals the per-layer
// path bit for bit.
//
// Launch contract (the launcher returns false outside it): H 128 or 512,
// C <= 16, 1..8 layers, M >= 1, in_dims of the first layer a multiple of
// 8, every pointer 16-B aligned, (rows, waves) one of the built arms.
// Arms, resources and the shipped choice: docs/KERNELS.md, "Chain
// kernels, wide"; profiles/r20_chain_wide.md.

// This file's device code is built without packed f32 arithmetic (no
// v_pk_add/mul/fma_f32), as a per-file -target-feature -packed-fp32-ops
// would: the attribute must also reach the helpers of the headers below,
// or they could not be inlined into the kernel.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// The kernel's text and its launch are fwd_chain_wide_kernel.h; this file
// compiles the plain arm (fwd_chain_wide_drop.hip the one under dropout).
#define FWD_WIDE_KERNEL fwd_chain_wide_kernel
#define FWD_WIDE_LAUNCH fwd_chain_wide_launch
#include "fwd_chain_wide_kernel.h"

bool ss_chain_wide_arm_built(int H, int rows, int waves) {
    if (H != 128 && H != 512) return false;
    chain_wide_shipped(H, 1, rows, waves);
    auto none = [](auto, auto, auto) {};
    return H == 128 ? with_chain_wide_arm<128>(rows, waves, none)
                    : with_chain_wide_arm<512>(rows, waves, none);
}

bool ss_fwd_chain_wide(const void* x, const void* const* w,
                       const void* const* b, void* const* h, int nlayers,
                       const void* W_head, const void* b_head, void* probs,
                       int M, int K0, int H, int C, int rows, int waves,
                       hipStream_t st) {
    return fwd_chain_wide_launch(x, w, b, h, nlayers, W_head, b_head, probs,
                                 M, K0, H, C, rows, waves, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
