// Backward data path of the training step as ONE kernel at hidden widths
// 128 and 512 (gfx950 / MI355X): the wide sibling of bwd_chain.hip, which
// serves width 256.
//
//   dz_head = bf16((probs − target)/GB)                      (stored)
//   dh      = bf16(dz_head · W_head)
//   per ReLU layer l, top to bottom (all H wide):
//     dz_l  = !(h_l > 0) ? +0 : dh                           (stored)
//             under dropout: !(h_l > 0) ? +0 : bf16(dh · dz_scale)
//     dh    = bf16(dz_l · W_l)          while the layer's dgrad is in
//                                       the chain; else the chain ends
//   dx      = dh of the last layer      (stored, when that dgrad is in)
//
// A block of NW waves owns R batch rows and keeps their dh in ONE tile,
// tile[R][H + 8] bf16 in LDS, rewritten in place: wave w holds all of
// its H/NW output columns of a layer's dgrad in FM x FN accumulator
// fragments, so the dz tile is not overwritten before the barrier that
// ends the K loop.  W^T goes from L2 straight into registers as the MFMA
// B operand (CHAIN_LAYER_MMA_AHEAD, three K-steps ahead).  The mask
// source h_{l+1} is loaded a phase ahead, under the K loop of layer l.
// The head's W^T is staged into LDS 256 rows at a time (one chunk at
// H = 128, two at 512), so its buffer stays 8 KB at every width.
//
// What goes to memory is dz_l, the MASKED gradient, as 16-B
// row-contiguous stores: every weight-gradient kernel downstream runs
// without a mask.  There is no W-through-LDS arm.  Layers that ran
// inverted dropout take the SCALED instantiations (dz_scale != 1, one
// value per launch): the stashed post-dropout h_l is the mask, and a kept
// element is relu_bwd_scaled_kernel's, bf16(f32(dh) · dz_scale).
//
// Bits: dz_head and the head's dh come from the device code that
// head_bwd_fused_kernel runs (head_dev.h: one MFMA per 16x16 fragment
// from a zero accumulator).  A layer's dh is the
// v_mfma_f32_16x16x32_bf16 chain of gemm_nt_kernel — A = dz rows, B =
// W^T rows ([in][out], K = out contiguous), 32-wide K-steps in
// increasing order from a zero accumulator, rounded once by f2bf — and
// the mask is StageReg's rule (a NaN or −0.0 in h masks to +0).  Every
// output equals the per-layer path bit for bit.
//
// Launch contract (the launcher returns false outside it): H 128 or 512,
// C <= 16, 1..8 layers, M >= 1 (rows past M are guarded), every layer
// but the last has its W^T, the last has it exactly when dx is wanted,
// every pointer 16-B aligned, (rows, waves) one of the built arms.
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

// The kernel's text and its launch are bwd_chain_wide_kernel.h; this
// file compiles the cross-entropy arm (bwd_chain_wide_mse.hip the
// squared-error one).
#define BWD_WIDE_KERNEL bwd_chain_wide_kernel
#define BWD_WIDE_LAUNCHER ss_bwd_chain_wide_xent
#define BWD_WIDE_MSE 0
#include "bwd_chain_wide_kernel.h"

// loss: 0 = cross-entropy (this file's instantiations), 1 = squared
// error (bwd_chain_wide_mse.hip's).  Both arms check the same contract
// first.
bool ss_bwd_chain_wide(const void* probs, const void* target,
                       const void* Wt_head, void* dz_head,
                       const void* const* h, const void* const* wt,
                       void* const* dz, int nlayers, void* dx, int M, int H,
                       int C, float inv_gb, int rows, int waves,
                       float dz_scale, int loss, hipStream_t st) {
    if (loss != 0 && loss != 1) return false;
    return (loss ? ss_bwd_chain_wide_mse : ss_bwd_chain_wide_xent)(
        probs, target, Wt_head, dz_head, h, wt, dz, nlayers, dx, M, H, C,
        inv_gb, rows, waves, dz_scale, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
