// The stage arm of the wide backward chain (gfx950 / MI355X, H = 128 and
// 512): the ReLU-layer data gradients of a pipeline stage that has no
// classifier head as ONE kernel, entered from the received gradient
// dout [M][H] in memory in place of the head.  The wide sibling of
// bwd_chain_stage.hip; loss-agnostic, so one translation unit.
//
//   dz_0  = !(h_0 > 0) ? +0 : dout                           (stored)
//           under dropout: !(h_0 > 0) ? +0 : bf16(dout · dz_scale)
//   per ReLU layer l, top to bottom (all H wide):
//     dh    = bf16(dz_l · W_l)          while the layer's dgrad is in
//                                       the chain; else the chain ends
//     dz_l+1 = !(h_l+1 > 0) ? +0 : dh   (· dz_scale)         (stored)
//   dx    = dh of the last layer        (stored, when that dgrad is in)
//
// The headed kernel reaches its first mask pass from MFMAs into LDS: the
// head's dz in dzs, W_head^T staged in wts, dh scattered into the tile, a
// barrier, then the pass reads the tile back.  A stage has none of that.
// Here a thread loads its NP 16-byte pieces of dout TOGETHER with the
// same pieces of h_0 into registers, masks there, and writes dz_0 once to
// the tile and once to memory: one LDS write, no LDS read, no barrier
// ahead of the pass, and no wts / dzs (at (512, 64, ·) 66 560 B of LDS
// against the headed 76 800 B).  From the first K loop on the text is
// bwd_chain_wide_kernel.h's, unchanged: the wt == nullptr end of chain,
// load_mask(l + 1) under the K loop, CHAIN_LAYER_MMA_AHEAD,
// CHAIN_ACC_TO_TILE, the dx store.
//
// Bits: the entry applies StageReg's rule to dout as relu_bwd does (a NaN
// or −0.0 in h masks to +0; a kept element is dout, or relu_bwd_scaled's
// bf16(f32(dout) · dz_scale): ONE v_mul_f32, this file is built without
// packed f32 arithmetic).  Every dz_l and dx equals relu_bwd → gemm_nt
// bit for bit.
//
// Launch contract (the launcher returns false outside it): H 128 or 512,
// 1..8 layers, M >= 1, every layer but the last has its W^T, the last has
// it exactly when dx is wanted, every pointer 16-B aligned, (rows, waves)
// one of the built arms.  Arms and resources: docs/KERNELS.md, "Stage
// arms, wide".

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define BWD_WIDE_KERNEL bwd_chain_wide_stage_kernel
#define BWD_WIDE_LAUNCHER ss_bwd_chain_wide_stage
#define BWD_WIDE_HEAD 0
#define BWD_WIDE_MSE 0
#include "bwd_chain_wide_kernel.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
