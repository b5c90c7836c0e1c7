// The backward chain under the softmax-MSE head (gfx950 / MI355X): the
// squared-error arm of ss_bwd_chain (bwd_chain.hip), the head backward of
// the default loss and the 256-wide ReLU-layer data gradients below it as
// ONE kernel.
//
//   g       = −2 (t − s) / GB
//   dz_head = bf16(s · (g − Σ_c s·g))     (stored; bits of head_mse_bwd)
//   dh      = bf16(dz_head · W_head)
//   then bwd_chain.hip's layer loop, unchanged.
//
// The kernel's text, its bits below the head and its launch contract are
// bwd_chain.hip's: see there and bwd_chain_kernel.h.  Only the head step
// differs: a row of the head tile sits in 16 adjacent lanes, so Σ_c is a
// 4-step xor tree in registers that every lane of the wave enters
// (head_dev.h: head_mse_dz_elem), with no LDS and no barrier added.
//
// A translation unit of its own: further instantiations inside
// bwd_chain.hip changed how kernels that were never touched are laid out
// and run (profiles/r16_stage_chain.md).  Built arms: the four (rows,
// waves) pairs and the scaled form of the shipped one; no W-through-LDS
// arm.

// New device code is built without packed f32 arithmetic (see
// bwd_chain_wide.hip): the attribute must also reach the helpers of the
// headers below, or they could not be inlined into the kernel.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define BWD_CHAIN_KERNEL bwd_chain_mse_kernel
#define BWD_CHAIN_HEAD 1
#define BWD_CHAIN_MSE 1
#define BWD_CHAIN_LAUNCHER ss_bwd_chain_mse
#define BWD_CHAIN_SCALE(f) ((f) * (dz_scale + ...))
#include "bwd_chain_kernel.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
