// The wide backward chain (H = 128 and 512) under the softmax-MSE head
// (gfx950 / MI355X): the squared-error arm of ss_bwd_chain_wide
// (bwd_chain_wide.hip), in a translation unit of its own.
//
//   g       = −2 (t − s) / GB
//   dz_head = bf16(s · (g − Σ_c s·g))     (stored; bits of head_mse_bwd)
//   dh      = bf16(dz_head · W_head)
//   then bwd_chain_wide.hip's layer loop, unchanged.
//
// Kernel text, bits below the head, launch contract and arms are
// bwd_chain_wide.hip's: see there and bwd_chain_wide_kernel.h.  Only the
// head step differs: Σ_c is a 4-step xor tree over the 16 adjacent lanes
// that hold a row, entered by every lane of the wave (head_dev.h:
// head_mse_dz_elem); no LDS and no barrier added.

// Built without packed f32 arithmetic, as bwd_chain_wide.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define BWD_WIDE_KERNEL bwd_chain_wide_mse_kernel
#define BWD_WIDE_LAUNCHER ss_bwd_chain_wide_mse
#define BWD_WIDE_MSE 1
#include "bwd_chain_wide_kernel.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
