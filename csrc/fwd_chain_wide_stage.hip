// The stage arm of the wide forward chain (gfx950 / MI355X, H = 128 and
// 512): the ReLU layers of a pipeline stage that has no classifier head
// as ONE kernel that ends with h of the top layer, which the stage sends
// on.  The wide sibling of fwd_chain_stage.hip.
//
//   per ReLU layer l, bottom to top (out = H):
//     h_l   = bf16(relu(h_{l-1} · W_l^T + b_l))              (stored)
//
// The split, the tile, the K loops and the epilogue are
// fwd_chain_wide.hip's text (fwd_chain_wide_kernel.h with FWD_WIDE_HEAD
// 0): no W_head / b_head / probs / C and no head block, the kernel ends
// after the last layer's h store.  What a stage adds is a second START,
// chosen by the launcher from K0 alone:
//
//   * K0 != H (stage 0, or any input width % 8 == 0): the streamed first
//     layer as it stands, x through two chunk buffers that alias the
//     still-empty tile, one barrier per chunk, B handed over one K-step
//     ahead;
//   * K0 == H (a middle stage, whose input is the stored H-wide
//     activation of the stage below): each thread loads its NP 16-byte
//     pieces of x INTO the tile, rows past M as zeros; after one barrier
//     layer 0 runs CHAIN_LAYER_MMA_AHEAD like every later layer, B three
//     K-steps ahead in the ring of four named sets.  No x stage, no chunk
//     barriers, no per-step hand-over of B.
//
// Bits: both starts run layer 0 as 32-wide K-steps in increasing order
// from a zero accumulator into gemm_nt_kernel's epilogue, so every h_l
// equals the per-layer path bit for bit whichever start ran.
//
// Launch contract (the launcher returns false outside it): H 128 or 512,
// 1..8 layers, M >= 1, K0 >= 8 and a multiple of 8, every pointer 16-B
// aligned, (rows, waves) one of the built arms, start 0 (by K0), 1
// (streamed) or 2 (tile; K0 == H only).  Arms, resources and the shipped
// start: docs/KERNELS.md, "Stage arms, wide".

// Built without packed f32 arithmetic, as fwd_chain_wide.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define FWD_WIDE_KERNEL fwd_chain_wide_stage_kernel
#define FWD_WIDE_LAUNCH fwd_chain_wide_stage_launch
#define FWD_WIDE_HEAD 0
#include "fwd_chain_wide_kernel.h"

bool ss_fwd_chain_wide_stage(const void* x, const void* const* w,
                             const void* const* b, void* const* h,
                             int nlayers, int M, int K0, int H, int rows,
                             int waves, int start, hipStream_t st) {
    return fwd_chain_wide_stage_launch(x, w, b, h, nlayers, M, K0, H, rows,
                                       waves, start, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
