// The stage arm of the wide forward chain under dropout (gfx950 /
// MI355X, H = 128 and 512): fwd_chain_wide_stage.hip's ONE launch for a
// training forward whose ReLU layers drop out; it ends with the
// dropped-out h of the top layer, which the stage sends on.
//
//   per ReLU layer l, bottom to top (out = H):
//     h_l   = bf16(keep_l ? relu(h_{l-1} · W_l^T + b_l) · scale_l : +0)
//
// The mask, its nibble-per-fragment registers and the epilogue are
// fwd_chain_wide_drop.hip's (fwd_chain_wide_kernel.h with FWD_WIDE_DROP 2
// and FWD_WIDE_HEAD 0): the keep bits are drawn AHEAD of each layer's K
// loop.  On the tile start (K0 == H, see fwd_chain_wide_stage.hip) layer
// 0 is an ordinary trip of the layer loop, so its bits are drawn ahead of
// its K loop too, after the barrier that makes the x tile whole.  Every
// h_l equals F.linear_fwd_dropout's bit for bit under either start.
//
// Launch contract: ss_fwd_chain_wide_stage's, plus ss_fwd_chain_wide_dropout's
// refusals: at least one layer with p > 0, every p in [0, 1) and every
// row's sample id below 2^32.

// Built without packed f32 arithmetic, as fwd_chain_wide.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define FWD_WIDE_KERNEL fwd_chain_wide_stage_drop_kernel
#define FWD_WIDE_LAUNCH fwd_chain_wide_stage_drop_launch
#define FWD_WIDE_HEAD 0
#define FWD_WIDE_DROP 2
#include "fwd_chain_wide_kernel.h"

bool ss_fwd_chain_wide_stage_dropout(const void* x, const void* const* w,
                                     const void* const* b, void* const* h,
                                     int nlayers, int M, int K0, int H,
                                     int rows, int waves, int start,
                                     const FwdChainDrop& drop,
                                     hipStream_t st) {
    return fwd_chain_wide_stage_drop_launch(x, w, b, h, nlayers, M, K0, H,
                                            rows, waves, start, drop, st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
