// The stage arm of the forward chain (gfx950 / MI355X): the 256-wide
// ReLU layers of a pipeline stage that has no classifier head, as ONE
// kernel that ends with h of the top layer, which the stage sends on.
// The kernel's text, its bits and its launch contract (minus C) are
// fwd_chain.hip's: see there and fwd_chain_kernel.h.

#define FWD_CHAIN_KERNEL fwd_chain_stage_kernel
#define FWD_CHAIN_HEAD 0
#include "fwd_chain_kernel.h"

// Same contract, arms and shipped choices as ss_fwd_chain, minus the
// head and the zeroing.
bool ss_fwd_chain_stage(const void* x, const void* const* w,
                        const void* const* b, void* const* h, int nlayers,
                        int M, int K0, int H, int rows, int waves, int l1,
                        int kloop, hipStream_t st) {
    return fwd_chain_launch(x, w, b, h, nlayers, nullptr, nullptr, nullptr, M,
                            K0, H, 1, rows, waves, l1, kloop, nullptr, 0, st);
}
