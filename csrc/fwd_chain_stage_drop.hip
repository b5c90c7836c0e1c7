// The stage arm of the forward chain under dropout (gfx950 / MI355X):
// the 256-wide ReLU layers of a pipeline stage that has no classifier
// head, each with its dropout mask in the epilogue, as ONE kernel that
// ends with the dropped-out h of the top layer, which the stage sends on.
// The kernel's text, its bits and its launch contract (minus C and the
// zero fill) are fwd_chain_drop.hip's: see there and fwd_chain_kernel.h.

#define FWD_CHAIN_KERNEL fwd_chain_stage_drop_kernel
#define FWD_CHAIN_HEAD 0
#define FWD_CHAIN_DROP 2
#include "fwd_chain_kernel.h"

bool ss_fwd_chain_stage_drop(const void* x, const void* const* w,
                             const void* const* b, void* const* h,
                             int nlayers, int M, int K0, int H, int rows,
                             int waves, int l1, int kloop,
                             const FwdChainDrop& drop, hipStream_t st) {
    return fwd_chain_launch(x, w, b, h, nlayers, nullptr, nullptr, nullptr, M,
                            K0, H, 1, rows, waves, l1, kloop, nullptr, 0,
                            drop, st);
}
