// Backward data path of the training step as ONE kernel (gfx950 /
// MI355X): the head backward and the ReLU-layer data gradients below it.
//
//   dz_head = bf16((probs − target)/GB)                      (stored)
//   dh      = bf16(dz_head · W_head)
//   per ReLU layer l, top to bottom (all 256 wide):
//     dz_l  = !(h_l > 0) ? +0 : dh                           (stored)
//     dh    = bf16(dz_l · W_l)          while the layer's dgrad is in
//                                       the chain; else the chain ends
//   dx      = dh of the last layer      (stored, when that dgrad is in)
//
// Replaces head_bwd_fused → gemm_nt<mask> → gemm_nt<mask> …: the chain
// is row-local, so a block that owns R batch rows keeps the dh tile in
// LDS from layer to layer instead of writing it to memory for the next
// launch to read back.  What goes to memory is dz_l, the MASKED
// gradient, in place of dh_l: the same bytes, and every weight-gradient
// kernel downstream then runs without a mask.
//
// Bits: dz_head and the head's dh come from the device code that
// head_bwd_fused_kernel runs (head_dev.h).  A layer's dh is the
// v_mfma_f32_16x16x32_bf16 chain of gemm_nt_kernel — A = dz rows, B =
// W^T rows ([in][out], K = out contiguous), 32-wide K-steps in
// increasing order from a zero accumulator, rounded once by f2bf — and
// the mask is StageReg's rule (a NaN or −0.0 in h masks to +0).  Every
// output equals the unfused chain bit for bit.
//
// W^T (128 KB per layer, L2-resident: every block reads all of it) goes
// L2 -> registers as the MFMA B operand, 16 B per lane and K-step, the
// next load group in flight under the current group's MFMAs, as in
// head_fwd_fused_kernel.  The A operand is the dz tile in LDS.
//
// Launch contract (the launcher returns false outside it): width 256,
// C <= 16, 1..8 layers, M >= 1 (rows past M are guarded), every layer
// but the last has its W^T, the last has it exactly when dx is wanted.
//
// A pipeline stage that has no head runs the same text as
// bwd_chain_stage_kernel, entered from the received gradient dout
// [M][256] in memory in place of the head (ss_bwd_chain_stage; the
// contract above minus C, dout 16-B aligned).

// The kernel's text is bwd_chain_kernel.h; this file is the arm under the
// head: the last stage's, or the whole model's, backward.
#define BWD_CHAIN_KERNEL bwd_chain_kernel
#define BWD_CHAIN_HEAD 1
#define BWD_CHAIN_SCALE(f) ((f) * (dz_scale + ...))
#include "bwd_chain_kernel.h"

// rows / waves: 0 = the shipped choice (64, 8); (32, 4), (32, 8),
// (64, 4) and (64, 8) are the measured arms (scripts/microbench_bwd_chain.py,
// docs/KERNELS.md).  w_lds: 0 = the shipped choice (W^T from L2 into
// registers), 1 = W^T through LDS, built for (64, 8) only.
// SS_BWD_CHAIN_ROWS / SS_BWD_CHAIN_WAVES / SS_BWD_CHAIN_WLDS (read once)
// override the shipped choice for tuning.
// dz_scale: 1.f runs the unscaled instantiations; any other value the
// scaled one, which only the shipped arm is built with.
bool ss_bwd_chain(const void* probs, const void* target, const void* Wt_head,
                  void* dz_head, const void* const* h, const void* const* wt,
                  void* const* dz, int nlayers, void* dx, int M, int H, int C,
                  float inv_gb, int rows, int waves, int w_lds,
                  float dz_scale, hipStream_t st) {
    if (M < 1 || H != 256 || C < 1 || C > 16 || nlayers < 1 ||
        nlayers > SS_BWD_CHAIN_MAX)
        return false;
    BwdChainLayers L = {};
    if (!bwd_chain_layers(L, h, wt, dz, nlayers, dx)) return false;
    bwd_chain_env(rows, waves, w_lds);
    if (!rows) rows = 64;
    if (!waves) waves = 8;
    if (dz_scale != 1.f) {
        if (rows != 64 || waves != 8 || w_lds != 0) return false;
        bwd_chain_launch<64, 8, false>(probs, target, Wt_head, dz_head, L,
                                       nlayers, dx, M, C, inv_gb, st,
                                       dz_scale);
        return true;
    }
    if (w_lds == 1) {
        if (rows != 64 || waves != 8) return false;
        bwd_chain_launch<64, 8, true>(probs, target, Wt_head, dz_head, L,
                                      nlayers, dx, M, C, inv_gb, st);
        return true;
    }
    return with_chain_arm(rows, waves, [&](auto r, auto nw) {
        bwd_chain_launch<r.value, nw.value>(probs, target, Wt_head, dz_head,
                                            L, nlayers, dx, M, C, inv_gb, st);
    });
}
