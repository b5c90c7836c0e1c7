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
#define BWD_CHAIN_LAUNCHER ss_bwd_chain_xent
#define BWD_CHAIN_SCALE(f) ((f) * (dz_scale + ...))
#include "bwd_chain_kernel.h"

// loss: 0 = cross-entropy (this file's instantiations), 1 = squared
// error (bwd_chain_mse.hip's).  Both arms check the same contract first.
bool ss_bwd_chain(const void* probs, const void* target, const void* Wt_head,
                  void* dz_head, const void* const* h, const void* const* wt,
                  void* const* dz, int nlayers, void* dx, int M, int H, int C,
                  float inv_gb, int rows, int waves, int w_lds,
                  float dz_scale, int loss, hipStream_t st) {
    if (loss != 0 && loss != 1) return false;
    return (loss ? ss_bwd_chain_mse : ss_bwd_chain_xent)(
        probs, target, Wt_head, dz_head, h, wt, dz, nlayers, dx, M, H, C,
        inv_gb, rows, waves, w_lds, dz_scale, st);
}
