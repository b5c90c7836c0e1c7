// Fused backward of the softmax-MSE classifier head (gfx950 / MI355X):
// the squared-error arm of head_bwd_fused (head.hip), in a translation
// unit of its own so that the cross-entropy instantiations are compiled
// as they were.
//
//   g  = −2 (t − s) / GB
//   dz = bf16(s · (g − Σ_c s·g))          (stored; bits of head_mse_bwd)
//   dx = bf16(dz · W)                     (B operand: W^T copy)
//   gW += dz^T · x ; gb += colsum(dz)     (optional, f32)
//
// Unlike cross-entropy's elementwise (s − t)/GB, no dz element exists
// before its row has been reduced.  The tile layout already puts the 16
// classes of a row into 16 adjacent lanes, so the reduction is a 4-step
// xor tree in registers (head_dev.h: head_mse_dz_elem), entered by every
// lane of the wave; it adds no LDS and no barrier.  The METRICS
// instantiations sum the squared error (t − p)² in the reduction they
// already run.  Everything from the dz tile on — the dx MFMA, the
// in-kernel gW / gb, the K chunks — is the text of head_bwd_kernel.h.
//
// Replaces softmax_fwd's consumer chain head_mse_bwd → gemm_nt(dz, Wt)
// (→ wgrad_tn) for the default loss.  Same launch contract and row arms
// (32 / 64 / 128) as the cross-entropy kernel.
#define HEAD_BWD_KERNEL head_bwd_mse_kernel
#define HEAD_BWD_LAUNCHER ss_head_bwd_fused_mse
#define HEAD_BWD_MSE 1
#include "head_bwd_kernel.h"
