// Training forward as ONE kernel (gfx950 / MI355X): the 256-wide ReLU
// layers under the classifier head and the head itself.
//
//   per ReLU layer l, bottom to top (out = 256):
//     h_l   = bf16(relu(h_{l-1} · W_l^T + b_l))              (stored)
//   probs   = softmax(bf16(h_top · W_head^T + b_head))       (stored)
//
// Replaces gemm_nt<bias, relu> → … → head_fwd_fused: the forward is
// row-local, so a block that owns R batch rows keeps its activation
// tile in LDS from layer to layer.  Every h_l is written once, because
// the backward needs it, and never read back.
//
// Bits: a layer is the v_mfma_f32_16x16x32_bf16 chain of gemm_nt_kernel
// — A = activation rows, B = W rows ([out][in], K contiguous), 32-wide
// K-steps in increasing order from a zero accumulator, K past in_dims
// as zeros in both operands — followed by that kernel's epilogue,
// v = acc + bias; v = v > 0 ? v : 0; f2bf(v).  The head is the MFMA
// chain and the register epilogue of head_fwd_fused_kernel (head_dev.h).
// Every output equals the unfused chain bit for bit.
//
// W (128 KB per 256-wide layer, L2-resident: every block reads all of
// it) goes L2 -> registers as the MFMA B operand, 16 B per lane and
// K-step.  The A operand is the tile in LDS.  Two texts of the K loops
// (AH): B one load group ahead as in bwd_chain_kernel (CHAIN_LAYER_MMA),
// or three K-steps ahead in a ring of named register sets
// (CHAIN_LAYER_MMA_AHEAD), which the eight-wave arms ship: in the first
// text the hand-over of the next group's registers makes every K-step
// wait for the loads it has just issued.
//
// The launch can also zero a buffer for its caller (the step's flat
// gradient buffer, in place of a memset launch): stores at kernel entry
// that nothing in the kernel waits for.
//
// Two arms for where the chain starts.  L1 = false: the input is a
// stored 256-wide activation and the kernel's first action is to load
// its tile into LDS.  L1 = true: the first layer has any in_dims % 8 ==
// 0 (784 at the flagship); its A operand x is streamed from memory in
// KC-wide chunks through a register-staged, double-buffered LDS stage,
// one barrier per chunk, columns past in_dims as zeros.
//
// Launch contract (the launcher returns false outside it): width 256,
// C <= 16, 1..8 layers, M >= 1 (rows past M are guarded), in_dims of the
// first layer 256 (L1 = false) or a multiple of 8 (L1 = true), every
// pointer 16-B aligned.
//
// A pipeline stage that has no head runs the same text as
// fwd_chain_stage_kernel: no W_head / b_head / probs, no zeroing, and the
// kernel ends with the top layer's h, which the stage sends on
// (ss_fwd_chain_stage; the contract above minus C).

// The kernel's text is fwd_chain_kernel.h; this file is the arm with the
// head: the last stage's, or the whole model's, forward.
#define FWD_CHAIN_KERNEL fwd_chain_kernel
#define FWD_CHAIN_HEAD 1
#include "fwd_chain_kernel.h"

bool ss_fwd_chain(const void* x, const void* const* w, const void* const* b,
                  void* const* h, int nlayers, const void* W_head,
                  const void* b_head, void* probs, int M, int K0, int H, int C,
                  int rows, int waves, int l1, int kloop, void* zero_ptr,
                  long zero_bytes, hipStream_t st) {
    return fwd_chain_launch(x, w, b, h, nlayers, W_head, b_head, probs, M, K0,
                            H, C, rows, waves, l1, kloop, zero_ptr,
                            zero_bytes, st);
}
