// The forward chain under dropout (gfx950 / MI355X): fwd_chain.hip's ONE
// launch for a training forward whose ReLU layers drop out.
//
//   per ReLU layer l, bottom to top (out = 256):
//     h_l   = bf16(keep_l ? relu(h_{l-1} · W_l^T + b_l) · scale_l : +0)
//   probs   = softmax(bf16(h_top · W_head^T + b_head))
//
// Replaces gemm_nt_dropout → … → head_fwd_fused.  The mask is
// dropout_dev.h's and the epilogue is gemm_nt_kernel<.., DROPOUT>'s, value
// for value: bias, ReLU, keep ? v · scale : +0, one rounding.  The
// dropped-out tile stays in LDS as the next layer's A operand and is
// stored once as h_l, which the backward reads as its mask (y > 0 <=>
// kept and active).  Every output equals the unfused chain bit for bit.
//
// The accumulators have gemm_nt_kernel's MFMA C layout, so the mask costs
// what it costs there: one Philox4x32-10 call per 16x16 fragment and
// lane, the four keep bits shared inside the lane quad by DPP
// (dropout_keep4_frag).  A layer's bits pack into nibbles of one register
// (two at 64 rows on four waves).  The Philox work depends on no
// accumulator, so the bits are drawn AHEAD of the layer's K loop, as
// integer VALU work that the other waves' MFMAs and the first B loads
// cover, and only the packed register stays live through the loop: the
// eight-wave arms sit at their 128-VGPR bound.  Drawing them in the
// epilogue instead (FWD_CHAIN_DROP == 1) measured 36.8 against 33.4 us
// at the flagship forward (profiles/r22_fwd_chain_dropout.md).
//
// A layer with p = 0 runs the plain epilogue by a block-uniform test and
// draws nothing.  The streamed first layer, both K loops and the four
// (rows, waves) arms are fwd_chain.hip's text (fwd_chain_kernel.h), and
// so is the deferred zero fill.
//
// Launch contract: ss_fwd_chain's, plus at least one layer with p > 0 and
// every row's sample id below 2^32.

#define FWD_CHAIN_KERNEL fwd_chain_drop_kernel
#define FWD_CHAIN_HEAD 1
#define FWD_CHAIN_DROP 2
#include "fwd_chain_kernel.h"

bool ss_fwd_chain_drop(const void* x, const void* const* w,
                       const void* const* b, void* const* h, int nlayers,
                       const void* W_head, const void* b_head, void* probs,
                       int M, int K0, int H, int C, int rows, int waves,
                       int l1, int kloop, void* zero_ptr, long zero_bytes,
                       const FwdChainDrop& drop, hipStream_t st) {
    return fwd_chain_launch(x, w, b, h, nlayers, W_head, b_head, probs, M, K0,
                            H, C, rows, waves, l1, kloop, zero_ptr,
                            zero_bytes, drop, st);
}
