// The wide forward chain under dropout (gfx950 / MI355X, H = 128 and
// 512): fwd_chain_wide.hip's ONE launch for a training forward whose ReLU
// layers drop out, the wide sibling of fwd_chain_drop.hip.
//
//   per ReLU layer l, bottom to top (out = H):
//     h_l   = bf16(keep_l ? relu(h_{l-1} · W_l^T + b_l) · scale_l : +0)
//   probs   = softmax(bf16(h_top · W_head^T + b_head))
//
// Replaces gemm_nt_dropout → … → head_fwd_fused.  The mask is
// dropout_dev.h's and the epilogue is gemm_nt_kernel<.., DROPOUT>'s, value
// for value: bias, ReLU, keep ? v · scale : +0, one rounding.  The
// dropped-out tile stays in LDS, rewritten in place, as the next layer's
// A operand and is stored once as h_l, which the backward reads as its
// mask (y > 0 <=> kept and active).  Every output equals the unfused
// chain bit for bit.
//
// The split is fwd_chain_wide.hip's: wave w holds ALL of its H/NW output
// columns of a layer in FM x FN accumulator fragments of gemm_nt_kernel's
// MFMA C layout, so the mask costs what it costs there: one
// Philox4x32-10 call per 16x16 fragment and lane, the four keep bits
// shared inside the lane quad by DPP (dropout_keep4_frag).  Fragment
// (i, j) owns nibble i * FN + j of (FM * FN + 7) / 8 registers: one, two
// for (64, 8) at 512.  The Philox work depends on no accumulator, so the
// bits are drawn AHEAD of the layer's K loop: for the streamed first
// layer before the chunk loop, next to the bias load; for a hidden layer
// before CHAIN_LAYER_MMA_AHEAD, where the integer VALU work sits under
// the other waves' MFMAs and the first B loads.  Only the packed
// registers stay live through the loop, which matters for (64, 16) at
// 512 and its 128-VGPR bound.  Rows past M draw too (the quad exchange
// needs every lane) and are never stored.
//
// A layer with p = 0 runs the plain epilogue by a block-uniform test and
// draws nothing.  The streamed first layer, the K loops, the head and
// the five (rows, waves) arms are fwd_chain_wide.hip's text
// (fwd_chain_wide_kernel.h).  Registers and LDS of the instantiations:
// profiles/r24_chain_wide_dropout.md.
//
// Launch contract: ss_fwd_chain_wide's, plus at least one layer with
// p > 0, every p in [0, 1) and every row's sample id below 2^32.

// Built without packed f32 arithmetic, as fwd_chain_wide.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define FWD_WIDE_KERNEL fwd_chain_wide_drop_kernel
#define FWD_WIDE_LAUNCH fwd_chain_wide_drop_launch
#define FWD_WIDE_DROP 2
#include "fwd_chain_wide_kernel.h"

bool ss_fwd_chain_wide_dropout(const void* x, const void* const* w,
                               const void* const* b, void* const* h,
                               int nlayers, const void* W_head,
                               const void* b_head, void* probs, int M, int K0,
                               int H, int C, int rows, int waves,
                               const FwdChainDrop& drop, hipStream_t st) {
    return fwd_chain_wide_drop_launch(x, w, b, h, nlayers, W_head, b_head,
                                      probs, M, K0, H, C, rows, waves, drop,
                                      st);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
