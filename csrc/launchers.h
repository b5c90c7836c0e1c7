// Host launchers of the HIP kernels: the one declaration of each.
//
// Every .hip file that defines a launcher includes this header, and so
// does bindings.cpp.  All have C++ linkage, so a parameter list that
// changes on one side only is another overload: the call or the symbol
// then has no match and the build fails, at the latest when it imports
// the extension, instead of passing arguments in the wrong slots.
// Pointers are untyped device
// pointers; every launcher enqueues on `stream` and returns at once.
// The bool launchers return false, with nothing launched, when the
// shape is outside their kernel's contract.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

// Non-null and 16-byte aligned: what a kernel that moves 16-byte pieces
// asks of a pointer.  The launchers and the bindings both test with it.
inline bool aligned16(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

// ---- gemm.hip
void ss_gemm_nt(const void* A, const void* B, const void* bias,
                const void* mask, void* C, int M, int N, int K, bool relu,
                hipStream_t stream);
void ss_colsum(const void* dY, const void* mask, void* gb, int M, int N,
               hipStream_t stream);

// Launch-constant part of the dropout mask (dropout_dev.h), passed by
// value to the kernels.  Row i of a launch is sample
// row_first + i * row_stride (32-bit).
struct DropoutArgs {
    unsigned key0, key1;   // seed low / high word
    unsigned layer, step;  // counter words 2, 3
    unsigned row_first, row_stride;
    unsigned thr;          // keep when word < thr
    float scale;           // float32(1 / (1 - p))
};
// C = dropout(relu(A · B^T + bias)) with the mask in the GEMM epilogue.
// bias is required.  Returns false when the
// shape's tier has no fused epilogue (256-tile, glds): C then holds the
// plain relu(A · B^T + bias) and the caller runs ss_dropout_fwd on it.
bool ss_gemm_nt_dropout(const void* A, const void* B, const void* bias,
                        void* C, int M, int N, int K,
                        const DropoutArgs& drop, hipStream_t stream);

// ---- gemm256.hip / gemm256w.hip
bool ss_gemm_nt_256(const void* A, const void* B, const void* bias, void* C,
                    int M, int N, int K, bool relu, hipStream_t stream);
bool ss_gemm_nt_256w(const void* A, const void* B, const void* bias, void* C,
                     int M, int N, int K, bool relu, hipStream_t stream);

// ---- fp8.hip
void ss_fp8_quantize(const void* X, void* Q, void* S, int R, int K,
                     hipStream_t stream);
bool ss_gemm_nt_f8(const void* A, const void* Asc, const void* B,
                   const void* Bsc, const void* bias, void* C, int M, int N,
                   int K, bool relu, hipStream_t stream);
bool ss_gemm_nt_f8_q(const void* A, const void* Asc, const void* B,
                     const void* Bsc, const void* bias, void* Cq, void* Cs,
                     int M, int N, int K, bool relu, hipStream_t stream);

// ---- wgrad.hip / wgrad256.hip
// stages: LDS staging sets of the K loop, 1 or 2; 0 = the launcher's
// choice (SS_WGRAD_STAGES, else the measured default).
void ss_wgrad_tn(const void* dY, const void* X, const void* mask, void* gW,
                 void* gb, int Mo, int N, int Kb, int split_k, int stages,
                 hipStream_t stream);
void ss_wgrad_tn_multi(const void* chunk_table, int nchunks, bool has_mask,
                       void* gW, void* gb, int Mo, int N, int Kb_chunk,
                       int split_k, hipStream_t stream);
bool ss_wgrad_tn_256(const void* dY, const void* X, void* gW, int Mo, int N,
                     int Kb, hipStream_t stream);

// Ordered split-K: the bitwise-reproducible wgrad at full width.  Each
// K-slice's partial tile goes to the workspace `part` by plain stores
// and a fold kernel leaves
//     gW = gW_old + (((p_0 + p_1) + p_2) + ... + p_{S-1})
// in f32, gb likewise: a pure function of the shapes and the build.
// split_k: 0 = one wave of blocks, as the default path's auto split;
// else the caller's, lowered to whole 64-row K-steps.  An effective
// split of 1 IS ss_wgrad_tn(..., split_k = 1): no workspace, no fold.
// The 256-tile tier (atomics) is never entered.  `part`: device memory,
// 16-byte aligned, part_bytes >= ss_wgrad_ordered_plan's; its contents
// before and after the call mean nothing.  False, with nothing launched,
// for a bad shape, split, pointer or a workspace too small.
bool ss_wgrad_tn_ordered(const void* dY, const void* X, const void* mask,
                         void* gW, void* gb, void* part, size_t part_bytes,
                         int Mo, int N, int Kb, int split_k,
                         hipStream_t stream);
// Host only: the workspace bytes of that call (0 when the split is 1),
// its effective split and the blocks of its partial launch.  With
// split_k = 0 at most 256 blocks of one tile (<= 64 KB) each: <= 16 MB.
size_t ss_wgrad_ordered_plan(int Mo, int N, int Kb, int split_k, int* split,
                             int* blocks);

// Grouped launch: independent unmasked problems, side by side.
constexpr int SS_WGRAD_GROUP_MAX = 8;  // problems per launch
struct WgradProblem {
    const void* dY;  // [Kb][Mo] bf16
    const void* X;   // [Kb][N] bf16
    void* gW;        // [Mo][N] f32, +=
    void* gb;        // [Mo] f32 or null, +=
    int Mo, N, Kb;
};
// One launch of a plan: problems [first, first + count) of the list,
// their splits and block counts.  count == 1 is a plain ss_wgrad_tn
// call (split 0 there = that launcher's own choice, blocks = its grid).
struct WgradGroupLaunch {
    int first, count;
    int split[SS_WGRAD_GROUP_MAX];
    int blocks[SS_WGRAD_GROUP_MAX];
};
// Plans the launches of a list from its shapes alone (pointers are not
// read): maximal runs of consecutive problems with the same tile
// configuration, at most SS_WGRAD_GROUP_MAX each.  splits: per problem,
// 0 (the group rule) or >= 2; null = all 0.  Writes at most n entries
// to `out`; returns their number, or -1 for a bad shape or split.
int ss_wgrad_group_plan(const WgradProblem* problems, int n,
                        const int* splits, WgradGroupLaunch* out);
// Runs the plan: a run of two or more is ONE wgrad_group_kernel launch,
// a run of one goes through ss_wgrad_tn.  False, with nothing launched,
// for a bad shape, split or pointer.
bool ss_wgrad_tn_group(const WgradProblem* problems, int n,
                       const int* splits, hipStream_t stream);

// Ordered grouped launch: the bitwise-reproducible form of the above.
// Each planned launch becomes ONE partial launch (every problem's
// K-slices to its own region of `workspace` by plain stores) and ONE
// fold launch over the same problems, which spreads a piece's S slices
// over the W = SS_WGRAD_FOLD_WAVES waves of a block in a fixed tree:
//     c = ceil(S / W),  q_w = ((p_{wc} + p_{wc+1}) + ...),
//     gW = gW_old + (((q_0 + q_1) + q_2) + ...)     in f32, gb likewise:
// a pure function of shapes, splits and the build.  For S <= W that is
// ss_wgrad_tn_ordered's serial order at the same split, bit for bit.
// A run of one goes through the same two kernels; a problem whose
// effective split is 1 takes ss_wgrad_tn(..., split_k = 1) and no
// workspace.  The 256-tile tier is never entered.  `workspace`: device
// memory, 16-byte aligned, bytes >= ss_wgrad_group_ordered_plan's.
// fold_waves: 0, or 4 / 8 / 16 to run another arm of the fold (a
// measuring aid: other bits).  False, with nothing launched, for a bad
// shape, split, pointer or a workspace too small.
constexpr int SS_WGRAD_FOLD_WAVES = 4;  // measured: docs/KERNELS.md
bool ss_wgrad_tn_group_ordered(const WgradProblem* problems, int n,
                               const int* splits, void* workspace,
                               size_t bytes, hipStream_t stream,
                               int fold_waves = 0);
// Host only, from the shapes alone: the launches of that call, cut where
// ss_wgrad_group_plan cuts (blocks = those of the partial launch, a
// split of 1 = a single-owner launch of its own), and the workspace
// bytes.  Returns the number of launches, or -1 for a bad shape or split.
int ss_wgrad_group_ordered_plan(const WgradProblem* problems, int n,
                                const int* splits, WgradGroupLaunch* out,
                                size_t* bytes);

// ---- head.hip
bool ss_head_fwd_fused(const void* x, const void* W, const void* bias,
                       void* probs, int M, int K, int C, int rows_per_block,
                       hipStream_t stream);
// loss (here and in the backward chains below): 0 = softmax
// cross-entropy, dz = (p − t)/GB; 1 = softmax squared error, dz =
// p·(g − Σ_c p·g) with g = −2(t − p)/GB; anything else returns false.
// Each loss's kernels live in a translation unit of their own, behind
// the *_xent / *_mse launchers, which take the same arguments and check
// the same contract; callers go through the one that takes `loss`.
bool ss_head_bwd_fused(const void* probs, const void* target, const void* x,
                       const void* Wt, void* dz, void* dx, void* gW, void* gb,
                       int M, int K, int C, float inv_gb, int rows_per_block,
                       void* metrics, int slots, int loss,
                       hipStream_t stream);
bool ss_head_bwd_fused_xent(const void* probs, const void* target,
                            const void* x, const void* Wt, void* dz, void* dx,
                            void* gW, void* gb, int M, int K, int C,
                            float inv_gb, int rows_per_block, void* metrics,
                            int slots, hipStream_t stream);  // head.hip
bool ss_head_bwd_fused_mse(const void* probs, const void* target,
                           const void* x, const void* Wt, void* dz, void* dx,
                           void* gW, void* gb, int M, int K, int C,
                           float inv_gb, int rows_per_block, void* metrics,
                           int slots, hipStream_t stream);  // head_mse.hip
bool ss_head_metrics(const void* probs, const void* target, void* acc,
                     int slots, int M, int C, int kind, hipStream_t stream);

// ---- bwd_chain.hip / bwd_chain_stage.hip
// h / wt / dz: nlayers pointers each, top layer first (post-ReLU output,
// W^T or null where the chain ends, masked gradient out).  dz_scale
// (inverted dropout's 1/keep) scales every dz_l: 1.f is the unscaled
// kernel, any other value is built for the shipped arm only, false for
// the others.
constexpr int SS_BWD_CHAIN_MAX = 8;
bool ss_bwd_chain(const void* probs, const void* target, const void* Wt_head,
                  void* dz_head, const void* const* h, const void* const* wt,
                  void* const* dz, int nlayers, void* dx, int M, int H, int C,
                  float inv_gb, int rows, int waves, int w_lds,
                  float dz_scale, int loss, hipStream_t stream);
// bwd_chain.hip; every arm
bool ss_bwd_chain_xent(const void* probs, const void* target,
                       const void* Wt_head, void* dz_head,
                       const void* const* h, const void* const* wt,
                       void* const* dz, int nlayers, void* dx, int M, int H,
                       int C, float inv_gb, int rows, int waves, int w_lds,
                       float dz_scale, hipStream_t stream);
// bwd_chain_mse.hip; no W-through-LDS arm (w_lds == 1 returns false)
bool ss_bwd_chain_mse(const void* probs, const void* target,
                      const void* Wt_head, void* dz_head,
                      const void* const* h, const void* const* wt,
                      void* const* dz, int nlayers, void* dx, int M, int H,
                      int C, float inv_gb, int rows, int waves, int w_lds,
                      float dz_scale, hipStream_t stream);
// The stage arm, for a pipeline stage with no head: the chain starts
// from dout [M][256], the received gradient of the top layer's output,
// 16-byte aligned.  Everything else as ss_bwd_chain, except that the
// shipped rows are 32 where 64-row tiles would cover at most half of the
// CUs, and the scaled form is built for both eight-wave arms.
bool ss_bwd_chain_stage(const void* dout, const void* const* h,
                        const void* const* wt, void* const* dz, int nlayers,
                        void* dx, int M, int H, int rows, int waves,
                        int w_lds, float dz_scale, hipStream_t stream);

// ---- fwd_chain.hip / fwd_chain_stage.hip
// w / b / h: nlayers pointers each, bottom layer first (W [256][in],
// bias, post-ReLU output).  x is the input of layer 0, [M][K0]; l1
// selects how the chain starts (0 = shipped choice, 1 = from a stored
// 256-wide activation, 2 = the first layer streams x, K0 % 8 == 0).
// kloop selects the K loops (0 = shipped choice, 1 = B one step ahead,
// 2 = B three steps ahead in named register sets; eight waves only).
// zero_ptr / zero_bytes: memory the launch also fills with zeros (the
// step's gradient buffer), 4-B aligned and a multiple of 4 bytes, or
// nullptr / 0.
constexpr int SS_FWD_CHAIN_MAX = 8;
bool ss_fwd_chain(const void* x, const void* const* w, const void* const* b,
                  void* const* h, int nlayers, const void* W_head,
                  const void* b_head, void* probs, int M, int K0, int H, int C,
                  int rows, int waves, int l1, int kloop, void* zero_ptr,
                  long zero_bytes, hipStream_t stream);
// The stage arm, for a pipeline stage with no head: the launch ends with
// h of the top layer.  Same contract, arms and shipped choices.
bool ss_fwd_chain_stage(const void* x, const void* const* w,
                        const void* const* b, void* const* h, int nlayers,
                        int M, int K0, int H, int rows, int waves, int l1,
                        int kloop, hipStream_t stream);

// ---- fwd_chain_drop.hip / fwd_chain_stage_drop.hip
// The two launches above under dropout: layer l's epilogue is
// gemm_nt_kernel<.., DROPOUT>'s, v = keep ? relu(acc + b) * scale : +0
// with one rounding, and the dropped-out tile is the next layer's input.
// Passed by value.  Row i of the launch is sample row_first + i *
// row_stride; layer l draws with counter word layer[l].  Bit l of `on`
// clear (p = 0): that layer runs the plain epilogue and draws nothing.
struct FwdChainDrop {
    unsigned key0, key1, step;  // seed low / high word, counter word 3
    unsigned row_first, row_stride;
    unsigned on;
    unsigned layer[SS_FWD_CHAIN_MAX];
    unsigned thr[SS_FWD_CHAIN_MAX];  // keep when word < thr
    float scale[SS_FWD_CHAIN_MAX];   // float32(1 / (1 - p))
};
// ss_fwd_chain's contract, plus: `on` names at least one layer and none
// at or past nlayers, and the last row's sample id stays below 2^32.
bool ss_fwd_chain_drop(const void* x, const void* const* w,
                       const void* const* b, void* const* h, int nlayers,
                       const void* W_head, const void* b_head, void* probs,
                       int M, int K0, int H, int C, int rows, int waves,
                       int l1, int kloop, void* zero_ptr, long zero_bytes,
                       const FwdChainDrop& drop, hipStream_t stream);
bool ss_fwd_chain_stage_drop(const void* x, const void* const* w,
                             const void* const* b, void* const* h,
                             int nlayers, int M, int K0, int H, int rows,
                             int waves, int l1, int kloop,
                             const FwdChainDrop& drop, hipStream_t stream);

// ---- fwd_chain_wide.hip / bwd_chain_wide.hip
// The headed chains at H = 128 and 512, with ss_fwd_chain's and
// ss_bwd_chain's pointer lists.  The first layer always streams x (any
// K0 % 8 == 0, K0 == H included).  rows / waves: both 0 = the shipped
// arm of (H, M), else one of the pairs built for H: (32, 4), (64, 4) at
// 128; (32, 8), (64, 8), (64, 16) at 512.  No zeroing, no W-through-LDS
// arm.  dz_scale as ss_bwd_chain's, built for every arm.
// Host only: whether (rows, waves) selects an arm built for H (both 0
// does, at H = 128 and 512), so that a caller can refuse before it
// allocates.
bool ss_chain_wide_arm_built(int H, int rows, int waves);
bool ss_fwd_chain_wide(const void* x, const void* const* w,
                       const void* const* b, void* const* h, int nlayers,
                       const void* W_head, const void* b_head, void* probs,
                       int M, int K0, int H, int C, int rows, int waves,
                       hipStream_t stream);
bool ss_bwd_chain_wide(const void* probs, const void* target,
                       const void* Wt_head, void* dz_head,
                       const void* const* h, const void* const* wt,
                       void* const* dz, int nlayers, void* dx, int M, int H,
                       int C, float inv_gb, int rows, int waves,
                       float dz_scale, int loss, hipStream_t stream);
bool ss_bwd_chain_wide_xent(const void* probs, const void* target,
                            const void* Wt_head, void* dz_head,
                            const void* const* h, const void* const* wt,
                            void* const* dz, int nlayers, void* dx, int M,
                            int H, int C, float inv_gb, int rows, int waves,
                            float dz_scale,
                            hipStream_t stream);  // bwd_chain_wide.hip
bool ss_bwd_chain_wide_mse(const void* probs, const void* target,
                           const void* Wt_head, void* dz_head,
                           const void* const* h, const void* const* wt,
                           void* const* dz, int nlayers, void* dx, int M,
                           int H, int C, float inv_gb, int rows, int waves,
                           float dz_scale,
                           hipStream_t stream);  // bwd_chain_wide_mse.hip

// ---- fwd_chain_wide_drop.hip
// ss_fwd_chain_wide under dropout, with fwd_chain_drop.hip's block and
// epilogue: false as well when `on` names no layer or one at or past
// nlayers, when a named layer's scale / threshold is none that a p in
// [0, 1) gives, or when the last row's sample id reaches 2^32.
bool ss_fwd_chain_wide_dropout(const void* x, const void* const* w,
                               const void* const* b, void* const* h,
                               int nlayers, const void* W_head,
                               const void* b_head, void* probs, int M, int K0,
                               int H, int C, int rows, int waves,
                               const FwdChainDrop& drop, hipStream_t stream);

// ---- fwd_chain_wide_stage.hip / fwd_chain_wide_stage_drop.hip /
// bwd_chain_wide_stage.hip
// The stage arms of the wide chains, for a pipeline stage with no head:
// the contract above without the head (H 128 or 512, 1..8 layers, M >= 1,
// K0 >= 8 and K0 % 8 == 0, 16-byte-aligned pointers, a built arm, the last
// layer's wt present exactly when dx is).  The forward ends with h of the
// top layer.  start: 0 = by K0 (K0 == H: x is loaded into the tile and
// layer 0 runs the in-place K loop; else the first layer streams x), 1 =
// streamed, 2 = tile, false unless K0 == H.  The backward starts from
// dout [M][H], the received gradient of the top layer's output.
bool ss_fwd_chain_wide_stage(const void* x, const void* const* w,
                             const void* const* b, void* const* h,
                             int nlayers, int M, int K0, int H, int rows,
                             int waves, int start, hipStream_t stream);
bool ss_fwd_chain_wide_stage_dropout(const void* x, const void* const* w,
                                     const void* const* b, void* const* h,
                                     int nlayers, int M, int K0, int H,
                                     int rows, int waves, int start,
                                     const FwdChainDrop& drop,
                                     hipStream_t stream);
bool ss_bwd_chain_wide_stage(const void* dout, const void* const* h,
                             const void* const* wt, void* const* dz,
                             int nlayers, void* dx, int M, int H, int rows,
                             int waves, float dz_scale, hipStream_t stream);

// ---- fused_mlp.hip
bool ss_fused_mlp_fwd(const void* x, const void* desc, int M, int in_dim,
                      int nhidden, int cout, void* out, hipStream_t stream);

// ---- fused_mlp_wide.hip
// The whole serving forward in one launch for H in {128, 256, 512, 1024}:
// x [M][in_dim] -> H (ReLU) x nhidden -> cout, any M >= 1, any
// in_dim >= 1, 1 <= nhidden <= SS_FUSED_MLP_MAX, 1 <= cout <= 16.
// w / b: nhidden pointers each, bottom layer first (W [H][in], bf16
// bias); w_head [cout][H].  Weights 16-byte aligned.  argmax: int32 [M],
// the lowest index among equal maxima; logits: f32 [M][cout], the values
// the argmax is taken over, or null.  rows / waves: 0 = the shipped
// choice, else one of the arms built for H.
constexpr int SS_FUSED_MLP_MAX = 8;
bool ss_fused_mlp_wide(const void* x, const void* const* w,
                       const void* const* b, int nhidden, const void* w_head,
                       const void* b_head, void* argmax, void* logits, int M,
                       int in_dim, int H, int cout, int rows, int waves,
                       hipStream_t stream);

// ---- fused_mlp_taper.hip
// The same forward for hidden widths that differ from layer to layer:
// x [M][in_dim] -> widths[0] (ReLU) -> .. -> widths[nhidden - 1] (ReLU) ->
// cout, every width one of 128 / 256 / 512 / 1024 (equal ones included).
// w[l] is [widths[l]][widths[l - 1]] ([widths[0]][in_dim] for l = 0),
// w_head [cout][widths[nhidden - 1]]; everything else as above.  False,
// with nothing launched, outside that contract or for a (rows, waves) that
// is not built for the largest width or leaves a wave fewer than 16
// columns of the narrowest layer.
bool ss_fused_mlp_taper(const void* x, const void* const* w,
                        const void* const* b, const int* widths, int nhidden,
                        const void* w_head, const void* b_head, void* argmax,
                        void* logits, int M, int in_dim, int cout, int rows,
                        int waves, hipStream_t stream);

// ---- elementwise.hip
void ss_relu_fwd(const void* x, void* y, long n, hipStream_t stream);
void ss_relu_bwd(const void* dy, const void* y, void* dx, long n,
                 hipStream_t stream);
void ss_relu_bwd_scaled(const void* dy, const void* y, void* dx, long n,
                        float scale, hipStream_t stream);
void ss_dropout_fwd(void* y, int M, int N, const DropoutArgs& drop,
                    hipStream_t stream);
void ss_dropout_mask(const void* sample_ids, void* keep, int M, int N,
                     const DropoutArgs& drop, hipStream_t stream);
void ss_softmax_fwd(const void* x, void* s, int B, int C, hipStream_t stream);
void ss_softmax_bwd(const void* dy, const void* s, void* dx, int B, int C,
                    hipStream_t stream);
void ss_head_mse_bwd(const void* s, const void* t, void* dz, int B, int C,
                     float inv_gb, hipStream_t stream);
void ss_head_xent_bwd(const void* s, const void* t, void* dz, long n,
                      float inv_gb, hipStream_t stream);
void ss_row_argmax(const void* x, void* out, int B, int C,
                   hipStream_t stream);
void ss_transpose_bf16(const void* src, void* dst, int rows, int cols,
                       hipStream_t stream);
void ss_sgd_multi(const void* desc, int ntensors, long total, float lr,
                  float momentum, float weight_decay, hipStream_t stream);
void ss_adamw_multi(const void* desc, int ntensors, long total, float lr,
                    float beta1, float beta2, float omb1, float omb2,
                    float eps, float weight_decay, float inv_bc1,
                    float inv_bc2, hipStream_t stream);
void ss_sgd_multi2(const void* desc, const void* bmap, int nblocks, float lr,
                   float momentum, float weight_decay, hipStream_t stream);
void ss_adamw_multi2(const void* desc, const void* bmap, int nblocks,
                     float lr, float beta1, float beta2, float omb1,
                     float omb2, float eps, float weight_decay,
                     float inv_bc1, float inv_bc2, hipStream_t stream);

// ---- norm.hip
void ss_ln_fwd(const void* x, const void* gamma, const void* beta, void* y,
               void* mean, void* rstd, int B, int C, float eps,
               hipStream_t stream);
void ss_ln_bwd_dx(const void* dy, const void* x, const void* gamma,
                  const void* mean, const void* rstd, void* dx, int B, int C,
                  hipStream_t stream);
void ss_ln_bwd_dparam(const void* dy, const void* x, const void* mean,
                      const void* rstd, void* dgamma, void* dbeta, int B,
                      int C, hipStream_t stream);
void ss_gelu_fwd(const void* z, void* y, long n, hipStream_t stream);
void ss_gelu_bwd(const void* dy, const void* z, void* dz, long n,
                 hipStream_t stream);
