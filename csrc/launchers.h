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

// ---- head.hip
bool ss_head_fwd_fused(const void* x, const void* W, const void* bias,
                       void* probs, int M, int K, int C, int rows_per_block,
                       hipStream_t stream);
bool ss_head_bwd_fused(const void* probs, const void* target, const void* x,
                       const void* Wt, void* dz, void* dx, void* gW, void* gb,
                       int M, int K, int C, float inv_gb, int rows_per_block,
                       void* metrics, int slots, hipStream_t stream);
bool ss_head_metrics(const void* probs, const void* target, void* acc,
                     int slots, int M, int C, int kind, hipStream_t stream);

// ---- bwd_chain.hip
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
                  float dz_scale, hipStream_t stream);

// ---- fwd_chain.hip
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

// ---- fused_mlp.hip
bool ss_fused_mlp_fwd(const void* x, const void* desc, int M, int in_dim,
                      int nhidden, int cout, void* out, hipStream_t stream);

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
