// Python bindings for the shallowspeed_amd HIP/CDNA4 kernels.
//
// Thin torch-extension layer: shape/dtype/contiguity checks + launch on
// the current torch stream.  All compute lives in the .hip files, behind
// the launchers declared in launchers.h.

#include <torch/extension.h>

#include <ATen/cuda/CUDAContext.h>

#include <climits>
#include <optional>
#include <string>

#include "launchers.h"

namespace {

hipStream_t cur_stream() {
    return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

void check_bf16(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_f32(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == torch::kFloat, name, " must be f32");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

bool has(const torch::Tensor& t) { return t.defined() && t.numel() > 0; }

// Optional tensor: null when absent, else checked and its data pointer.
void* opt_bf16(const torch::Tensor& t, const char* name) {
    if (!has(t)) return nullptr;
    check_bf16(t, name);
    return t.data_ptr();
}

void* opt_f32(const torch::Tensor& t, const char* name) {
    if (!has(t)) return nullptr;
    check_f32(t, name);
    return t.data_ptr();
}

// int64 CUDA table of `cols` columns (descriptor rows holding pointers
// and sizes); `what` is the error text.
void check_table(const torch::Tensor& t, int64_t cols, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kLong &&
                    t.is_contiguous() && t.dim() == 2 && t.size(1) == cols,
                what);
}

// Output of an elementwise op: a fresh tensor like `like`, or the
// caller's `out` (bf16, contiguous, same element count; may be a view
// into a larger buffer, which is how the tests watch the elements behind
// the written range).
torch::Tensor out_like(const torch::Tensor& like,
                       const std::optional<torch::Tensor>& out) {
    if (!out.has_value()) return torch::empty_like(like);
    check_bf16(*out, "out");
    TORCH_CHECK(out->numel() == like.numel(), "out must hold ",
                like.numel(), " elements, has ", out->numel());
    return *out;
}

torch::Tensor gemm_nt(torch::Tensor a, torch::Tensor b, torch::Tensor bias,
                      torch::Tensor mask, bool relu) {
    check_bf16(a, "a");
    check_bf16(b, "b");
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "a/b must be 2-D");
    const int M = a.size(0), K = a.size(1), N = b.size(0);
    TORCH_CHECK(b.size(1) == K, "K mismatch: ", K, " vs ", b.size(1));
    const void* bias_p = opt_bf16(bias, "bias");
    TORCH_CHECK(!bias_p || bias.numel() == N, "bias size");
    const void* mask_p = opt_bf16(mask, "mask");
    TORCH_CHECK(!mask_p || mask.sizes() == a.sizes(), "mask must match A");
    auto c = torch::empty({M, N}, a.options());
    ss_gemm_nt(a.data_ptr(), b.data_ptr(), bias_p, mask_p, c.data_ptr(), M, N,
               K, relu, cur_stream());
    return c;
}

// The mask constants as Python passes them (ops/functional.py computes
// thr and scale, the one definition): every field is checked to fit its
// 32 bits, and the launch's last row to stay a 32-bit sample id.
DropoutArgs drop_args(int64_t key0, int64_t key1, int64_t step, int64_t layer,
                      int64_t row_first, int64_t row_stride, int64_t thr,
                      double scale, int64_t rows) {
    auto u32 = [](int64_t v) { return v >= 0 && v <= (int64_t)UINT_MAX; };
    TORCH_CHECK(u32(key0) && u32(key1) && u32(step) && u32(layer) &&
                    u32(row_first) && u32(row_stride) && u32(thr),
                "dropout: seed words, step, layer, rows and thr are 32-bit");
    TORCH_CHECK(rows < 1 ||
                    row_first + (rows - 1) * row_stride <= (int64_t)UINT_MAX,
                "dropout: sample id past 2^32");
    DropoutArgs d;
    d.key0 = (unsigned)key0;
    d.key1 = (unsigned)key1;
    d.layer = (unsigned)layer;
    d.step = (unsigned)step;
    d.row_first = (unsigned)row_first;
    d.row_stride = (unsigned)row_stride;
    d.thr = (unsigned)thr;
    d.scale = (float)scale;
    return d;
}

// C = dropout(relu(a @ b^T + bias)): the fused epilogue where the shape's
// tier has one, else gemm_nt followed by the in-place standalone pass
// (also with fused = false, the measured alternative).
torch::Tensor gemm_nt_dropout(torch::Tensor a, torch::Tensor b,
                              torch::Tensor bias, int64_t key0, int64_t key1,
                              int64_t step, int64_t layer, int64_t row_first,
                              int64_t row_stride, int64_t thr, double scale,
                              bool fused) {
    check_bf16(a, "a");
    check_bf16(b, "b");
    check_bf16(bias, "bias");
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "a/b must be 2-D");
    const int M = a.size(0), K = a.size(1), N = b.size(0);
    TORCH_CHECK(b.size(1) == K, "K mismatch: ", K, " vs ", b.size(1));
    TORCH_CHECK(bias.numel() == N, "bias size");
    const DropoutArgs d = drop_args(key0, key1, step, layer, row_first,
                                    row_stride, thr, scale, M);
    auto c = torch::empty({M, N}, a.options());
    if (fused)
        fused = ss_gemm_nt_dropout(a.data_ptr(), b.data_ptr(),
                                   bias.data_ptr(), c.data_ptr(), M, N, K, d,
                                   cur_stream());
    else
        ss_gemm_nt(a.data_ptr(), b.data_ptr(), bias.data_ptr(), nullptr,
                   c.data_ptr(), M, N, K, true, cur_stream());
    if (!fused) ss_dropout_fwd(c.data_ptr(), M, N, d, cur_stream());
    return c;
}

// y = dropout(y) in place on a finished post-ReLU activation.
void dropout_fwd_(torch::Tensor y, int64_t key0, int64_t key1, int64_t step,
                  int64_t layer, int64_t row_first, int64_t row_stride,
                  int64_t thr, double scale) {
    check_bf16(y, "y");
    TORCH_CHECK(y.dim() == 2, "y must be 2-D");
    const DropoutArgs d = drop_args(key0, key1, step, layer, row_first,
                                    row_stride, thr, scale, y.size(0));
    ss_dropout_fwd(y.data_ptr(), (int)y.size(0), (int)y.size(1), d,
                   cur_stream());
}

// keep[r][c] (bool) for explicit int64 sample ids; the caller has checked
// each id < 2^32.
torch::Tensor dropout_keep_mask(torch::Tensor sample_ids, int64_t ncols,
                                int64_t key0, int64_t key1, int64_t step,
                                int64_t layer, int64_t thr) {
    TORCH_CHECK(sample_ids.is_cuda() &&
                    sample_ids.scalar_type() == torch::kLong &&
                    sample_ids.dim() == 1 && sample_ids.is_contiguous(),
                "sample_ids must be a contiguous CUDA int64 vector");
    TORCH_CHECK(ncols >= 0 && ncols <= INT_MAX &&
                    sample_ids.numel() <= INT_MAX, "mask too large");
    const DropoutArgs d = drop_args(key0, key1, step, layer, 0, 1, thr, 1.0,
                                    0);
    auto keep = torch::empty({sample_ids.numel(), ncols},
                             sample_ids.options().dtype(torch::kBool));
    ss_dropout_mask(sample_ids.data_ptr(), keep.data_ptr(),
                    (int)sample_ids.numel(), (int)ncols, d, cur_stream());
    return keep;
}

// shared body of the two 256-tile wrappers; `tier` names it in the error
torch::Tensor gemm_nt_256_tier(decltype(&ss_gemm_nt_256) launcher,
                               const char* tier, const torch::Tensor& a,
                               const torch::Tensor& b,
                               const torch::Tensor& bias, bool relu) {
    check_bf16(a, "a");
    check_bf16(b, "b");
    const int M = a.size(0), K = a.size(1), N = b.size(0);
    TORCH_CHECK(b.size(1) == K, "K mismatch");
    auto c = torch::empty({M, N}, a.options());
    TORCH_CHECK(launcher(a.data_ptr(), b.data_ptr(), opt_bf16(bias, "bias"),
                         c.data_ptr(), M, N, K, relu, cur_stream()),
                "shape outside the ", tier, " tier: ", M, "x", N, "x", K);
    return c;
}

torch::Tensor gemm_nt_256(torch::Tensor a, torch::Tensor b,
                          torch::Tensor bias, bool relu) {
    return gemm_nt_256_tier(&ss_gemm_nt_256, "256-tile", a, b, bias, relu);
}

torch::Tensor gemm_nt_256w(torch::Tensor a, torch::Tensor b,
                           torch::Tensor bias, bool relu) {
    return gemm_nt_256_tier(&ss_gemm_nt_256w, "256w", a, b, bias, relu);
}

std::vector<torch::Tensor> fp8_quantize(torch::Tensor x) {
    check_bf16(x, "x");
    TORCH_CHECK(x.dim() == 2 && x.size(1) % 128 == 0,
                "x must be 2-D with K % 128 == 0");
    const int R = x.size(0), K = x.size(1);
    auto q = torch::empty({R, K}, x.options().dtype(torch::kUInt8));
    auto s = torch::empty({K / 128, R, 4}, x.options().dtype(torch::kUInt8));
    ss_fp8_quantize(x.data_ptr(), q.data_ptr(), s.data_ptr(), R, K,
                    cur_stream());
    return {q, s};
}

// shared body of the two fp8 GEMM wrappers: bf16 output C, or with
// quantized = true the fused-quantised pair (e4m3 data, e8m0 scales)
std::vector<torch::Tensor> gemm_nt_f8_any(bool quantized,
                                          const torch::Tensor& a,
                                          const torch::Tensor& asc,
                                          const torch::Tensor& b,
                                          const torch::Tensor& bsc,
                                          const torch::Tensor& bias,
                                          bool relu) {
    TORCH_CHECK(a.scalar_type() == torch::kUInt8 &&
                b.scalar_type() == torch::kUInt8, "a/b must be u8 (e4m3)");
    TORCH_CHECK(a.is_contiguous() && b.is_contiguous() &&
                asc.is_contiguous() && bsc.is_contiguous(), "contiguous");
    const int M = a.size(0), K = a.size(1), N = b.size(0);
    TORCH_CHECK(b.size(1) == K, "K mismatch");
    const void* bias_p = opt_bf16(bias, "bias");
    std::vector<torch::Tensor> out;
    bool ok;
    if (quantized) {
        out = {torch::empty({M, N}, a.options()),
               torch::empty({N / 128, M, 4}, a.options())};
        ok = ss_gemm_nt_f8_q(a.data_ptr(), asc.data_ptr(), b.data_ptr(),
                             bsc.data_ptr(), bias_p, out[0].data_ptr(),
                             out[1].data_ptr(), M, N, K, relu, cur_stream());
    } else {
        out = {torch::empty({M, N}, a.options().dtype(torch::kBFloat16))};
        ok = ss_gemm_nt_f8(a.data_ptr(), asc.data_ptr(), b.data_ptr(),
                           bsc.data_ptr(), bias_p, out[0].data_ptr(), M, N, K,
                           relu, cur_stream());
    }
    TORCH_CHECK(ok, "shape outside the fp8 tier: ", M, "x", N, "x", K);
    return out;
}

torch::Tensor gemm_nt_f8(torch::Tensor a, torch::Tensor asc, torch::Tensor b,
                         torch::Tensor bsc, torch::Tensor bias, bool relu) {
    return gemm_nt_f8_any(false, a, asc, b, bsc, bias, relu)[0];
}

std::vector<torch::Tensor> gemm_nt_f8_q(torch::Tensor a, torch::Tensor asc,
                                         torch::Tensor b, torch::Tensor bsc,
                                         torch::Tensor bias, bool relu) {
    return gemm_nt_f8_any(true, a, asc, b, bsc, bias, relu);
}

void wgrad_tn_256(torch::Tensor dy, torch::Tensor x, torch::Tensor gw) {
    check_bf16(dy, "dy");
    check_bf16(x, "x");
    check_f32(gw, "gw");
    const int Kb = dy.size(0), Mo = dy.size(1), N = x.size(1);
    TORCH_CHECK(x.size(0) == Kb, "batch mismatch");
    TORCH_CHECK(gw.size(0) == Mo && gw.size(1) == N, "gw shape");
    TORCH_CHECK(ss_wgrad_tn_256(dy.data_ptr(), x.data_ptr(), gw.data_ptr(),
                                Mo, N, Kb, cur_stream()),
                "shape outside the 256-tile wgrad tier");
}

void wgrad_tn(torch::Tensor dy, torch::Tensor x, torch::Tensor gw,
              torch::Tensor gb, torch::Tensor mask, int64_t split_k,
              int64_t stages) {
    check_bf16(dy, "dy");
    check_bf16(x, "x");
    check_f32(gw, "gw");
    const int Kb = dy.size(0), Mo = dy.size(1), N = x.size(1);
    TORCH_CHECK(x.size(0) == Kb, "batch mismatch");
    TORCH_CHECK(gw.size(0) == Mo && gw.size(1) == N, "gw shape");
    const void* mask_p = opt_bf16(mask, "mask");
    TORCH_CHECK(!mask_p || mask.sizes() == dy.sizes(), "mask must match dy");
    void* gb_p = opt_f32(gb, "gb");
    TORCH_CHECK(!gb_p || gb.numel() == Mo, "gb size");
    TORCH_CHECK(stages >= 0 && stages <= 2, "stages must be 0, 1 or 2");
    // bias grad is FUSED into the wgrad kernel (n-tile-0 blocks sum
    // the already-masked LDS dY tile) — no separate colsum launch or
    // extra dY read on the hot path.
    ss_wgrad_tn(dy.data_ptr(), x.data_ptr(), mask_p, gw.data_ptr(), gb_p, Mo,
                N, Kb, (int)split_k, (int)stages, cur_stream());
}

void wgrad_tn_multi(torch::Tensor chunk_table, int64_t nchunks,
                    bool has_mask, torch::Tensor gw, torch::Tensor gb,
                    int64_t Mo, int64_t N, int64_t kb_chunk,
                    int64_t split_k) {
    // chunk_table: CUDA int64 [nchunks, 3] = {dY*, X*, mask*} per
    // µbatch; all chunks share (Kb, Mo, N).  Deferred-µbatch wgrad:
    // one launch accumulates every chunk into gw/gb.
    check_table(chunk_table, 3, "chunk_table must be CUDA int64 [nchunks,3]");
    TORCH_CHECK(chunk_table.size(0) == nchunks,
                "chunk_table must be CUDA int64 [nchunks,3]");
    check_f32(gw, "gw");
    TORCH_CHECK(gw.size(0) == Mo && gw.size(1) == N, "gw shape");
    void* gb_p = opt_f32(gb, "gb");
    TORCH_CHECK(!gb_p || gb.numel() == Mo, "gb size");
    ss_wgrad_tn_multi(chunk_table.data_ptr(), (int)nchunks, has_mask,
                      gw.data_ptr(), gb_p, (int)Mo, (int)N, (int)kb_chunk,
                      (int)split_k, cur_stream());
}

// Grouped launch.  A problem is (dy, x, gw, gb); gb may be None or empty.
using WgradGroupProblem = std::tuple<torch::Tensor, torch::Tensor,
                                     torch::Tensor,
                                     std::optional<torch::Tensor>>;

std::vector<int> wgrad_group_splits(
    const std::optional<std::vector<int64_t>>& splits, size_t n) {
    std::vector<int> s(n, 0);
    if (!splits) return s;
    TORCH_CHECK(splits->size() == n, "splits: one per problem");
    for (size_t i = 0; i < n; ++i) {
        const int64_t v = (*splits)[i];
        TORCH_CHECK(v == 0 || (v >= 2 && v <= INT_MAX),
                    "split must be 0 (the group rule) or >= 2");
        s[i] = (int)v;
    }
    return s;
}

void wgrad_tn_group(std::vector<WgradGroupProblem> problems,
                    std::optional<std::vector<int64_t>> splits) {
    // every check before the first launch: a refused call touches nothing
    std::vector<WgradProblem> p;
    for (const auto& [dy, x, gw, gb] : problems) {
        check_bf16(dy, "dy");
        check_bf16(x, "x");
        check_f32(gw, "gw");
        TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && gw.dim() == 2,
                    "dy, x, gw must be 2-D");
        const int Kb = dy.size(0), Mo = dy.size(1), N = x.size(1);
        TORCH_CHECK(x.size(0) == Kb, "batch mismatch");
        TORCH_CHECK(gw.size(0) == Mo && gw.size(1) == N, "gw shape");
        void* gb_p = gb ? opt_f32(*gb, "gb") : nullptr;
        TORCH_CHECK(!gb_p || gb->numel() == Mo, "gb size");
        p.push_back({dy.data_ptr(), x.data_ptr(), gw.data_ptr(), gb_p, Mo, N,
                     Kb});
    }
    const std::vector<int> s = wgrad_group_splits(splits, p.size());
    if (p.empty()) return;
    TORCH_CHECK(ss_wgrad_tn_group(p.data(), (int)p.size(), s.data(),
                                  cur_stream()),
                "wgrad_tn_group: bad shape, split or pointer");
}

// The launches wgrad_tn_group makes for these (Kb, Mo, N) shapes: per
// launch (problem indices, splits, block counts).  Host only.
std::vector<std::tuple<std::vector<int64_t>, std::vector<int64_t>,
                       std::vector<int64_t>>>
wgrad_group_plan(std::vector<std::tuple<int64_t, int64_t, int64_t>> shapes,
                 std::optional<std::vector<int64_t>> splits) {
    std::vector<WgradProblem> p;
    for (const auto& [Kb, Mo, N] : shapes) {
        TORCH_CHECK(Kb >= 1 && Mo >= 1 && N >= 1 && Kb <= INT_MAX &&
                        Mo <= INT_MAX && N <= INT_MAX,
                    "shape (Kb, Mo, N)");
        p.push_back({nullptr, nullptr, nullptr, nullptr, (int)Mo, (int)N,
                     (int)Kb});
    }
    const std::vector<int> s = wgrad_group_splits(splits, p.size());
    std::vector<WgradGroupLaunch> plan(p.size());
    const int nl =
        ss_wgrad_group_plan(p.data(), (int)p.size(), s.data(), plan.data());
    TORCH_CHECK(nl >= 0, "wgrad_group_plan: bad shape or split");
    std::vector<std::tuple<std::vector<int64_t>, std::vector<int64_t>,
                           std::vector<int64_t>>> out;
    for (int l = 0; l < nl; ++l) {
        std::vector<int64_t> idx, sp, bl;
        for (int k = 0; k < plan[l].count; ++k) {
            idx.push_back(plan[l].first + k);
            sp.push_back(plan[l].split[k]);
            bl.push_back(plan[l].blocks[k]);
        }
        out.emplace_back(idx, sp, bl);
    }
    return out;
}

torch::Tensor colsum(torch::Tensor dy, torch::Tensor mask) {
    check_bf16(dy, "dy");
    const void* mask_p = opt_bf16(mask, "mask");
    auto gb = torch::zeros({dy.size(1)},
                           dy.options().dtype(torch::kFloat));
    ss_colsum(dy.data_ptr(), mask_p, gb.data_ptr(), dy.size(0), dy.size(1),
              cur_stream());
    return gb;
}

torch::Tensor relu_fwd(torch::Tensor x, std::optional<torch::Tensor> out) {
    check_bf16(x, "x");
    auto y = out_like(x, out);
    ss_relu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), cur_stream());
    return y;
}

torch::Tensor relu_bwd(torch::Tensor dy, torch::Tensor y,
                       std::optional<torch::Tensor> out) {
    check_bf16(dy, "dy");
    check_bf16(y, "y");
    TORCH_CHECK(dy.sizes() == y.sizes(), "shape mismatch");
    auto dx = out_like(dy, out);
    ss_relu_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dy.numel(),
                cur_stream());
    return dx;
}

torch::Tensor relu_bwd_scaled(torch::Tensor dy, torch::Tensor y,
                              double scale,
                              std::optional<torch::Tensor> out) {
    check_bf16(dy, "dy");
    check_bf16(y, "y");
    TORCH_CHECK(dy.sizes() == y.sizes(), "shape mismatch");
    auto dx = out_like(dy, out);
    ss_relu_bwd_scaled(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dy.numel(),
                       (float)scale, cur_stream());
    return dx;
}

torch::Tensor softmax_fwd(torch::Tensor x) {
    check_bf16(x, "x");
    TORCH_CHECK(x.dim() == 2, "x must be 2-D");
    auto s = torch::empty_like(x);
    ss_softmax_fwd(x.data_ptr(), s.data_ptr(), x.size(0), x.size(1),
                   cur_stream());
    return s;
}

torch::Tensor softmax_bwd(torch::Tensor dy, torch::Tensor s) {
    check_bf16(dy, "dy");
    check_bf16(s, "s");
    TORCH_CHECK(dy.sizes() == s.sizes(), "shape mismatch");
    auto dx = torch::empty_like(dy);
    ss_softmax_bwd(dy.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.size(0),
                   dy.size(1), cur_stream());
    return dx;
}

torch::Tensor head_mse_bwd(torch::Tensor s, torch::Tensor t,
                           double global_batch) {
    check_bf16(s, "probs");
    check_bf16(t, "target");
    TORCH_CHECK(s.sizes() == t.sizes(), "shape mismatch");
    auto dz = torch::empty_like(s);
    ss_head_mse_bwd(s.data_ptr(), t.data_ptr(), dz.data_ptr(), s.size(0),
                    s.size(1), (float)(1.0 / global_batch), cur_stream());
    return dz;
}

torch::Tensor head_xent_bwd(torch::Tensor s, torch::Tensor t,
                            double global_batch,
                            std::optional<torch::Tensor> out) {
    check_bf16(s, "probs");
    check_bf16(t, "target");
    TORCH_CHECK(s.sizes() == t.sizes(), "shape mismatch");
    auto dz = out_like(s, out);
    ss_head_xent_bwd(s.data_ptr(), t.data_ptr(), dz.data_ptr(), s.numel(),
                     (float)(1.0 / global_batch), cur_stream());
    return dz;
}

// Metrics accumulator (head.hip): int32 [slots][4], slots a power of
// two; word 0 of a slot holds the bits of an f32.
int check_metrics_acc(const torch::Tensor& acc) {
    TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == torch::kInt &&
                    acc.is_contiguous() && acc.dim() == 2 &&
                    acc.size(1) == 4,
                "metrics accumulator must be CUDA int32 [slots][4]");
    const int64_t slots = acc.size(0);
    TORCH_CHECK(slots >= 1 && slots <= (1 << 20) &&
                    (slots & (slots - 1)) == 0,
                "metrics slots must be a power of two, got ", slots);
    return (int)slots;
}

void check_align16(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, name,
                " must be 16-byte aligned");
}

// Operand of the chain kernels: CUDA, bf16, `dim`-D, contiguous,
// non-empty, 16-byte aligned.  The chain bindings refuse (return [])
// where another binding would raise.
bool plain(const torch::Tensor& t, int64_t dim) {
    return t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
           t.dim() == dim && t.is_contiguous() && t.numel() > 0 &&
           aligned16(t.data_ptr());
}

// Fused classifier head (head.hip): probs = softmax(bf16(x @ w^T + b)).
// rows_per_block: 0 = shipped choice, 32/64/128 = the measured arms.
torch::Tensor head_fwd_fused(torch::Tensor x, torch::Tensor w,
                             torch::Tensor b, int64_t rows_per_block) {
    check_bf16(x, "x");
    check_bf16(w, "w");
    check_bf16(b, "b");
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "x/w must be 2-D");
    const int M = x.size(0), K = x.size(1), C = w.size(0);
    TORCH_CHECK(w.size(1) == K, "K mismatch: ", K, " vs ", w.size(1));
    TORCH_CHECK(b.numel() == C, "bias size");
    check_align16(x, "x");
    check_align16(w, "w");
    auto probs = torch::empty({M, C}, x.options());
    TORCH_CHECK(ss_head_fwd_fused(x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                  probs.data_ptr(), M, K, C,
                                  (int)rows_per_block, cur_stream()),
                "shape outside the fused-head contract (C<=16, K%32==0, "
                "K<=1024): ", M, "x", C, "x", K);
    return probs;
}

// Fused head backward: dz = (probs - target)/GB, dx = dz @ W (w_t is the
// transposed bf16 copy [K][C]); with non-empty grad tensors also
// grad_w += dz^T @ x and grad_b += colsum(dz).  Returns (dz, dx).
std::vector<torch::Tensor> head_bwd_fused(torch::Tensor probs,
                                          torch::Tensor target,
                                          torch::Tensor x, torch::Tensor w_t,
                                          double global_batch,
                                          torch::Tensor grad_w,
                                          torch::Tensor grad_b,
                                          int64_t rows_per_block,
                                          std::optional<torch::Tensor> metrics,
                                          int64_t slots) {
    check_bf16(probs, "probs");
    check_bf16(target, "target");
    check_bf16(x, "x");
    check_bf16(w_t, "w_t");
    TORCH_CHECK(probs.dim() == 2 && x.dim() == 2 && w_t.dim() == 2,
                "probs/x/w_t must be 2-D");
    TORCH_CHECK(probs.sizes() == target.sizes(), "shape mismatch");
    const int M = x.size(0), K = x.size(1), C = probs.size(1);
    TORCH_CHECK(probs.size(0) == M, "batch mismatch");
    TORCH_CHECK(w_t.size(0) == K && w_t.size(1) == C, "w_t must be [K][C]");
    check_align16(x, "x");
    void* gw_p = opt_f32(grad_w, "grad_w");
    TORCH_CHECK(!gw_p || (grad_w.dim() == 2 && grad_w.size(0) == C &&
                          grad_w.size(1) == K), "grad_w shape");
    TORCH_CHECK(gw_p || !has(grad_b), "grad_b given without grad_w");
    void* gb_p = opt_f32(grad_b, "grad_b");
    TORCH_CHECK(!gb_p || grad_b.numel() == C, "grad_b size");
    // metrics: the kernel also adds the batch's metric totals into this
    // accumulator, using its first `slots` slots (0 = all of them)
    void* met_p = nullptr;
    int nslots = 1;
    if (metrics.has_value()) {
        nslots = check_metrics_acc(*metrics);
        if (slots) {
            TORCH_CHECK(slots >= 1 && slots <= nslots &&
                            (slots & (slots - 1)) == 0,
                        "slots must be a power of two <= ", nslots);
            nslots = (int)slots;
        }
        met_p = metrics->data_ptr();
    }
    auto dz = torch::empty_like(probs);
    auto dx = torch::empty({M, K}, x.options());
    TORCH_CHECK(ss_head_bwd_fused(probs.data_ptr(), target.data_ptr(),
                                  x.data_ptr(), w_t.data_ptr(), dz.data_ptr(),
                                  dx.data_ptr(), gw_p, gb_p, M, K, C,
                                  (float)(1.0 / global_batch),
                                  (int)rows_per_block, met_p, nslots,
                                  cur_stream()),
                "shape outside the fused-head contract (C<=16, K%32==0, "
                "K<=1024): ", M, "x", C, "x", K);
    return {dz, dx};
}

// Backward chain (bwd_chain.hip): head backward and the 256-wide ReLU
// layers' data gradients below it in one launch.  hs[l] / w_ts[l], top
// layer first: the layer's post-ReLU output and its W^T; w_ts holds one
// entry per dgrad in the chain, so len(w_ts) is len(hs) (dx of the last
// layer is returned too) or len(hs) - 1 (the chain ends at dz of the
// last layer).  Returns [dz_head, dz_0, ..., dz_{n-1}(, dx)], or an
// EMPTY list, with nothing launched, when the inputs are outside the
// kernel's contract: the caller then takes the per-layer path.
std::vector<torch::Tensor> bwd_chain(torch::Tensor probs, torch::Tensor target,
                                     torch::Tensor w_head_t,
                                     double global_batch,
                                     std::vector<torch::Tensor> hs,
                                     std::vector<torch::Tensor> w_ts,
                                     int64_t rows, int64_t waves,
                                     int64_t w_lds, double dz_scale) {
    const int64_t n = (int64_t)hs.size();
    const int64_t nw = (int64_t)w_ts.size();
    if (n < 1 || n > SS_BWD_CHAIN_MAX || (nw != n && nw != n - 1)) return {};
    if (!plain(probs, 2) || !plain(target, 2) || !plain(w_head_t, 2))
        return {};
    if (probs.sizes() != target.sizes()) return {};
    const int64_t M = probs.size(0), C = probs.size(1), H = w_head_t.size(0);
    if (M < 1 || M > INT_MAX / 512 || w_head_t.size(1) != C) return {};
    const void* hp[SS_BWD_CHAIN_MAX] = {};
    const void* wp[SS_BWD_CHAIN_MAX] = {};
    void* dp[SS_BWD_CHAIN_MAX] = {};
    for (int64_t l = 0; l < n; ++l) {
        if (!plain(hs[l], 2) || hs[l].size(0) != M || hs[l].size(1) != H)
            return {};
        hp[l] = hs[l].data_ptr();
        if (l < nw) {
            if (!plain(w_ts[l], 2) || w_ts[l].size(0) != H ||
                w_ts[l].size(1) != H)
                return {};
            wp[l] = w_ts[l].data_ptr();
        }
    }
    std::vector<torch::Tensor> out;
    out.push_back(torch::empty_like(probs));
    for (int64_t l = 0; l < n; ++l) {
        out.push_back(torch::empty_like(hs[l]));
        dp[l] = out.back().data_ptr();
    }
    void* dx_p = nullptr;
    if (nw == n) {
        out.push_back(torch::empty_like(hs[n - 1]));
        dx_p = out.back().data_ptr();
    }
    if (!ss_bwd_chain(probs.data_ptr(), target.data_ptr(),
                      w_head_t.data_ptr(), out[0].data_ptr(), hp, wp, dp,
                      (int)n, dx_p, (int)M, (int)H, (int)C,
                      (float)(1.0 / global_batch), (int)rows, (int)waves,
                      (int)w_lds, (float)dz_scale, cur_stream()))
        return {};
    return out;
}

// Forward chain (fwd_chain.hip): the 256-wide ReLU layers under the
// head and the fused head in one launch.  ws[l] / bs[l], bottom layer
// first; x is the input of layer 0 (256 wide, or any multiple of 8 when
// the first layer streams it).  Returns [h_0, ..., h_{n-1}, probs], or
// an EMPTY list, with nothing allocated or launched, when the inputs are
// outside the kernel's contract: the caller then takes the per-layer
// path.  zero: a contiguous f32 tensor on x's device that the launch
// also fills with zeros (the step's flat gradient buffer), or None; it
// is left untouched when the launch is refused.
std::vector<torch::Tensor> fwd_chain(torch::Tensor x,
                                     std::vector<torch::Tensor> ws,
                                     std::vector<torch::Tensor> bs,
                                     torch::Tensor w_head,
                                     torch::Tensor b_head, int64_t rows,
                                     int64_t waves, int64_t l1,
                                     int64_t kloop,
                                     std::optional<torch::Tensor> zero) {
    constexpr int64_t H = 256;
    const int64_t n = (int64_t)ws.size();
    if (n < 1 || n > SS_FWD_CHAIN_MAX || (int64_t)bs.size() != n) return {};
    if (kloop < 0 || kloop > 2) return {};
    void* zero_p = nullptr;
    int64_t zero_bytes = 0;
    if (zero.has_value() && zero->defined() && zero->numel() > 0) {
        if (zero->scalar_type() != torch::kFloat32 || !zero->is_contiguous() ||
            zero->device() != x.device())
            return {};
        zero_p = zero->data_ptr();
        zero_bytes = zero->numel() * 4;
    }
    if (!plain(x, 2) || !plain(w_head, 2) || !plain(b_head, 1)) return {};
    const int64_t M = x.size(0), K0 = x.size(1), C = w_head.size(0);
    if (M > INT_MAX / 1024 || K0 % 8 != 0 || C > 16 ||
        w_head.size(1) != H || b_head.numel() != C)
        return {};
    if ((rows != 0 && rows != 32 && rows != 64) ||
        (waves != 0 && waves != 4 && waves != 8) || l1 < 0 || l1 > 2 ||
        (l1 == 1 && K0 != H))
        return {};
    const void* wp[SS_FWD_CHAIN_MAX] = {};
    const void* bp[SS_FWD_CHAIN_MAX] = {};
    void* hp[SS_FWD_CHAIN_MAX] = {};
    for (int64_t l = 0; l < n; ++l) {
        if (!plain(ws[l], 2) || !plain(bs[l], 1) || ws[l].size(0) != H ||
            ws[l].size(1) != (l == 0 ? K0 : H) || bs[l].numel() != H)
            return {};
        wp[l] = ws[l].data_ptr();
        bp[l] = bs[l].data_ptr();
    }
    std::vector<torch::Tensor> out;
    for (int64_t l = 0; l < n; ++l) {
        out.push_back(torch::empty({M, H}, x.options()));
        hp[l] = out.back().data_ptr();
    }
    out.push_back(torch::empty({M, C}, x.options()));
    if (!ss_fwd_chain(x.data_ptr(), wp, bp, hp, (int)n, w_head.data_ptr(),
                      b_head.data_ptr(), out.back().data_ptr(), (int)M,
                      (int)K0, (int)H, (int)C, (int)rows, (int)waves, (int)l1,
                      (int)kloop, zero_p, (long)zero_bytes, cur_stream()))
        return {};
    return out;
}

// Adds the metric totals of (probs, target) into acc: loss_sum (kind
// "xent" or "mse"), argmax matches, rows, non-finite rows.
void head_metrics(torch::Tensor probs, torch::Tensor target,
                  torch::Tensor acc, const std::string& kind) {
    check_bf16(probs, "probs");
    check_bf16(target, "target");
    TORCH_CHECK(probs.dim() == 2 && probs.sizes() == target.sizes(),
                "probs/target must be 2-D of one shape");
    TORCH_CHECK(kind == "xent" || kind == "mse", "kind must be xent or mse");
    const int slots = check_metrics_acc(acc);
    TORCH_CHECK(probs.size(0) >= 1 && probs.size(1) >= 1 &&
                    probs.size(0) <= INT_MAX && probs.size(1) <= INT_MAX,
                "empty or oversized probs");
    TORCH_CHECK(ss_head_metrics(probs.data_ptr(), target.data_ptr(),
                                acc.data_ptr(), slots, (int)probs.size(0),
                                (int)probs.size(1), kind == "mse" ? 1 : 0,
                                cur_stream()),
                "head_metrics launch rejected");
}

std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor gamma,
                                  torch::Tensor beta, double eps) {
    check_bf16(x, "x");
    check_bf16(gamma, "gamma");
    check_bf16(beta, "beta");
    TORCH_CHECK(x.dim() == 2, "x must be 2-D");
    const int B = x.size(0), C = x.size(1);
    TORCH_CHECK(gamma.numel() == C && beta.numel() == C, "param size");
    auto y = torch::empty_like(x);
    auto mean = torch::empty({B}, x.options().dtype(torch::kFloat));
    auto rstd = torch::empty({B}, x.options().dtype(torch::kFloat));
    ss_ln_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
              mean.data_ptr(), rstd.data_ptr(), B, C, (float)eps,
              cur_stream());
    return {y, mean, rstd};
}

torch::Tensor ln_bwd_dx(torch::Tensor dy, torch::Tensor x,
                        torch::Tensor gamma, torch::Tensor mean,
                        torch::Tensor rstd) {
    check_bf16(dy, "dy");
    check_bf16(x, "x");
    check_bf16(gamma, "gamma");
    check_f32(mean, "mean");
    check_f32(rstd, "rstd");
    auto dx = torch::empty_like(dy);
    ss_ln_bwd_dx(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(),
                 mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dy.size(0),
                 dy.size(1), cur_stream());
    return dx;
}

void ln_bwd_dparam(torch::Tensor dy, torch::Tensor x, torch::Tensor mean,
                   torch::Tensor rstd, torch::Tensor dgamma,
                   torch::Tensor dbeta) {
    check_bf16(dy, "dy");
    check_bf16(x, "x");
    check_f32(dgamma, "dgamma");
    check_f32(dbeta, "dbeta");
    ss_ln_bwd_dparam(dy.data_ptr(), x.data_ptr(), mean.data_ptr(),
                     rstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                     dy.size(0), dy.size(1), cur_stream());
}

torch::Tensor gelu_fwd(torch::Tensor z, std::optional<torch::Tensor> out) {
    check_bf16(z, "z");
    auto y = out_like(z, out);
    ss_gelu_fwd(z.data_ptr(), y.data_ptr(), z.numel(), cur_stream());
    return y;
}

torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor z,
                       std::optional<torch::Tensor> out) {
    check_bf16(dy, "dy");
    check_bf16(z, "z");
    TORCH_CHECK(dy.sizes() == z.sizes(), "shape mismatch");
    auto dz = out_like(dy, out);
    ss_gelu_bwd(dy.data_ptr(), z.data_ptr(), dz.data_ptr(), dy.numel(),
                cur_stream());
    return dz;
}

torch::Tensor row_argmax(torch::Tensor x) {
    check_bf16(x, "x");
    TORCH_CHECK(x.dim() == 2, "x must be 2-D");
    auto out = torch::empty({x.size(0)}, x.options().dtype(torch::kInt));
    ss_row_argmax(x.data_ptr(), out.data_ptr(), x.size(0), x.size(1),
                  cur_stream());
    return out;
}

void sgd_multi(torch::Tensor desc, double lr, int64_t total,
               double momentum, double weight_decay) {
    // total passed by the caller (cached host-side) — no device sync.
    check_table(desc, 8, "desc must be CUDA int64 [T,8]");
    ss_sgd_multi(desc.data_ptr(), (int)desc.size(0), (long)total, (float)lr,
                 (float)momentum, (float)weight_decay, cur_stream());
}

// omb1 / omb2 are 1 - beta1 / 1 - beta2 as the caller formed them in
// double: rounded once here, never recomputed from the f32 betas.
void adamw_multi(torch::Tensor desc, double lr, int64_t total, double beta1,
                 double beta2, double omb1, double omb2, double eps,
                 double weight_decay, double inv_bc1, double inv_bc2) {
    check_table(desc, 9, "desc must be CUDA int64 [T,9]");
    ss_adamw_multi(desc.data_ptr(), (int)desc.size(0), (long)total,
                   (float)lr, (float)beta1, (float)beta2, (float)omb1,
                   (float)omb2, (float)eps, (float)weight_decay,
                   (float)inv_bc1, (float)inv_bc2, cur_stream());
}

void sgd_multi2(torch::Tensor desc, torch::Tensor bmap, double lr,
                double momentum, double weight_decay) {
    check_table(desc, 8, "desc must be CUDA int64 [T,8]");
    check_table(bmap, 2, "bmap must be CUDA int64 [B,2]");
    ss_sgd_multi2(desc.data_ptr(), bmap.data_ptr(), (int)bmap.size(0),
                  (float)lr, (float)momentum, (float)weight_decay,
                  cur_stream());
}

void adamw_multi2(torch::Tensor desc, torch::Tensor bmap, double lr,
                  double beta1, double beta2, double omb1, double omb2,
                  double eps, double weight_decay, double inv_bc1,
                  double inv_bc2) {
    check_table(desc, 9, "desc must be CUDA int64 [T,9]");
    check_table(bmap, 2, "bmap must be CUDA int64 [B,2]");
    ss_adamw_multi2(desc.data_ptr(), bmap.data_ptr(), (int)bmap.size(0),
                    (float)lr, (float)beta1, (float)beta2, (float)omb1,
                    (float)omb2, (float)eps, (float)weight_decay,
                    (float)inv_bc1, (float)inv_bc2, cur_stream());
}

torch::Tensor fused_mlp_argmax(torch::Tensor x, torch::Tensor desc,
                               int64_t in_dim, int64_t nhidden,
                               int64_t cout) {
    check_bf16(x, "x");
    TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == torch::kLong &&
                    desc.is_contiguous() &&
                    desc.numel() == (nhidden + 1) * 2,
                "desc must be CUDA int64 [(nhidden+1)*2]");
    const int M = x.size(0);
    TORCH_CHECK(x.size(1) == in_dim, "in_dim mismatch");
    auto out = torch::empty({M}, x.options().dtype(torch::kInt32));
    TORCH_CHECK(ss_fused_mlp_fwd(x.data_ptr(), desc.data_ptr(), M,
                                 (int)in_dim, (int)nhidden, (int)cout,
                                 out.data_ptr(), cur_stream()),
                "shape outside the fused-MLP tier");
    return out;
}

void transpose_bf16(torch::Tensor src, torch::Tensor dst) {
    check_bf16(src, "src");
    check_bf16(dst, "dst");
    const int rows = src.size(0), cols = src.size(1);
    TORCH_CHECK(src.dim() == 2 && dst.dim() == 2 &&
                    dst.size(0) == cols && dst.size(1) == rows &&
                    rows % 64 == 0 && cols % 64 == 0,
                "transpose_bf16 needs 64-aligned 2-D shapes");
    ss_transpose_bf16(src.data_ptr(), dst.data_ptr(), rows, cols,
                      cur_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("gemm_nt", &gemm_nt, "C = A @ B^T (+bias)(+relu) with optional A-mask");
    m.def("gemm_nt_256", &gemm_nt_256,
          "256-tile 8-phase GEMM (M%256==N%256==K%128==0)");
    m.def("gemm_nt_256w", &gemm_nt_256w,
          "256-tile 8-phase GEMM, 4-wave 128x128-wave-tile variant");
    m.def("wgrad_tn_256", &wgrad_tn_256,
          "256-tile 8-phase wgrad: gw += dy^T @ x (no mask/bias)");
    m.def("fp8_quantize", &fp8_quantize,
          "bf16 [R,K] -> (e4m3 u8 [R,K], e8m0 scales [K/128,R,4])");
    m.def("gemm_nt_f8", &gemm_nt_f8,
          "MX-fp8 256-tile GEMM: C=bf16(A@B^T) (+bias)(+relu)");
    m.def("gemm_nt_f8_q", &gemm_nt_f8_q,
          "MX-fp8 GEMM with FUSED output quantization -> (e4m3, scales)");
    m.def("wgrad_tn", &wgrad_tn,
          "gW += (dy⊙mask)^T @ x; gb += colsum (fused); stages = LDS "
          "staging sets of the K loop (0 = the launcher's choice)",
          py::arg("dy"), py::arg("x"), py::arg("gw"), py::arg("gb"),
          py::arg("mask"), py::arg("split_k"), py::arg("stages") = 0);
    m.def("wgrad_tn_group", &wgrad_tn_group,
          "unmasked wgrads of a list of (dy, x, gw, gb): consecutive "
          "problems of one tile configuration share a launch",
          py::arg("problems"), py::arg("splits") = py::none());
    m.def("wgrad_group_plan", &wgrad_group_plan,
          "launches of wgrad_tn_group for (Kb, Mo, N) shapes: per launch "
          "(problem indices, splits, block counts)",
          py::arg("shapes"), py::arg("splits") = py::none());
    m.def("colsum", &colsum, "standalone column sum (bias grad)");
    m.def("wgrad_tn_multi", &wgrad_tn_multi,
          "chunked (deferred-µbatch) wgrad: one launch, many (dy,x) pairs");
    m.def("relu_fwd", &relu_fwd, py::arg("x"), py::arg("out") = py::none());
    m.def("relu_bwd", &relu_bwd, py::arg("dy"), py::arg("y"),
          py::arg("out") = py::none());
    m.def("relu_bwd_scaled", &relu_bwd_scaled,
          "dz = bf16(dy * scale) where y > 0, else +0", py::arg("dy"),
          py::arg("y"), py::arg("scale"), py::arg("out") = py::none());
    m.def("gemm_nt_dropout", &gemm_nt_dropout,
          "C = dropout(relu(A @ B^T + bias)), mask in the GEMM epilogue",
          py::arg("a"), py::arg("b"), py::arg("bias"), py::arg("key0"),
          py::arg("key1"), py::arg("step"), py::arg("layer"),
          py::arg("row_first"), py::arg("row_stride"), py::arg("thr"),
          py::arg("scale"), py::arg("fused") = true);
    m.def("dropout_fwd_", &dropout_fwd_,
          "in-place dropout of a finished post-ReLU activation");
    m.def("dropout_keep_mask", &dropout_keep_mask,
          "keep bits (bool [M][ncols]) for explicit sample ids");
    m.def("softmax_fwd", &softmax_fwd);
    m.def("softmax_bwd", &softmax_bwd);
    m.def("head_mse_bwd", &head_mse_bwd);
    m.def("head_xent_bwd", &head_xent_bwd, py::arg("probs"),
          py::arg("target"), py::arg("global_batch"),
          py::arg("out") = py::none());
    m.def("head_fwd_fused", &head_fwd_fused,
          "fused head forward: softmax(bf16(x @ w^T + b))", py::arg("x"),
          py::arg("w"), py::arg("b"), py::arg("rows_per_block") = 0);
    m.def("head_bwd_fused", &head_bwd_fused,
          "fused head backward -> (dz, dx); optional gW/gb accumulate",
          py::arg("probs"), py::arg("target"), py::arg("x"), py::arg("w_t"),
          py::arg("global_batch"), py::arg("grad_w"), py::arg("grad_b"),
          py::arg("rows_per_block") = 0,
          py::arg("metrics") = py::none(), py::arg("slots") = 0);
    m.def("bwd_chain", &bwd_chain,
          "head backward + 256-wide ReLU dgrads in one launch -> "
          "[dz_head, dz_l..., (dx)], or [] outside the contract",
          py::arg("probs"), py::arg("target"), py::arg("w_head_t"),
          py::arg("global_batch"), py::arg("hs"), py::arg("w_ts"),
          py::arg("rows") = 0, py::arg("waves") = 0, py::arg("w_lds") = 0,
          py::arg("dz_scale") = 1.0);
    m.def("fwd_chain", &fwd_chain,
          "256-wide ReLU layers + fused head forward in one launch -> "
          "[h_l..., probs], or [] outside the contract",
          py::arg("x"), py::arg("ws"), py::arg("bs"), py::arg("w_head"),
          py::arg("b_head"), py::arg("rows") = 0, py::arg("waves") = 0,
          py::arg("l1") = 0, py::arg("kloop") = 0,
          py::arg("zero") = py::none());
    m.def("head_metrics", &head_metrics,
          "metric totals of (probs, target) into a slotted accumulator",
          py::arg("probs"), py::arg("target"), py::arg("acc"),
          py::arg("kind") = "xent");
    m.def("sgd_multi", &sgd_multi);
    m.def("adamw_multi", &adamw_multi);
    m.def("transpose_bf16", &transpose_bf16);
    m.def("sgd_multi2", &sgd_multi2);
    m.def("adamw_multi2", &adamw_multi2);
    m.def("fused_mlp_argmax", &fused_mlp_argmax,
          "persistent fused MLP forward + per-row argmax (serving)");
    m.def("ln_fwd", &ln_fwd);
    m.def("ln_bwd_dx", &ln_bwd_dx);
    m.def("ln_bwd_dparam", &ln_bwd_dparam);
    m.def("gelu_fwd", &gelu_fwd, py::arg("z"), py::arg("out") = py::none());
    m.def("gelu_bwd", &gelu_bwd, py::arg("dy"), py::arg("z"),
          py::arg("out") = py::none());
    m.def("row_argmax", &row_argmax);
}
