"""Stateless math ops, dual-backend.

Reference: shallowspeed/functional.py:4-44 — 8 pure NumPy functions
(linear/relu/softmax/mse + grads).  Here every op has

  * a CPU reference implementation in plain torch float32 — used by
    host-only tests and as the numerics oracle for the HIP kernels, and
  * a GPU implementation dispatching to the in-tree HIP/CDNA4 extension
    (csrc/) — MFMA bf16 GEMMs, fused epilogues.  On a CUDA/HIP device
    the extension is REQUIRED: there is no silent torch fallback.

Differences from the reference, by design:
  * reference softmax uses a GLOBAL max and a +1e-7 denominator fudge
    (functional.py:26); we use the correct per-row max and exact rowsum.
  * the backward of the loss head is fused: softmax∘MSE and
    softmax∘cross-entropy each produce d(logits) in one op instead of
    chaining mse_loss_grad (functional.py:43-44) through softmax_grad
    (functional.py:30-35).
"""

import functools

import torch

from ._ext import load_ext


_DETERMINISTIC = False


def set_deterministic(flag: bool):
    """Bitwise run-to-run reproducible GPU training.

    Forces the single-owner (split_k=1) wgrad path so f32 atomicAdd
    ARRIVAL ORDER cannot perturb gradient bits; all other hot kernels
    (fwd/dgrad GEMMs, fused SGD, loss heads) are deterministic by
    construction (fixed tile ownership, no atomics), and the DP bucket
    all-reduce order is fixed by construction in GradReducer.  Matches
    the reference's exact-equality replica gate (train.py:154-155) at
    the bitwise level on GPU.  Costs wgrad parallelism on small-M
    shapes (split-K is what fills the chip there) — opt-in via
    --deterministic."""
    global _DETERMINISTIC
    _DETERMINISTIC = bool(flag)


def deterministic() -> bool:
    return _DETERMINISTIC


_HEAD_FUSED = None


def set_head_fused(flag: bool):
    """Run the classifier head (last Linear + softmax-cross-entropy) as
    the two fused kernels of csrc/head.hip instead of the six-launch
    chain.  probs, dz and dx are bit-identical either way; the head's
    own gW/gb differ in f32 summation order only.  Default on;
    SS_HEAD_FUSED=0 (read once) turns it off."""
    global _HEAD_FUSED
    _HEAD_FUSED = bool(flag)


def head_fused() -> bool:
    global _HEAD_FUSED
    if _HEAD_FUSED is None:
        import os

        _HEAD_FUSED = os.environ.get("SS_HEAD_FUSED", "1") != "0"
    return _HEAD_FUSED


_HEAD_WGRAD_FUSED = None


def set_head_wgrad_fused(flag: bool):
    """Let the fused head backward also accumulate the head's gW/gb
    (one f32 atomic set per block).  Default OFF: at the flagship shape
    that is 256 partial sums per gradient element, and same-address f32
    atomics complete one after another (~50 ns each, measured), so the
    existing wgrad_tn launch (64 partials) is faster end to end — see
    docs/KERNELS.md.  SS_HEAD_WGRAD_FUSED=1 (read once) turns it on."""
    global _HEAD_WGRAD_FUSED
    _HEAD_WGRAD_FUSED = bool(flag)


def head_wgrad_fused() -> bool:
    global _HEAD_WGRAD_FUSED
    if _HEAD_WGRAD_FUSED is None:
        import os

        _HEAD_WGRAD_FUSED = os.environ.get("SS_HEAD_WGRAD_FUSED", "0") == "1"
    return _HEAD_WGRAD_FUSED


_BWD_CHAIN = None


def set_bwd_chain(flag: bool):
    """Run the head backward and the 256-wide ReLU layers' data
    gradients below it as the one kernel of csrc/bwd_chain.hip (see
    bwd_chain).  Every dz and dx keeps its bits; the weight gradients
    then run unmasked on dz.  Default on; SS_BWD_CHAIN=0 (read once)
    turns it off."""
    global _BWD_CHAIN
    _BWD_CHAIN = bool(flag)


def bwd_chain_enabled() -> bool:
    global _BWD_CHAIN
    if _BWD_CHAIN is None:
        import os

        _BWD_CHAIN = os.environ.get("SS_BWD_CHAIN", "1") != "0"
    return _BWD_CHAIN


_BWD_CHAIN_DZ_LAST = None


def bwd_chain_dz_last() -> bool:
    """Whether the chain also takes a last layer whose dgrad it does not
    run (the flagship's first layer), emitting that layer's dz so its
    wgrad runs unmasked.  Off (SS_BWD_CHAIN_DZ1=0, read once: the
    measured alternative), the chain ends at dh of that layer, which
    keeps today's masked backward."""
    global _BWD_CHAIN_DZ_LAST
    if _BWD_CHAIN_DZ_LAST is None:
        import os

        _BWD_CHAIN_DZ_LAST = os.environ.get("SS_BWD_CHAIN_DZ1", "1") != "0"
    return _BWD_CHAIN_DZ_LAST


_FWD_CHAIN = None


def set_fwd_chain(flag: bool):
    """Run the 256-wide ReLU layers under the fused head and the head
    forward as the one kernel of csrc/fwd_chain.hip (see fwd_chain).
    Every h_l and probs keeps its bits.  Default on; SS_FWD_CHAIN=0
    (read once) turns it off."""
    global _FWD_CHAIN
    _FWD_CHAIN = bool(flag)


def fwd_chain_enabled() -> bool:
    global _FWD_CHAIN
    if _FWD_CHAIN is None:
        import os

        _FWD_CHAIN = os.environ.get("SS_FWD_CHAIN", "1") != "0"
    return _FWD_CHAIN


_FWD_CHAIN_L1 = None


def fwd_chain_l1() -> bool:
    """Whether the forward chain also takes a lowest layer that is not
    256 wide at its input (the flagship's 784-wide first layer),
    streaming x through LDS.  Default on.  Off (SS_FWD_CHAIN_L1=0, read
    once: the measured alternative), that layer stays a gemm_nt launch
    and the chain starts from its stored output."""
    global _FWD_CHAIN_L1
    if _FWD_CHAIN_L1 is None:
        import os

        _FWD_CHAIN_L1 = os.environ.get("SS_FWD_CHAIN_L1", "1") != "0"
    return _FWD_CHAIN_L1


_FWD_ZERO_GRADS = None


def fwd_zero_grads() -> bool:
    """Whether Sequential.zero_grad(defer=True) may leave the memset of
    the flat gradient buffer to the next forward chain launch.  Default
    OFF, SS_FWD_ZERO_GRADS=1 (read once) turns it on: at the flagship it
    measured 2.4 us of a 124 us step, 7 kernels instead of 8, every run
    faster than every run without it, but under the bar of five times
    the run-to-run spread that a change has to clear to ship switched on
    (profiles/r14_fwd_loader.md section 5)."""
    global _FWD_ZERO_GRADS
    if _FWD_ZERO_GRADS is None:
        import os

        _FWD_ZERO_GRADS = os.environ.get("SS_FWD_ZERO_GRADS", "0") == "1"
    return _FWD_ZERO_GRADS


def _is_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _ext_for(t: torch.Tensor):
    return load_ext(required=True) if _is_gpu(t) else None


# ---------------------------------------------------------------- linear

def linear_fwd(x, w, b=None, relu=False):
    """y = x @ W^T (+ b) (+ ReLU).

    x: (M, K); w: (N, K) row-major ("NT" GEMM — both operands row-major
    with contiguous K, the natural MFMA layout); b: (N,) or None.
    Reference: functional.py:13-17 with the module-level fused ReLU of
    layers.py:120-122 moved into the GEMM epilogue.
    """
    if _is_gpu(x):
        ext = _ext_for(x)
        empty = torch.Tensor()
        return ext.gemm_nt(x, w, b if b is not None else empty, empty, bool(relu))
    y = x @ w.t()
    if b is not None:
        y = y + b
    if relu:
        y = torch.clamp(y, min=0)
    return y


def fp8_quantize(x):
    """bf16 (R, K) -> (e4m3 u8 data (R, K), E8M0 scales (K/128, R, 4)).

    MX block quantization matching the gfx950 scaled-MFMA's hardware
    scale-group partition (csrc/fp8.hip; probes in
    scripts/probe_mx*.hip).  GPU only; K % 128 == 0.
    """
    return _ext_for(x).fp8_quantize(x)


def linear_fwd_fp8(xq, xs, wq, ws, b=None, relu=False):
    """y = dequant(xq) @ dequant(wq)^T (+ b)(+ ReLU) on the MX-fp8
    scaled-MFMA tier (~1.7x the bf16 8-phase kernel).  Opt-in serving
    precision (beyond the reference's scope); shapes must satisfy
    M%256 == N%256 == 0, K%256 == 0."""
    ext = _ext_for(xq)
    empty = torch.Tensor()
    return ext.gemm_nt_f8(xq, xs, wq, ws, b if b is not None else empty,
                          bool(relu))


def linear_dgrad(dy, w, w_t=None, mask_src=None):
    """dx = (dy ⊙ 1[mask_src>0]) @ W.

    The ReLU backward (reference functional.py:8-10, layers.py:75) is
    fused into the GEMM A-operand read: when mask_src (the stashed
    post-ReLU output of THIS layer) is given, dy elements where
    mask_src<=0 are zeroed during LDS staging.

    GPU path multiplies by the transposed bf16 weight copy w_t ((K, N)
    row-major) so the kernel is the same NT GEMM as the forward;
    w_t is maintained by the fused SGD step.
    Reference: functional.py:20-21 first return value.
    """
    if _is_gpu(dy):
        ext = _ext_for(dy)
        assert w_t is not None, "GPU dgrad needs the transposed weight copy"
        # Tiered dispatch: a PLAIN wide dgrad (no mask, no epilogue) is
        # exactly the "plain library GEMM" case where hipBLASLt belongs
        # — measured 1362-1665 TF vs our 256-tile kernel's 1155-1305 at
        # >=1024-wide shapes (scripts/test_gemm256.py ladder); at the
        # flagship 256-wide shapes our kernel wins and keeps the lane.
        # Fused ops (bias/ReLU epilogues, mask prologue, wgrad's f32
        # atomic accumulate) always stay on the HIP kernels.
        M, O = dy.shape
        if (mask_src is None and not _DETERMINISTIC
                and M >= 2048 and O >= 1024 and w.shape[1] >= 1024
                and _dgrad_lib_enabled()):
            # NT layout: w_t is (I, O) row-major (K=O contiguous), so
            # w_t.t() presents hipBLASLt the transposed-B problem — the
            # fast MFMA-native layout (NN with a row-major B measured
            # only ~+1% end-to-end; NT is the library's 1.4-1.66 PF lane)
            return torch.matmul(dy, w_t.t())
        empty = torch.Tensor()
        return ext.gemm_nt(dy, w_t, empty, mask_src if mask_src is not None else empty, False)
    if mask_src is not None:
        dy = dy * (mask_src > 0).to(dy.dtype)
    return dy @ w


_DGRAD_LIB = None


def _dgrad_lib_enabled() -> bool:
    global _DGRAD_LIB
    if _DGRAD_LIB is None:
        import os

        _DGRAD_LIB = os.environ.get("SS_DGRAD_LIB", "1") == "1"
    return _DGRAD_LIB


def linear_wgrad_acc(dy, x, grad_w, grad_b=None, mask_src=None, split_k=0):
    """grad_w += (dy ⊙ mask)^T @ x ; grad_b += colsum(dy ⊙ mask).

    Accumulates IN PLACE into f32 grad buffers — this is how both
    µbatch gradient accumulation (reference layers.py:135-136) and
    split-K parallelism work: the GPU kernel uses f32 atomicAdd, so a
    K-split over the batch dimension and accumulation across µbatches
    compose for free.  split_k=0 lets the kernel pick; split_k=1 is the
    deterministic single-owner path (forced by set_deterministic).
    Reference: functional.py:21 (dW = dout.T @ x, db = dout.sum(0)).
    """
    if split_k == 0 and _DETERMINISTIC:
        split_k = 1
    if _is_gpu(dy):
        ext = _ext_for(dy)
        ext.wgrad_tn(
            dy,
            x,
            grad_w,
            grad_b if grad_b is not None else torch.Tensor(),
            mask_src if mask_src is not None else torch.Tensor(),
            int(split_k),
        )
        return
    if mask_src is not None:
        dy = dy * (mask_src > 0).to(dy.dtype)
    grad_w += (dy.t() @ x).to(grad_w.dtype)
    if grad_b is not None:
        grad_b += dy.sum(dim=0).to(grad_b.dtype)


_WGRAD_GROUP = None


def set_wgrad_group(flag: bool):
    """Issue the unmasked weight gradients that follow the backward
    chain through one linear_wgrad_group call, so that same-tile layers
    (the flagship's head and hidden layers) share a launch.  Off, each
    layer is its own launch.  Gradients differ in f32 atomic arrival
    order only.  SS_WGRAD_GROUP=0 (read once) turns it off."""
    global _WGRAD_GROUP
    _WGRAD_GROUP = bool(flag)


def wgrad_group_enabled() -> bool:
    global _WGRAD_GROUP
    if _WGRAD_GROUP is None:
        import os

        _WGRAD_GROUP = os.environ.get("SS_WGRAD_GROUP", "1") != "0"
    return _WGRAD_GROUP


def wgrad_group_plan(shapes, splits=None):
    """The launches linear_wgrad_group makes on the GPU for problems of
    these (Kb, Mo, N) shapes: a list, in launch order, of
    {"problems": indices into `shapes`, "splits": ..., "blocks": ...}.
    A launch of one problem is a plain wgrad_tn call.  Host-side only,
    but needs the built extension."""
    ext = load_ext(required=True)
    return [dict(problems=list(i), splits=list(s), blocks=list(b))
            for i, s, b in ext.wgrad_group_plan(
                [tuple(int(v) for v in sh) for sh in shapes],
                None if splits is None else [int(s) for s in splits])]


def linear_wgrad_group(problems, splits=None):
    """linear_wgrad_acc (unmasked) for each (dy, x, grad_w, grad_b) of
    `problems`, grad_b may be None.  On the GPU consecutive problems of
    one tile configuration run side by side in one launch; splits is
    None or one value per problem, 0 (the launcher's rule) or >= 2."""
    problems = list(problems)
    if not problems:
        return
    if _is_gpu(problems[0][0]):
        load_ext(required=True).wgrad_tn_group(
            [tuple(p) for p in problems],
            None if splits is None else [int(s) for s in splits])
        return
    for dy, x, gw, gb in problems:
        linear_wgrad_acc(dy, x, gw, gb)


# ---------------------------------------------------------------- relu

def relu_fwd(x):
    """Standalone ReLU (reference functional.py:4-5); the hot path uses
    the fused GEMM epilogue instead."""
    if _is_gpu(x):
        return _ext_for(x).relu_fwd(x)
    # x where x > 0, else +0: -0.0 gives +0 like the kernel (clamp keeps
    # its sign); NaN stays NaN here, the kernel maps it to +0
    # (docs/KERNELS.md)
    return torch.where(x <= 0, torch.zeros_like(x), x)


def relu_bwd(dy, y, scale=1.0):
    """dx = dy ⊙ 1[y>0] from the stashed ReLU OUTPUT (for relu,
    out>0 ⟺ in>0, so stashing the output replaces the reference's
    bitmask stash at layers.py:70).

    scale != 1: the backward of ReLU + inverted dropout.  The stashed
    output y = relu(z)·m/keep already is the mask (y>0 ⟺ z>0 ∧ m=1), so
    dz = dy·scale where y>0 (rounded once, on GPU to bf16), +0 elsewhere
    — NaN and −0.0 in y mask to +0, as without scale."""
    if float(scale) == 1.0:
        if _is_gpu(dy):
            return _ext_for(dy).relu_bwd(dy, y)
        # not dy * mask: that leaves -0 under a negative dy and NaN under
        # an infinite one
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    if _is_gpu(dy):
        return _ext_for(dy).relu_bwd_scaled(dy, y, float(scale))
    return torch.where(y > 0, dy * float(scale), torch.zeros_like(dy))


# ---------------------------------------------------------------- dropout
#
# One mask definition for every path (csrc/dropout_dev.h on the GPU, the
# numpy code below on the CPU).  Element (sample, col) of layer `layer`
# at optimizer step `step` under a 64-bit `seed`:
#
#   words = Philox4x32-10(counter = (sample, col >> 2, layer, step),
#                         key     = (seed & 0xffffffff, seed >> 32))
#   keep  = words[col & 3] < thr,   thr = min(2^32 − 1, round((1−p)·2^32))
#   y     = keep ? y·float32(1/(1−p)) : +0       (f32, then ONE rounding)
#
# `sample` is the row's index in the UNSHARDED dataset order and `layer`
# the Linear's index in the full `sizes` list, so the bits do not depend
# on how DP, PP or micro-batching cut the batch.

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit values:
    counter = four arrays (broadcastable), key = two ints.  Returns the
    four output words as uint64 arrays (< 2^32)."""
    import numpy as np

    c0, c1, c2, c3 = np.broadcast_arrays(
        *[np.asarray(c, dtype=np.uint64) for c in counter])
    k0, k1 = int(key[0]) & _U32, int(key[1]) & _U32
    m32 = np.uint64(_U32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c0  # 32 x 32 bits: fits 64
        p1 = np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0 = (k0 + _PHILOX_W0) & _U32
        k1 = (k1 + _PHILOX_W1) & _U32
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=64)
def dropout_params(p):
    """(thr, scale) of drop probability p: keep when word < thr;
    scale = float32(1/(1−p)) as a Python float.  Cached: the training
    hot path asks for it per layer and step."""
    import numpy as np

    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout p must be in [0, 1), got {p}")
    thr = min(_U32, int(np.floor((1.0 - p) * 4294967296.0 + 0.5)))
    return thr, float(np.float32(1.0 / (1.0 - p)))


def _seed_words(seed):
    seed = int(seed)
    assert 0 <= seed < 1 << 64, "dropout seed is 64 bits"
    return seed & _U32, seed >> 32


def dropout_keep_mask(seed, step, layer, sample_ids, ncols, p):
    """Keep mask (bool, len(sample_ids) x ncols) of the dropout
    definition above.  sample_ids: 1-D integer tensor (or sequence) of
    unsharded sample indices, each < 2^32.  CPU: vectorised integer
    numpy; a CUDA sample_ids tensor runs the small HIP kernel
    (csrc/elementwise.hip) and returns a CUDA mask — same bits."""
    import numpy as np

    thr, _ = dropout_params(p)
    k0, k1 = _seed_words(seed)
    step, layer, ncols = int(step), int(layer), int(ncols)
    assert 0 <= step <= _U32 and 0 <= layer <= _U32 and ncols >= 0
    if not torch.is_tensor(sample_ids):
        sample_ids = torch.as_tensor(list(sample_ids), dtype=torch.int64)
    sample_ids = sample_ids.to(torch.int64).reshape(-1)
    if sample_ids.numel():
        assert int(sample_ids.min()) >= 0 and \
            int(sample_ids.max()) <= _U32, "sample id must be < 2^32"
    if _is_gpu(sample_ids):
        return _ext_for(sample_ids).dropout_keep_mask(
            sample_ids.contiguous(), ncols, k0, k1, step, layer, thr)
    ngroups = (ncols + 3) // 4
    s = sample_ids.numpy().astype(np.uint64)[:, None]
    g = np.arange(ngroups, dtype=np.uint64)[None, :]
    words = philox4x32_10((s, g, np.uint64(layer), np.uint64(step)),
                          (k0, k1))
    # (rows, groups, 4) -> (rows, 4 * groups): word col & 3 of group col >> 2
    w = np.stack(words, axis=-1).reshape(s.shape[0], ngroups * 4)[:, :ncols]
    return torch.from_numpy(w < np.uint64(thr))


def _sample_ids(rows, row_first, row_stride, device):
    assert row_first + max(rows - 1, 0) * row_stride <= _U32, \
        "sample id must be < 2^32"
    return row_first + row_stride * torch.arange(rows, dtype=torch.int64,
                                                 device=device)


def dropout_fwd_(y, seed, step, layer, row_first, row_stride, p):
    """In-place inverted dropout of a finished post-ReLU activation y
    (rows x cols); row i is sample row_first + i·row_stride.  The GPU
    kernel (dropout_fwd_kernel: 16-B accesses, one Philox call per four
    columns) serves the forward GEMM tiers without the fused epilogue
    (glds, 256-tile, fp8).  Same mask as the fused path; a kept bf16
    value is rounded a second time here, so it may differ from the
    fused epilogue's by one bf16 ulp."""
    thr, scale = dropout_params(p)
    if _is_gpu(y):
        k0, k1 = _seed_words(seed)
        _ext_for(y).dropout_fwd_(y, k0, k1, int(step), int(layer),
                                 int(row_first), int(row_stride), thr, scale)
        return y
    keep = dropout_keep_mask(
        seed, step, layer,
        _sample_ids(y.shape[0], row_first, row_stride, y.device),
        y.shape[1], p)
    y.copy_(torch.where(keep, y * scale, torch.zeros_like(y)))
    return y


def linear_fwd_dropout(x, w, b, seed, step, layer, row_first, row_stride, p,
                       fused=True):
    """y = dropout(relu(x @ W^T + b)), the training forward of a ReLU
    Linear with drop probability p.

    GPU: the mask rides in the epilogue of gemm_nt_kernel while the f32
    accumulator is still in registers (one rounding to bf16); shapes
    that dispatch to a tier without that epilogue (glds, 256-tile) run
    the plain GEMM and then dropout_fwd_.  fused=False takes that
    two-launch path at any shape (the measured alternative)."""
    if _is_gpu(x):
        thr, scale = dropout_params(p)
        k0, k1 = _seed_words(seed)
        return _ext_for(x).gemm_nt_dropout(
            x, w, b, k0, k1, int(step), int(layer), int(row_first),
            int(row_stride), thr, scale, bool(fused))
    y = linear_fwd(x, w, b, relu=True)
    return dropout_fwd_(y, seed, step, layer, row_first, row_stride, p)


# ---------------------------------------------------------------- softmax

def softmax_fwd(x):
    """Row softmax with per-row max subtraction.

    Reference: functional.py:24-27 (which uses a global max and +1e-7;
    we use the numerically correct form — divergence documented)."""
    if _is_gpu(x):
        return _ext_for(x).softmax_fwd(x)
    m = x.max(dim=-1, keepdim=True).values
    e = torch.exp(x - m)
    return e / e.sum(dim=-1, keepdim=True)


def softmax_bwd(dy, s):
    """ds/dx given softmax OUTPUT s (we stash the output; the reference
    stashes the input and recomputes, noted wasteful at
    functional.py:31-32).  dx = s*(dy - rowsum(s*dy))."""
    if _is_gpu(dy):
        return _ext_for(dy).softmax_bwd(dy, s)
    dot = (s * dy).sum(dim=-1, keepdim=True)
    return s * (dy - dot)


# ---------------------------------------------------------------- loss heads

def mse_loss(x, t, global_batch):
    """Σ(t−x)²/global_batch (reference functional.py:38-40; only used
    by tests/logging — training fwd is identity, layers.py:150-155)."""
    return ((t - x) ** 2).sum() / global_batch


def head_softmax_mse_bwd(probs, target, global_batch):
    """Fused backward of Softmax→MSELoss w.r.t. logits.

    g = −2(t−s)/GB (mse_loss_grad, functional.py:43-44), then the
    softmax Jacobian (functional.py:30-35):
      dz = s ⊙ (g − rowsum(s ⊙ g)).
    global_batch is the GLOBAL batch size so µbatch/DP gradients sum to
    the sequential gradient (reference layers.py:146-148).
    """
    if _is_gpu(probs):
        return _ext_for(probs).head_mse_bwd(probs, target, float(global_batch))
    g = -2.0 * (target - probs) / global_batch
    dot = (probs * g).sum(dim=-1, keepdim=True)
    return probs * (g - dot)


def head_softmax_xent_bwd(probs, target, global_batch):
    """Fused backward of softmax cross-entropy: dz = (s − t)/GB."""
    if _is_gpu(probs):
        return _ext_for(probs).head_xent_bwd(probs, target, float(global_batch))
    return (probs - target) / global_batch


def head_fused_ok(x, linear) -> bool:
    """True when `linear` (the Linear feeding a SoftmaxXent head) and
    its input meet the launch contract of the fused head kernels:
    GPU, bf16, no activation, no fp8 forward, out <= 16, in % 32 == 0,
    in <= 1024."""
    return (head_fused()
            and _is_gpu(x) and x.dtype == torch.bfloat16 and x.dim() == 2
            and x.shape[0] >= 1 and x.is_contiguous()
            and x.data_ptr() % 16 == 0
            and linear.activation is None and not linear.fp8_fwd
            and linear.weight.lp is not None
            and linear.weight.lp_t is not None
            and linear.out_dims <= 16
            and linear.in_dims % 32 == 0 and linear.in_dims <= 1024)


def head_fwd_fused(x, w, b):
    """probs = softmax(bf16(x @ W^T + b)) in one kernel (GPU only;
    bit-identical to linear_fwd -> softmax_fwd)."""
    return _ext_for(x).head_fwd_fused(x, w, b)


def head_bwd_fused(probs, target, x, w_t, global_batch, grad_w=None,
                   grad_b=None, metrics=None):
    """(dz, dx) of the fused head in one kernel: dz = (probs - t)/GB,
    dx = dz @ W — bit-identical to head_softmax_xent_bwd ->
    linear_dgrad.  With grad_w (and grad_b) given, the same kernel also
    accumulates grad_w += dz^T @ x and grad_b += colsum(dz) with f32
    atomics (one set per block, at most 256 blocks).  With `metrics` (an
    accumulator of new_metrics_acc) it also adds the cross-entropy
    metric totals of (probs, target) — same values as head_metrics, no
    second launch; dz and dx keep their bits."""
    empty = torch.Tensor()
    args = (probs, target, x, w_t, float(global_batch),
            grad_w if grad_w is not None else empty,
            grad_b if grad_b is not None else empty)
    if metrics is None:
        return tuple(_ext_for(probs).head_bwd_fused(*args))
    return tuple(_ext_for(probs).head_bwd_fused(*args, 0, metrics, 0))


def bwd_chain(probs, target, w_head_t, global_batch, hs, w_ts, rows=0,
              waves=0, w_lds=0, dz_scale=1.0):
    """Head backward plus the ReLU-layer data gradients below it in one
    kernel (GPU only, csrc/bwd_chain.hip).

    hs: post-ReLU outputs of the chain's layers, top layer first (all
    (M, 256)); w_ts: the transposed weights of the layers whose dgrad is
    in the chain — all of them (dx of the last layer is returned) or all
    but the last (the chain ends at dz of the last layer).

      dz_head = (probs − target)/GB ;  dh = dz_head @ W_head
      dz_l = dh ⊙ 1[h_l > 0] ;  dh = dz_l @ W_l ;  ...

    Returns (dz_head, [dz_l, ...], dx or None), each bit-identical to
    head_bwd_fused -> relu_bwd -> linear_dgrad -> ..., or None, with
    nothing launched, when the inputs are outside the kernel's contract
    (the caller takes the per-layer path).  rows / waves / w_lds select
    the measured arms; 0 is the shipped choice.

    dz_scale != 1 (layers under inverted dropout, all with one p): every
    kept dz_l element is bf16(dh · dz_scale), bit-identical to
    relu_bwd(dh, h_l, scale=dz_scale).  One scale per launch; built for
    the shipped arm only, so another arm returns None.  dz_scale == 1
    runs the unscaled kernel."""
    if not _is_gpu(probs):
        return None
    out = _ext_for(probs).bwd_chain(probs, target, w_head_t,
                                    float(global_batch), list(hs), list(w_ts),
                                    int(rows), int(waves), int(w_lds),
                                    float(dz_scale))
    if not out:
        return None
    n = len(hs)
    return out[0], out[1:1 + n], (out[1 + n] if len(w_ts) == n else None)


def fwd_chain(x, ws, bs, w_head, b_head, rows=0, waves=0, l1=0, kloop=0,
              zero=None):
    """The ReLU layers under the fused head and the head forward in one
    kernel (GPU only, csrc/fwd_chain.hip).

    ws / bs: weights (256, in) and biases of the chain's layers, bottom
    layer first; x: the input of the lowest one, (M, 256), or (M, any
    multiple of 8) when that layer streams its input.

      h_l = relu(h_{l-1} @ W_l^T + b_l) ; probs = softmax(h @ W_head^T + b)

    Returns ([h_l, ...], probs), each bit-identical to linear_fwd(relu)
    -> ... -> head_fwd_fused, or None, with nothing launched, when the
    inputs are outside the kernel's contract (the caller takes the
    per-layer path).  rows / waves select the measured arms, l1 how the
    chain starts (1: from a stored 256-wide activation, 2: streaming
    x), kloop its K loops (1: B fragments one step ahead, 2: three
    steps ahead, eight waves only); 0 is the shipped choice.

    zero: a contiguous f32 tensor on x's device, or None.  The launch
    fills it with zeros as well (the step's flat gradient buffer: see
    Sequential.zero_grad(defer=True)); when the launch is refused it is
    left as it was."""
    if not _is_gpu(x):
        return None
    out = _ext_for(x).fwd_chain(x, list(ws), list(bs), w_head, b_head,
                                int(rows), int(waves), int(l1), int(kloop),
                                zero)
    if not out:
        return None
    return out[:-1], out[-1]


def xent_loss(probs, target, global_batch, eps=1e-9):
    """−Σ t·log(p)/GB (logging only)."""
    return -(target * torch.log(probs.float() + eps)).sum() / global_batch


# ------------------------------------------------------- training metrics
#
# One definition for every path (GPU kernels in csrc/head.hip, torch on
# the CPU).  For probs p and target t of shape (M, C), a call adds
#   rows      += M
#   nonfinite += rows with any NaN / ±Inf in p (these add nothing below)
#   loss_sum  += Σ_r −Σ_c t·log(max(p, FLT_MIN))  over t != 0     (xent)
#                Σ_r Σ_c (t − p)²                                  (mse)
#   correct   += rows with argmax_c p == argmax_c t, lowest index on ties
# to an accumulator of S slots x 4 32-bit words (word 0: f32 loss_sum,
# words 1..3: int32 correct, rows, nonfinite).  A GPU block adds into
# slot blockIdx % S so a launch's atomics do not queue on one address;
# the slots are folded on the host, in f64 / int64, at read time only.

METRICS_SLOTS = 16  # the shipped S on GPU (docs/KERNELS.md, head metrics)
_FLT_MIN = 1.1754943508222875e-38

_HEAD_METRICS_FUSED = None


def set_head_metrics_fused(flag: bool):
    """Let the fused head backward count the training metrics itself
    (default).  Off: the fused backward runs without them and a
    head_metrics launch follows — the measured alternative,
    SS_HEAD_METRICS_FUSED=0 (read once)."""
    global _HEAD_METRICS_FUSED
    _HEAD_METRICS_FUSED = bool(flag)


def head_metrics_fused() -> bool:
    global _HEAD_METRICS_FUSED
    if _HEAD_METRICS_FUSED is None:
        import os

        _HEAD_METRICS_FUSED = \
            os.environ.get("SS_HEAD_METRICS_FUSED", "1") != "0"
    return _HEAD_METRICS_FUSED


def new_metrics_acc(device, slots=None):
    """A zeroed metrics accumulator on `device`.  slots: a power of two;
    default METRICS_SLOTS on GPU, 1 on CPU."""
    device = torch.device(device)
    if slots is None:
        slots = METRICS_SLOTS if device.type == "cuda" else 1
    assert slots >= 1 and slots & (slots - 1) == 0, \
        f"slots must be a power of two, got {slots}"
    return torch.zeros(slots, 4, dtype=torch.int32, device=device)


def head_metrics(probs, target, acc, kind="xent"):
    """Add the metric totals of (probs, target) to `acc` (definition
    above).  GPU: one launch of head_metrics_kernel, no host sync."""
    assert kind in ("xent", "mse"), kind
    assert probs.dim() == 2 and probs.shape == target.shape, \
        (probs.shape, target.shape)
    if _is_gpu(probs):
        if target.dtype != probs.dtype:
            target = target.to(probs.dtype)
        _ext_for(probs).head_metrics(
            probs if probs.is_contiguous() else probs.contiguous(),
            target if target.is_contiguous() else target.contiguous(),
            acc, kind)
        return
    p, t = probs.float(), target.float()
    fin = torch.isfinite(p).all(dim=1)
    if kind == "xent":
        logp = torch.log(torch.clamp(p, min=_FLT_MIN))
        terms = torch.where(t != 0, -t * logp, torch.zeros_like(p))
    else:
        terms = (t - p) ** 2
    loss = terms.sum(dim=1)[fin].double().sum()
    hit = (p.argmax(dim=1) == t.argmax(dim=1)) & fin
    acc.view(torch.float32)[0, 0] += loss.float()
    acc[0, 1] += int(hit.sum())
    acc[0, 2] += p.shape[0]
    acc[0, 3] += int((~fin).sum())


def read_metrics_acc(acc, reset=True):
    """Fold the slots on the host (one device-to-host copy, f64 / int64
    sums) into {loss_sum, correct, rows, nonfinite}; reset=True zeroes
    the accumulator afterwards."""
    host = acc.to("cpu", copy=True)
    if reset:
        acc.zero_()
    counts = host[:, 1:].to(torch.int64).sum(dim=0)
    return {
        "loss_sum": float(host.view(torch.float32)[:, 0].double().sum()),
        "correct": int(counts[0]),
        "rows": int(counts[1]),
        "nonfinite": int(counts[2]),
    }


# ----------------------------------------------- layernorm / gelu (extras)

def layernorm_fwd(x, gamma, beta, eps=1e-5):
    """Rowwise LayerNorm.  Returns (y, mean, rstd) — the f32 row stats
    feed the backward.  Beyond-reference extension (modern-MLP blocks);
    HIP kernel: csrc/norm.hip."""
    if _is_gpu(x):
        return tuple(_ext_for(x).ln_fwd(x, gamma, beta, float(eps)))
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    y = ((xf - mu) * rstd * gamma.float() + beta.float()).to(x.dtype)
    return y, mu.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta):
    """dx plus in-place accumulation of dγ/dβ (f32 grads)."""
    if _is_gpu(dy):
        e = _ext_for(dy)
        dx = e.ln_bwd_dx(dy, x, gamma, mean, rstd)
        e.ln_bwd_dparam(dy, x, mean, rstd, dgamma, dbeta)
        return dx
    xf, dyf = x.float(), dy.float()
    xh = (xf - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    g = dyf * gamma.float()
    C = x.shape[-1]
    dx = rstd.unsqueeze(-1) * (
        g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    dgamma += (dyf * xh).sum(0)
    dbeta += dyf.sum(0)
    return dx.to(dy.dtype)


def gelu_fwd(z):
    """tanh-approximation GELU (elementwise HIP kernel on GPU)."""
    if _is_gpu(z):
        return _ext_for(z).gelu_fwd(z)
    return torch.nn.functional.gelu(z.float(), approximate="tanh").to(z.dtype)


def gelu_bwd(dy, z):
    if _is_gpu(dy):
        return _ext_for(dy).gelu_bwd(dy, z)
    zf = z.float().detach().requires_grad_(True)
    y = torch.nn.functional.gelu(zf, approximate="tanh")
    y.backward(dy.float())
    return zf.grad.to(dy.dtype)


from collections import OrderedDict  # noqa: E402

# LRU-capped cache of (pinned-host, device) pointer tables for the
# chunked wgrad kernel, keyed by (grad_w ptr, n_chunks).  The cap plus
# clear_wgrad_tables() (called from Sequential.materialize_device)
# keeps long-lived processes that build/destroy many models from
# leaking pinned+device entries; a freed-then-reallocated grad buffer
# at the same address is safe regardless (rows are re-checked), the
# eviction is purely about memory growth.
_WGRAD_TABLES = OrderedDict()
_WGRAD_TABLES_CAP = 64


def clear_wgrad_tables():
    _WGRAD_TABLES.clear()


def linear_wgrad_multi(chunks, grad_w, grad_b=None, split_k=0):
    """Deferred-µbatch weight gradients: ONE kernel launch accumulates
    every (dy, x[, mask]) chunk of a layer into grad_w/grad_b.

    chunks: list of (dy, x, mask_or_None) with identical shapes.
    Replaces num_µbatches separate wgrad launches under pipeline
    schedules (each launch re-pays prologue + atomic epilogue).
    GPU only; the CPU path loops (it has no launch cost to amortize).
    """
    if split_k == 0 and _DETERMINISTIC:
        split_k = 1
    dy0 = chunks[0][0]
    if not _is_gpu(dy0) or split_k == 1:
        # split_k==1 (deterministic mode): the chunked kernel would
        # still run one block PER CHUNK per tile, all atomicAdd-ing
        # the same gW element — chunk ARRIVAL order is scheduling-
        # dependent, which broke bitwise reproducibility (flaky GPU
        # determinism test).  Sequential per-chunk launches fix the
        # accumulation order at a small launch-count cost; perf mode
        # (split_k=0) keeps the single fused launch.
        for dy, x, m in chunks:
            linear_wgrad_acc(dy, x, grad_w, grad_b, m, split_k)
        return
    ext = _ext_for(dy0)
    has_mask = chunks[0][2] is not None
    # Pinned-host staging + cached device table: the H2D becomes an
    # async (capture-legal) copy, so the flush works INSIDE hipGraph
    # capture — the pinned buffer stays alive with stable content, and
    # replays re-copy it (chunk pointers are stable under the graph
    # memory pool).
    rows = []
    for dy, x, m in chunks:
        assert dy.shape == dy0.shape and (m is not None) == has_mask
        rows.append(dy.data_ptr())
        rows.append(x.data_ptr())
        rows.append(m.data_ptr() if m is not None else 0)
    key = (grad_w.data_ptr(), len(chunks))
    entry = _WGRAD_TABLES.get(key)
    if entry is None:
        while len(_WGRAD_TABLES) >= _WGRAD_TABLES_CAP:
            _WGRAD_TABLES.popitem(last=False)
        pinned = torch.empty(len(chunks), 3, dtype=torch.int64,
                             pin_memory=True)
        dev = torch.empty(len(chunks), 3, dtype=torch.int64,
                          device=dy0.device)
        entry = _WGRAD_TABLES[key] = [pinned, dev, None]
    else:
        _WGRAD_TABLES.move_to_end(key)
    pinned, table, last_rows = entry
    if rows != last_rows:
        # chunk pointers are usually STABLE step to step (caching
        # allocator steady state / graph pool), so the host-side table
        # rebuild + H2D is skipped on the hot path
        pinned.view(-1).copy_(torch.tensor(rows, dtype=torch.int64))
        table.copy_(pinned, non_blocking=True)
        entry[2] = rows
    ext.wgrad_tn_multi(table, len(chunks), has_mask, grad_w,
                       grad_b if grad_b is not None else torch.Tensor(),
                       dy0.shape[1], chunks[0][1].shape[1], dy0.shape[0],
                       int(split_k))


def row_argmax(x):
    """Per-row argmax (eval/serving).  torch's ROCm argmax on skinny
    bf16 tensors is pathologically slow (~1.3 ms at 16384x10); the HIP
    wave-per-row kernel is ~5 µs.  CPU falls back to torch."""
    if _is_gpu(x) and x.dtype == torch.bfloat16:
        return _ext_for(x).row_argmax(x).long()
    return x.argmax(dim=-1)
