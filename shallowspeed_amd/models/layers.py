"""Model layer: Parameter / Module / Linear / loss heads / Sequential / MLP.

Reference: shallowspeed/layers.py (270 LoC, NumPy).  Behavioral parity:

  * explicit forward/backward (no autograd), per-µbatch activation
    stash keyed by mubatch_id (layers.py:70,117) so multiple µbatches
    can be in flight under pipeline schedules,
  * deterministic SHAPE-SEEDED weight init (layers.py:106-113): the
    same (in,out) shape produces bit-identical weights regardless of
    DP/PP partitioning — the load-bearing trick behind replica-sync
    and pipeline-vs-serial equivalence testing,
  * gradient ACCUMULATION in backward (layers.py:135-136) — wgrad does
    `grad +=`, enabling µbatch accumulation,
  * Sequential grad-hook API (layers.py:182-213): after each layer's
    backward the per-parameter hooks fire (this is where the Worker
    injects the DP all-reduce, pipe.py:389-400), then post-grad hooks,
  * MLP stage construction with one-element overlap slicing and no
    activation on the very last Linear (layers.py:242-263).

MI355X-native differences:
  * tensors are torch; on GPU the compute dtype is bf16 and every hot
    op dispatches to the in-tree HIP/CDNA4 extension,
  * parameters keep an f32 master + bf16 copy + transposed bf16 copy
    (the transposed copy makes dgrad the same NT MFMA kernel as fwd),
  * all f32 grads of a model live in ONE flat buffer (views per param)
    — zero_grad is one memset and DP bucketing operates on flat slices
    (the reference's own docstring asks for bucketing, pipe.py:309-310),
  * the loss head is a fused softmax-cross-entropy (or softmax-MSE for
    reference parity) producing d(logits) in one op.
"""

import math

import torch

from ..ops import functional as F


_DZ_FIRST = None


def _dz_first_enabled() -> bool:
    global _DZ_FIRST
    if _DZ_FIRST is None:
        import os

        # default OFF: A/B'd neutral at the flagship (0.2072 vs 0.2081
        # ms within one call) — the mask re-reads are L2-absorbed there
        _DZ_FIRST = os.environ.get("SS_DZ_FIRST", "0") == "1"
    return _DZ_FIRST


def _shape_seed(in_dims: int, out_dims: int) -> int:
    # Same spirit as reference layers.py:106-108 (seed from the layer
    # shape only): partition-invariant deterministic init.
    return (in_dims * 1_000_003 + out_dims * 7919) & 0x7FFFFFFF


class Parameter:
    """f32 master tensor + f32 grad (+ bf16 / transposed-bf16 device
    copies on GPU).  Reference: layers.py:17-28."""

    def __init__(self, data: torch.Tensor, requires_grad: bool = True):
        self.data = data.float()
        self.requires_grad = requires_grad
        self.grad = torch.zeros_like(self.data) if requires_grad else None
        self.lp = None    # bf16 compute copy (GPU)
        self.lp_t = None  # transposed bf16 copy (GPU, 2-D weights only)
        # DP all-reduce bookkeeping (reference parks the MPI request on
        # the parameter, pipe.py:314): we park the async work handle.
        self._comm_handle = None

    @property
    def shape(self):
        return self.data.shape

    def compute(self) -> torch.Tensor:
        """The tensor GEMMs consume: bf16 copy on GPU, master on CPU."""
        return self.lp if self.lp is not None else self.data

    def compute_t(self):
        return self.lp_t

    def materialize_device(self, device, compute_dtype):
        self.data = self.data.to(device)
        if self.grad is not None:
            self.grad = self.grad.to(device)
        if compute_dtype == torch.bfloat16:
            self.lp = self.data.to(torch.bfloat16)
            if self.data.dim() == 2:
                self.lp_t = self.lp.t().contiguous()

    def sync_lp(self):
        """Refresh low-precision copies from the master (used by the CPU
        SGD path and by checkpoint load; the fused GPU SGD kernel does
        this in-kernel)."""
        if self.lp is not None:
            self.lp.copy_(self.data.to(torch.bfloat16))
            if self.lp_t is not None:
                self.lp_t.copy_(self.lp.t())


class Module:
    """Stateful op with per-µbatch cache.  Reference: layers.py:31-64."""

    def __init__(self):
        self._params = {}
        self._cache = {}
        self._training = True

    def forward(self, inputs: torch.Tensor, mubatch_id: int = 0):
        raise NotImplementedError

    def backward(self, dout: torch.Tensor, mubatch_id: int = 0):
        raise NotImplementedError

    def parameters(self):
        return list(self._params.values())

    def zero_grad(self):
        for p in self._params.values():
            if p.grad is not None:
                p.grad.zero_()

    def train(self):
        self._training = True

    def eval(self):
        self._training = False

    def _stash(self, name, mubatch_id, value):
        if self._training:
            self._cache[(name, mubatch_id)] = value

    def _unstash(self, name, mubatch_id):
        return self._cache.pop((name, mubatch_id))

    def materialize_device(self, device, compute_dtype):
        for p in self._params.values():
            p.materialize_device(device, compute_dtype)


class DropoutState:
    """What the dropout mask depends on besides the layer and the
    element (F.dropout_keep_mask): the 64-bit seed, the number of
    optimizer steps taken, and per µbatch the sample ids of its rows as
    (first, stride) — row i of µbatch m is sample first + i·stride of
    the unsharded dataset order.  One object per Sequential, shared by
    its Linears; a hand-driven Linear owns a default one (seed 0, step
    0, rows 0, 1, 2, ...)."""

    def __init__(self, seed: int = 0):
        self.seed = int(seed)
        self.step = 0
        self.rows = {}

    def sample_rows(self, mubatch_id):
        return self.rows.get(mubatch_id, (0, 1))


class Linear(Module):
    """y = x @ W^T + b with optional FUSED ReLU (GEMM epilogue).

    dropout=p (0 <= p < 1, ReLU layers only): inverted dropout on the
    ReLU output in training mode, y = relu(z)·m/(1−p), with the
    counter-based mask of F.dropout_keep_mask keyed on (seed, step,
    layer_index, sample, column) — on GPU in the forward GEMM's
    epilogue.  Only ReLU, because the stashed output then already is the
    backward's mask (y>0 ⟺ z>0 ∧ m=1): dz = dh ⊙ 1[y>0]/(1−p), no mask
    and no RNG kept.  layer_index is the Linear's index in the full
    model, so pipeline stage slicing does not change the bits.  In eval
    mode, or with p = 0, the forward is exactly the call without it.

    Reference: layers.py:99-142 (module-level ReLU fusion at
    layers.py:120-122 becomes a kernel epilogue; backward unwinds the
    activation first via the stashed post-ReLU output, then runs
    dgrad/wgrad — layers.py:124-139).
    Init: W ~ N(0,1)/√in_dims f32, b = 0, shape-seeded
    (layers.py:106-113).
    """

    def __init__(self, in_dims: int, out_dims: int, activation=None,
                 dropout: float = 0.0, layer_index: int = 0):
        super().__init__()
        assert activation in (None, "relu", "gelu")
        dropout = float(dropout)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        if dropout > 0.0 and activation != "relu":
            raise ValueError(
                "dropout needs activation='relu': the post-ReLU output "
                "doubles as the backward mask (y > 0 <=> kept and active)")
        self.in_dims, self.out_dims = in_dims, out_dims
        self.activation = activation
        self.dropout = dropout
        self.layer_index = int(layer_index)
        self._drop_state = DropoutState()  # Sequential shares its own
        if dropout > 0.0:
            self.forward = self._forward_dropout
            self.backward = self._backward_dropout
        g = torch.Generator().manual_seed(_shape_seed(in_dims, out_dims))
        w = torch.randn(out_dims, in_dims, generator=g, dtype=torch.float32)
        w /= math.sqrt(in_dims)
        self._params["weight"] = Parameter(w)
        self._params["bias"] = Parameter(torch.zeros(out_dims))
        self.weight = self._params["weight"]
        self.bias = self._params["bias"]
        # deferred-µbatch wgrad (GPU): collect (dy, x, mask) per
        # µbatch and launch ONE chunked kernel at flush time.  The
        # WINDOW caps how many µbatches are retained (holding every
        # µbatch's dout/x would break 1F1B's bounded activation stash
        # — the schedule's whole memory story): when the window fills,
        # the pending chunks flush early (grads accumulate atomically,
        # so partial flushes compose).
        self._defer_wgrad = False
        self._wgrad_window = 1 << 30
        self._wgrad_pending = []
        # MX-fp8 forward (training): quantize activations per µbatch
        # and keep an fp8 copy of the weight, refreshed lazily after
        # each optimizer step (invalidate_fp8()).  Backward stays bf16
        # (dgrad/wgrad on the bf16 stash); the f32 master is untouched
        # — this is the training-forward extension of the round-1
        # serving tier (csrc/fp8.hip, ~1.7x the bf16 8-phase GEMM).
        self.fp8_fwd = False
        self._wq = None
        self._ws = None

    def _fp8_ok(self, rows: int) -> bool:
        return (self.fp8_fwd and self.activation in (None, "relu")
                and rows % 256 == 0
                and self.out_dims % 256 == 0 and self.in_dims % 256 == 0)

    def _drop_on(self) -> bool:
        return self.dropout > 0.0 and self._training

    def dz_scale(self) -> float:
        """What the backward multiplies kept gradients by: float32
        1/(1−p) under dropout, else 1."""
        return F.dropout_params(self.dropout)[1] if self._drop_on() else 1.0

    def _drop_key(self, mubatch_id):
        """(seed, step, layer, row_first, row_stride, p) of this forward."""
        st = self._drop_state
        first, stride = st.sample_rows(mubatch_id)
        return (st.seed, st.step, self.layer_index, first, stride,
                self.dropout)

    def forward(self, inputs, mubatch_id: int = 0):
        self._stash("x", mubatch_id, inputs)
        if inputs.is_cuda and self._fp8_ok(inputs.shape[0]):
            if self._wq is None:
                self._wq, self._ws = F.fp8_quantize(self.weight.compute())
            xq, xs = F.fp8_quantize(inputs)
            y = F.linear_fwd_fp8(xq, xs, self._wq, self._ws,
                                 self.bias.compute(),
                                 relu=(self.activation == "relu"))
            if self.activation == "relu":
                self._stash("y", mubatch_id, y)
            return y
        if self.activation == "gelu":
            z = F.linear_fwd(inputs, self.weight.compute(),
                             self.bias.compute(), relu=False)
            self._stash("z", mubatch_id, z)
            return F.gelu_fwd(z)
        y = F.linear_fwd(
            inputs, self.weight.compute(), self.bias.compute(),
            relu=(self.activation == "relu"),
        )
        if self.activation == "relu":
            # post-ReLU output doubles as the backward mask source
            # (out>0 ⟺ pre-act>0); replaces the reference's separate
            # bitmask stash (layers.py:70).
            self._stash("y", mubatch_id, y)
        return y

    def backward(self, dout, mubatch_id: int = 0, need_dx: bool = True):
        x = self._unstash("x", mubatch_id)
        mask_src = None
        if self.activation == "relu":
            mask_src = self._unstash("y", mubatch_id)
            if dout.is_cuda:
                B, O = dout.shape
                I = self.in_dims
                # WIDE aligned layers: materializing dz once lets
                # dgrad take the unmasked glds tier and strips the
                # mask re-reads from wgrad (mask fusion wins at small
                # shapes where L2 absorbs the re-reads — measured).
                # Second disjunct: any shape the 256²-tile wgrad tier
                # can take (O%256, I%256, B%128) unmasks too — the
                # masked path would silently fall back to the 128²
                # wgrad tier (~0.65 PF vs 1.1-1.2 PF), which costs far
                # more than one elementwise dz pass.  dz is shared by
                # dgrad and (deferred) wgrad, so the pass amortizes
                # over both GEMMs.
                wide_glds = (B % 128 == 0 and I % 128 == 0 and O % 32 == 0
                             and (B // 128) * (I // 128) >= 512
                             and O >= 512 and I >= 512)
                wgrad256_ok = (O % 256 == 0 and I % 256 == 0
                               and B % 128 == 0 and B >= 128
                               and O >= 512 and I >= 512
                               and (O // 256) * (I // 256) >= 64)
                # dgrad-skipped layers (pipeline stage 0's first
                # Linear): wgrad is the mask's only consumer and
                # re-reads it once per N-tile — one elementwise dz
                # pass is cheaper (A/B'd on the flagship first layer,
                # SS_DZ_FIRST=0 reverts)
                first_layer_dz = (not need_dx and B >= 4096
                                  and _dz_first_enabled())
                if wide_glds or wgrad256_ok or first_layer_dz:
                    dout = F.relu_bwd(dout, mask_src)
                    mask_src = None
        elif self.activation == "gelu":
            z = self._unstash("z", mubatch_id)
            dout = F.gelu_bwd(dout, z)
        dx = None
        if need_dx:
            dx = F.linear_dgrad(dout, self.weight.compute(),
                                self.weight.compute_t(), mask_src)
        if self._defer_wgrad:
            self._wgrad_pending.append((dout, x, mask_src))
            if len(self._wgrad_pending) >= self._wgrad_window:
                self.flush_wgrad()
        else:
            F.linear_wgrad_acc(dout, x, self.weight.grad, self.bias.grad,
                               mask_src)
        return dx

    # ---- dropout: bound over forward / backward per INSTANCE when
    # dropout > 0 (see __init__), so a layer without it runs the two
    # methods above and nothing else
    def _forward_dropout(self, inputs, mubatch_id: int = 0):
        if not self._training:
            return Linear.forward(self, inputs, mubatch_id)
        self._stash("x", mubatch_id, inputs)
        key = self._drop_key(mubatch_id)
        if inputs.is_cuda and self._fp8_ok(inputs.shape[0]):
            # the fp8 tier has no dropout epilogue: standalone pass
            if self._wq is None:
                self._wq, self._ws = F.fp8_quantize(self.weight.compute())
            xq, xs = F.fp8_quantize(inputs)
            y = F.linear_fwd_fp8(xq, xs, self._wq, self._ws,
                                 self.bias.compute(), relu=True)
            F.dropout_fwd_(y, *key)
        else:
            y = F.linear_fwd_dropout(inputs, self.weight.compute(),
                                     self.bias.compute(), *key)
        # the post-dropout output is the backward's mask source
        self._stash("y", mubatch_id, y)
        return y

    def _backward_dropout(self, dout, mubatch_id: int = 0,
                          need_dx: bool = True):
        x = self._unstash("x", mubatch_id)
        y = self._unstash("y", mubatch_id)
        # dz = dout ⊙ 1[y>0]/(1−p), materialised once; dgrad and wgrad
        # then run unmasked (the masked-operand kernels carry no scale)
        # — the path wide layers take anyway
        dz = F.relu_bwd(dout, y, scale=self.dz_scale())
        dx = None
        if need_dx:
            dx = F.linear_dgrad(dz, self.weight.compute(),
                                self.weight.compute_t())
        if self._defer_wgrad:
            self._wgrad_pending.append((dz, x, None))
            if len(self._wgrad_pending) >= self._wgrad_window:
                self.flush_wgrad()
        else:
            F.linear_wgrad_acc(dz, x, self.weight.grad, self.bias.grad)
        return dx

    def flush_wgrad(self):
        """Launch the deferred µbatch weight gradients as ONE chunked
        kernel (see functional.linear_wgrad_multi)."""
        if self._wgrad_pending:
            F.linear_wgrad_multi(self._wgrad_pending, self.weight.grad,
                                 self.bias.grad)
            self._wgrad_pending = []


class ReLU(Module):
    """Standalone ReLU (reference layers.py:67-80); the hot path uses
    Linear's fused epilogue instead."""

    def forward(self, inputs, mubatch_id: int = 0):
        y = F.relu_fwd(inputs)
        self._stash("y", mubatch_id, y)
        return y

    def backward(self, dout, mubatch_id: int = 0):
        y = self._unstash("y", mubatch_id)
        return F.relu_bwd(dout, y)


class GELU(Module):
    """Standalone GELU (tanh approximation) — beyond-reference module
    for modern MLP blocks; the fused path is Linear(activation="gelu")."""

    def forward(self, inputs, mubatch_id: int = 0):
        self._stash("z", mubatch_id, inputs)
        return F.gelu_fwd(inputs)

    def backward(self, dout, mubatch_id: int = 0):
        z = self._unstash("z", mubatch_id)
        return F.gelu_bwd(dout, z)


class LayerNorm(Module):
    """Rowwise LayerNorm with learnable scale/shift — beyond-reference
    module (HIP kernels: csrc/norm.hip; wave-per-row f32 statistics)."""

    def __init__(self, dim: int, eps: float = 1e-5):
        super().__init__()
        self.dim, self.eps = dim, eps
        self._params["gamma"] = Parameter(torch.ones(dim))
        self._params["beta"] = Parameter(torch.zeros(dim))
        self.gamma = self._params["gamma"]
        self.beta = self._params["beta"]

    def forward(self, inputs, mubatch_id: int = 0):
        y, mean, rstd = F.layernorm_fwd(
            inputs, self.gamma.compute(), self.beta.compute(), self.eps)
        self._stash("x", mubatch_id, inputs)
        self._stash("stats", mubatch_id, (mean, rstd))
        return y

    def backward(self, dout, mubatch_id: int = 0):
        x = self._unstash("x", mubatch_id)
        mean, rstd = self._unstash("stats", mubatch_id)
        return F.layernorm_bwd(dout, x, self.gamma.compute(), mean, rstd,
                               self.gamma.grad, self.beta.grad)


class Softmax(Module):
    """Standalone row softmax (reference layers.py:83-96).  Stashes the
    OUTPUT (reference stashes input and recomputes — functional.py:31-32
    notes that as wasteful; we fix it)."""

    def forward(self, inputs, mubatch_id: int = 0):
        s = F.softmax_fwd(inputs)
        self._stash("s", mubatch_id, s)
        return s

    def backward(self, dout, mubatch_id: int = 0):
        s = self._unstash("s", mubatch_id)
        return F.softmax_bwd(dout, s)


class MSELoss(Module):
    """Standalone MSE loss head for API parity with the reference
    (layers.py:145-166): forward is the IDENTITY (the loss value is
    never computed in training, layers.py:150-155); backward takes the
    TARGET as its dout argument and emits −2(t−x)/global_batch
    (functional.py:43-44).  The fused SoftmaxMSE head below is the hot
    path; this module exists for hand-built Sequential stacks.

    GPU note: −2(t−x)/GB == (x−t)/(GB/2), so the backward reuses the
    fused xent elementwise kernel with a halved batch scale."""

    def __init__(self, global_batch_size: int):
        super().__init__()
        self.global_batch_size = global_batch_size

    def forward(self, inputs, mubatch_id: int = 0):
        self._stash("x", mubatch_id, inputs)
        return inputs

    def backward(self, target, mubatch_id: int = 0):
        x = self._unstash("x", mubatch_id)
        if target.dtype != x.dtype:
            target = target.to(x.dtype)
        return F.head_softmax_xent_bwd(x, target, self.global_batch_size / 2.0)


class _LossHead(Module):
    """Fused softmax+loss head.

    Forward emits PROBS (so the pipeline output buffer holds softmax
    probabilities, same as the reference where MSELoss.forward is the
    identity after Softmax — layers.py:150-155, and eval argmaxes the
    output buffer, train.py:40-43).  Backward takes the TARGET as its
    dout argument (reference layers.py:157-163) and emits d(logits)
    in one fused op, scaled by the GLOBAL batch size so µbatch/DP
    gradients sum to the sequential gradient (layers.py:146-148).

    Training metrics: with an accumulator in `_metrics` (see
    Sequential.set_metrics) a training-mode backward also adds the
    µbatch's loss sum, argmax matches and row counts to it
    (F.head_metrics, one small launch, no host sync).
    """

    kind = None      # "xent" | "mse": the loss F.head_metrics reports
    _metrics = None  # metrics accumulator, or None (off)

    def __init__(self, global_batch_size: int):
        super().__init__()
        self.global_batch_size = global_batch_size

    def forward(self, inputs, mubatch_id: int = 0):
        s = F.softmax_fwd(inputs)
        self._stash("s", mubatch_id, s)
        return s

    def _bwd(self, probs, target):
        raise NotImplementedError

    def backward(self, target, mubatch_id: int = 0):
        s = self._unstash("s", mubatch_id)
        if target.dtype != s.dtype:
            target = target.to(s.dtype)
        if self._metrics is not None and self._training:
            F.head_metrics(s, target, self._metrics, self.kind)
        return self._bwd(s, target)


class SoftmaxMSE(_LossHead):
    """Softmax → MSE, matching the reference's Softmax+MSELoss pair
    (layers.py:83-96,145-166) as ONE fused head."""

    kind = "mse"

    def _bwd(self, probs, target):
        return F.head_softmax_mse_bwd(probs, target, self.global_batch_size)


class SoftmaxXent(_LossHead):
    """Fused softmax-cross-entropy head: dz = (s − t)/GB.  The improved
    default loss head (BASELINE.json north star)."""

    kind = "xent"

    def _bwd(self, probs, target):
        return F.head_softmax_xent_bwd(probs, target, self.global_batch_size)


class Sequential(Module):
    """Layer chain with the grad-hook API.  Reference: layers.py:169-233.

    backward() reverse-chains layers and, after each layer's backward,
    fires the per-parameter grad hooks (layers.py:201-208) — the
    injection point for the DP all-reduce overlap — then the post-grad
    hooks over all parameters (layers.py:210-211).
    """

    def __init__(self, layers):
        super().__init__()
        self.layers = list(layers)
        # dropout state shared by every Linear of the chain; whether any
        # layer drops is fixed here, so the p = 0 hot path pays one
        # attribute test for the feature
        self._dropout = DropoutState()
        for layer in self.layers:
            if isinstance(layer, Linear):
                layer._drop_state = self._dropout
        self._has_dropout = any(getattr(l, "dropout", 0.0) > 0.0
                                for l in self.layers)
        self._grad_hooks = []
        self._post_grad_hooks = []
        # set True on pipeline stage 0: the first Linear's input grad is
        # dL/d(data) — never consumed — so its dgrad GEMM is skipped
        # (the most expensive dgrad: K = input width).
        self._skip_input_grad = False
        # set by the Worker for the temporally-LAST backward of a batch
        # under deferred wgrad: each layer's pending µbatch wgrad chunks
        # flush the moment that layer's backward completes, so its grads
        # are final MID-backward and the DP bucket all-reduce fired from
        # the grad hooks overlaps the remaining layers' dgrad/wgrad
        # kernels (reference pipe.py:302-316 semantics, restored for the
        # deferred path — round-1 deferred all grads to OptimizerStep).
        self._flush_in_backward = False

    # Linear(activation=None) -> SoftmaxXent at the end of the chain may
    # run as the fused head kernels (csrc/head.hip); subclasses whose
    # last Linear is not a plain one opt out.
    _fuse_head = True

    # ---- dropout state (see DropoutState / F.dropout_keep_mask)
    @property
    def dropout_seed(self) -> int:
        return self._dropout.seed

    @dropout_seed.setter
    def dropout_seed(self, seed: int):
        self._dropout.seed = int(seed)

    @property
    def dropout_step(self) -> int:
        """Optimizer steps taken: the mask's `step` counter word."""
        return self._dropout.step

    @dropout_step.setter
    def dropout_step(self, step: int):
        self._dropout.step = int(step)

    def set_sample_rows(self, mubatch_id: int, first: int, stride: int = 1):
        """Row i of µbatch `mubatch_id` is sample first + i·stride of
        the unsharded dataset order (the Worker sets this before each
        Forward; default (0, 1) for hand-driven models)."""
        self._dropout.rows[mubatch_id] = (int(first), int(stride))

    def has_dropout(self) -> bool:
        """Whether any layer was built with dropout > 0."""
        return self._has_dropout

    def _head_pair(self):
        """(last Linear, SoftmaxXent head) when the chain ends in that
        pair, else None."""
        if not self._fuse_head or len(self.layers) < 2:
            return None
        lin, head = self.layers[-2], self.layers[-1]
        if type(head) is SoftmaxXent and type(lin) is Linear \
                and lin.activation is None:
            return lin, head
        return None

    # width of the chain kernels (csrc/fwd_chain.hip, csrc/bwd_chain.hip)
    # and the most ReLU layers one launch of either takes
    _CHAIN_WIDTH = 256
    _CHAIN_MAX_LAYERS = 8

    def _chain_head_pair(self):
        """_head_pair() when its Linear has the head geometry of the
        chain kernels (256 -> C <= 16, no fp8 forward), else None."""
        pair = self._head_pair()
        if pair is None or pair[0].in_dims != self._CHAIN_WIDTH \
                or pair[0].out_dims > 16 or pair[0].fp8_fwd:
            return None
        return pair

    def _chain_run(self):
        """Indices, top first, of the consecutive Linear(activation=
        "relu") layers with out_dims == 256 right under the head pair,
        at most _CHAIN_MAX_LAYERS.  A chain plan is a prefix of it."""
        run = []
        for i in range(len(self.layers) - 3, -1, -1):
            layer = self.layers[i]
            if len(run) == self._CHAIN_MAX_LAYERS \
                    or type(layer) is not Linear \
                    or layer.activation != "relu" \
                    or layer.out_dims != self._CHAIN_WIDTH:
                break
            run.append(i)
        return run

    def _fwd_chain_plan(self):
        """Which layers the forward chain kernel (F.fwd_chain) takes
        together with the head: their indices, bottom first, or None
        when the head or the layers under it do not qualify.

        The chain is the fused head (Linear(256 -> C <= 16) +
        SoftmaxXent) and the run of Linear(activation="relu") layers
        with out_dims == 256 right below it, at most eight.  A layer is
        in the chain when in_dims == 256, or, with F.fwd_chain_l1(),
        when it ends the run and in_dims % 8 == 0.  No chain with
        dropout or an fp8 forward on a layer it would take.  Looks at
        the layer configuration only — no tensors, no device."""
        if not F.fwd_chain_enabled() or not F.head_fused() \
                or self._chain_head_pair() is None:
            return None
        plan = []
        for i in self._chain_run():
            layer = self.layers[i]
            streamed = layer.in_dims != self._CHAIN_WIDTH
            if streamed and not (F.fwd_chain_l1() and layer.in_dims >= 8
                                 and layer.in_dims % 8 == 0):
                break
            if layer.dropout > 0.0 or layer.fp8_fwd:
                return None
            plan.append(i)
            if streamed:
                break
        return plan[::-1] or None

    def _forward_chain(self, plan, lin, head, x, mubatch_id):
        """Forward of the planned ReLU layers and the head pair through
        ONE F.fwd_chain launch, leaving the stashes the layers' own
        forwards leave.  Returns probs, or None with no stash touched
        when the tensors do not meet the kernel's contract."""
        if not F.head_fused_ok(x, lin):
            return None
        chain = [self.layers[i] for i in plan]
        # a deferred zero_grad rides in this launch (same stream, ahead
        # of every kernel that adds to the gradients)
        zero = self._flat_grad if getattr(self, "_zero_pending", False) \
            and self._flat_grad.device == x.device else None
        res = F.fwd_chain(x, [l.weight.compute() for l in chain],
                          [l.bias.compute() for l in chain],
                          lin.weight.compute(), lin.bias.compute(),
                          zero=zero)
        if res is None:
            return None
        if zero is not None:
            self._zero_pending = False
        hs, probs = res
        for layer, h in zip(chain, hs):
            layer._stash("x", mubatch_id, x)
            layer._stash("y", mubatch_id, h)
            x = h
        lin._stash("x", mubatch_id, x)
        head._stash("s", mubatch_id, probs)
        return probs

    def forward(self, inputs, mubatch_id: int = 0):
        x = inputs
        pair = self._head_pair()
        n_plain = len(self.layers) - 2 if pair else len(self.layers)
        plan = self._fwd_chain_plan() if pair and inputs.is_cuda else None
        if plan:
            # layers below the chain run their own forward first
            for layer in self.layers[:plan[0]]:
                x = layer.forward(x, mubatch_id)
            s = self._forward_chain(plan, pair[0], pair[1], x, mubatch_id)
            if s is not None:
                return s
            first = plan[0]
        else:
            first = 0
        # no chain launch took a deferred zero_grad along
        self._settle_zero_grad()
        for layer in self.layers[first:n_plain]:
            x = layer.forward(x, mubatch_id)
        if pair:
            lin, head = pair
            if F.head_fused_ok(x, lin):
                # same stashes as the two layers' own forwards, so
                # either backward path can follow
                lin._stash("x", mubatch_id, x)
                s = F.head_fwd_fused(x, lin.weight.compute(),
                                     lin.bias.compute())
                head._stash("s", mubatch_id, s)
                return s
            x = head.forward(lin.forward(x, mubatch_id), mubatch_id)
        return x

    def _fire_grad_hooks(self, layer):
        # deferred-wgrad final backward: complete this layer's grads
        # NOW (before its grad hooks fire) so param_done sees final
        # values and the bucket all-reduce launches mid-backward
        if self._flush_in_backward and hasattr(layer, "flush_wgrad"):
            layer.flush_wgrad()
        for hook in self._grad_hooks:
            for p in layer.parameters():
                if p.requires_grad:
                    hook(p)

    def _backward_head_fused(self, lin, head, target, mubatch_id):
        """Fused backward of the head pair; returns dx of the Linear.
        The weight gradient can ride in the same kernel
        (F.set_head_wgrad_fused) unless it is deferred (chunk kept for
        the flush) or deterministic (the single-owner wgrad kernel
        keeps the bitwise contract); otherwise the wgrad kernel takes
        the fused kernel's dz."""
        s = head._unstash("s", mubatch_id)
        x = lin._unstash("x", mubatch_id)
        if target.dtype != s.dtype:
            target = target.to(s.dtype)
        if not target.is_contiguous():
            target = target.contiguous()
        in_kernel = (F.head_wgrad_fused() and not lin._defer_wgrad
                     and not F.deterministic())
        # training metrics ride in the same kernel (no second launch)
        # unless the standalone launch is asked for
        acc = head._metrics if head._training else None
        if acc is not None and not F.head_metrics_fused():
            F.head_metrics(s, target, acc, head.kind)
            acc = None
        dz, dx = F.head_bwd_fused(
            s, target, x, lin.weight.compute_t(), head.global_batch_size,
            lin.weight.grad if in_kernel else None,
            lin.bias.grad if in_kernel else None, metrics=acc)
        if lin._defer_wgrad:
            lin._wgrad_pending.append((dz, x, None))
            if len(lin._wgrad_pending) >= lin._wgrad_window:
                lin.flush_wgrad()
        elif not in_kernel:
            F.linear_wgrad_acc(dz, x, lin.weight.grad, lin.bias.grad)
        self._fire_grad_hooks(head)
        self._fire_grad_hooks(lin)
        return dx

    def _bwd_chain_plan(self, mubatch_rows: int = 1):
        """Which layers the backward chain kernel (F.bwd_chain) takes:
        a list of (layer index, dgrad_in_chain), top layer first, or
        None when the head or the layers under it do not qualify.

        The chain is the fused head (Linear(256 -> C <= 16) +
        SoftmaxXent) and the run of Linear(activation="relu") layers
        with out_dims == 256 right below it.  A layer's dgrad is in the
        chain when in_dims == 256 and its dx is needed; the chain ends
        with the first layer whose dgrad is not (that layer still gets
        its dz from the kernel), or above the first layer that is no
        such Linear.  Looks at the layer configuration only — no
        tensors, no device."""
        if mubatch_rows < 1 or not F.bwd_chain_enabled() \
                or not F.head_fused() or F.head_wgrad_fused() \
                or self._chain_head_pair() is None:
            return None
        plan = []
        for i in self._chain_run():
            layer = self.layers[i]
            need_dx = not (i == 0 and self._skip_input_grad)
            in_chain = need_dx and layer.in_dims == self._CHAIN_WIDTH
            if not in_chain and plan and not F.bwd_chain_dz_last():
                break  # measured alternative: stop at dh of this layer
            plan.append((i, in_chain))
            if not in_chain:
                break
        # one dz scale per launch: the chain only when every planned
        # layer has the same drop probability (all 0: today's kernel);
        # a mix takes the per-layer path
        if self._has_dropout and \
                len({self.layers[i].dz_scale() for i, _ in plan}) > 1:
            return None
        return plan or None

    def _wgrad_of(self, layer, dz, x):
        """Unmasked weight gradient of `layer` from its dz: now, or kept
        for the deferred flush (same window logic as Linear.backward)."""
        if layer._defer_wgrad:
            layer._wgrad_pending.append((dz, x, None))
            if len(layer._wgrad_pending) >= layer._wgrad_window:
                layer.flush_wgrad()
        else:
            F.linear_wgrad_acc(dz, x, layer.weight.grad, layer.bias.grad)

    def _backward_chain(self, plan, lin, head, target, mubatch_id):
        """Backward of the head pair and the planned ReLU layers through
        ONE F.bwd_chain launch, then the unmasked wgrads in the
        per-layer order (head, then top to bottom): through one grouped
        call (_wgrad_group), or one launch per layer in deterministic
        mode, under deferred wgrad and with F.set_wgrad_group(False);
        grad hooks fire after the launch that holds the layer.  Returns (True, dx of the lowest planned layer), or
        (False, None) with no stash touched when the tensors do not meet
        the kernel's contract."""
        s = head._cache.get(("s", mubatch_id))
        x = lin._cache.get(("x", mubatch_id))
        chain = [self.layers[i] for i, _ in plan]
        hs = [l._cache.get(("y", mubatch_id)) for l in chain]
        if s is None or x is None or any(h is None for h in hs) \
                or not F.head_fused_ok(x, lin):
            return False, None
        if target.dtype != s.dtype:
            target = target.to(s.dtype)
        if not target.is_contiguous():
            target = target.contiguous()
        w_ts = [l.weight.compute_t() for l, (_, dg) in zip(chain, plan) if dg]
        res = F.bwd_chain(s, target, lin.weight.compute_t(),
                          head.global_batch_size, hs, w_ts,
                          dz_scale=chain[0].dz_scale())
        if res is None:
            return False, None
        dz_head, dzs, dx = res
        # the chain kernel does not count: the standalone metrics launch
        # reads the same probs / target (only when metrics are on)
        if head._metrics is not None and head._training:
            F.head_metrics(s, target, head._metrics, head.kind)
        head._unstash("s", mubatch_id)
        lin._unstash("x", mubatch_id)
        # deterministic mode keeps the single-owner kernel per layer,
        # deferred wgrad keeps its chunks for the flush
        grouped = F.wgrad_group_enabled() and not F.deterministic() \
            and not any(l._defer_wgrad for l in [lin] + chain)
        items = [(lin, dz_head, x, (head, lin))]
        if not grouped:
            self._wgrad_of(lin, dz_head, x)
            self._fire_grad_hooks(head)
            self._fire_grad_hooks(lin)
        for layer, (i, dg), dz in zip(chain, plan, dzs):
            xl = layer._unstash("x", mubatch_id)
            layer._unstash("y", mubatch_id)
            if not dg and not (i == 0 and self._skip_input_grad):
                # the chain ended at this layer's dz but its dx is
                # needed (in_dims != 256): the ordinary unmasked dgrad
                dx = F.linear_dgrad(dz, layer.weight.compute(),
                                    layer.weight.compute_t())
            if grouped:
                items.append((layer, dz, xl, (layer,)))
                continue
            self._wgrad_of(layer, dz, xl)
            self._fire_grad_hooks(layer)
        if grouped:
            self._wgrad_group(items)
        return True, dx

    def _wgrad_group(self, items):
        """Weight gradients of `items`, (layer, dz, x, layers whose grad
        hooks follow), through F.linear_wgrad_group: same-tile layers
        share a launch.  Without grad hooks that is one call.  With
        hooks the list is cut at the launch boundaries and a layer's
        hooks fire right after the launch that holds its gradient, in
        the per-layer order, so a later launch (the first layer's) is
        issued after the hooks of the layers before it and no bucket
        waits on a wgrad it does not need."""
        probs = [(dz, x, l.weight.grad, l.bias.grad) for l, dz, x, _ in items]
        if not self._grad_hooks:
            cuts = [list(range(len(items)))]
        elif probs[0][0].is_cuda:
            cuts = [la["problems"] for la in F.wgrad_group_plan(
                [(dz.shape[0], dz.shape[1], x.shape[1])
                 for dz, x, _, _ in probs])]
        else:
            cuts = [[k] for k in range(len(items))]
        for cut in cuts:
            F.linear_wgrad_group([probs[k] for k in cut])
            for k in cut:
                for hl in items[k][3]:
                    self._fire_grad_hooks(hl)

    def backward(self, dout, mubatch_id: int = 0):
        self._settle_zero_grad()
        d = dout
        last = len(self.layers) - 1
        pair = self._head_pair()
        plan = self._bwd_chain_plan(dout.shape[0]) \
            if pair and dout.is_cuda else None
        if plan:
            ok, dx = self._backward_chain(plan, pair[0], pair[1], d,
                                          mubatch_id)
            if ok:
                d = dx
                last = plan[-1][0] - 1
                pair = None
        if pair:
            lin, head = pair
            x = lin._cache.get(("x", mubatch_id))
            need_dx = not (last == 1 and self._skip_input_grad)
            if x is not None and need_dx and F.head_fused_ok(x, lin):
                d = self._backward_head_fused(lin, head, d, mubatch_id)
                last -= 2
        for i in range(last, -1, -1):
            layer = self.layers[i]
            if i == 0 and self._skip_input_grad and isinstance(layer, Linear):
                d = layer.backward(d, mubatch_id, need_dx=False)
            else:
                d = layer.backward(d, mubatch_id)
            self._fire_grad_hooks(layer)
        for hook in self._post_grad_hooks:
            hook(self.parameters())
        return d

    # hook (de)registration — reference layers.py:182-199
    def register_grad_hook(self, fn):
        self._grad_hooks.append(fn)

    def reset_grad_hooks(self):
        self._grad_hooks = []

    def register_post_grad_hook(self, fn):
        self._post_grad_hooks.append(fn)

    def reset_post_grad_hooks(self):
        self._post_grad_hooks = []

    def parameters(self):
        return [p for layer in self.layers for p in layer.parameters()]

    def zero_grad(self, defer=False):
        """Zero every gradient.  defer=True lets the next forward chain
        launch write the zeros (F.fwd_chain(zero=...)) instead of a
        memset launch of its own: the buffer is only marked, and holds
        its old values until that forward, or until _settle_zero_grad()
        at whatever reads or adds to the gradients first.  Deferred only
        with a flat gradient buffer on the GPU and a forward chain plan
        (F.fwd_zero_grads() on); the memset is done at once otherwise."""
        flat = getattr(self, "_flat_grad", None)
        self._zero_pending = False
        if flat is None:
            for layer in self.layers:
                layer.zero_grad()
        elif defer and flat.is_cuda and F.fwd_zero_grads() \
                and self._fwd_chain_plan():
            self._zero_pending = True
        else:
            flat.zero_()

    def _settle_zero_grad(self):
        """The memset a zero_grad(defer=True) still owes, now."""
        if getattr(self, "_zero_pending", False):
            self._zero_pending = False
            self._flat_grad.zero_()

    def train(self):
        self._training = True
        for l in self.layers:
            l.train()

    def eval(self):
        self._training = False
        for l in self.layers:
            l.eval()

    def set_metrics(self, acc):
        """Point the loss head at a metrics accumulator
        (F.new_metrics_acc), or at None to stop counting.  Returns True
        when this chain ends in a loss head."""
        head = self.layers[-1] if self.layers else None
        if not isinstance(head, _LossHead):
            return False
        head._metrics = acc
        return True

    def set_fp8_fwd(self, flag: bool):
        """Enable the MX-fp8 training forward on every qualifying
        Linear (O%256, I%256; per-call µbatch%256 check in _fp8_ok).
        Backward stays bf16; masters stay f32."""
        n = 0
        for layer in self.layers:
            if isinstance(layer, Linear) and layer.activation in (None, "relu") \
                    and layer.out_dims % 256 == 0 and layer.in_dims % 256 == 0:
                layer.fp8_fwd = flag
                layer._wq = layer._ws = None
                n += 1
        return n

    def invalidate_fp8(self):
        """Drop cached fp8 weight copies (call after every optimizer
        step / checkpoint load so the next forward re-quantizes)."""
        for layer in self.layers:
            if getattr(layer, "_wq", None) is not None:
                layer._wq = layer._ws = None

    def set_defer_wgrad(self, flag: bool, window: int = 1 << 30):
        """Enable/disable deferred-µbatch wgrad on every Linear
        (pipeline schedules with >1 µbatch; flushed before the
        optimizer step).  window caps retained µbatches — pass the
        schedule's max_in_flight so 1F1B's activation-memory bound
        survives deferral."""
        for layer in self.layers:
            if hasattr(layer, "_defer_wgrad"):
                layer._defer_wgrad = flag
                layer._wgrad_window = max(1, window)

    def flush_wgrads(self, per_layer_hook=None):
        """Flush any REMAINING deferred weight gradients layer by layer
        in backward order; returns how many layers still had pending
        chunks.  On the normal path this is a no-op safety net — the
        final (AllReduce) backward flushes in-backward via
        _flush_in_backward; leftovers here mean a schedule never issued
        BackwardGradAllReduce."""
        self._settle_zero_grad()
        n = 0
        for layer in reversed(self.layers):
            if hasattr(layer, "flush_wgrad") and layer._wgrad_pending:
                layer.flush_wgrad()
                n += 1
            if per_layer_hook is not None:
                per_layer_hook(layer)
        return n

    def materialize_device(self, device, compute_dtype=None):
        """Move to device, set compute dtype, and re-point every
        parameter grad into ONE flat f32 buffer (bucketing substrate;
        the reference's per-param MPI messages are called out as
        wasteful in its own docstring, pipe.py:309-310)."""
        device = torch.device(device)
        if compute_dtype is None:
            compute_dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        F.clear_wgrad_tables()  # grad buffers are about to be repointed
        self.device = device
        self.compute_dtype = compute_dtype
        for layer in self.layers:
            layer.materialize_device(device, compute_dtype)
        params = [p for p in self.parameters() if p.requires_grad]
        total = sum(p.data.numel() for p in params)
        flat = torch.zeros(total, dtype=torch.float32, device=device)
        off = 0
        for p in params:
            n = p.data.numel()
            p.grad = flat[off:off + n].view(p.data.shape)
            off += n
        self._flat_grad = flat
        self._zero_pending = False
        return self


class MLP(Sequential):
    """Stage-sliced deep MLP.  Reference: layers.py:236-270.

    sizes: full list of layer boundaries.  Each pipeline stage takes its
    slice with ONE-ELEMENT OVERLAP (layers.py:247-250), builds
    Linear(..., relu) per consecutive pair with NO activation on the
    very last Linear of the last stage (layers.py:251-260), and the last
    stage appends the fused loss head (reference: Softmax+MSELoss,
    layers.py:261-263; default here: softmax-cross-entropy).

    dropout=p puts inverted dropout on every ReLU Linear (never on the
    head Linear) with layer_index = the Linear's index in the full
    `sizes` list, and dropout_seed seeds the mask: every stage of every
    partition then draws the serial model's bits.
    """

    def __init__(self, sizes, stage_idx=0, n_stages=1, global_batch_size=1,
                 loss="xent", dropout=0.0, dropout_seed=0):
        assert len(sizes) % n_stages == 0, (
            f"len(sizes)={len(sizes)} must divide into {n_stages} stages"
        )
        stage_size = len(sizes) // n_stages
        lo = stage_idx * stage_size
        bounds = sizes[lo:lo + stage_size + 1]
        is_last = stage_idx == n_stages - 1
        layers = []
        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            last_linear = is_last and i == len(bounds) - 2
            # dropout on every ReLU Linear, never on the head Linear;
            # layer_index is global so stage slicing keeps the mask
            if last_linear:
                layers.append(Linear(a, b, activation=None,
                                     layer_index=lo + i))
            else:
                layers.append(Linear(a, b, activation="relu",
                                     dropout=dropout, layer_index=lo + i))
        if is_last:
            head = {"xent": SoftmaxXent, "mse": SoftmaxMSE}[loss](global_batch_size)
            layers.append(head)
        super().__init__(layers)
        self.dropout_seed = dropout_seed
        self.stage_idx, self.n_stages = stage_idx, n_stages
        self._skip_input_grad = stage_idx == 0
        self.in_dim = bounds[0]
        self.out_dim = bounds[-1] if not is_last else sizes[-1]
