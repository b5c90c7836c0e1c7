"""The fused optimizer kernels of csrc/elementwise.hip against float64:
sgd_multi / adamw_multi (v1) and sgd_multi2 / adamw_multi2 (v2) called
directly through the extension on the tables of optimizer_oracle.Arena,
then through SGD / AdamW with the block-map threshold lowered, and the
tiled bf16 transpose.  References, bounds, cases and the bitwise checks
(lp, lp_t, grad, margins, buffers the table does not point to) are in
tests/optimizer_oracle.py; tests/test_optimizer_oracle.py holds the CPU
paths to the same bounds.

v1 and v2 see the same inputs and are each held to the same reference;
they are not required to agree bitwise (FMA contraction may differ).
"""

import pytest
import torch

import optimizer_oracle as O
from optimizer_oracle import BF

pytestmark = pytest.mark.gpu


def ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def launch(ar, ver):
    e, hp = ext(), ar.hp
    if ar.kind == "sgd":
        args = (hp["lr"], hp["momentum"], hp["weight_decay"])
        if ver == "v1":
            e.sgd_multi(ar.desc, args[0], ar.total, *args[1:])
        else:
            e.sgd_multi2(ar.desc, ar.bmap, *args)
    else:
        args = O.adamw_host_args(hp)
        if ver == "v1":
            e.adamw_multi(ar.desc, args[0], ar.total, *args[1:])
        else:
            e.adamw_multi2(ar.desc, ar.bmap, *args)
    torch.cuda.synchronize()


def run_case(device, kind, hp, ver, name, shapes, no_lpt=frozenset()):
    ar = O.Arena(kind, hp, O.make_state(name, shapes), device, no_lpt)
    launch(ar, ver)
    ar.check(f"{kind}_multi{'2' if ver == 'v2' else ''} {O.hyper_id(hp)} "
             f"{name}")


HYPERS = [("sgd", hp) for hp in O.SGD_HYPERS] \
    + [("adamw", hp) for hp in O.ADAMW_HYPERS]
HYPER_IDS = [f"{k}-{O.hyper_id(hp)}" for k, hp in HYPERS]
FULL = [("sgd", O.SGD_FULL), ("adamw", O.ADAMW_FULL)]
FULL_IDS = ["sgd", "adamw"]


@pytest.mark.parametrize("kind,hp", HYPERS, ids=HYPER_IDS)
@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_mixed_table(gpu_device, ver, kind, hp):
    """Sizes around 4 / 1024 / 16384, grads at all four offsets mod 4,
    2-D weights with the in-kernel lp_t scatter (130 x 127 over two
    blocks), and the (64, 1024) weight whose lp_t pointer is 0."""
    run_case(gpu_device, kind, hp, ver, "mixed", O.MIXED_SHAPES,
             O.MIXED_NO_LPT)


@pytest.mark.parametrize("kind,hp", FULL, ids=FULL_IDS)
@pytest.mark.parametrize("ver", ["v1", "v2"])
@pytest.mark.parametrize("T", list(O.V1_SMALL))
def test_small_tables(gpu_device, T, ver, kind, hp):
    """The descriptor search at T in {1, 2, 3, 7, 8, 9} with one-element
    tensors first and last."""
    run_case(gpu_device, kind, hp, ver, f"T{T}", O.V1_SMALL[T])


@pytest.mark.parametrize("kind,hp", FULL, ids=FULL_IDS)
@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_second_grid_stride_pass(gpu_device, ver, kind, hp):
    """262144 + 773 elements: the v1 grid (1024 x 256) takes a second,
    partial pass, with a tensor split between the passes."""
    run_case(gpu_device, kind, hp, ver, "two_pass", O.V1_TWO_PASS)


# ------------------------------------------------------ through the classes

class _Recorder:
    """The extension, noting which entry points are called."""

    def __init__(self, e):
        self._e, self.calls = e, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._e, name)


def _snapshot(params, s1, s2):
    def cpu(ts):
        return None if ts is None else [t.detach().cpu().clone() for t in ts]

    return {"master": cpu([p.data for p in params]),
            "grad": cpu([p.grad for p in params]), "s1": cpu(s1),
            "s2": cpu(s2)}


@pytest.mark.parametrize("kind,hp", FULL, ids=FULL_IDS)
def test_classes_on_the_blockmap_path(gpu_device, monkeypatch, kind, hp):
    """SGD (momentum + wd) and AdamW, three steps each, on a 127 -> 130
    -> 10 stack plus a Linear(1024, 64), whose weight goes to the tiled
    transpose after the block-map kernel; each step against the oracle
    from the device's own state before it."""
    from shallowspeed_amd.models import SGD, AdamW, Linear, Sequential
    from shallowspeed_amd.models import optimizer as opt_mod

    rec = _Recorder(ext())
    monkeypatch.setattr(opt_mod, "BLOCKMAP_MIN_ELEMS", 1)
    monkeypatch.setattr(opt_mod, "load_ext", lambda required=False: rec)
    model = Sequential([Linear(127, 130, activation="relu"),
                        Linear(130, 10), Linear(1024, 64)])
    model.materialize_device(gpu_device)
    params = model.parameters()
    if kind == "sgd":
        opt = SGD(params, lr=hp["lr"], momentum=hp["momentum"],
                  weight_decay=hp["weight_decay"])
        s1, s2 = opt._vel, None
    else:
        opt = AdamW(params, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                    weight_decay=hp["weight_decay"])
        s1, s2 = opt._m, opt._v
    shapes = tuple(tuple(p.data.shape) for p in params)
    for step in range(1, 4):
        grads = O.make_state(f"class_step{step}", shapes)["grad"]
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        before = _snapshot(params, s1, s2)
        opt.step()
        torch.cuda.synchronize()
        after = _snapshot(params, s1, s2)
        O.check_step(kind, dict(hp, step=step), before, after,
                     f"{kind} class step {step}")
        for p, g0, g1 in zip(params, before["grad"], after["grad"]):
            assert torch.equal(O.bits(g0), O.bits(g1)), "grad changed"
            assert torch.equal(O.bits(p.lp), O.bits(p.data.to(BF)))
            if p.lp_t is not None:
                assert torch.equal(O.bits(p.lp_t),
                                   O.bits(p.lp.t().contiguous()))
    v2, v1 = f"{kind}_multi2", f"{kind}_multi"
    assert rec.calls.count(v2) == 3 and v1 not in rec.calls, rec.calls
    tiled = [p for p, _, _ in opt._tiled_t]
    assert [tuple(p.data.shape) for p in tiled] == [(64, 1024)]
    assert rec.calls.count("transpose_bf16") == 3, rec.calls
    assert rec.calls.index(v2) < rec.calls.index("transpose_bf16")


# ---------------------------------------------------------------- transpose

@pytest.mark.parametrize("rows,cols", [(64, 64), (64, 1024), (192, 1088)])
def test_transpose_bf16(gpu_device, rows, cols):
    g = O.gen("transpose", rows, cols)
    x = torch.randn(rows, cols, generator=g).to(BF)
    n = rows * cols
    buf = torch.full((n + O.MARGIN,), O.SENTINEL, dtype=BF,
                     device=gpu_device)
    dst = buf[:n].view(cols, rows)
    src = x.to(gpu_device)
    ext().transpose_bf16(src, dst)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(O.bits(got[:n].view(cols, rows)),
                       O.bits(x.t().contiguous()))
    assert torch.equal(got[n:], torch.full((O.MARGIN,), O.SENTINEL,
                                           dtype=BF)), "wrote past dst"
    assert torch.equal(O.bits(src), O.bits(x)), "src changed"
