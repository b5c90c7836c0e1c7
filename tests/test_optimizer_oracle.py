"""The optimizer oracle on the CPU: every case of optimizer_oracle.py
through the CPU paths of SGD / AdamW and through torch.optim, all inside
the derived bounds, so the bounds are shown to hold for the reference
paths alone; a control showing that the bounds REJECT an exp_avg_sq
formed with 1 - f32(beta2); the table builder's layout and its bitwise
checks against a CPU stand-in for the kernels, correct and with the two
defects the cases are chosen to catch; and _build_blockmap's properties.

tests/test_gpu_optimizer.py runs the same cases through the HIP kernels.
"""

import pytest
import torch

import optimizer_oracle as O
from optimizer_oracle import BF
from shallowspeed_amd.models import SGD, AdamW, Parameter
from shallowspeed_amd.models import optimizer as opt_mod

CASES = {"mixed": O.MIXED_SHAPES, "two_pass": O.V1_TWO_PASS}
CASES.update({f"T{t}": s for t, s in O.V1_SMALL.items()})
HYPERS = [("sgd", hp) for hp in O.SGD_HYPERS] \
    + [("adamw", hp) for hp in O.ADAMW_HYPERS]
HYPER_IDS = [f"{k}-{O.hyper_id(hp)}" for k, hp in HYPERS]


# ----------------------------------------------------------- CPU backends

def step_repo(kind, hp, st):
    """One step of the repository's CPU path from the case's state."""
    params = [Parameter(m.clone()) for m in st["master"]]
    for p, g in zip(params, st["grad"]):
        p.grad = g.clone()
    if kind == "sgd":
        opt = SGD(params, lr=hp["lr"], momentum=hp["momentum"],
                  weight_decay=hp["weight_decay"])
        if opt._vel is not None:
            for v, s in zip(opt._vel, st["s1"]):
                v.copy_(s)
        s1, s2 = opt._vel, None
    else:
        opt = AdamW(params, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                    weight_decay=hp["weight_decay"])
        opt.step_count = hp["step"] - 1
        for dst, src in zip(opt._m + opt._v, st["s1"] + st["s2"]):
            dst.copy_(src)
        s1, s2 = opt._m, opt._v
    opt.step()
    for p, g in zip(params, st["grad"]):
        assert torch.equal(p.grad, g)
    return {"master": [p.data for p in params], "s1": s1, "s2": s2}


def step_torch(kind, hp, st):
    """One step of torch.optim from the case's state."""
    params = [m.clone().requires_grad_(True) for m in st["master"]]
    for p, g in zip(params, st["grad"]):
        p.grad = g.clone()
    if kind == "sgd":
        opt = torch.optim.SGD(params, lr=hp["lr"], momentum=hp["momentum"],
                              weight_decay=hp["weight_decay"])
        s1 = [s.clone() for s in st["s1"]] if hp["momentum"] else None
        if s1 is not None:
            for p, v in zip(params, s1):
                opt.state[p]["momentum_buffer"] = v
        s2 = None
    else:
        opt = torch.optim.AdamW(params, lr=hp["lr"], betas=hp["betas"],
                                eps=hp["eps"],
                                weight_decay=hp["weight_decay"])
        s1 = [s.clone() for s in st["s1"]]
        s2 = [s.clone() for s in st["s2"]]
        for p, a, b in zip(params, s1, s2):
            opt.state[p]["step"] = torch.tensor(float(hp["step"] - 1))
            opt.state[p]["exp_avg"] = a
            opt.state[p]["exp_avg_sq"] = b
    opt.step()
    if kind == "adamw":
        assert all(int(opt.state[p]["step"]) == hp["step"] for p in params)
    return {"master": [p.detach() for p in params], "s1": s1, "s2": s2}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind,hp", HYPERS, ids=HYPER_IDS)
@pytest.mark.parametrize("backend", [step_repo, step_torch],
                         ids=["repo", "torch"])
def test_cpu_paths_inside_bounds(backend, kind, hp, case):
    st = O.make_state(case, CASES[case])
    after = backend(kind, hp, st)
    O.check_step(kind, hp, st, after,
                 f"{backend.__name__} {kind} {O.hyper_id(hp)} {case}")


# ---------------------------------------------------------------- control

def test_f32_one_minus_beta2_is_a_different_number():
    b2 = 0.999
    host = O.f32(1 - b2)
    kernel = 1.0 - O.f32(b2)  # exact in double, and what 1.f - beta2 gives
    assert O.f32(kernel) == kernel
    rel = (kernel - host) / host
    print(f"f32(1 - b2) = {host!r}  1 - f32(b2) = {kernel!r}  rel {rel:.3e} "
          f"= {rel / O.U:.0f} u")
    assert -1.4e-5 < rel < -1.2e-5


@pytest.mark.parametrize("hp", O.ADAMW_HYPERS, ids=O.hyper_id)
def test_bounds_reject_f32_one_minus_beta2(hp):
    """exp_avg_sq and master of a step taken with 1 - f32(beta2), each
    rounded ONCE from float64 (no other error at all), against the
    oracle: exp_avg_sq must fall outside its bound.  That is the value
    a kernel computing 1.f - beta2 lands on, so the GPU test sees it."""
    st = O.make_state("two_pass", O.V1_TWO_PASS)
    m, g = O.cat(st["master"]), O.cat(st["grad"])
    ea, es = O.cat(st["s1"]), O.cat(st["s2"])
    b2 = hp["betas"][1]
    good = O.adamw_ref(m, g, ea, es, hp)
    bad = O.adamw_ref(m, g, ea, es, hp, omb2=1.0 - O.f32(b2))
    # the rounded reference itself passes: the bound is not vacuous
    for name, (ref, bound) in good.items():
        O.check(ref.float(), ref, bound, f"control {name}: f32(ref)")
    ref, bound = good["exp_avg_sq"]
    got = bad["exp_avg_sq"][0].float()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"1 - f32(b2): exp_avg_sq worst err / bound {ratio:.1f}")
    with pytest.raises(AssertionError, match="outside the bound"):
        O.check(got, ref, bound, "control exp_avg_sq: 1 - f32(b2)")
    # 1.29e-5 / 5u = 43: wherever g^2 dominates the new moment
    assert ratio > 30


# ---------------------------------------------------------- table builder

def test_mixed_case_covers_the_v2_paths():
    ar = O.Arena("adamw", O.ADAMW_FULL, O.make_state("mixed", O.MIXED_SHAPES),
                 "cpu", O.MIXED_NO_LPT)
    # all four grad offsets mod 4 among tensors with a vector path: only
    # offset 0 is 16-byte aligned, the others take the scalar grad loads
    offs = {o % 4 for o, n in zip(ar.grad_offsets, ar.numels) if n >= 4}
    assert offs == {0, 1, 2, 3}, offs
    # aligned AND misaligned grads both occur with a tail and with a
    # second block
    for aligned in (True, False):
        sel = [n for o, n in zip(ar.grad_offsets, ar.numels)
               if (o % 4 == 0) == aligned]
        assert any(n % 4 and n > 4 for n in sel), aligned
        assert any(n > O.EPB for n in sel), aligned
    # a 2-D tensor with lp_t on, more than one block, and rows that end
    # inside a 4-group; one with lp_t = 0 in the table
    assert any(on and n > O.EPB and s[1] % 4
               for on, n, s in zip(ar.lpt_on, ar.numels, ar.shapes))
    assert [s for on, s in zip(ar.lpt_on, ar.shapes)
            if len(s) == 2 and not on] == [(64, 1024)]
    # alignment of the spans: as the kernels need, and no better
    for role, need in (("master", 4), ("s1", 4), ("s2", 4), ("lp", 4)):
        offs = [o for o, _ in ar.spans[role]]
        assert all(o % need == 0 for o in offs)
        assert any(o % (2 * need) for o in offs), role
    assert {o % 2 for o, _ in ar.spans["lp_t"]} == {0, 1}
    # spans are disjoint with a margin between them
    for role in ar.ROLES:
        end = 0
        for o, n in ar.spans[role]:
            assert o >= end + O.MARGIN
            end = o + n
        assert ar.cpu0[role].numel() >= end + O.MARGIN
    assert ar.total == sum(ar.numels) and len(ar.bmap_rows) == sum(
        -(-n // O.EPB) for n in ar.numels)


def test_v1_tables():
    for t, shapes in O.V1_SMALL.items():
        assert len(shapes) == t
        if t > 1:
            assert shapes[0] == (1,) and shapes[-1] == (1,)
    starts, s = [], 0
    for shape in O.V1_TWO_PASS:
        starts.append(s)
        s += O._numel(shape)
    assert s > O.V1_GRID and s - O.V1_GRID < O.V1_GRID
    assert any(a < O.V1_GRID < a + O._numel(sh)
               for a, sh in zip(starts, O.V1_TWO_PASS))


def _stand_in(ar, drop_tail=False, lpt_by_row=False):
    """Writes f32(reference) into the arena's (CPU) buffers the way a
    correct kernel would; drop_tail leaves out the last n % 4 elements of
    every tensor, lpt_by_row stores lp_t in lp's own order."""
    st = ar.state
    for k, (shape, n) in enumerate(zip(ar.shapes, ar.numels)):
        one = {r: [st[r][k]] for r in ("master", "grad", "s1", "s2")}
        m, g = O.cat(one["master"]), O.cat(one["grad"])
        if ar.kind == "sgd":
            v = O.cat(one["s1"]) if ar.hp["momentum"] else None
            ref = O.sgd_ref(m, g, v, ar.hp)
            outs = {"master": ref["master"][0]}
            if v is not None:
                outs["s1"] = ref["velocity"][0]
        else:
            ref = O.adamw_ref(m, g, O.cat(one["s1"]), O.cat(one["s2"]),
                              ar.hp)
            outs = {"master": ref["master"][0], "s1": ref["exp_avg"][0],
                    "s2": ref["exp_avg_sq"][0]}
        done = n - n % 4 if drop_tail else n
        for role, val in outs.items():
            ar.view(ar.dev, role, k)[:done] = val.float()[:done]
        lp = ar.view(ar.dev, "master", k).to(BF)
        ar.view(ar.dev, "lp", k)[:done] = lp[:done]
        if ar.lpt_on[k]:
            r, c = shape
            i = torch.arange(done)
            where = i if lpt_by_row else (i % c) * r + i // c
            ar.view(ar.dev, "lp_t", k)[where] = lp[:done]


@pytest.mark.parametrize(
    "kind,hp", [("sgd", O.SGD_FULL), ("sgd", O.SGD_HYPERS[0]),
                ("adamw", O.ADAMW_FULL)],
    ids=["sgd-full", "sgd-plain", "adamw-full"])
def test_checks_accept_a_correct_step_and_catch_two_defects(kind, hp):
    st = O.make_state("mixed", O.MIXED_SHAPES)

    def arena():
        return O.Arena(kind, hp, st, "cpu", O.MIXED_NO_LPT)

    ar = arena()
    _stand_in(ar)
    ar.check(f"stand-in {kind}")
    # the e + 4 > n tail dropped: the skipped masters miss the bound
    # wherever the step moves them, and their lp keeps UNWRITTEN
    ar = arena()
    _stand_in(ar, drop_tail=True)
    with pytest.raises(AssertionError) as e:
        ar.check(f"no tail {kind}")
    assert "outside the bound" in str(e.value) and "!= bf16(master)" in \
        str(e.value)
    # lp_t stored in row order
    ar = arena()
    _stand_in(ar, lpt_by_row=True)
    with pytest.raises(AssertionError, match=r"!= lp\.t\(\)"):
        ar.check(f"lp_t by row {kind}")
    # a store one element past a tensor's end lands in a margin
    ar = arena()
    _stand_in(ar)
    off, n = ar.spans["s1" if kind == "adamw" else "master"][5]
    ar.dev["s1" if kind == "adamw" else "master"][off + n] = 1.0
    with pytest.raises(AssertionError, match="margins"):
        ar.check(f"overrun {kind}")


# ---------------------------------------------------------- _build_blockmap

class _P:
    def __init__(self, n):
        self.data = torch.empty(n)


@pytest.mark.parametrize("epb", [16384, 4, 1])
@pytest.mark.parametrize("numels", [
    (1,), (16384,), (16385,), (5, 1, 32768, 16383, 49153, 2),
    tuple(O._numel(s) for s in O.MIXED_SHAPES)], ids=str)
def test_build_blockmap_properties(numels, epb):
    if epb < 16384:
        numels = tuple(min(n, 37) for n in numels)
    bmap = opt_mod._build_blockmap([_P(n) for n in numels], "cpu", epb=epb)
    assert bmap.dtype == torch.int64 and bmap.dim() == 2 \
        and bmap.shape[1] == 2
    rows = bmap.tolist()
    # the row count, and rows in tensor order (bases ascending within one)
    assert len(rows) == sum(-(-n // epb) for n in numels)
    assert rows == sorted(rows)
    seen = [torch.zeros(n, dtype=torch.int32) for n in numels]
    for t, base in rows:
        assert 0 <= t < len(numels)
        assert base % epb == 0 and 0 <= base < numels[t]
        seen[t][base:base + epb] += 1
    # every element of every tensor in exactly one block
    assert all(bool((s == 1).all()) for s in seen)
    assert rows == O.blockmap_rows(numels, epb)


def test_threshold_is_one_module_attribute():
    assert opt_mod.BLOCKMAP_MIN_ELEMS == 1 << 22


def test_build_desc_alignment_assertion():
    ok = [[1 << 20, 4, 1 << 12, 2, 8, 1, 0, 1 << 16, 1 << 17]]
    opt_mod._check_blockmap_alignment(ok)
    opt_mod._check_blockmap_alignment([[1 << 20, 4, 0, 0, 8, 1, 0, 0]])
    for col, delta in ((0, 4), (0, 8), (7, 4), (8, 8), (2, 2), (2, 4)):
        bad = [list(ok[0])]
        bad[0][col] += delta
        with pytest.raises(AssertionError, match="aligned"):
            opt_mod._check_blockmap_alignment(bad)
