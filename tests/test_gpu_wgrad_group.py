"""wgrad_tn_group: independent unmasked weight gradients side by side in
one launch (wgrad_group_kernel), planned by wgrad_group_plan.

Operands are small integers, as in test_wgrad_onchip_reduce: every sum
is exact in f32, so a result must be BITWISE equal to the f64 reference
whatever the split or the arrival order.  A block that decodes the wrong
problem, tile, K-range or bias owner cannot hide in rounding noise.
"""

import pytest
import torch

from test_wgrad_onchip_reduce import _int_case

pytestmark = pytest.mark.gpu

_cache = {}


def _ext():
    from shallowspeed_amd.ops import load_ext

    return load_ext(required=True)


def _plan(shapes, splits=None):
    from shallowspeed_amd.ops import functional as F

    return F.wgrad_group_plan(shapes, splits)


def _case(dev, shape, seed=0):
    """Unmasked integer case of `shape`; seed 0 is _int_case's own, any
    other seed gives other data of the same shape (computed once,
    shared, never modified)."""
    if seed == 0:
        return _int_case(dev, shape, False)
    key = (shape, seed)
    if key not in _cache:
        Kb, Mo, N = shape
        g = torch.Generator().manual_seed(7919 * seed + 1000 * Kb + 10 * Mo + N)
        dy = torch.randint(-2, 3, (Kb, Mo), generator=g).to(dev)
        x = torch.randint(-2, 3, (Kb, N), generator=g).to(dev)
        w0 = torch.randint(-3, 4, (Mo, N), generator=g).to(dev)
        b0 = torch.randint(-3, 4, (Mo,), generator=g).to(dev)
        ref_w = dy.double().t() @ x.double()
        ref_b = dy.double().sum(0)
        assert (w0.abs().max() + 2 * ref_w.abs().max()) < 2 ** 24
        _cache[key] = dict(dy=dy.bfloat16(), x=x.bfloat16(),
                           w0=w0.float(), b0=b0.float(),
                           ref_w=ref_w.float(), ref_b=ref_b.float())
    return _cache[key]


def _run_and_check(dev, shapes, splits=None, seeds=None, times=1):
    seeds = seeds or [0] * len(shapes)
    cs = [_case(dev, s, sd) for s, sd in zip(shapes, seeds)]
    outs = [(c["w0"].clone(), c["b0"].clone()) for c in cs]
    probs = [(c["dy"], c["x"], gw, gb) for c, (gw, gb) in zip(cs, outs)]
    for _ in range(times):
        _ext().wgrad_tn_group(probs, splits)
    for c, (gw, gb) in zip(cs, outs):
        assert torch.equal(gw, c["w0"] + times * c["ref_w"])
        assert torch.equal(gb, c["b0"] + times * c["ref_b"])


SMALL64 = [(264, 10, 256), (328, 256, 256), (200, 64, 80)]
BIG128 = [(192, 256, 528), (448, 256, 528)]
MIXED = [(264, 10, 256), (328, 256, 256), (192, 256, 528), (128, 64, 80)]


def test_group_of_one(gpu_device):
    _run_and_check(gpu_device, [(64, 64, 64)])


@pytest.mark.parametrize("order", [1, -1], ids=["fwd", "rev"])
def test_three_64_tile_shapes(gpu_device, order):
    shapes = SMALL64[::order]
    assert [la["problems"] for la in _plan(shapes)] == [[0, 1, 2]]
    _run_and_check(gpu_device, shapes)


def test_two_problems_of_one_shape_with_different_data(gpu_device):
    _run_and_check(gpu_device, [(328, 256, 256)] * 2, seeds=[0, 1])


def test_two_128_tile_problems(gpu_device):
    assert [la["problems"] for la in _plan(BIG128)] == [[0, 1]]
    _run_and_check(gpu_device, BIG128)


def test_mixed_list_becomes_the_expected_launches(gpu_device):
    assert [la["problems"] for la in _plan(MIXED)] == [[0, 1], [2], [3]]
    _run_and_check(gpu_device, MIXED)


def test_nine_problems_split_eight_and_one(gpu_device):
    shapes = [(128, 64, 80)] * 9
    assert [la["problems"] for la in _plan(shapes)] == \
        [list(range(8)), [8]]
    _run_and_check(gpu_device, shapes, seeds=list(range(9)))


@pytest.mark.parametrize("splits", [
    [0, 0, 0], [2, 2, 2], [4, 4, 4], [7, 7, 7], [2, 7, 4], [0, 4, 2],
], ids=lambda s: "-".join(map(str, s)))
def test_splits_per_problem(gpu_device, splits):
    _run_and_check(gpu_device, SMALL64, splits=splits)


def test_split_4_of_one_k_step_leaves_k_groups_empty(gpu_device):
    _run_and_check(gpu_device, [(64, 64, 64), (200, 64, 80)], splits=[4, 2])


def test_two_problems_into_the_same_buffers(gpu_device):
    shape = (328, 256, 256)
    a, b = _case(gpu_device, shape, 0), _case(gpu_device, shape, 1)
    gw, gb = a["w0"].clone(), a["b0"].clone()
    _ext().wgrad_tn_group([(a["dy"], a["x"], gw, gb),
                           (b["dy"], b["x"], gw, gb)])
    assert torch.equal(gw, a["w0"] + a["ref_w"] + b["ref_w"])
    assert torch.equal(gb, a["b0"] + a["ref_b"] + b["ref_b"])


def test_same_call_twice(gpu_device):
    _run_and_check(gpu_device, SMALL64, times=2)
    _run_and_check(gpu_device, BIG128, times=2)


@pytest.mark.parametrize("shapes", [SMALL64, BIG128, MIXED],
                         ids=["64", "128", "mixed"])
def test_sentinel_margins_between_the_outputs(gpu_device, shapes):
    """All gW / gb are carved out of ONE flat buffer with margins: a
    decode that takes another problem's N or Mo writes into a margin or
    into a neighbour."""
    cs = [_case(gpu_device, s) for s in shapes]
    margin, sentinel = 64, -12345.0
    sizes = []
    for c in cs:
        sizes += [c["w0"].numel(), c["b0"].numel()]
    flat = torch.full((margin + sum(n + margin for n in sizes),), sentinel,
                      device=gpu_device)
    views, off = [], margin
    for n in sizes:
        views.append(flat[off:off + n])
        off += n + margin
    probs, keep = [], torch.ones_like(flat, dtype=torch.bool)
    for k, c in enumerate(cs):
        gw = views[2 * k].view_as(c["w0"])
        gb = views[2 * k + 1]
        gw.copy_(c["w0"])
        gb.copy_(c["b0"])
        probs.append((c["dy"], c["x"], gw, gb))
    off = margin
    for n in sizes:
        keep[off:off + n] = False
        off += n + margin
    _ext().wgrad_tn_group(probs)
    for c, (_, _, gw, gb) in zip(cs, probs):
        assert torch.equal(gw, c["w0"] + c["ref_w"])
        assert torch.equal(gb, c["b0"] + c["ref_b"])
    assert torch.equal(flat[keep], torch.full_like(flat[keep], sentinel))


@pytest.mark.parametrize("absent", [None, "empty"])
def test_gb_absent_for_one_problem(gpu_device, absent):
    cs = [_case(gpu_device, s) for s in SMALL64]
    outs = [(c["w0"].clone(), c["b0"].clone()) for c in cs]
    no_gb = None if absent is None else torch.Tensor()
    probs = [(c["dy"], c["x"], gw, no_gb if k == 1 else gb)
             for k, (c, (gw, gb)) in enumerate(zip(cs, outs))]
    _ext().wgrad_tn_group(probs)
    for k, (c, (gw, gb)) in enumerate(zip(cs, outs)):
        assert torch.equal(gw, c["w0"] + c["ref_w"])
        assert torch.equal(gb, c["b0"] + (0 if k == 1 else 1) * c["ref_b"])


def _refused(dev, mutate, splits=None):
    cs = [_case(dev, s) for s in SMALL64]
    outs = [(c["w0"].clone(), c["b0"].clone()) for c in cs]
    probs = [[c["dy"], c["x"], gw, gb] for c, (gw, gb) in zip(cs, outs)]
    mutate(probs)
    with pytest.raises(RuntimeError):
        _ext().wgrad_tn_group([tuple(p) for p in probs], splits)
    torch.cuda.synchronize()
    for c, (gw, gb) in zip(cs, outs):
        assert torch.equal(gw, c["w0"]) and torch.equal(gb, c["b0"])


def test_refuses_a_shape_mismatch_and_touches_nothing(gpu_device):
    def bad_x(probs):  # last problem: x of another batch size
        probs[2][1] = _case(gpu_device, (264, 10, 256))["x"][:, :80] \
            .contiguous()
    _refused(gpu_device, bad_x)

    def bad_gw(probs):
        probs[2][2] = torch.zeros(64, 64, device=gpu_device)
    _refused(gpu_device, bad_gw)


def test_refuses_a_non_bf16_operand_and_touches_nothing(gpu_device):
    def f32_dy(probs):
        probs[2][0] = probs[2][0].float()
    _refused(gpu_device, f32_dy)


def test_refuses_split_1_and_touches_nothing(gpu_device):
    _refused(gpu_device, lambda probs: None, splits=[0, 0, 1])


def test_empty_list_is_a_no_op(gpu_device):
    _ext().wgrad_tn_group([])
    assert _plan([]) == []


@pytest.mark.parametrize("shapes,splits", [
    (SMALL64, None), (BIG128, None), (MIXED, None), (MIXED, [2, 7, 0, 4]),
    ([(128, 64, 80)] * 9, None),
    ([(16384, 10, 256), (16384, 256, 256), (16384, 256, 256),
      (16384, 256, 784)], None),
], ids=["64", "128", "mixed", "mixed-splits", "nine", "flagship"])
def test_plan_properties(gpu_device, shapes, splits):
    plan = _plan(shapes, splits)
    seen = [k for la in plan for k in la["problems"]]
    assert seen == list(range(len(shapes)))  # each once, order kept

    def cfg(shape):  # (tile rows, tile cols) as wgrad_cfg picks them
        _, Mo, N = shape
        big = (Mo >= 256 and N >= 512) or (Mo >= 512 and N >= 256)
        return (128, 128) if big else (64, 64)

    for la in plan:
        assert 1 <= len(la["problems"]) <= 8
        assert len({cfg(shapes[k]) for k in la["problems"]}) == 1
        for k, s, b in zip(la["problems"], la["splits"], la["blocks"]):
            Kb, Mo, N = shapes[k]
            bm, bn = cfg(shapes[k])
            tiles = -(-Mo // bm) * -(-N // bn)
            assert b == tiles * s  # the grid
            assert 1 <= s <= -(-Kb // 64)
            if splits and splits[k]:
                assert s <= splits[k]
