"""Float64 references, derived error bounds, the seeded cases and a
descriptor-table builder for the fused optimizer kernels of
csrc/elementwise.hip: sgd_multi / adamw_multi (v1, grid-stride with a
per-element search of the descriptor table) and sgd_multi2 / adamw_multi2
(v2, block map: 16384 elements of one tensor per block, 1024 per
iteration, 4 per thread, a scalar tail, scalar grad loads when the grad
view is not 16-byte aligned).

A plain helper module (no tests, no fixtures), like rowwise_oracle.py.
tests/test_optimizer_oracle.py runs every case through the CPU paths of
SGD / AdamW and through torch.optim, tests/test_gpu_optimizer.py through
the kernels; both see the same tensors, references and bounds.

The reference is ONE optimizer step in float64 from the same f32 tensors
the kernel reads.  A test of several steps feeds the device's own f32
state back into the reference at every step, so nothing compounds and
every bound stays a statement about one step.

Hyper-parameters enter the reference as the f32 values the launcher
receives (each rounded once from the host double).  1 - beta is
f32(1 - beta) with the difference taken in double: that is what the CPU
path (`add_(g, alpha=1 - b1)`) and torch.optim.AdamW use.  1 - f32(beta)
is a different number: for beta2 = 0.999 it is 0.00099998713, 1.29e-5
(216 u) below 0.001.

Bounds, with u = 2^-24 (one f32 rounding: |fl(a) - a| <= u|a|) and a
2^-126 floor per product that may underflow (flushed or subnormal).  None
comes from the code under test, and each holds with or without FMA
contraction (an FMA only removes a rounding):

SGD    g' = g + wd m ; v' = mu v + g' ; m' = m - lr v'
       with mag = |g| + |wd m| + |mu v|:
  v'   wd m and mu v round once each (u|wd m|, u|mu v|), the two sums
       once each, of partial sums <= mag: below 3u mag, held to
           4u mag + 2 floors.
  m'   lr v' rounds once (u lr|v'|), the difference once
       (u|m'| <= u(|m| + lr|v'|)), |v'| <= mag, and the error of v' comes
       through multiplied by lr:
           2u(|m| + lr mag) + lr bound(v') + floor.

AdamW  m1 = b1 ea + (1-b1) g ; v1 = b2 es + (1-b2) g^2
       p  = m (1 - lr wd) - term, term = lr m1 ibc1 / (sqrt(v1 ibc2) + eps)
  m1   two products and a sum: 4u(b1|ea| + (1-b1)|g|) + 2 floors.
  v1   ((1-b2) g) g, b2 es and the sum: four roundings of non-negative
       terms, each relative: below 4u v1, held to 5u v1 + 2 floors (g^2
       leaves the normal range for |g| < 1e-19).
  p    the decay m - (lr wd) m: lr wd and its product with m round once
       each (2u lr wd|m|), the difference once (u|m|).  term from the
       computed moments: m1 ibc1, lr times it, v1 ibc2 (halved by the
       root), the root, the sum with eps and the quotient round once
       each, 5.5u|term| (10.5u if root and quotient are 2.5-ulp
       approximations).  The last difference: u(|m| + |term|).  In all
       below 2.1u|m| + 11.5u|term|, held to
           4u(|m| + |term|) + 8u|term| + floor
       plus the moments' own bounds carried through term: bound(m1)
       times lr ibc1 / den, and |term(v1 +- bound(v1)) - term(v1)|
       evaluated in f64 (the derivative has a pole at v1 = 0), capped at
       |term|.

Exact, bit for bit: lp == bf16(the device's own new master), lp_t ==
lp.t(), grad unchanged, every buffer whose table pointer is 0 unchanged,
and the margin around every buffer unchanged.
"""

import functools

import torch

from rowwise_oracle import BF, FLOOR, U, bits, check, gen

EPB = 16384          # elements a v2 block owns (SS_OPT_EPB)
V1_GRID = 1024 * 256  # threads of a full v1 grid: one grid-stride pass
MARGIN = 61          # elements between two tensors of one buffer
SENTINEL = -7.5      # fills margins and unowned buffers
UNWRITTEN = 3.25     # fills lp / lp_t, which the kernel must overwrite


def f32(x):
    """The f32 nearest to x, as a Python float (a double holding it)."""
    return float(torch.tensor(x, dtype=torch.float64).float())


# ------------------------------------------------------------ hyper-params

SGD_HYPERS = tuple(dict(lr=0.05, momentum=mu, weight_decay=wd)
                   for mu in (0.0, 0.9) for wd in (0.0, 0.01))
ADAMW_HYPERS = tuple(dict(lr=0.02, betas=(0.9, 0.999), eps=1e-8,
                          weight_decay=wd, step=step)
                     for step in (1, 1000) for wd in (0.0, 0.01))
SGD_FULL = SGD_HYPERS[3]      # momentum + weight decay
ADAMW_FULL = ADAMW_HYPERS[3]  # step 1000, weight decay


def hyper_id(hp):
    if "betas" in hp:
        return f"step{hp['step']}-wd{hp['weight_decay']}"
    return f"mu{hp['momentum']}-wd{hp['weight_decay']}"


def adamw_host_args(hp):
    """The doubles AdamW.step hands the extension: (lr, b1, b2, 1 - b1,
    1 - b2, eps, wd, inv_bc1, inv_bc2)."""
    b1, b2 = hp["betas"]
    t = hp["step"]
    return (hp["lr"], b1, b2, 1 - b1, 1 - b2, hp["eps"],
            hp["weight_decay"], 1.0 / (1.0 - b1 ** t), 1.0 / (1.0 - b2 ** t))


# --------------------------------------------------------------- references

def cat(ts):
    return torch.cat([t.detach().cpu().reshape(-1) for t in ts])


def sgd_ref(m, g, v, hp):
    """(ref, bound) per output of one SGD step from flat f32 tensors;
    v is None when there is no velocity."""
    lr, mu, wd = f32(hp["lr"]), f32(hp["momentum"]), f32(hp["weight_decay"])
    md, gd = m.double(), g.double()
    wdm = wd * md
    muv = mu * v.double() if v is not None else torch.zeros_like(md)
    mag = gd.abs() + wdm.abs() + muv.abs()
    v1 = muv + (gd + wdm)
    bv = 4 * U * mag + 2 * FLOOR
    m1 = md - lr * v1
    bm = 2 * U * (md.abs() + lr * mag) + lr * bv + FLOOR
    out = {"master": (m1, bm)}
    if v is not None:
        out["velocity"] = (v1, bv)
    return out


def adamw_ref(m, g, ea, es, hp, omb2=None):
    """(ref, bound) per output of one AdamW step from flat f32 tensors.
    omb2 overrides the reference's 1 - beta2 (the control of
    test_optimizer_oracle.py)."""
    lr, b1, b2, omb1_d, omb2_d, eps, wd, ibc1, ibc2 = adamw_host_args(hp)
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    ibc1, ibc2 = f32(ibc1), f32(ibc2)
    omb1 = f32(omb1_d)
    omb2 = f32(omb2_d) if omb2 is None else omb2
    md, gd, ead, esd = m.double(), g.double(), ea.double(), es.double()
    m1 = b1 * ead + omb1 * gd
    bm1 = 4 * U * (b1 * ead.abs() + omb1 * gd.abs()) + 2 * FLOOR
    v1 = b2 * esd + omb2 * gd * gd
    bv1 = 5 * U * v1 + 2 * FLOOR

    def term_at(v):
        return lr * (m1 * ibc1) / ((v * ibc2).sqrt() + eps)

    term = term_at(v1)
    den = (v1 * ibc2).sqrt() + eps
    from_m1 = lr * ibc1 / den * bm1
    from_v1 = torch.maximum((term_at(v1 + bv1) - term).abs(),
                            (term_at((v1 - bv1).clamp_min(0)) - term).abs())
    from_v1 = torch.minimum(from_v1, term.abs())
    p = md * (1.0 - lr * wd) - term
    bp = (4 * U * (md.abs() + term.abs()) + 8 * U * term.abs()
          + from_m1 + from_v1 + FLOOR)
    return {"exp_avg": (m1, bm1), "exp_avg_sq": (v1, bv1), "master": (p, bp)}


def check_step(kind, hp, before, after, what):
    """One step's outputs against the reference formed from `before`.
    before / after: dicts of lists of tensors — master, grad, and s1 / s2
    (velocity, or exp_avg / exp_avg_sq) where they exist.  Reports every
    output before it fails."""
    m0, g0 = cat(before["master"]), cat(before["grad"])
    if kind == "sgd":
        v0 = cat(before["s1"]) if hp["momentum"] else None
        ref = sgd_ref(m0, g0, v0, hp)
        got = {"master": after["master"]}
        if v0 is not None:
            got["velocity"] = after["s1"]
    else:
        ref = adamw_ref(m0, g0, cat(before["s1"]), cat(before["s2"]), hp)
        got = {"exp_avg": after["s1"], "exp_avg_sq": after["s2"],
               "master": after["master"]}
    errors = []
    for name, ts in got.items():
        out = cat(ts)
        assert out.dtype == torch.float32, (what, name, out.dtype)
        try:
            check(out, ref[name][0], ref[name][1], f"{what} {name}")
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, "\n".join(errors)


# -------------------------------------------------------------------- cases

def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


# Sizes around the v2 structure (4 a thread, 1024 an iteration, 16384 a
# block) and 2-D weights with the in-kernel lp_t scatter: 130 x 127 spans
# two blocks and its row ends fall inside 4-groups; (64, 1024) is the
# shape the optimizers hand to the tiled transpose, so its table entry
# has lp_t = 0.  The order puts the grad views of the tensors of four
# and more elements at all four offsets mod 4 (asserted by
# test_optimizer_oracle.py).
MIXED_SHAPES = (
    (1,), (3,), (4,), (5,), (3, 5), (1023,), (1024,), (33, 65), (1025,),
    (16383,), (16384,), (130, 127), (16385,), (64, 320),
    (16384 + 1024 + 2,), (2 * 16384 + 7,), (64, 1024),
)
MIXED_NO_LPT = frozenset({(64, 1024)})

# v1 tables of T tensors, one-element tensors first and last
V1_SMALL = {
    1: ((300,),),
    2: ((1,), (1,)),
    3: ((1,), (3, 5), (1,)),
    7: ((1,), (257,), (2, 3), (1,), (64,), (9, 7), (1,)),
    8: ((1,), (5,), (256,), (255,), (1,), (7, 9), (31,), (1,)),
    9: ((1,), (1,), (513,), (2,), (33, 3), (1,), (100,), (3,), (1,)),
}

# 262144 + 3 * 256 + 5 elements: a second (partial) grid-stride pass of
# the v1 kernels; the (500,) tensor holds elements 262051 .. 262550, so
# it is split between the passes
V1_TWO_PASS = ((1,), (150, 127), (243000,), (500,), (365,), (1,))
assert sum(_numel(s) for s in V1_TWO_PASS) == V1_GRID + 3 * 256 + 5

_GRAD_SCALES = (0.0, 1e-20, 1e-4, 1.0, 1e3)


@functools.lru_cache(maxsize=None)
def make_state(name, shapes):
    """Seeded inputs of one step: dict of tuples of CPU f32 tensors
    (master, grad, s1, s2).  Shared between tests: never written to.

    grad    N(0, 1) times a per-element scale from {0, 1e-20, 1e-4, 1,
            1e3}: exact zeros are what dead ReLU units produce
    master  N(0, 1), some exact zeros, some +-1e-30
    s1      half exact zeros, otherwise 0.1 N(0, 1) times the grad scale
            mix (a velocity or an exp_avg)
    s2      half exact zeros, otherwise a square of such values (an
            exp_avg_sq: never negative)"""
    g = gen("optimizer", name, len(shapes))
    out = {"master": [], "grad": [], "s1": [], "s2": []}
    scales = torch.tensor(_GRAD_SCALES)
    for shape in shapes:
        def randn():
            return torch.randn(shape, generator=g)

        def pick(n):
            return torch.randint(0, n, shape, generator=g)

        grad = randn() * scales[pick(5)]
        master = randn()
        kind = pick(20)
        master[kind == 0] = 0.0
        master[kind == 1] = 1e-30
        master[kind == 2] = -1e-30
        s1 = 0.1 * randn() * scales[pick(5)]
        s1[pick(2) == 0] = 0.0
        s2 = (randn() * scales[pick(5)]) ** 2
        s2[pick(2) == 0] = 0.0
        for k, t in (("master", master), ("grad", grad), ("s1", s1),
                     ("s2", s2)):
            assert t.dtype == torch.float32 and torch.isfinite(t).all()
            out[k].append(t)
    return {k: tuple(v) for k, v in out.items()}


# ------------------------------------------------------------ table builder

def blockmap_rows(numels, epb=EPB):
    return [[i, b] for i, n in enumerate(numels) for b in range(0, n, epb)]


def _round_up(x, k):
    return (x + k - 1) // k * k


class Arena:
    """The buffers of one launch and its descriptor table.

    Every tensor is a span of one flat buffer per role, with MARGIN
    sentinel elements before and after it:
      master, s1, s2  f32, spans 16-byte aligned; every other span is NOT
                      32-byte aligned
      lp              bf16, spans 8-byte aligned; every other span is NOT
                      16-byte aligned
      lp_t            bf16, spans at even and odd element offsets
      grad            f32, ONE flat buffer without margins, each tensor
                      at its running offset, as
                      Sequential.materialize_device lays it out
    lp and lp_t start out as UNWRITTEN, so an element the kernel skips
    shows in the bitwise checks whatever its value would have been.

    kind "sgd" gives [T, 8] rows (velocity pointer 0 unless
    hp["momentum"]), "adamw" [T, 9].  Shapes in `no_lpt` get lp_t = 0 in
    the table although their lp_t span exists."""

    ROLES = ("master", "s1", "s2", "lp", "lp_t")

    def __init__(self, kind, hp, state, device, no_lpt=frozenset()):
        self.kind, self.hp, self.state = kind, hp, state
        self.shapes = [tuple(t.shape) for t in state["master"]]
        self.numels = [_numel(s) for s in self.shapes]
        T = len(self.shapes)
        self.spans = {r: [] for r in self.ROLES}
        ends = {}
        for role in self.ROLES:
            off = MARGIN
            for k, n in enumerate(self.numels):
                if role == "lp_t":
                    off += k % 2
                else:
                    off = _round_up(off, 8) + (4 if k % 2 else 0)
                self.spans[role].append((off, n))
                off += n + MARGIN
            ends[role] = off
        self.cpu0 = {}
        for role in self.ROLES:
            dt = BF if role in ("lp", "lp_t") else torch.float32
            buf = torch.full((ends[role],), SENTINEL, dtype=dt)
            for k, (off, n) in enumerate(self.spans[role]):
                if role in ("lp", "lp_t"):
                    buf[off:off + n] = UNWRITTEN
                else:
                    buf[off:off + n] = state[role][k].reshape(-1)
            self.cpu0[role] = buf
        self.cpu0["grad"] = cat(state["grad"])
        self.dev = {r: b.to(device, copy=True) for r, b in self.cpu0.items()}

        # which spans the step must write; all else must keep its bits
        has_s1 = kind == "adamw" or bool(hp["momentum"])
        self.lpt_on = [len(s) == 2 and s not in no_lpt for s in self.shapes]
        self.written = {
            "master": [True] * T, "lp": [True] * T,
            "s1": [has_s1] * T, "s2": [kind == "adamw"] * T,
            "lp_t": self.lpt_on}

        def ptr(role, k):
            b = self.dev[role]
            return b.data_ptr() + self.spans[role][k][0] * b.element_size()

        rows, start = [], 0
        gbase = self.dev["grad"].data_ptr()
        self.grad_offsets = []
        for k, (shape, n) in enumerate(zip(self.shapes, self.numels)):
            row = [ptr("master", k), gbase + 4 * start, ptr("lp", k),
                   ptr("lp_t", k) if self.lpt_on[k] else 0, n,
                   shape[1] if len(shape) == 2 else 1, start,
                   ptr("s1", k) if has_s1 else 0]
            if kind == "adamw":
                row.append(ptr("s2", k))
            assert row[0] % 16 == 0 and row[2] % 8 == 0
            assert all(p % 16 == 0 for p in row[7:])
            rows.append(row)
            self.grad_offsets.append(start)
            start += n
        self.total = start
        self.rows = rows
        self.bmap_rows = blockmap_rows(self.numels)
        self.desc = torch.tensor(rows, dtype=torch.int64).to(device)
        self.bmap = torch.tensor(self.bmap_rows, dtype=torch.int64).to(device)

    def view(self, bufs, role, k):
        off, n = self.spans[role][k]
        return bufs[role][off:off + n]

    def readback(self):
        """(raw CPU buffers, the after-state as check_step takes it)."""
        raw = {r: b.detach().cpu() for r, b in self.dev.items()}
        T = len(self.shapes)
        after = {r: [self.view(raw, r, k) for k in range(T)]
                 for r in ("master", "s1", "s2")}
        return raw, after

    def check_exact(self, raw, what):
        """The bitwise half of the contract, on the buffers read back."""
        errors = []

        def same(got, want, msg):
            gb, wb = bits(got), bits(want)
            if not torch.equal(gb, wb):
                bad = (gb != wb).flatten().nonzero().flatten()
                errors.append(f"{what}: {msg}: {bad.numel()} of "
                              f"{gb.numel()} elements differ, first at "
                              f"{int(bad[0])}: got "
                              f"{got.flatten()[int(bad[0])].item()!r} want "
                              f"{want.flatten()[int(bad[0])].item()!r}")

        same(raw["grad"], self.cpu0["grad"], "grad changed")
        for role in self.ROLES:
            keep = torch.ones(raw[role].numel(), dtype=torch.bool)
            for k, (off, n) in enumerate(self.spans[role]):
                if self.written[role][k]:
                    keep[off:off + n] = False
            same(raw[role][keep], self.cpu0[role][keep],
                 f"{role}: margins / spans the table does not point to")
        for k, shape in enumerate(self.shapes):
            master = self.view(raw, "master", k)
            lp = self.view(raw, "lp", k)
            same(lp, master.to(BF), f"lp[{k}] {shape} != bf16(master)")
            if self.lpt_on[k]:
                want = lp.view(shape).t().contiguous().reshape(-1)
                same(self.view(raw, "lp_t", k), want,
                     f"lp_t[{k}] {shape} != lp.t()")
        assert not errors, "\n".join(errors)

    def check(self, what):
        raw, after = self.readback()
        errors = []
        for f in (lambda: check_step(self.kind, self.hp, self.state, after,
                                     what),
                  lambda: self.check_exact(raw, what)):
            try:
                f()
            except AssertionError as e:
                errors.append(str(e))
        assert not errors, "\n".join(errors)
