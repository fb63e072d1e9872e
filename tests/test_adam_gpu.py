"""Adam in the three places it is applied -- ``adam_kernel`` (flat), ``adam_tiled_kernel`` (64 x 64 tiles, transposed
shadow) and the epilogue of ``gemm_bf16_grouped_wgrad_adam_kernel`` -- against Adam written out in fp64 (``adam_ref``), each
through the C ABI on its own.  tests/test_wgrad_routes_gpu.py has the gradient kernels and the helpers used here.

The reference is fed the FLOAT32 values of lr, betas, eps, weight_decay, grad_scale that the ABI passes (the kernel cannot
know the double 0.98) and the step t read back from the device counter.  Compared, each on its own: exp_avg, exp_avg_sq,
the UPDATE p_old - p_new (not the parameter: p_new is a large number minus a small one, an update that is 0.3 % wrong moves
it by 1e-6 of its scale), the bf16 shadow (== p_new rounded to bf16, exactly, from the kernel's own fp32 result), the
transposed shadow (== shadow.t(), exactly) and every byte outside the updated ranges (``Sentinel``).

Bars (elementwise, absolute; u = 2^-24; worst case, no headroom factor), from ``adam_update1`` (csrc/common.h):
    gk = fma(wd, p, g gs)                 2 roundings of terms no larger than G = |g gs| + |wd p|:   |err| <= 2 u G
    m' = fma(b1, m, (1 - b1) gk)          (1 - b1 is exact for b1 >= 0.5) product + fma + gk's error:
                                          |err| <= u (|m'| + (1 - b1) |gk| + 2 (1 - b1) G) <= 4 u A_m,  A_m = b1 |m| + (1 - b1) G
    v' = fma(b2, v, ((1 - b2) gk) gk)     two products, the fma, gk's error twice:
                                          |err| <= u (|v'| + 2 (1 - b2) gk^2 + 4 (1 - b2) G^2) <= 7 u A_v,  A_v = b2 v + (1 - b2) G^2
    denom = fma(sqrtf(v'), isb, eps)      sqrtf and the fma are correctly rounded, eps only shrinks the relative error:
                                          denom_kernel / denom >= sqrt(1 - r_v) (1 - 2 u - e_isb),  r_v = 7 u A_v / v'
    p' = p - (step m') / denom            product, quotient (correctly rounded under the default -fhip-fp32-correctly-
                                          rounded-divide-sqrt), then ONE rounding of p': u |p'| <= u (|p| + |update|)
  and the two scalar factors, whose error is the device library's powf / rsqrtf error amplified by A(t) = b^t / (1 - b^t):
    step = lr_eff / (1 - powf(b1, t))     e_step = POW_ULP 2^-23 A_1(t) + 3 u      (lr lr_scale, the subtraction, the quotient)
    isb  = rsqrtf(1 - powf(b2, t))        e_isb  = (POW_ULP 2^-23 A_2(t) + u) / 2 + RSQRT_ULP 2^-23
An fp32 emulation of the update with a correctly rounded pow needs at most 2.3 u relative on m', 3.7 u on v' and
u |p| + k u |update| with k <= 5.2 (k = 57 at b2 = 0.999, t = 2, where A = 499), so the structure is right and the
per-element part is a handful of roundings.  POW_ULP and RSQRT_ULP cannot be derived here: see their definition.

A compared quantity passes when max_i |got_i - ref_i| / bar_i <= 1; that ratio is what ``parity_record`` gets (bar 1).
Rows that set t <= 1000, weight_decay or grad_scale assert FROM THE REFERENCE ALONE that the reference with t + 1 in place
of t (weight_decay ignored, grad_scale ignored) reaches a ratio >= 10; rows at t = 100000 cannot see a step that is off by
one and do not claim to.
"""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch

from test_kernel_routes_gpu import BF16, DEV, EPS32, FORCED_SIMPLE, Sentinel, bar_gemm, launched, record, rel_max
from test_wgrad_routes_gpu import (Outputs, assert_exact, check_outputs, device_image, hand_made_tiles, operand,
                                   wgrad_reference)

pytestmark = pytest.mark.gpu
F32 = torch.float32

# Accuracy of the DEVICE LIBRARY's powf and rsqrtf in ulps.  HIP's are OCML's; the OpenCL accuracy table OCML is built to
# gives <= 16 ulp for pow and <= 2 ulp for rsqrt (quoted from memory of the OpenCL C specification's "relative error as
# ULPs" table; no copy of it ships with ROCm's documentation).  They bound the library, not the code under test: they are
# NOT to be tuned to make a case pass.  test_scalar_factors_against_the_allowances measures what the device really does
# (profiles/README.md quotes the figures), so whoever learns the real bound can tighten them from data.
POW_ULP = 16.0
RSQRT_ULP = 2.0
ULP = 2.0 ** -23


@pytest.fixture(autouse=True)
def _red_zones(request, monkeypatch):
    """The red zones of conftest.py (which installs them for three named files only), for this module's buffers too."""
    if os.environ.get("OVQA_TEST_REDZONE", "1") == "0" or not torch.cuda.is_available():
        yield
        return
    import redzone
    rz = redzone.install(monkeypatch, request.module)
    yield
    torch.cuda.synchronize()
    rz.check()


def ops():
    from openvivqa_amd import ops as o
    return o


def lib():
    from openvivqa_amd import _lib
    return _lib


def rnd(t):
    return t.to(DEV).contiguous()


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(x):
    return float(np.float32(x))


class HP:
    """Hyper-parameters as the ABI passes them: float32 values."""

    def __init__(self, lr=5e-3, betas=(0.9, 0.98), eps=1e-8, wd=0.0, gs=1.0, lr_scale=None):
        self.lr, self.b1, self.b2, self.eps, self.wd, self.gs = (f32(x) for x in (lr, betas[0], betas[1], eps, wd, gs))
        self.lr_scale = None if lr_scale is None else f32(lr_scale)

    def but(self, **kw):
        h = HP.__new__(HP)
        h.__dict__.update(self.__dict__)
        h.__dict__.update(kw)
        return h


def scalar_allowances(hp, t):
    """(e_step, e_isb, step, isb): the relative error allowed on the two scalar factors, and their fp64 values."""
    p1, p2 = hp.b1 ** t, hp.b2 ** t
    bc1, bc2 = 1.0 - p1, 1.0 - p2
    e_step = POW_ULP * ULP * (p1 / bc1) + 3 * EPS32
    e_isb = (POW_ULP * ULP * (p2 / bc2) + EPS32) / 2 + RSQRT_ULP * ULP
    step = hp.lr * (1.0 if hp.lr_scale is None else hp.lr_scale) / bc1
    return e_step, e_isb, step, 1.0 / math.sqrt(bc2)


def adam_ref(p, g, m, v, t, hp):
    """torch.optim.Adam's update (L2 weight decay, no amsgrad) in fp64 on tensors holding the kernels' inputs exactly.
    Returns (m', v', update, bar_m, bar_v, bar_update): the bars of the module docstring, elementwise."""
    u = EPS32
    gs, wp = g * hp.gs, hp.wd * p
    gk, G = gs + wp, gs.abs() + wp.abs()
    m2 = hp.b1 * m + (1 - hp.b1) * gk
    v2 = hp.b2 * v + (1 - hp.b2) * gk * gk
    bar_m = 4 * u * (hp.b1 * m.abs() + (1 - hp.b1) * G)
    bar_v = 7 * u * (hp.b2 * v + (1 - hp.b2) * G * G)
    e_step, e_isb, step, isb = scalar_allowances(hp, t)
    denom = v2.sqrt() * isb + hp.eps
    num = step * m2
    upd = num / denom
    r_v = torch.where(v2 > 0, bar_v / v2.clamp_min(1e-300), torch.zeros_like(v2))
    lo = (1 - r_v).clamp_min(0).sqrt() * (1 - 2 * u - e_isb)
    r_d = torch.where(lo > 0, 1 / lo.clamp_min(1e-300) - 1, torch.full_like(lo, float("inf")))
    num_err = step * bar_m * (1 + e_step) * (1 + u) + num.abs() * (e_step + u + e_step * u)
    bar_u = (num_err * (1 + r_d) * (1 + u) + num.abs() * (r_d + u + r_d * u)) / denom
    bar_u = bar_u + u * (p.abs() + upd.abs() + bar_u)
    return m2, v2, upd, bar_m, bar_v, bar_u


def ratio(got, ref, bar):
    """max_i |got_i - ref_i| / bar_i (0 where equal, inf where a bar of 0 is missed)."""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar)
    assert not bool(r.isnan().any())
    return r.max().item() if r.numel() else 0.0


def state(n, t, hp, gdt, seed=0):
    """(p, g, m, v) of n elements on the device; for t > 1 moments as t - 1 steps of N(0, 1) gradients would leave them."""
    g_ = torch.Generator().manual_seed(seed + n + t)
    r = lambda: torch.randn(n, generator=g_)
    p, g = r(), r().to(gdt)
    if t > 1:
        m = 0.5 * r() * (1 - hp.b1 ** (t - 1))
        v = (0.5 * r() ** 2 + 0.1) * (1 - hp.b2 ** (t - 1))
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v


def embed(t, front=8, back=8):
    """``t`` in the middle of a sentinel-filled parent (front / back elements around it); returns (Sentinel, view)."""
    s = Sentinel((t.numel() + front + back,), t.dtype)
    v = s.parent[front:front + t.numel()]
    v.copy_(t)
    s.before = s.parent.clone()
    return s, v


def check_adam(request, tag, hp, t, old, new, shadow, sel=None):
    """m, v, update of the selected elements against the fp64 reference; the shadow exactly; the sensitivity of the bars."""
    p0, g, m0, v0 = (x.double() for x in old)
    p1, m1, v1 = new
    if sel is not None:
        p0, g, m0, v0, p1, m1, v1 = (x[sel] for x in (p0, g, m0, v0, p1, m1, v1))
        shadow = shadow[sel] if shadow is not None else None
    m2, v2, upd, bm, bv, bu = adam_ref(p0, g, m0, v0, t, hp)
    out = {}
    for what, got, ref, bar in (("exp_avg", m1, m2, bm), ("exp_avg_sq", v1, v2, bv), ("update", p0 - p1.double(), upd, bu)):
        out[what] = record(request, f"{tag} {what} (max err / elementwise bar)", ratio(got, ref, bar), 1.0)
    assert all(r <= 1.0 for r in out.values()), (tag, out)
    if shadow is not None:
        assert torch.equal(shadow, p1.to(BF16)), f"{tag}: the bf16 shadow is not the kernel's own fp32 result rounded"
    if p0.numel() < 1000:
        return out
    if t <= 1000 and (t <= 10 or hp.b2 > 0.99):
        s = ratio(adam_ref(p0, g, m0, v0, t + 1, hp)[2], upd, bu)
        assert s >= 10, (tag, "t + 1 in place of t", s)
    if hp.wd != 0:
        w = adam_ref(p0, g, m0, v0, t, hp.but(wd=0.0))
        s = max(ratio(w[0], m2, bm), ratio(w[2], upd, bu))
        assert s >= 10, (tag, "weight_decay ignored", s)
    if hp.gs != 1:
        w = adam_ref(p0, g, m0, v0, t, hp.but(gs=1.0))
        assert ratio(w[0], m2, bm) >= 10 and ratio(w[1], v2, bv) >= 10, (tag, "grad_scale ignored")
    return out


# (id, t, betas, weight_decay, grad_scale, lr_scale, step_ptr given)
CASES = [
    ("t1", 1, (0.9, 0.98), 0.0, 1.0, None, True),
    ("t1_nostep", 1, (0.9, 0.98), 0.0, 1.0, None, False),        # step_ptr NULL: t = 1
    ("t2", 2, (0.9, 0.98), 0.0, 1.0, None, True),
    ("t10_wd_gs_scale", 10, (0.9, 0.98), 0.01, 0.25, 0.37, True),
    ("t1000", 1000, (0.9, 0.98), 0.0, 1.0, None, True),
    ("t100000_wd", 100000, (0.9, 0.98), 0.01, 1.0, 0.37, True),
    ("t1_b999", 1, (0.9, 0.999), 0.0, 1.0, None, True),           # 1 - powf(b2, 1) cancels 1000-fold
    ("t2_b999_gs", 2, (0.9, 0.999), 0.0, 0.25, None, True),
    ("t10_b999_wd", 10, (0.9, 0.999), 0.01, 1.0, None, True),
    ("t1000_b999", 1000, (0.9, 0.999), 0.0, 1.0, 0.37, True),
    ("t100000_b999_gs", 100000, (0.9, 0.999), 0.0, 0.25, None, True),
]


def case_hp(case):
    cid, t, betas, wd, gs, scale, has_step = case
    return HP(betas=betas, wd=wd, gs=gs, lr_scale=scale), t, has_step


def device_scalars(hp, t, has_step):
    step = rnd(torch.tensor([t], dtype=torch.int32)) if has_step else None
    scale = None if hp.lr_scale is None else rnd(torch.tensor([hp.lr_scale], dtype=F32))
    t_dev = int(step.item()) if has_step else 1  # the step the reference uses is the one read back from the device
    return step, scale, t_dev


def test_fp64_reference_equals_torch_optim_adam():
    """The ten lines above against torch.optim.Adam on fp64 CPU tensors (one case with everything switched on)."""
    hp, t = HP(betas=(0.9, 0.999), wd=0.01, gs=0.25, lr_scale=0.37), 10
    p, g, m, v = (x.double() for x in state(4096, t, hp, F32))
    m2, v2, upd, *_ = adam_ref(p, g, m, v, t, hp)
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=hp.lr * hp.lr_scale, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd)
    q.grad = g * hp.gs
    opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    st = opt.state[q]
    assert float(st["step"]) == t
    for a, b in ((st["exp_avg"], m2), (st["exp_avg_sq"], v2), (p - q.detach(), upd)):
        assert ((a - b).abs() <= 1e-12 * b.abs() + 1e-15).all()


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["g32", "g16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_flat_adam_against_fp64(request, case, gdt):
    """ovqa_adam_step, n = 65539: 16384 float4 groups (grid-stride) and a 3-element tail."""
    o = ops()
    hp, t, has_step = case_hp(case)
    n = 65539
    old = [rnd(x) for x in state(n, t, hp, gdt)]
    (sp, p), (sm, m), (sv, v) = embed(old[0]), embed(old[2]), embed(old[3])
    ss, sh = embed(torch.zeros(n, dtype=BF16, device=DEV))
    step, scale, t_dev = device_scalars(hp, t, has_step)
    _, log = launched(lambda: o.adam_step(p, old[1], m, v, sh, hp.lr, step, lr_scale=scale, betas=(hp.b1, hp.b2), eps=hp.eps,
                                          weight_decay=hp.wd, grad_scale=hp.gs))
    torch.cuda.synchronize()
    assert t_dev == t
    check_adam(request, case[0], hp, t_dev, old, (p, m, v), sh)
    for s, view in ((sp, p), (sm, m), (sv, v), (ss, sh)):
        s.check(view)
    assert log == ["adam_kernel<float>" if gdt == F32 else "adam_kernel<bf16>"], log


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["g32", "g16"])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 7])
def test_flat_adam_tiny_arrays(request, n, gdt):
    """The tail path alone (n < 4), n = 0 (nothing is launched, nothing changes), one group with and without a tail; with
    and without a shadow."""
    o = ops()
    hp, t = HP(wd=0.01, gs=0.25), 2
    for with_shadow in (True, False):
        old = [rnd(x) for x in state(max(n, 1), t, hp, gdt)]
        old = [x[:n] for x in old]
        (sp, p), (sm, m), (sv, v) = embed(old[0]), embed(old[2]), embed(old[3])
        ss, sh = embed(torch.zeros(n, dtype=BF16, device=DEV))
        step = rnd(torch.tensor([t], dtype=torch.int32))
        # (an empty view has no address of its own: pass the places where the arrays would start)
        ptr = lambda s: s.parent.data_ptr() + 8 * s.parent.element_size()
        _lib = lib()
        g = old[1] if n else rnd(torch.zeros(4, dtype=gdt))
        _, log = launched(lambda: _lib.check(_lib.load().ovqa_adam_step(
            ptr(sp), g.data_ptr(), o.OVQA_F32 if gdt == F32 else o.OVQA_BF16, ptr(sm), ptr(sv), ptr(ss) if with_shadow else None,
            n, hp.lr, None, hp.b1, hp.b2, hp.eps, hp.wd, hp.gs, step.data_ptr(), stream()), "adam_step"))
        torch.cuda.synchronize()
        if n:
            check_adam(request, f"n={n} shadow={int(with_shadow)}", hp, t, old, (p, m, v), sh if with_shadow else None)
        for s, view in ((sp, p), (sm, m), (sv, v)):
            s.check(view)
        if with_shadow:
            ss.check(sh)
        else:
            ss.check()
        assert log == ([] if n == 0 else ["adam_kernel<float>" if gdt == F32 else "adam_kernel<bf16>"]), log


def test_scalar_factors_against_the_allowances(request):
    """What the device's powf / rsqrtf really give, read off elements built for it (recorded against the POW_ULP / RSQRT_ULP
    allowances; nothing here depends on the code under test beyond adam_update1's own formula).
      element 0: g = 0, m = 1, v = 0, p = 0, eps = 1 -> m' = b1 exactly, denom = 1 exactly, p' = -fl(step b1):
                 step = -p' / b1 to within one rounding (u);
      element 1: g = 0, m = 1, v = 1, p = 0, eps = 0 -> v' = b2, denom = fl(fl(sqrt b2) isb), p' = -fl(fl(step b1) / denom):
                 isb to within step's own error and four roundings."""
    o = ops()
    for b2 in (0.98, 0.999):
        for t in (1, 2, 10, 1000, 100000):
            hp = HP(betas=(0.9, b2))
            e_step, e_isb, step_ref, isb_ref = scalar_allowances(hp, t)
            stp = rnd(torch.tensor([t], dtype=torch.int32))
            got = []
            for eps, v0 in ((1.0, 0.0), (0.0, 1.0)):
                p, g, m = rnd(torch.zeros(4)), rnd(torch.zeros(4)), rnd(torch.ones(4))
                v = rnd(torch.full((4,), v0))
                o.adam_step(p, g, m, v, None, hp.lr, stp, betas=(hp.b1, hp.b2), eps=eps)
                torch.cuda.synchronize()
                assert m.double()[0].item() == hp.b1 and v.double()[0].item() == hp.b2 * v0
                got.append(-p.double()[0].item())
            step_got = got[0] / hp.b1
            isb_got = got[0] / (got[1] * math.sqrt(hp.b2))
            r_step = abs(step_got / step_ref - 1)
            r_isb = abs(isb_got / isb_ref - 1)
            record(request, f"step_size b2={b2} t={t}: relative error (bar: allowance + 1 rounding)", r_step, e_step + EPS32)
            record(request, f"inv_sqrt_bc2 b2={b2} t={t}: relative error (bar: allowance + 4 roundings)", r_isb,
                   e_isb + 4 * EPS32)
            assert r_step <= e_step + EPS32, (b2, t, r_step / ULP, "ulp")
            assert r_isb <= e_isb + 4 * EPS32, (b2, t, r_isb / ULP, "ulp")


# ---------------------------------------------------------------------------------------------------------------------------
# ovqa_adam_step_tiled
# ---------------------------------------------------------------------------------------------------------------------------
class Arena:
    """Matrices (or adjacency groups of matrices: [sum rows, cols]) and a 1-D tail at element offsets of one arena, 8
    untouched elements in front of, between and behind them."""

    def __init__(self, mats, flat=0, untouched=()):
        """mats: {name: (rows, cols)}; untouched: names that get no tile entry (they must not change)."""
        self.off, self.shape, total = {}, dict(mats), 8
        for name, (r, c) in mats.items():
            self.off[name] = total
            total += r * c + 8
        self.flat_lo, self.flat_hi = total + 12, total + 12 + flat  # 12 tail elements in front of flat_lo stay as they are
        self.n = self.flat_hi + 20
        self.tiled = [k for k in mats if k not in untouched]

    def tiles(self, shuffle_seed=0):
        _lib = lib()
        out = []
        for name in self.tiled:
            r, c = self.shape[name]
            out += [_lib.AdamTile(self.off[name], r, c, r0, c0, (C.c_int32 * 2)(0, 0))
                    for r0 in range(0, r, 64) for c0 in range(0, c, 64)]
        random.Random(shuffle_seed).shuffle(out)
        return out

    def mask(self):
        m = torch.zeros(self.n, dtype=torch.bool, device=DEV)
        for name in self.tiled:
            r, c = self.shape[name]
            m[self.off[name]:self.off[name] + r * c] = True
        m[self.flat_lo:self.flat_hi] = True
        return m

    def views(self, parent, flat=True):
        v = [parent[self.off[k]:self.off[k] + self.shape[k][0] * self.shape[k][1]] for k in self.tiled]
        return v + ([parent[self.flat_lo:self.flat_hi]] if flat and self.flat_hi > self.flat_lo else [])


def arena_state(ar, t, hp, gdt):
    """Sentinel-backed p / m / v / shadow / shadow_t arenas and a gradient array, filled with a plausible state."""
    p, g, m, v = (rnd(x) for x in state(ar.n, t, hp, gdt))
    S = {}
    for k, x in (("p", p), ("m", m), ("v", v)):  # real values everywhere: what the launch must not touch is a number too
        S[k] = Sentinel((ar.n,), F32)
        S[k].parent.copy_(x)
        S[k].before = S[k].parent.clone()
    S["sh"], S["sht"] = Sentinel((ar.n,), BF16), Sentinel((ar.n,), BF16)  # the shadows keep the byte pattern
    return S, g


def check_transposed(ar, sh, sht):
    for name in ar.tiled:
        r, c = ar.shape[name]
        a = sh[ar.off[name]:ar.off[name] + r * c].view(r, c)
        b = sht[ar.off[name]:ar.off[name] + r * c].view(c, r)
        assert torch.equal(b, a.t()), f"transposed shadow of {name} ({r} x {c}) is not shadow.t()"


TILED_MATS = {"one_tile": (64, 64), "sliver_rows": (8, 2048), "sliver_cols": (2048, 8), "ragged": (360, 128),
              "no_tiles": (64, 128), "group_of_three": (128 + 64 + 192, 256)}


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["g32", "g16"])
@pytest.mark.parametrize("case", [CASES[i] for i in (0, 1, 3, 5, 6, 9)], ids=[CASES[i][0] for i in (0, 1, 3, 5, 6, 9)])
def test_tiled_adam_against_fp64(request, case, gdt):
    """ovqa_adam_step_tiled: a single 64 x 64 matrix, 8 x 2048 and 2048 x 8 (one sliver of a tile), 360 x 128 (ragged tiles),
    an adjacency group of three matrices (128 | 64 | 192 rows of 256: ONE [384, 256] entry whose transposed copy is
    [256, 384]), a matrix WITHOUT tile entries (untouched) and a flat tail [flat_lo, flat_hi) with elements of the arena on
    both sides of it; tile entries in shuffled order."""
    o, _lib = ops(), lib()
    hp, t, has_step = case_hp(case)
    ar = Arena(TILED_MATS, flat=4100, untouched=("no_tiles",))
    S, g = arena_state(ar, t, hp, gdt)
    old = [S["p"].parent.clone(), g, S["m"].parent.clone(), S["v"].parent.clone()]
    tiles = ar.tiles()
    table = rnd(torch.frombuffer(bytearray(bytes((_lib.AdamTile * len(tiles))(*tiles))), dtype=torch.uint8))
    step, scale, t_dev = device_scalars(hp, t, has_step)
    _, log = launched(lambda: o.adam_step_tiled(S["p"].parent, g, S["m"].parent, S["v"].parent, S["sh"].parent,
                                                S["sht"].parent, table, len(tiles), ar.flat_lo, ar.flat_hi, hp.lr, step,
                                                lr_scale=scale, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd,
                                                grad_scale=hp.gs))
    torch.cuda.synchronize()
    sel = ar.mask()
    check_adam(request, case[0], hp, t_dev, old, (S["p"].parent, S["m"].parent, S["v"].parent), S["sh"].parent, sel)
    check_transposed(ar, S["sh"].parent, S["sht"].parent)
    for k in ("p", "m", "v", "sh"):
        S[k].check(*ar.views(S[k].parent))
    S["sht"].check(*ar.views(S["sht"].parent, flat=False))
    assert log == ["adam_tiled_kernel<float>" if gdt == F32 else "adam_tiled_kernel<bf16>"], log


def test_tiled_adam_without_tiles_or_without_flat_range(request):
    """n_tiles = 0 with a flat range; tiles with flat_lo == flat_hi; shadow_t NULL."""
    o, _lib = ops(), lib()
    hp, t = HP(), 2
    for mats, flat, with_t in (({}, 516, True), ({"a": (72, 136)}, 0, True), ({"a": (72, 136)}, 8, False)):
        ar = Arena(mats, flat=flat)
        S, g = arena_state(ar, t, hp, F32)
        old = [S["p"].parent.clone(), g, S["m"].parent.clone(), S["v"].parent.clone()]
        tiles = ar.tiles()
        table = rnd(torch.frombuffer(bytearray(bytes((_lib.AdamTile * max(len(tiles), 1))(*tiles))), dtype=torch.uint8))
        step = rnd(torch.tensor([t], dtype=torch.int32))
        o.adam_step_tiled(S["p"].parent, g, S["m"].parent, S["v"].parent, S["sh"].parent, S["sht"].parent if with_t else None,
                          table, len(tiles), ar.flat_lo, ar.flat_hi, hp.lr, step, betas=(hp.b1, hp.b2), eps=hp.eps)
        torch.cuda.synchronize()
        check_adam(request, f"mats={list(mats)} flat={flat}", hp, t, old, (S["p"].parent, S["m"].parent, S["v"].parent),
                   S["sh"].parent, ar.mask())
        for k in ("p", "m", "v", "sh"):
            S[k].check(*ar.views(S[k].parent))
        if with_t:
            check_transposed(ar, S["sh"].parent, S["sht"].parent)
            S["sht"].check(*ar.views(S["sht"].parent, flat=False))
        else:
            S["sht"].check()


# ---------------------------------------------------------------------------------------------------------------------------
# The fused epilogue: ovqa_grouped_linear_bwd_weight_adam with targets, through the C ABI, tables built here
# ---------------------------------------------------------------------------------------------------------------------------
# fused problems: (name, M, N, K, arena matrix, first row of the problem in it, has db, accumulate bits (bit 0 clear))
FUSED = [
    ("one_tile", 64, 128, 128, "one_tile", 0, False, 0),
    ("wide", 192, 512, 2048, "wide", 0, True, 0),
    ("tall", 64, 2048, 512, "tall", 0, False, 0),
    ("m4c_ffn", 6400, 768, 3072, "m4c_ffn", 0, True, 2),
    # an adjacency group [2048, 512] (transposed [512, 2048], ld_transposed = 2048) owned by two problems of the launch
    ("group_head", 64, 512, 512, "group", 0, False, 0),
    ("group_tail", 192, 1536, 512, "group", 512, True, 0),
]
# unfused problems of the same launch (NULL target): ragged N / K, accumulate bits, db, the ragged M4C classifier
UNFUSED = [("u_72x40", 64, 72, 40, 3, True), ("u_304x264", 192, 304, 264, 0, True), ("u_5000x768", 192, 5000, 768, 1, False),
           ("u_128x128", 6400, 128, 128, 2, True)]
FUSED_MATS = {"one_tile": (128, 128), "wide": (512, 2048), "tall": (2048, 512), "m4c_ffn": (768, 3072), "group": (2048, 512)}


def fused_launch(kind, hp, t, table, absent=()):
    o, _lib = ops(), lib()
    fused = [f for f in FUSED if f[0] not in absent]
    ar = Arena(FUSED_MATS)
    S, _ = arena_state(ar, t, hp, F32)
    old = {k: S[k].parent.clone() for k in ("p", "m", "v")}
    names = [f[0] for f in fused] + [u[0] for u in UNFUSED]
    shapes = [(f[1], f[2], f[3]) for f in fused] + [(u[1], u[2], u[3]) for u in UNFUSED]
    flags = [f[7] for f in fused] + [u[4] for u in UNFUSED]
    has_db = [f[6] for f in fused] + [u[5] for u in UNFUSED]
    outs = Outputs(kind, [(N, K, fl, hb) for (M, N, K), fl, hb in zip(shapes, flags, has_db)])
    operands, problems, targets = [], [], []
    for i, (M, N, K) in enumerate(shapes):
        dy, x = operand(kind, M, N, 100 + i, i % 2 == 1), operand(kind, M, K, 200 + i, i % 3 == 1)
        operands.append((dy, x))
        db = outs.db[i]
        problems.append(_lib.WgradProblem(dy.data_ptr(), x.data_ptr(), outs.dw[i].data_ptr(),
                                          None if db is None else db.data_ptr(), dy.stride(0), x.stride(0), M, N, K, flags[i]))
        if i < len(fused):
            mat, row0 = fused[i][4], fused[i][5]
            rows, cols = FUSED_MATS[mat]
            assert cols == K
            e = ar.off[mat] + row0 * K
            targets.append(_lib.AdamTarget(S["p"].parent.data_ptr() + 4 * e, S["m"].parent.data_ptr() + 4 * e,
                                           S["v"].parent.data_ptr() + 4 * e, S["sh"].parent.data_ptr() + 2 * e,
                                           S["sht"].parent.data_ptr() + 2 * (ar.off[mat] + row0), rows))
        else:
            targets.append(_lib.AdamTarget())
    tiles = hand_made_tiles(shapes) if table == "hand_made" else o.WgradQueue.tile_table(shapes)
    buf, toff, goff, n_tiles = device_image(problems, tiles, targets)
    step, scale, t_dev = device_scalars(hp, t, True)
    consts = _lib.AdamConsts(hp.lr, hp.b1, hp.b2, hp.eps, hp.wd, hp.gs, None if scale is None else scale.data_ptr(),
                             step.data_ptr())
    base = buf.data_ptr()
    rc_call = lambda: _lib.load().ovqa_grouped_linear_bwd_weight_adam(o.OVQA_BF16, base, base + toff, n_tiles, base + goff,
                                                                      C.addressof(consts), stream())
    if FORCED_SIMPLE:
        assert rc_call() != 0
        pytest.skip("ovqa_grouped_linear_bwd_weight_adam refuses under OVQA_FORCE_SIMPLE=1 (asserted)")
    _, log = launched(lambda: _lib.check(rc_call(), "grouped_linear_bwd_weight_adam"))
    torch.cuda.synchronize()
    assert log == ["gemm_bf16_grouped_wgrad_adam_kernel"], log
    return dict(ar=ar, S=S, old=old, outs=outs, operands=operands, shapes=shapes, flags=flags, names=names, t=t_dev,
                problems=problems, step=step, scale=scale, fused=fused)


def fused_region(ar, f):
    """(slice of the row-major arenas, function giving the [K, N] view of the transposed-shadow arena) of a fused problem."""
    name, M, N, K, mat, row0 = f[:6]
    rows = FUSED_MATS[mat][0]
    lo = ar.off[mat] + row0 * K
    return slice(lo, lo + N * K), lambda sht: sht[ar.off[mat]:ar.off[mat] + rows * K].view(K, rows)[:, row0:row0 + N]


def separate_launches(L, kind, hp):
    """The same step as two launches on copies of the same state: form-1 grouped dW into a gradient arena (the fused
    problems at their matrices' offsets), then ovqa_adam_step_tiled over the arena.  A matrix whose rows are all owned by
    problems of the launch is ONE tiled entry (its transposed copy then has the fused launch's layout); of a group with an
    absent owner only the present rows get an entry -- their transposed copy is laid out differently and is not compared."""
    o, _lib = ops(), lib()
    ar, fused = L["ar"], L["fused"]
    grad = rnd(torch.zeros(ar.n))
    B = {k: L["old"][k].clone() for k in ("p", "m", "v")}
    B["sh"], B["sht"] = L["S"]["sh"].before.clone(), L["S"]["sht"].before.clone()
    problems = []
    for i, f in enumerate(fused):
        pr = L["problems"][i]
        e = ar.off[f[4]] + f[5] * f[3]
        problems.append(_lib.WgradProblem(pr.dy, pr.x, grad.data_ptr() + 4 * e, None, pr.lddy, pr.ldx, pr.M, pr.N, pr.K, 0))
    shapes = L["shapes"][:len(fused)]
    buf, toff, _, n_tiles = device_image(problems, o.WgradQueue.tile_table(shapes))
    _lib.check(_lib.load().ovqa_grouped_linear_bwd_weight(o.OVQA_BF16, buf.data_ptr(), buf.data_ptr() + toff, n_tiles, 1,
                                                          stream()), "grouped_linear_bwd_weight")
    whole = len(fused) == len(FUSED)
    if whole:
        tiles = ar.tiles()
    else:
        tiles = [_lib.AdamTile(ar.off[f[4]] + f[5] * f[3], f[2], f[3], r0, c0, (C.c_int32 * 2)(0, 0))
                 for f in fused for r0 in range(0, f[2], 64) for c0 in range(0, f[3], 64)]
    table = rnd(torch.frombuffer(bytearray(bytes((_lib.AdamTile * len(tiles))(*tiles))), dtype=torch.uint8))
    o.adam_step_tiled(B["p"], grad, B["m"], B["v"], B["sh"], B["sht"], table, len(tiles), ar.n - 20, ar.n - 20, hp.lr,
                      L["step"], lr_scale=L["scale"], betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd, grad_scale=hp.gs)
    torch.cuda.synchronize()
    return B, (("p", "m", "v", "sh", "sht") if whole else ("p", "m", "v", "sh"))


FUSED_CASES = [("int", CASES[0], "hand_made", ()), ("int", CASES[3], "queue", ()), ("int", CASES[9], "hand_made", ()),
               ("int", CASES[5], "queue", ()), ("gauss", CASES[3], "hand_made", ()),
               ("int", CASES[3], "hand_made", ("group_head",)), ("gauss", CASES[0], "queue", ("group_head", "m4c_ffn"))]


@pytest.mark.parametrize("kind,case,table,absent", FUSED_CASES,
                         ids=[f"{k}-{c[0]}-{tb}" + "".join("-no_" + a for a in ab) for k, c, tb, ab in FUSED_CASES])
def test_fused_adam_epilogue(request, kind, case, table, absent):
    """Fused problems 128 x 128 (one tile), 512 x 2048, 2048 x 512, 768 x 3072 (M = 6400) and a 1536 x 512 product that owns
    rows 512.. of a 2048-row adjacency group whose first 512 rows belong to ANOTHER problem of the launch -- or, in the
    ``no_group_head`` cases, to no problem of the launch: those rows, and their 512 columns of the [512, 2048] transposed
    copy, must then stay as they are; unfused problems (NULL target) with ragged N / K, accumulate bits and db in the same
    launch; db of fused problems.
      * integer operands: the gradient is exact, so exp_avg, exp_avg_sq and the update against fp64 Adam on the exact
        gradient with the module's bars; unfused dw / db and fused db exactly;
      * both kinds: the shadows by the exact identities; the dw buffer of a fused problem is untouched; nothing outside the
        fused problems' own elements changes in any arena; fused db (Gaussian: the format bar); and (an extra -- the fp64
        comparison is the test) the arenas are bit-equal to the form-1 grouped dW followed by ovqa_adam_step_tiled on copies
        of the same state.
    Gaussian operands stop there: the gradient's own bar pushed through Adam's sensitivity to g has no closed form near
    v = 0."""
    hp, t, _ = case_hp(case)
    L = fused_launch(kind, hp, t, table, absent)
    ar, S, outs, fused = L["ar"], L["S"], L["outs"], L["fused"]
    row_major, transposed = [], []
    for i, name in enumerate(L["names"]):
        M, N, K = L["shapes"][i]
        ref = wgrad_reference(*L["operands"][i], False)
        if i >= len(fused):
            check_outputs(request, name, kind, M, L["flags"][i], ref, outs.init_dw[i], outs.init_db[i], outs.dw[i], outs.db[i])
            continue
        assert torch.equal(outs.dw[i], outs.init_dw[i]), f"{name}: the fp32 gradient tile of a fused problem was stored"
        if outs.db[i] is not None:  # db of a fused problem is written as before
            want = ref["db"] + (outs.init_db[i].double() if L["flags"][i] & 2 else 0.0)
            if kind == "int":
                record(request, f"{name} db (integer operands: max |err|)", assert_exact(outs.db[i], want, name + " db", 1 << 30), 0.0)
            else:
                absdy = ref["absdy"] + (outs.init_db[i].double().abs() if L["flags"][i] & 2 else 0.0)
                bar = bar_gemm(absdy.max().item(), want.abs().max().item(), M, bf16_out=False)
                err = record(request, f"{name} db", rel_max(outs.db[i], want), bar)
                assert err < bar, (name, "db", err, bar)
        sl, tview = fused_region(ar, fused[i])
        row_major.append(sl)
        transposed.append(tview(S["sht"].parent))
        if kind == "int":
            old = [L["old"]["p"][sl], ref["dw"].reshape(-1), L["old"]["m"][sl], L["old"]["v"][sl]]
            check_adam(request, f"fused {name}", hp, L["t"], old, (S["p"].parent[sl], S["m"].parent[sl], S["v"].parent[sl]),
                       S["sh"].parent[sl])
        else:
            assert torch.equal(S["sh"].parent[sl], S["p"].parent[sl].to(BF16)), f"{name}: shadow != bf16(param)"
        assert torch.equal(transposed[-1], S["sh"].parent[sl].view(N, K).t()), f"{name}: transposed shadow != shadow.t()"
        del ref
    for k in ("p", "m", "v", "sh"):
        S[k].check(*[S[k].parent[sl] for sl in row_major])
    S["sht"].check(*transposed)
    outs.sent.check(*[v for v in outs.dw + outs.db if v is not None])  # (only the listed outputs and nothing between them)
    B, arenas = separate_launches(L, kind, hp)
    for k in arenas:
        same = torch.equal(S[k].parent, B[k])
        assert same, f"arena {k}: the fused launch and grouped dW + tiled Adam differ in " \
                     f"{int((S[k].parent != B[k]).sum())} elements"
