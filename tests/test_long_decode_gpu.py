"""Single-query decode attention (ovqa_attention_decode) past one LDS window and with beam groups up to 8.

Up to 512 keys a wave of attn_decode_kernel takes its keys in one pass; longer key lists are walked in windows of the
wave's LDS slot (128 keys per wave: the four waves of a workgroup share a problem) under an online softmax.  Groups of
2 .. 8 beams share one read of their sample's K / V rows.

Bars, on ``rel_max`` = max |out - ref| / max |ref| (no floor: these outputs are near 0.1, ``nerr``'s floor of 1 would hide
a lost window): bf16 2^-7 (one rounding of the output is at most 2^-8; doubled for the fp32 sums and the fast
exponential), fp32 the project's tol(F32) = 1e-4.  The reference is fp64 softmax attention on the same operands; where a
mask is given its addition is done in fp32, as the model and the kernel do it (a score of -1e5 + s has an fp32 ulp of
2^-7, which is part of what the reference module computes).

Random inputs alone cannot show a lost key (dropping the last 16-key pass moves the output by 0.011 .. 0.037 of max |ref|),
so every length also runs with one boosted key j* (+8 in every query's additive mask row): the test first asserts, in fp64
on its own inputs, that removing j* moves the tensor by >= 10 bars and every (row, head) by more than one bar, and only
then compares the kernel.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from test_kernels_gpu import BF16, DEV, F32, rel_max, tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the library's A/B switches move calls between forms: the form assertions hold for the defaults only
SWITCHES_DEFAULT = "OVQA_DECODE_SPLIT_MIN" not in os.environ and "OVQA_DECODE_GROUP_MAX" not in os.environ
LONG_N = [513, 577, 617, 1024, 2049]
ONE_WINDOW_N = [1, 511, 512]
GROUPS = [1, 3, 5, 8]


def bar(dtype):
    return 2 ** -7 if dtype == BF16 else tol(F32)


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


@pytest.fixture(autouse=True)
def _red_zones(request, monkeypatch):
    """Guard bands (tests/redzone.py) around what ops allocates and what this module's rnd() makes, as in the kernel tests."""
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


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def samples_for(group, H):
    """Cache rows of a test row: two, or -- for groups of 5 .. 8 -- as many as the shared forms ask for (two workgroups
    per CU at one workgroup per (sample, head); launch_decode in csrc/attention_decode.hip)."""
    return 2 if group <= 4 else -(-2 * cus() // H)


def expected_form(dtype, d, n, group, R, H):
    """A copy of launch_decode's predicates (default OVQA_DECODE_SPLIT_MIN / OVQA_DECODE_GROUP_MAX): the instantiation a
    call launches, as the launch log names it."""
    win = n > 512
    split = win or n >= 64
    G = 1
    if 2 <= group <= 8 and R % group == 0:
        for g in range(group, 1, -1):
            if group % g:
                continue
            if g > 4 and (not split or (R // g) * H < 2 * cus() or (win and g > 6)):
                continue
            G = g
            break
    t = "float" if dtype == F32 else "__bf16"
    b = lambda x: "true" if x else "false"
    return f"attn_decode_kernel<{t},{d},{G},{b(split)},{b(win)}>"


def decode(q, kc, vc, n, H, mask=None, group=1, out=None):
    """ops.attention_decode; the call must dispatch "decode" and launch exactly the instantiation the rule names."""
    from openvivqa_amd import _lib
    _lib.launch_log_clear()
    o = ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group, out=out)
    assert _lib.last_dispatch() == "decode"
    if SWITCHES_DEFAULT:
        assert _lib.launch_log() == [expected_form(q.dtype, q.shape[-1] // H, n, group, q.shape[0], H)], _lib.launch_log()
    return o


def ref_decode(q, kc, vc, n, H, mask=None, group=1, drop=None):
    """fp64 torch math: o[r] = softmax(q[r] K[r // group]^T / sqrt(d) + mask[r]) V[r // group] over the first n keys
    (``drop``: a key index left out).  The mask is added in fp32, as the model does."""
    R, F = q.shape[0], q.shape[-1]
    d = F // H
    qd = q.detach().double().reshape(R // group, group, H, d)
    k = kc[:, :n].detach().double().reshape(-1, n, H, d)
    v = vc[:, :n].detach().double().reshape(-1, n, H, d)
    s = torch.einsum("bghd,bnhd->bghn", qd, k) / d ** 0.5
    if mask is not None:
        s = (s.float() + mask[:, None, :n].detach().float().reshape(R // group, group, 1, n)).double()
    if drop is not None:
        keep = torch.ones(n, dtype=torch.bool, device=s.device)
        keep[drop] = False
        s, v = s[..., keep], v[:, keep]
    p = torch.softmax(s, -1)
    return torch.einsum("bghn,bnhd->bghd", p, v).reshape(R, F).cpu()


def caches(Bc, Lmax, F, dtype):
    return rnd(Bc, Lmax, F, dtype=dtype, seed=2), rnd(Bc, Lmax, F, dtype=dtype, seed=3)


def run_strided(q, kc, vc, n, H, mask, group):
    """The call with a strided output between sentinel columns; returns the output view after checking the sentinels."""
    R, F = q.shape[0], q.shape[-1]
    buf = torch.full((R, 3 * F), 7.0, dtype=q.dtype, device=DEV)
    decode(q.view(R, F), kc, vc, n, H, mask=mask, group=group, out=buf[:, F:2 * F])
    assert bool((buf[:, :F] == 7.0).all()) and bool((buf[:, 2 * F:] == 7.0).all()), "sentinel columns changed"
    return buf[:, F:2 * F]


def check_row(dtype, Bc, group, H, d, n, Lmax=None, mask_kind="pad"):
    R, F = Bc * group, H * d
    Lmax = n + 9 if Lmax is None else Lmax
    assert Lmax > n
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, Lmax, F, dtype)
    mask = torch.zeros(R, Lmax, device=DEV)
    if n > 4:  # padded tails and heads (-1e5, models/utils.py:44-73), different per row
        mask[1 % R, n - max(1, n // 5):] = -1e5
        mask[R - 1, :max(1, n // 3)] = -1e5
    out = decode(q, kc, vc, n, H, mask=mask, group=group)
    assert out.shape == q.shape and out.dtype == dtype
    ref = ref_decode(q, kc, vc, n, H, mask, group)
    e = rel_max(out.reshape(R, F), ref)
    assert e < bar(dtype), ("mask", e, bar(dtype))
    # no mask, strided output with sentinel columns
    o2 = run_strided(q, kc, vc, n, H, None, group)
    ref2 = ref_decode(q, kc, vc, n, H, None, group)
    e2 = rel_max(o2, ref2)
    assert e2 < bar(dtype), ("no mask", e2, bar(dtype))
    # mask and strided output together
    o3 = run_strided(q, kc, vc, n, H, mask, group)
    assert torch.equal(o3, out.reshape(R, F))
    return e, e2


# -------------------------------------------------------------------------------------------------------------------------
# 1. against fp64
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("n", LONG_N + ONE_WINDOW_N)
def test_decode_against_fp64(dtype, d, n):
    """Every group in {1, 3, 5, 8} at H = 8, with a mask and without one, dense and strided output."""
    for group in GROUPS:
        check_row(dtype, samples_for(group, 8), group, 8, d, n)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("group", [6, 7])
@pytest.mark.parametrize("n", [512, 617, 2049])
def test_decode_groups_of_six_and_seven(dtype, group, n):
    """6 is the largest windowed shared form; 7 shares up to 512 keys and reads per row past them."""
    check_row(dtype, samples_for(group, 8), group, 8, 64, n)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [512, 617, 2049])
def test_decode_group_nine_reads_per_row(dtype, n):
    """group = 9 has no shared form: every row reads its sample's cache row by itself (G = 1), same results."""
    check_row(dtype, 2, 9, 8, 64, n)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", [512, 617, 1024])
def test_decode_odd_head_count(dtype, group, n):
    check_row(dtype, samples_for(group, 5) + 1, group, 5, 64, n, Lmax=n + 1)


# -------------------------------------------------------------------------------------------------------------------------
# 2. planted keys: the bars can see a lost key
# -------------------------------------------------------------------------------------------------------------------------
def wave_ranges(n):
    """Key ranges of the four waves of a workgroup in the split form (csrc/attention_decode.hip: a quarter of the keys
    rounded up to whole 16-key passes)."""
    quarter = ((n + 3) // 4 + 15) & ~15
    out = []
    for w in range(4):
        lo = min(w * quarter, n)
        hi = min(lo + quarter, n)
        if hi > lo:
            out.append((lo, hi))
    return out


def planted(n):
    js = {0, 511, 512, n - 1}
    for lo, hi in wave_ranges(n):
        js.update((lo, hi - 1))
    return sorted(j for j in js if 0 <= j < n)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("n", LONG_N)
def test_decode_planted_key(dtype, d, n):
    Bc, group, H = 8, 3, 8
    R, F = Bc * group, H * d
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, n + 3, F, dtype)
    b = bar(dtype)
    for js in planted(n):
        mask = torch.zeros(R, n + 3, device=DEV)
        mask[:, js] = 8.0
        ref = ref_decode(q, kc, vc, n, H, mask, group)
        lost = ref_decode(q, kc, vc, n, H, mask, group, drop=js)
        scale = ref.abs().max()
        per = ((ref - lost).abs().reshape(R, H, d).amax(-1) / scale)
        assert rel_max(lost, ref) >= 10 * b, (js, rel_max(lost, ref))  # the bar sees a lost j* ten times over ...
        assert per.min().item() > b, (js, per.min().item())            # ... and in every (row, head)
        out = decode(q, kc, vc, n, H, mask=mask, group=group)
        e = rel_max(out.reshape(R, F), ref)
        assert e < b, (js, e, b)
        got = ((out.reshape(R, F).double().cpu() - ref).abs().reshape(R, H, d).amax(-1) / scale)
        assert got.max().item() < b


# -------------------------------------------------------------------------------------------------------------------------
# 3. mask placements that stress the running maximum
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("group", [1, 5])
@pytest.mark.parametrize("n", [577, 617, 1024, 2049])
def test_decode_running_maximum(dtype, group, n):
    H, d = 8, 64
    Bc = max(4, samples_for(group, H))
    R, F = Bc * group, H * d
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, n + 5, F, dtype)
    q[1] = 0  # the fully masked row: equal scores, exactly uniform over its n keys
    mask = torch.zeros(R, n + 5, device=DEV)
    mask[0, :512] = -1e5      # the first 512 keys contribute about nothing: the maximum arrives late
    mask[1, :] = -1e5         # fully masked (finite): uniform over n keys
    mask[2, 512:] = -1e5      # only the first 512 keys live
    mask[R - 1, n - 1] = 12.0  # the largest score is the very last key
    out = decode(q, kc, vc, n, H, mask=mask, group=group).reshape(R, F)
    assert bool(torch.isfinite(out.float()).all())
    ref = ref_decode(q, kc, vc, n, H, mask, group)
    b = bar(dtype)
    scale = ref.abs().max()
    for r in range(R):  # row by row, each against the tensor's scale
        e = ((out[r].double().cpu() - ref[r]).abs().max() / scale).item()
        assert e < b, (r, e, b)
    uni = vc[1 // group, :n].double().mean(0).cpu()
    assert ((out[1].double().cpu() - uni).abs().max() / uni.abs().max()).item() < b
    # the late-maximum row without its dead keys gives the same answer
    tail = ref_decode(q[:1], kc[:1, 512:], vc[:1, 512:], n - 512, H, None, 1)
    assert ((out[0].double().cpu() - tail[0]).abs().max() / tail.abs().max()).item() < b


# -------------------------------------------------------------------------------------------------------------------------
# 4. sharing a read changes no arithmetic
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("g", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("n", [237, 617])
def test_decode_group_identity(dtype, d, g, n):
    """group = g equals, bit for bit, the same queries at group = 1 on gathered caches."""
    H = 8
    Bc = samples_for(g, H) + 1
    R, F = Bc * g, H * d
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, n + 2, F, dtype)
    mask = torch.zeros(R, n + 2, device=DEV)
    mask[1, n - 40:] = -1e5
    mask[R - 1, 5] = 8.0
    shared = decode(q, kc, vc, n, H, mask=mask, group=g)
    kg, vg = kc.repeat_interleave(g, 0).contiguous(), vc.repeat_interleave(g, 0).contiguous()
    alone = decode(q, kg, vg, n, H, mask=mask, group=1)
    assert torch.equal(shared, alone)
    assert rel_max(shared.reshape(R, F), ref_decode(q, kc, vc, n, H, mask, g)) < bar(dtype)


# -------------------------------------------------------------------------------------------------------------------------
# 5. one kernel family: OVQA_REQUIRE_MFMA=1 changes nothing
# -------------------------------------------------------------------------------------------------------------------------
ROUTE_ROWS = [(dt, n, g) for dt in ("f32", "bf16") for n in (237, 617, 2049) for g in (1, 5)]
ROUTE_SAMPLES = 66  # (528 workgroups of 5 queries: the shared form on a 256-CU chip)


def _route_outputs():
    from openvivqa_amd import _lib
    o_ = ops()
    rows = []
    for dt, n, g in ROUTE_ROWS:
        dtype = F32 if dt == "f32" else BF16
        q = rnd(ROUTE_SAMPLES * g, 1, 512, dtype=dtype, seed=1)
        kc, vc = caches(ROUTE_SAMPLES, n + 1, 512, dtype)
        _lib.launch_log_clear()
        out = o_.attention_decode(q, kc, vc, n, 8, group=g)
        rows.append({"dispatch": _lib.last_dispatch(), "launched": _lib.launch_log(), "sum": out.double().sum().item(),
                     "bits": out.float().cpu().view(torch.int32).sum().item()})
    return rows


def test_decode_route_is_the_same_under_require_mfma():
    here = _route_outputs()
    assert all(r["dispatch"] == "decode" for r in here), here
    env = dict(os.environ, OVQA_REQUIRE_MFMA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "route"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    there = json.loads(r.stdout.strip().splitlines()[-1])
    assert there == here, (there, here)


if __name__ == "__main__" and sys.argv[1:] == ["route"]:
    sys.path.insert(0, ROOT)
    print(json.dumps(_route_outputs()))
