"""Kernel-level parity of every C-ABI entry point against plain fp64/fp32 torch math.

Tolerances (written here, per the north star): OVQA_F32 paths <= 1e-3 (in fact
~1e-5); OVQA_BF16 paths <= 1e-2 *normalised* max error, i.e.
max|a-b| / max(1, max|b|), inputs/outputs being bf16-rounded.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# A/B switches of the library (scripts/gpu_alt_paths.sh runs this suite under them): assertions about WHICH kernel
# family ran hold for the default paths only
FORCED_SIMPLE = os.environ.get("OVQA_FORCE_SIMPLE", "0") == "1"
NO_FUSED_QKV = os.environ.get("OVQA_NO_FUSED_QKV", "0") == "1"

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


def ops():
    from openvivqa_amd import ops as o
    return o


def test_red_zone_harness_sees_a_store_one_byte_out_of_bounds():
    """The guard bands of tests/redzone.py (conftest.py puts them around every buffer of this file's tests) do catch a
    store directly behind the last byte and directly in front of the first one."""
    import redzone
    rz = redzone.RedZone()
    t = rz.alloc((5, 7), BF16, DEV)
    t.zero_()
    raw = rz.live[0][0]
    rz.check()  # (a store that stays inside leaves the bands alone)
    t = rz.alloc((5, 7), BF16, DEV)
    raw = rz.live[0][0]
    raw[redzone.BAND + 70] = 0
    with pytest.raises(AssertionError, match="0 bytes BEHIND"):
        rz.check()
    t = rz.alloc((3,), F32, DEV)
    rz.live[0][0][redzone.BAND - 1] = 0
    with pytest.raises(AssertionError, match="1 bytes IN FRONT"):
        rz.check()


def nerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def rel_max(a, ref):
    """max |a - ref| / max |ref| (the reference's own scale, no floor)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / ref.abs().max()).item()


def tol(dtype):
    return 1e-4 if dtype == F32 else 1e-2


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


LIN_SHAPES = [(37, 50, 29), (64, 64, 16), (256, 128, 64), (300, 256, 128), (6400, 512, 512), (1280, 1536, 512),
              (128, 512, 2048),
              # a decoding step's products: few activation rows (one-wave tiles, reductions split over 1 / 2 / 4 waves)
              (1, 512, 512), (17, 4000, 512), (64, 768, 768), (128, 2048, 32), (100, 512, 1024),
              # the BASELINE products (and ragged row counts of the same widths)
              (6400, 2048, 512), (6400, 1536, 512), (6400, 512, 2048), (6001, 2048, 512), (5555, 512, 512)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,N,K", LIN_SHAPES)
def test_linear_fwd_epilogues(dtype, M, N, K):
    o = ops()
    x, w = rnd(M, K, dtype=dtype), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=1)
    b, res = rnd(N, seed=2), rnd(M, N, dtype=dtype, seed=3)
    xd, wd, bd, rd = x.double(), w.double(), b.double(), res.double()
    u = xd @ wd.t() + bd
    assert nerr(o.linear_fwd(x, w, b), u) < tol(dtype)
    assert nerr(o.linear_fwd(x, w, None), xd @ wd.t()) < tol(dtype)
    y, pre = o.linear_fwd(x, w, b, o.EPI_BIAS_GELU, want_preact=True)
    assert nerr(pre, u) < tol(dtype) and nerr(y, gelu(u)) < tol(dtype)
    assert nerr(o.linear_fwd(x, w, b, o.EPI_BIAS_RESIDUAL, residual=res), u + rd) < tol(dtype)


@pytest.mark.parametrize("M,N,K", [(37, 48, 40), (256, 128, 64), (6400, 512, 512), (1280, 512, 2048), (300, 768, 3072)])
@pytest.mark.parametrize("lazy", [False, True], ids=["plain-residual", "lazy-layernorm-residual"])
def test_linear_fwd_res32(M, N, K, lazy):
    """fp32 residual stream epilogue: pre32 = res + drop(x W^T + b) in fp32; res either a plain fp32 tensor or the
    LayerNorm of the previous block's fp32 pre-LN sum, recomputed from its saved row statistics.  fp32 OUTPUT of a
    bf16 product: held to 2e-3 normalised (bf16 inputs are exact in the fp64 reference, only accumulation order and
    the fp32 epilogue differ)."""
    o = ops()
    x, w = rnd(M, K, dtype=BF16), rnd(N, K, dtype=BF16, scale=K ** -0.5, seed=1)
    b = rnd(N, seed=2)
    u = x.double() @ w.double().t() + b.double()
    if lazy:
        prev = rnd(M, N, scale=2.0, seed=3) + 0.3
        g, be = rnd(N, seed=4) * 0.2 + 1.0, rnd(N, seed=5) * 0.1
        yb, y32, mean, rstd = o.layernorm_fwd(prev, g, be, 1e-5, out_dtype=BF16, want_f32=True)
        ry, _, _ = ln_ref(prev, g, be)
        assert nerr(y32, ry) < 1e-5 and torch.equal(yb, y32.bfloat16())  # the bf16 operand is the rounded twin
        res = o.LnRef(prev, mean, rstd, g, be, 1e-5)
        assert nerr(res.materialize(), ry) < 1e-5
        rres = ry
    else:
        res = rnd(M, N, scale=2.0, seed=3)
        rres = res.double()
    pre = o.linear_fwd_res32(x, w, b, res)
    assert pre.dtype == F32 and nerr(pre, rres + u) < 2e-3
    if K % 8 == 0 and N % 8 == 0:
        from openvivqa_amd import _lib
        assert FORCED_SIMPLE or _lib.last_dispatch() == "mfma"
    d = o.DropSpec(p=0.3, seed=9, site=11, step=torch.tensor([3], dtype=torch.int32, device=DEV))
    keep = o.dropout_keep_mask(d, M * N, DEV).view(M, N).double() / 0.7
    assert nerr(o.linear_fwd_res32(x, w, b, res, drop=d), rres + u * keep) < 2e-3


def test_layernorm_bwd_fp32_input_bf16_gradient():
    """LayerNorm backward of the residual stream: bf16 dy, fp32 x (the pre-LN sum), bf16 dx (+ dropped branch)."""
    o = ops()
    M, D = 77, 512
    x = rnd(M, D, scale=2.0) + 0.5
    g, b = rnd(D, seed=1) * 0.2 + 1.0, rnd(D, seed=2) * 0.1
    _, mean, rstd = o.layernorm_fwd(x, g, b, 1e-5, out_dtype=BF16)
    dy = rnd(M, D, dtype=BF16, seed=9)
    xd = x.double().detach().cpu().requires_grad_(True)
    gd, bd = g.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (D,), gd, bd, 1e-5).backward(dy.double().cpu())
    dg, dbt = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    drop = o.DropSpec(p=0.25, seed=123, site=7, step=torch.tensor([5], dtype=torch.int32, device=DEV))
    dx, dxd = o.layernorm_bwd(dy, x, g, mean, rstd, dg, dbt, drop=drop)
    assert dx.dtype == BF16 and dxd.dtype == BF16
    assert nerr(dx, xd.grad) < 1e-2 and nerr(dg, gd.grad) < 1e-2 and nerr(dbt, bd.grad) < 1e-2
    keep = o.dropout_keep_mask(drop, M * D, DEV).view(M, D).double()
    assert nerr(dxd, dx.double() * keep / 0.75) < 1e-2


@pytest.mark.skipif(FORCED_SIMPLE, reason="OVQA_FORCE_SIMPLE=1 routes everything to the VALU kernels")
def test_dispatch_hook_reports_kernel_family():
    """ovqa_last_dispatch(): BASELINE shapes run the MFMA kernels, fp32 / ragged shapes the VALU ones."""
    from openvivqa_amd import _lib
    o = ops()
    x, w = rnd(6400, 512, dtype=BF16), rnd(1536, 512, dtype=BF16, scale=0.04, seed=1)
    o.linear_fwd(x, w, None)
    assert _lib.last_dispatch() == "mfma"
    o.linear_fwd(x.float(), w.float(), None)
    assert _lib.last_dispatch() == "simple"
    o.linear_fwd(rnd(37, 29, dtype=BF16), rnd(50, 29, dtype=BF16, seed=1), None)  # K % 8 != 0
    assert _lib.last_dispatch() == "simple"
    for d in (96, 128):  # M4C's heads of 96 features, and 128
        q, k = rnd(4, 182, 8 * d, dtype=BF16, seed=2), rnd(4, 182, 8 * d, dtype=BF16, seed=3)
        out, lse, _ = o.attention_fwd(q, k, k, None, 8)
        assert _lib.last_dispatch() == "mfma"
        o.attention_bwd(rnd(4, 182, 8 * d, dtype=BF16, seed=4), q, k, k, out, lse, None, 8)
        assert _lib.last_dispatch() == "mfma"
    for nq, nk in ((100, 100), (100, 20), (20, 20)):
        q = rnd(64, nq, 1536, dtype=BF16, seed=2)
        kv = rnd(64, nk, 1024, dtype=BF16, seed=3)
        out, lse, _ = o.attention_fwd(q[..., :512], kv[..., :512], kv[..., 512:], None, 8)
        assert _lib.last_dispatch() == "mfma"
        o.attention_bwd(rnd(64, nq, 512, dtype=BF16, seed=4), q[..., :512], kv[..., :512], kv[..., 512:], out, lse, None, 8)
        assert _lib.last_dispatch() == "mfma"


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_linear_fwd_strided_and_3d(dtype):
    o = ops()
    big = rnd(4, 10, 3 * 64, dtype=dtype)
    x = big[..., 64:128]  # row-strided view
    w, b = rnd(128, 64, dtype=dtype, scale=0.1, seed=5), rnd(128, seed=6)
    y = o.linear_fwd(x, w, b)
    assert y.shape == (4, 10, 128)
    assert nerr(y, x.double() @ w.double().t() + b.double()) < tol(dtype)


def test_linear_fwd_256_tiles_grouped_raster_and_ragged_edges():
    """The 256 x 256-tile form (csrc/gemm_tile256.h): a grid large enough for the grouped tile order (>= 512 tiles, >= 8
    panels each way), and ragged edges in both dimensions (straight-line epilogue inside, guarded one on the edge tiles),
    every epilogue, against fp32 products of the same bf16 operands.  The first three shapes (K < 1024) run the 128-tile
    forms; the last two reach the 256-tile form itself (K >= 1024, >= 3/4 of a round of a 256-CU chip: plain raster with
    ragged edges, and the grouped raster with a short last group, 588 tiles for the XCD remap, 17 K steps), which the
    launch log must show."""
    from openvivqa_amd import _lib
    o = ops()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for (M, N, K) in [(8192, 4096, 256), (6001, 2040, 320), (8000, 4104, 64), (6000, 2000, 1024), (12500, 3000, 1088)]:
        x, w = rnd(M, K, dtype=BF16), rnd(N, K, dtype=BF16, scale=K ** -0.5, seed=1)
        b, res = rnd(N, seed=2), rnd(M, N, dtype=BF16, seed=3)
        u = x.float() @ w.float().t() + b
        _lib.launch_log_clear()
        assert nerr(o.linear_fwd(x, w, b), u) < 1e-2
        if K >= 1024 and ncu == 256 and not FORCED_SIMPLE and os.environ.get("OVQA_GEMM_T256", "1") != "0":
            assert _lib.launch_log() == ["ovqa_t256::kernel<MEpiBias,3>"], _lib.launch_log()
        y, pre = o.linear_fwd(x, w, b, o.EPI_BIAS_GELU, want_preact=True)
        assert nerr(pre, u) < 1e-2 and nerr(y, gelu(u.double())) < 1e-2
        assert nerr(o.linear_fwd(x, w, b, o.EPI_BIAS_RESIDUAL, residual=res), u + res.float()) < 1e-2
    if ncu != 256:  # (the parity checks above ran; the 256-tile grid rule depends on the CU count)
        pytest.skip(f"the 256-tile route of the K >= 1024 shapes is laid out for 256 CUs; this device has {ncu}: not checked")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,N,K", [(37, 50, 29), (256, 128, 64), (640, 512, 2048), (1280, 2048, 512)])
def test_linear_bwd_data(dtype, M, N, K):
    o = ops()
    dy, w = rnd(M, N, dtype=dtype), rnd(N, K, dtype=dtype, scale=N ** -0.5, seed=1)
    ref = dy.double() @ w.double()
    assert nerr(o.linear_bwd_data(dy, w), ref) < tol(dtype)
    base = rnd(M, K, dtype=dtype, seed=4)
    assert nerr(o.linear_bwd_data(dy, w, addend=base), ref + base.double()) < tol(dtype)
    out = base.clone()
    o.linear_bwd_data(dy, w, out=out, addend=out)  # aliasing addend == out is allowed
    assert nerr(out, ref + base.double()) < tol(dtype)
    u = rnd(M, K, dtype=dtype, seed=7)
    assert nerr(o.linear_bwd_data(dy, w, preact=u), ref * gelu_grad(u.double())) < tol(dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,N,K", [(37, 50, 29), (256, 128, 64), (6400, 512, 512), (1280, 2048, 512)])
def test_linear_bwd_weight(dtype, M, N, K):
    o = ops()
    dy, x = rnd(M, N, dtype=dtype, scale=M ** -0.5), rnd(M, K, dtype=dtype, seed=1)
    dw = torch.full((N, K), 7.0, device=DEV)
    db = torch.full((N,), 7.0, device=DEV)
    o.linear_bwd_weight(dy, x, dw, db)
    rw, rb = dy.double().t() @ x.double(), dy.double().sum(0)
    assert nerr(dw, rw) < tol(dtype) and nerr(db, rb) < tol(dtype)
    o.linear_bwd_weight(dy, x, dw, db, accumulate=True)
    assert nerr(dw, 2 * rw) < 2 * tol(dtype) and nerr(db, 2 * rb) < 2 * tol(dtype)
    dw2 = torch.zeros(N, K, device=DEV)
    o.linear_bwd_weight(dy, x, dw2, None)
    assert nerr(dw2, rw) < tol(dtype)


@pytest.mark.parametrize("specs", [
    [(6400, 512, 512), (1280, 1024, 512), (400, 1536, 512), (1280, 2048, 512), (6400, 512, 2048), (37, 32, 64)],
    # every M a multiple of 64: the direct-to-LDS form (ragged N / K included, partial tiles in both directions)
    [(6400, 512, 512), (1280, 1024, 512), (448, 1536, 512), (64, 72, 40), (128, 8, 2048), (6400, 512, 2048),
     (64, 304, 264), (192, 768, 3072), (1280, 2048, 512)],
], ids=["register-staged", "direct-to-lds"])
def test_grouped_wgrad_and_bias_grad(specs):
    o = ops()
    q = o.WgradQueue()
    refs, outs = [], []
    for i, (M, N, K) in enumerate(specs):
        dy, x = rnd(M, N, dtype=BF16, scale=M ** -0.5, seed=i), rnd(M, K, dtype=BF16, seed=10 + i)
        dw = torch.full((N, K), 3.0, device=DEV)
        dbq = torch.full((N,), 5.0, device=DEV)
        acc = i % 2 == 1
        q.add(dy, x, dw, acc, dbq, not acc)
        refs.append((dy.double().t() @ x.double() + (3.0 if acc else 0.0), dy.double().sum(0) + (0.0 if acc else 5.0)))
        outs.append((dw, dbq))
        db = torch.full((N,), 2.0, device=DEV)
        o.bias_grad(dy, db)
        assert nerr(db, dy.double().sum(0)) < 1e-2
        o.bias_grad(dy, db, accumulate=True)
        assert nerr(db, 2 * dy.double().sum(0)) < 2e-2
    q.finish()
    torch.cuda.synchronize()
    for (M, N, K), (dw, dbq), (ref, refb) in zip(specs, outs, refs):
        assert nerr(dw, ref) < 1e-2, (M, N, K, nerr(dw, ref))
        assert nerr(dbq, refb) < 1e-2, (M, N, K, "bias", nerr(dbq, refb))
    assert not q.items and not q.inflight


def ln_ref(x, g, b, eps=1e-5):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double(), mu.squeeze(-1), 1 / torch.sqrt(var + eps).squeeze(-1)


@pytest.mark.parametrize("in_dtype,out_dtype", [(F32, F32), (BF16, BF16), (F32, BF16)])
@pytest.mark.parametrize("D", [32, 512, 768])
def test_layernorm_fwd_bwd(in_dtype, out_dtype, D):
    o = ops()
    B, N = 3, 11
    x = rnd(B, N, D, dtype=in_dtype, scale=2.0) + 0.5
    g, b = (rnd(D, seed=1) * 0.2 + 1.0), rnd(D, seed=2) * 0.1
    pos = rnd(N, D, seed=3)
    y, mean, rstd = o.layernorm_fwd(x, g, b, 1e-5, out_dtype=out_dtype)
    ry, rmu, rrs = ln_ref(x, g, b)
    assert nerr(y, ry) < tol(out_dtype) and nerr(mean, rmu.reshape(-1)) < 1e-4 and nerr(rstd, rrs.reshape(-1)) < 1e-4
    yp, _, _ = o.layernorm_fwd(x, g, b, 1e-5, out_dtype=out_dtype, pos=pos)
    assert nerr(yp, ry + pos.double()[None]) < tol(out_dtype)
    # backward vs autograd (fp64)
    dy = rnd(B, N, D, dtype=out_dtype, seed=9)
    xd = x.double().detach().cpu().requires_grad_(True)
    gd, bd = g.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (D,), gd, bd, 1e-5).backward(dy.double().cpu())
    dg, dbt = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dx, dxd = o.layernorm_bwd(dy, x, g, mean, rstd, dg, dbt, dx_dtype=in_dtype)
    assert dxd is dx
    t = max(tol(in_dtype), tol(out_dtype))
    assert nerr(dx, xd.grad) < t and nerr(dg, gd.grad) < t and nerr(dbt, bd.grad) < t
    o.layernorm_bwd(dy, x, g, mean, rstd, dg, dbt, dx_dtype=in_dtype, accumulate=True)
    assert nerr(dg, 2 * gd.grad) < 2 * t


@pytest.mark.parametrize("M,D", [(4096, 2048), (4100, 1168), (4096, 1176), (5000, 1024)])
def test_layernorm_bwd_long_activation_wide_rows(M, D):
    """the 8-wave backward (M >= 4096) asks for 56 * D bytes of dynamic LDS, more than a launch gets by
    default once D > 1168; such rows keep the 4-wave form.  Both sides of the switch, at sizes that need it."""
    o = ops()
    x, dy = rnd(M, D, dtype=BF16, scale=1.5), rnd(M, D, dtype=BF16, seed=4)
    g, b = (rnd(D, seed=1) * 0.2 + 1.0), rnd(D, seed=2) * 0.1
    _, mean, rstd = o.layernorm_fwd(x, g, b, 1e-5)
    xd = x.double().detach().cpu().requires_grad_(True)
    gd, bd = g.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (D,), gd, bd, 1e-5).backward(dy.double().cpu())
    dg, dbt = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dx, _ = o.layernorm_bwd(dy, x, g, mean, rstd, dg, dbt)
    assert nerr(dx, xd.grad) < 1e-2 and nerr(dg, gd.grad) < 1e-2 and nerr(dbt, bd.grad) < 1e-2


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_layernorm_bwd_dropout_branch(dtype):
    o = ops()
    M, D = 40, 512
    x, dy = rnd(M, D, dtype=dtype), rnd(M, D, dtype=dtype, seed=1)
    g, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    _, mean, rstd = o.layernorm_fwd(x, g, b)
    drop = o.DropSpec(p=0.25, seed=123, site=7, step=torch.tensor([5], dtype=torch.int32, device=DEV))
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dx, dxd = o.layernorm_bwd(dy, x, g, mean, rstd, dg, db, drop=drop)
    keep = o.dropout_keep_mask(drop, M * D, DEV).view(M, D).double()
    assert nerr(dxd, dx.double() * keep / 0.75) < tol(dtype)


ATT_SHAPES = [(2, 4, 5, 7, 8), (3, 8, 100, 100, 64), (2, 8, 100, 20, 64), (2, 8, 20, 20, 64), (2, 8, 20, 100, 64),
              (2, 2, 1, 7, 16), (1, 8, 237, 237, 64), (2, 8, 182, 182, 96),
              # heads of 96 / 128 features on the MFMA kernels (256-byte image rows): M4C's 182 positions, short and
              # ragged key counts, more queries than one workgroup's tiles
              (2, 8, 12, 50, 96), (3, 4, 100, 100, 128), (2, 4, 150, 192, 96), (2, 4, 64, 128, 128), (2, 8, 33, 1, 96), (1, 8, 160, 64, 64),
              # merged small-n_k backward: 2 and 3(->4) query tiles, ragged packing (9 problems, 4 per workgroup)
              (3, 8, 50, 32, 64), (2, 8, 70, 13, 64), (5, 8, 128, 20, 64), (2, 8, 33, 1, 64), (3, 3, 20, 20, 64)]


def att_ref(q, k, v, mask, H):
    B, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    dk, dv = q.shape[2] // H, v.shape[2] // H
    qh = q.double().view(B, nq, H, dk).transpose(1, 2)
    kh = k.double().view(B, nk, H, dk).transpose(1, 2)
    vh = v.double().view(B, nk, H, dv).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dk)
    if mask is not None:
        s = s + mask.double()
    p = torch.softmax(s, -1)
    return (p @ vh).transpose(1, 2).reshape(B, nq, H * dv), p, torch.logsumexp(s, -1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("mask_kind", ["none", "pad", "full", "causal"])
@pytest.mark.parametrize("B,H,nq,nk,d", ATT_SHAPES)
def test_attention_fwd_bwd(dtype, mask_kind, B, H, nq, nk, d):
    o = ops()
    if mask_kind == "causal" and nq != nk:
        pytest.skip("causal needs nq == nk")
    qkv_q = rnd(B, nq, 3 * H * d, dtype=dtype, seed=1)  # packed buffer: q is a strided view
    q = qkv_q[..., :H * d]
    k, v = rnd(B, nk, H * d, dtype=dtype, seed=2), rnd(B, nk, H * d, dtype=dtype, seed=3)
    mask = None
    if mask_kind == "pad":
        mask = torch.zeros(B, 1, 1, nk, device=DEV)
        mask[0, ..., nk // 2:] = -1e5
        mask[-1] = -1e5  # fully padded sample -> uniform attention, no NaN
    elif mask_kind == "full":
        mask = (torch.rand(B, 1, nq, nk, generator=torch.Generator().manual_seed(4)) < 0.3).float().to(DEV) * -1e5
    elif mask_kind == "causal":
        mask = (torch.ones(nq, nq).triu(1) * -1e5)[None, None].to(DEV)
    out, lse, att = o.attention_fwd(q, k, v, mask, H, need_att=True)
    ro, rp, rl = att_ref(q, k, v, mask, H)
    assert torch.isfinite(out.float()).all()
    if mask_kind == "pad":
        # a fully masked sample adds -1e5 to every score: in fp32 (kernel AND reference, attentions.py:55)
        # the scores are then quantised to ulp(1e5) = 2^-7, so that sample is only comparable to ~1e-2
        assert nerr(out[-1], ro[-1]) < 2e-2 and nerr(att[-1], rp[-1]) < 2e-2
        out_c, ro_c, att_c, rp_c = out[:-1], ro[:-1], att[:-1], rp[:-1]
    else:
        out_c, ro_c, att_c, rp_c = out, ro, att, rp
    assert nerr(out_c, ro_c) < tol(dtype) and nerr(att_c, rp_c) < tol(dtype) and nerr(lse, rl) < 1e-2
    # backward vs autograd fp64
    d_o = rnd(B, nq, H * d, dtype=dtype, seed=5)
    qd, kd, vd = (t.double().cpu().detach().clone().requires_grad_(True) for t in (q, k, v))
    att_ref(qd, kd, vd, None if mask is None else mask.cpu(), H)[0].backward(d_o.double().cpu())
    dq, dk, dv = o.attention_bwd(d_o, q, k, v, out, lse, mask, H)
    t = tol(dtype) * (3 if dtype == BF16 else 1)
    sl = slice(0, -1) if mask_kind == "pad" else slice(None)
    assert nerr(dq[sl], qd.grad[sl]) < t and nerr(dk[sl], kd.grad[sl]) < t and nerr(dv[sl], vd.grad[sl]) < t
    if mask_kind == "pad":
        assert nerr(dq[-1], qd.grad[-1]) < 3e-2 and nerr(dv[-1], vd.grad[-1]) < 3e-2


@pytest.mark.parametrize("B,H,nq,nk", [(4, 8, 100, 100), (4, 8, 100, 20), (6, 8, 20, 20), (2, 8, 237, 237)])
def test_attention_bwd_delta_uses_the_output_residual(B, H, nq, nk):
    """delta_i = dO_i . O_i is where the bf16 rounding of O is amplified: dS = P (dP - delta) cancels, and with
    near-uniform attention (small scores: a freshly initialised stack) dQ / dK are orders of magnitude smaller than the
    cancelling terms.  The forward kernels write the rounding residual o_lo = bf16(o_exact - o); with it the backward's
    dQ / dK come within a few percent of fp64 math on the same bf16 inputs, without it they are off by their own size.
    One case per MFMA backward kernel (role-split, merged small-n_k x2, two-kernel)."""
    o_ = ops()
    d = 64
    q = rnd(B, nq, H * d, dtype=BF16, scale=0.05, seed=1)
    k = rnd(B, nk, H * d, dtype=BF16, scale=0.05, seed=2)
    # values nearly equal across the keys (what LayerNorm-ed features through a fresh fc_v look like to dP = dO V^T):
    # dP is then almost constant along a row, dP - delta cancels to ~2 % of dP
    v = (rnd(B, 1, H * d, seed=3) + 0.02 * rnd(B, nk, H * d, seed=5)).to(BF16)
    mask = torch.zeros(B, 1, 1, nk, device=DEV)
    mask[1, ..., nk - 3:] = -1e5
    lo = []
    o, lse, _ = o_.attention_fwd(q, k, v, mask, H, lo_out=lo)
    assert len(lo) == 1 and lo[0].dtype == BF16 and lo[0].shape == o.shape
    ro, _, _ = att_ref(q, k, v, mask, H)
    # o + o_lo carries 16 significant bits of the exact output
    assert nerr(o.double() + lo[0].double(), ro) < 2e-4 and nerr(o, ro) < 1e-2
    d_o = rnd(B, nq, H * d, dtype=BF16, seed=4)
    qd, kd, vd = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    att_ref(qd, kd, vd, mask.cpu(), H)[0].backward(d_o.double().cpu())
    rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()
    dq1, dk1, dv1 = o_.attention_bwd(d_o, q, k, v, o, lse, mask, H, o_lo=lo[0])
    dq0, dk0, dv0 = o_.attention_bwd(d_o, q, k, v, o, lse, mask, H)
    e1, e0 = (rel(dq1, qd.grad), rel(dk1, kd.grad)), (rel(dq0, qd.grad), rel(dk0, kd.grad))
    assert rel(dv1, vd.grad) < 1e-2 and rel(dv0, vd.grad) < 1e-2
    assert e1[0] < 2e-2 and e1[1] < 2e-2, (e1, e0)           # bf16 dS into the matrix cores is what is left
    if not FORCED_SIMPLE:  # (the VALU kernels take delta = rowsum(P dP) from fp32 probabilities: no O involved)
        assert e1[0] < 0.2 * e0[0] and e1[1] < 0.2 * e0[1], (e1, e0)  # ... and the rounded-O delta was most of the error


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Bc,group,H,d,Lmax,n", [(4, 1, 8, 64, 20, 1), (4, 1, 8, 64, 20, 13), (5, 3, 8, 64, 237, 237),
                                                 (3, 2, 4, 32, 40, 33), (2, 1, 8, 128, 300, 257), (64, 3, 8, 64, 237, 200)])
def test_attention_decode_single_query(dtype, Bc, group, H, d, Lmax, n):
    """ovqa_attention_decode: one query per row against in-place K / V caches [rows / group, Lmax, H*d] of which n keys
    are live (rows of a group share a cache row), additive per-row mask; against fp64 softmax attention and against the
    general attention kernel on the gathered prefix."""
    o_ = ops()
    R, F = Bc * group, H * d
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = rnd(Bc, Lmax, F, dtype=dtype, seed=2), rnd(Bc, Lmax, F, dtype=dtype, seed=3)
    mask = torch.zeros(R, Lmax, device=DEV)
    if n > 4:
        mask[1, n - 3:] = -1e5
        mask[R - 1, :2] = -1e5
    out = o_.attention_decode(q, kc, vc, n, H, mask=mask, group=group)
    assert out.shape == q.shape and out.dtype == dtype
    kg, vg = kc[:, :n].repeat_interleave(group, 0), vc[:, :n].repeat_interleave(group, 0)
    ro, _, _ = att_ref(q, kg, vg, mask[:, None, None, :n], H)
    assert nerr(out, ro) < tol(dtype), nerr(out, ro)
    if d == 64:
        o2, _, _ = o_.attention_fwd(q, kg.contiguous(), vg.contiguous(), mask[:, None, None, :n].contiguous(), H, save_lse=False)
        assert nerr(out, o2) < tol(dtype)
    # strided output and no mask
    buf = torch.zeros(R, 2 * F, dtype=dtype, device=DEV)
    o_.attention_decode(q.view(R, F), kc, vc, n, H, group=group, out=buf[:, F:])
    ro2, _, _ = att_ref(q, kg, vg, None, H)
    assert nerr(buf[:, F:].reshape(R, 1, F), ro2) < tol(dtype) and float(buf[:, :F].abs().max()) == 0.0


@pytest.mark.parametrize("R,V,k", [(192, 4000, 3), (5, 37, 1), (64, 4000, 8), (3, 9, 4), (7, 130, 5)])
def test_topk_rows_matches_torch(R, V, k):
    o_ = ops()
    x = torch.log_softmax(rnd(R, V, seed=3) * 3, -1)
    x[0, :] = x[0, 0]          # a row of ties: indices 0..k-1 in order
    if V > 70:
        x[1, 5] = x[1, 69] = 9.0   # a tie between two lanes' heads
    v, i = o_.topk_rows(x, k)
    tv, ti = torch.topk(x, k, dim=-1, largest=True, sorted=True)
    assert torch.equal(v, tv)
    assert torch.equal(torch.gather(x, 1, i), v)  # the indices point at the values
    assert torch.equal(i[0], torch.arange(k, device=DEV)) and (V <= 70 or i[1, :2].tolist() == [5, 69])
    rows = torch.ones(R, dtype=torch.bool)
    rows[:2] = False
    assert torch.equal(i[rows], ti[rows])  # (no ties elsewhere: random floats)
    x3 = x.view(1, R, V).expand(2, R, V).contiguous()
    v3, i3 = o_.topk_rows(x3, k)
    assert v3.shape == (2, R, k) and torch.equal(v3[1], v) and torch.equal(i3[0], i)


def test_attention_bwd_with_att_gradient():
    """d_att: gradient w.r.t. the returned attention weights (reference att is differentiable)."""
    o = ops()
    B, H, nq, nk, d = 2, 4, 9, 11, 16
    q, k, v = rnd(B, nq, H * d, seed=1), rnd(B, nk, H * d, seed=2), rnd(B, nk, H * d, seed=3)
    mask = torch.zeros(B, 1, 1, nk, device=DEV)
    mask[0, ..., 8:] = -1e5
    out, lse, att = o.attention_fwd(q, k, v, mask, H, need_att=True)
    d_o, d_att = rnd(B, nq, H * d, seed=5), rnd(B, H, nq, nk, seed=6)
    qd, kd, vd = (t.double().cpu().detach().clone().requires_grad_(True) for t in (q, k, v))
    ro, rp, _ = att_ref(qd, kd, vd, mask.cpu(), H)
    ((ro * d_o.double().cpu()).sum() + (rp * d_att.double().cpu()).sum()).backward()
    dq, dk, dv = o.attention_bwd(d_o, q, k, v, out, lse, mask, H, d_att=d_att)
    assert nerr(dq, qd.grad) < 1e-4 and nerr(dk, kd.grad) < 1e-4 and nerr(dv, vd.grad) < 1e-4


def test_dropout_mask_statistics_and_epilogue():
    o = ops()
    n = 1 << 20
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    d1 = o.DropSpec(p=0.1, seed=42, site=1, step=step)
    m1 = o.dropout_keep_mask(d1, n, DEV)
    assert abs(m1.float().mean().item() - 0.9) < 3e-3
    assert torch.equal(m1, o.dropout_keep_mask(d1, n, DEV))  # pure function
    for other in (o.DropSpec(0.1, 43, 1, step), o.DropSpec(0.1, 42, 2, step),
                  o.DropSpec(0.1, 42, 1, torch.tensor([4], dtype=torch.int32, device=DEV))):
        m2 = o.dropout_keep_mask(other, n, DEV)
        agree = (m1 == m2).float().mean().item()
        assert abs(agree - (0.81 + 0.01)) < 5e-3  # independent masks
    # fused epilogues use exactly this mask (index = m*N + n)
    for dtype, (M, N, K) in [(F32, (40, 48, 32)), (BF16, (256, 128, 64))]:
        x, w, b = rnd(M, K, dtype=dtype), rnd(N, K, dtype=dtype, scale=0.2, seed=1), rnd(N, seed=2)
        res = rnd(M, N, dtype=dtype, seed=3)
        d = o.DropSpec(p=0.3, seed=9, site=11, step=step)
        keep = o.dropout_keep_mask(d, M * N, DEV).view(M, N).double() / 0.7
        u = x.double() @ w.double().t() + b.double()
        assert nerr(o.linear_fwd(x, w, b, o.EPI_BIAS_RESIDUAL, residual=res, drop=d), res.double() + u * keep) < tol(dtype)
        assert nerr(o.linear_fwd(x, w, b, o.EPI_BIAS_GELU, drop=d), gelu(u) * keep) < tol(dtype)
        dy, pre = rnd(M, N, dtype=dtype, seed=4), rnd(M, K, dtype=dtype, seed=5)
        keep_k = o.dropout_keep_mask(d, M * K, DEV).view(M, K).double() / 0.7
        ref = (dy.double() @ w.double()) * keep_k * gelu_grad(pre.double())
        assert nerr(o.linear_bwd_data(dy, w, preact=pre, drop=d), ref) < tol(dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_pointer_score_and_batched_gemm(dtype):
    o = ops()
    B, T, N, D = 3, 12, 50, 96
    q, k = rnd(B, T, D, dtype=dtype), rnd(B, N, D, dtype=dtype, seed=1)
    s0 = q.double() @ k.double().transpose(1, 2) / math.sqrt(D)
    am = torch.zeros(B, N, device=DEV)
    am[1, 40:] = -1e5
    assert nerr(o.pointer_score(q, k, 1 / math.sqrt(D), add_mask=am), s0 + am.double()[:, None]) < tol(dtype)
    kf = torch.zeros(B, N, dtype=torch.uint8, device=DEV)
    kf[2, 10:] = 1
    s = o.pointer_score(q, k, 1 / math.sqrt(D), key_fill=kf)
    assert torch.isinf(s[2, :, 10:]).all() and nerr(s[:2], s0[:2]) < tol(dtype)
    qf = torch.zeros(B, T, dtype=torch.uint8, device=DEV)
    qf[0, 5:] = 1
    s = o.pointer_score(q, k, 1 / math.sqrt(D), query_fill=qf)
    assert torch.isinf(s[0, 5:]).all() and nerr(s[1:], s0[1:]) < tol(dtype)
    a, b = rnd(B, T, N, dtype=dtype, seed=2), rnd(B, N, D, dtype=dtype, seed=3)
    assert nerr(o.batched_gemm(a, b, alpha=0.5), 0.5 * a.double() @ b.double()) < tol(dtype) * 4
    assert nerr(o.batched_gemm(a, q, trans_a=True), a.double().transpose(1, 2) @ q.double()) < tol(dtype) * 4
    assert nerr(o.batched_gemm(q, k, trans_b=True), q.double() @ k.double().transpose(1, 2)) < tol(dtype) * 4
    if dtype == BF16 and not FORCED_SIMPLE:
        from openvivqa_amd import _lib
        assert _lib.last_dispatch() == "mfma"  # the NT form runs on the matrix cores


@pytest.mark.parametrize("B,T,N,D", [(5, 12, 50, 768), (2, 33, 17, 64), (1, 1, 1, 32), (3, 12, 50, 1536), (2, 20, 100, 2048)])
def test_pointer_score_mfma_shapes(B, T, N, D):
    """The one-wave MFMA tiles of the pointer scorers (bf16): M4C's 12 x 50 x 768 (mmf_m4c.py:391-394), ragged tile
    edges, reductions split over 1 / 2 / 4 waves; masks and fills as in the VALU form."""
    o = ops()
    q, k = rnd(B, T, D, dtype=BF16), rnd(B, N, D, dtype=BF16, seed=1)
    s0 = q.double() @ k.double().transpose(1, 2) / math.sqrt(D)
    am = torch.zeros(B, N, device=DEV)
    am[B - 1, N // 2:] = -1e5
    kf = torch.zeros(B, N, dtype=torch.uint8, device=DEV)
    kf[0, N - 1:] = 1
    qf = torch.zeros(B, T, dtype=torch.uint8, device=DEV)
    qf[0, T - 1:] = 1
    s = o.pointer_score(q, k, 1 / math.sqrt(D), add_mask=am, key_fill=kf, query_fill=qf)
    if not FORCED_SIMPLE:
        from openvivqa_amd import _lib
        assert _lib.last_dispatch() == "mfma"
    want = s0 + am.double()[:, None]
    want[0, :, N - 1:] = -math.inf
    want[0, T - 1:] = -math.inf
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(s), fin.to(s.device))
    assert nerr(torch.where(fin.to(s.device), s, torch.zeros_like(s)), torch.where(fin, want, torch.zeros_like(want))) < 1e-2
    c = o.batched_gemm(q, k, trans_b=True, alpha=0.25, out_dtype=F32)
    assert nerr(c, 0.25 * q.double() @ k.double().transpose(1, 2)) < 1e-2


@pytest.mark.parametrize("grad_dtype", [F32, BF16])
def test_adam_matches_torch_and_shadow(grad_dtype):
    o = ops()
    n = 4099
    p0 = rnd(n)
    ref = torch.nn.Parameter(p0.clone().cpu())
    opt = torch.optim.Adam([ref], lr=0.01, betas=(0.9, 0.98))
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pad = (n + 3) // 4 * 4
    shadow = torch.zeros(pad, dtype=BF16, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_scale = torch.tensor([0.5], device=DEV)
    for it in range(3):
        g = rnd(n, seed=10 + it).to(grad_dtype)  # bf16: the data-parallel staging buffer is read directly
        ref.grad = g.float().cpu().clone() / 4.0
        for grp in opt.param_groups:
            grp["lr"] = 0.01 * 0.5
        opt.step()
        o.increment_step(step)
        o.adam_step(p, g, m, v, shadow, lr=0.01, step=step, lr_scale=lr_scale, grad_scale=0.25)
    assert int(step.item()) == 3
    assert nerr(p, ref.detach()) < 1e-5
    assert torch.equal(shadow[:n], p.to(BF16))


def test_grouped_transpose_and_dx_from_transposed_weights():
    """ovqa_grouped_transpose (ragged sizes) and ovqa_linear_bwd_data_wt == ovqa_linear_bwd_data, including a
    column block of a wider transposed matrix, the fused dropout*GELU' epilogue and the addend."""
    import ctypes as C
    import numpy as np
    from openvivqa_amd import _lib
    from openvivqa_amd.ops import DropSpec
    o = ops()
    mats = [rnd(512, 512, dtype=BF16, seed=1), rnd(1536, 512, dtype=BF16, seed=2), rnd(72, 200, dtype=BF16, seed=3)]
    outs = [torch.zeros(m.shape[1], m.shape[0], dtype=BF16, device=DEV) for m in mats]
    probs = (_lib.TransposeProblem * len(mats))()
    for i, (m, t) in enumerate(zip(mats, outs)):
        probs[i] = _lib.TransposeProblem(m.data_ptr(), t.data_ptr(), m.shape[1], m.shape[0], m.shape[0], m.shape[1])
    table = torch.from_numpy(np.frombuffer(bytes(probs), dtype=np.uint8).copy()).to(DEV)
    o.grouped_transpose(table, len(mats), max(((m.shape[0] + 63) // 64) * ((m.shape[1] + 63) // 64) for m in mats))
    for m, t in zip(mats, outs):
        assert torch.equal(t, m.t().contiguous())
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for M in (6400, 1280, 72):
        w = mats[1]                      # packed [1536, 512] weight, wt = [512, 1536]
        wt = outs[1]
        dy = rnd(M, 1536, dtype=BF16, seed=4)
        add = rnd(M, 512, dtype=BF16, seed=5)
        a = o.linear_bwd_data(dy, w, addend=add)
        b = o.linear_bwd_data_wt(dy, wt, addend=add)
        assert nerr(b, a) < 6e-3  # identical on the MFMA path; one bf16 ulp (0.125 at ~25) when OVQA_FORCE_SIMPLE reroutes `a`
        ref = dy.double() @ w.double() + add.double()  # and both against fp64 math: one bf16 rounding of the output
        assert rel_max(b, ref) < 2 ** -8 and rel_max(a, ref) < 2 ** -8
        # column block: the middle 512 weight rows only (a strided [512, 512] view of wt)
        a = o.linear_bwd_data(dy[:, 512:1024].contiguous(), w[512:1024])
        blk = wt[:, 512:1024]
        b = o.linear_bwd_data_wt(dy[:, 512:1024], blk)
        assert nerr(b, a) < 6e-3  # identical on the MFMA path; one bf16 ulp (0.125 at ~25) when OVQA_FORCE_SIMPLE reroutes `a`
        assert rel_max(b, dy[:, 512:1024].double() @ w[512:1024].double()) < 2 ** -8
        # FFN seam: dy [M, 512] x W2 [512, 2048] with dropout * gelu'(u)
        w2 = rnd(512, 2048, dtype=BF16, seed=6)
        w2t = w2.t().contiguous()
        u = rnd(M, 2048, dtype=BF16, seed=7)
        dyo = rnd(M, 512, dtype=BF16, seed=8)
        drop = DropSpec(p=0.1, seed=123, site=4, step=step)
        a = o.linear_bwd_data(dyo, w2, preact=u, drop=drop)
        b = o.linear_bwd_data_wt(dyo, w2t, preact=u, drop=drop)
        assert nerr(b, a) < 6e-3  # identical on the MFMA path; one bf16 ulp (0.125 at ~25) when OVQA_FORCE_SIMPLE reroutes `a`
        keep = o.dropout_keep_mask(drop, M * 2048, DEV).view(M, 2048).double() / 0.9
        assert rel_max(b, (dyo.double() @ w2.double()) * keep * gelu_grad(u.double())) < 2 ** -8


def test_layernorm_bwd_deferred_grouped_reduce():
    """dgamma/dbeta of several LayerNorms via per-call partials + ONE grouped reduce == the immediate form."""
    from openvivqa_amd.ops import WgradQueue
    o = ops()
    q = WgradQueue()
    cases = [(6400, 512), (1280, 512), (37, 64), (5000, 768)]
    outs = []
    for i, (M, D) in enumerate(cases):
        x, dy = rnd(M, D, dtype=BF16, seed=i), rnd(M, D, dtype=BF16, seed=10 + i)
        gamma = rnd(D, seed=20 + i)
        mean, rstd = x.float().mean(-1), (x.float().var(-1, unbiased=False) + 1e-5).rsqrt()
        g0, b0 = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        dx0, _ = o.layernorm_bwd(dy, x, gamma, mean, rstd, g0, b0)
        acc = i % 2 == 1
        g1 = torch.full((D,), 3.0 if acc else 7.0, device=DEV)  # 7.0 must be overwritten, 3.0 accumulated into
        b1 = torch.full((D,), -2.0 if acc else 7.0, device=DEV)
        dx1, _ = o.layernorm_bwd(dy, x, gamma, mean, rstd, g1, b1, accumulate=acc, defer=q)
        assert torch.equal(dx0, dx1)
        outs.append((g0, b0, g1, b1, acc))
    assert len(q.reduces) == len(cases)
    q.finish()
    torch.cuda.synchronize()
    for g0, b0, g1, b1, acc in outs:
        assert nerr(g1 - (3.0 if acc else 0.0), g0) < 1e-5 and nerr(b1 - (-2.0 if acc else 0.0), b0) < 1e-5


def test_sq_loss_and_cast():
    o = ops()
    for dtype in (F32, BF16):
        x = rnd(7, 300, dtype=dtype)
        loss = torch.full((1,), 5.0, device=DEV)
        dx = o.sq_loss_fwd_bwd(x, loss)
        assert abs(loss.item() - x.double().pow(2).mean().item()) < 1e-4
        assert nerr(dx, 2 * x.double() / x.numel()) < tol(dtype)
        o.sq_loss_fwd_bwd(x, loss, accumulate=True)
        assert abs(loss.item() - 2 * x.double().pow(2).mean().item()) < 2e-4
        t = rnd(7, 300, dtype=dtype, seed=3)
        dx = o.sq_loss_fwd_bwd(x, loss, target=t)
        d = x.double() - t.double()
        assert abs(loss.item() - d.pow(2).mean().item()) < 1e-4 and nerr(dx, 2 * d / x.numel()) < tol(dtype)
        # ragged length (16-byte passes + scalar tail) and an unaligned slice (scalar path throughout)
        big = rnd(70001 + 1, dtype=dtype, seed=5)
        for xs in (big[:70001], big[1:]):
            dx = o.sq_loss_fwd_bwd(xs, loss)
            assert abs(loss.item() - xs.double().pow(2).mean().item()) < 1e-4
            assert nerr(dx * xs.numel(), 2 * xs.double()) < tol(dtype)
    a = rnd(1000)
    b = torch.empty(1000, dtype=BF16, device=DEV)
    assert torch.equal(o.cast(a, b), a.to(BF16))
    for n in (8, 1003, 70001):  # vector path + ragged tail, both directions, and an unaligned (scalar) slice
        a = rnd(n + 1)
        b = torch.empty(n + 1, dtype=BF16, device=DEV)
        assert torch.equal(o.cast(a[:n], b[:n]), a[:n].to(BF16))
        back = torch.empty(n, device=DEV)
        assert torch.equal(o.cast(b[:n], back), b[:n].float())
        assert torch.equal(o.cast(a[1:], b[1:]), a[1:].to(BF16))


def test_errors_are_loud():
    o = ops()
    with pytest.raises(RuntimeError):
        o.linear_fwd(torch.zeros(4, 4), torch.zeros(4, 4))  # CPU tensors
    with pytest.raises(RuntimeError):
        o.layernorm_fwd(rnd(4, 12), torch.ones(12, device=DEV), torch.zeros(12, device=DEV))  # D % 8 != 0


@pytest.mark.skipif(FORCED_SIMPLE, reason="the timed launches are those of the MFMA GEMM kernels")
def test_launch_timing_hook():
    """ovqa_launch_timing_begin/_end: per-launch kernel durations of the bf16 GEMM kernels (bench.py's roofline figure
    is built on them).  Counts only MFMA GEMM launches, in order, also from another thread; durations are sane."""
    import ctypes as C
    import threading
    from openvivqa_amd import _lib
    o = ops()
    lib = _lib.load()
    x, w, b = rnd(6400, 512, dtype=BF16), rnd(512, 512, dtype=BF16, scale=0.05), rnd(512)
    o.linear_fwd(x, w, b)  # warm
    torch.cuda.synchronize()
    assert lib.ovqa_launch_timing_begin(8) == 0
    assert lib.ovqa_launch_timing_begin(8) != 0          # already armed
    o.linear_fwd(x, w, b)
    o.linear_fwd(x.float(), w.float(), b)                # fp32: VALU kernel, not recorded
    assert lib.ovqa_launch_timing_count() == 1
    t = threading.Thread(target=lambda: o.linear_bwd_data(x, w))   # autograd runs backward on its own thread
    t.start()
    t.join()
    assert lib.ovqa_launch_timing_count() == 2
    us = (C.c_float * 8)()
    assert lib.ovqa_launch_timing_end(us, 1) < 0          # output too small; disarms
    assert lib.ovqa_launch_timing_begin(2) == 0
    for _ in range(3):
        o.linear_fwd(x, w, b)                             # the third launch is beyond the capacity: not timed
    n = lib.ovqa_launch_timing_end(us, 8)
    assert n == 2
    assert all(2.0 < us[i] < 500.0 for i in range(n)), list(us)[:n]   # 3.4 GFLOP: ~10 us on an MI355X
    assert lib.ovqa_launch_timing_end(us, 8) < 0          # not armed


QKV_SHAPES = [
    # B, n, H, d_model, masked   (d = 64: the fused kernel; anything else: the library's two-kernel route)
    (64, 100, 8, 512, True),    # MCAN vision SA (BASELINE configs[1]): 128-row panels, 2 samples / workgroup
    (64, 20, 8, 512, True),     # MCAN text SA: 32-row panels, 4 samples / workgroup
    (7, 49, 8, 512, True),      # 64-row panels, ragged last workgroup (7 = 4 + 3 samples)
    (3, 128, 4, 256, False),    # full panel, no mask, odd batch
    (5, 1, 8, 512, False),      # a single position
    (2, 33, 12, 768, True),     # BERT-base geometry (M4C MMT): d_model = 768, 12 heads
    (2, 150, 8, 512, True),     # n > 128: separate kernels
    (2, 20, 4, 384, False),     # d = 96: separate kernels
]


@pytest.mark.parametrize("B,n,H,Dm,masked", QKV_SHAPES)
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_attention_qkv_fwd(B, n, H, Dm, masked, dtype):
    """Fused projection + attention (ovqa_attention_qkv_fwd) against fp64 math AND against the separate
    ovqa_linear_fwd + ovqa_attention_fwd route on the same inputs; the stored projections must equal the
    separate GEMM's output (backward reads them)."""
    o = ops()
    d = (Dm // H) if Dm != 384 else 96
    x = rnd(B, n, Dm, dtype=dtype, seed=1)
    w = rnd(3 * H * d, Dm, dtype=dtype, scale=Dm ** -0.5, seed=2)
    b = rnd(3 * H * d, scale=0.1, seed=3)
    mask = None
    if masked:
        mask = torch.zeros(B, 1, 1, n, device=DEV)
        for i in range(B):
            mask[i, ..., n - (i % max(1, n // 2)):] = -1e5 if i % 3 else float("-inf")
        mask[0] = 0
        if n > 4 and dtype == BF16:  # (fp32: score + (-1e5) rounds to 2^-7, which the fp64 reference does not do)
            mask[B - 1, ..., :] = -1e5  # a fully padded sample: uniform attention (models/utils.py:44-73 semantics)
    qkv, out, lse = o.attention_qkv_fwd(x, w, b, mask, H)
    from openvivqa_amd import _lib
    disp = _lib.last_dispatch()
    if not (FORCED_SIMPLE or NO_FUSED_QKV):
        assert (disp == "mfma-fused") == (dtype == BF16 and d == 64 and n <= 128), (disp, d, n)
    qkv_ref = (x.double() @ w.double().t() + b.double())
    assert nerr(qkv, qkv_ref) < tol(dtype)
    hd = H * d
    q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
    ref, _, lse_ref = att_ref(q, k, v, mask, H)   # attention of the STORED projections
    ok = torch.isfinite(lse_ref)
    assert nerr(out, ref) < tol(dtype)
    assert nerr(torch.where(ok, lse, 0), torch.where(ok, lse_ref.to(lse.dtype), 0)) < tol(dtype)
    # the two-kernel route on the same inputs
    qkv2 = o.linear_fwd(x, w, b)
    out2, lse2, _ = o.attention_fwd(qkv2[..., :hd], qkv2[..., hd:2 * hd], qkv2[..., 2 * hd:], mask, H)
    assert nerr(qkv, qkv2) < (1e-6 if dtype == F32 else 8e-3)  # same fp32 sums, at most a bf16 rounding flip
    assert nerr(out, out2) < tol(dtype)


def test_empty_and_limit_shapes():
    """Edge cases: empty batches go through every entry point (no launch, right shapes); the MFMA attention's
    limits (n_k = 256 resident keys, then the LDS-resident VALU kernel takes over at 257) and LayerNorm's widest
    row (D = 2048) agree with the reference math."""
    o = ops()
    for dtype in (F32, BF16):
        x0 = torch.empty(0, 512, dtype=dtype, device=DEV)
        w = rnd(256, 512, dtype=dtype)
        b = rnd(256)
        assert o.linear_fwd(x0, w, b).shape == (0, 256)
        assert o.linear_bwd_data(torch.empty(0, 256, dtype=dtype, device=DEV), w).shape == (0, 512)
        dw, db = torch.full((256, 512), 7.0, device=DEV), torch.full((256,), 7.0, device=DEV)
        o.linear_bwd_weight(torch.empty(0, 256, dtype=dtype, device=DEV), x0, dw, db)
        assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0  # an empty sum overwrites with zeros
        y, mean, rstd = o.layernorm_fwd(x0, torch.ones(512, device=DEV), torch.zeros(512, device=DEV))
        assert y.shape == (0, 512)
        q0 = torch.empty(0, 5, 128, dtype=dtype, device=DEV)
        out, lse, _ = o.attention_fwd(q0, q0, q0, None, 2)
        assert out.shape == (0, 5, 128)
    # n_k at and just above the MFMA kernel's limit, padded keys included
    for nk in (256, 257):
        q = rnd(2, 40, 8 * 64, dtype=BF16, seed=1)
        k = rnd(2, nk, 8 * 64, dtype=BF16, seed=2)
        v = rnd(2, nk, 8 * 64, dtype=BF16, seed=3)
        mask = torch.zeros(2, 1, 1, nk, device=DEV)
        mask[1, ..., nk - 9:] = -1e5
        out, _, _ = o.attention_fwd(q, k, v, mask, 8)
        ref, _, _ = att_ref(q, k, v, mask, 8)
        assert nerr(out, ref) < 1e-2, nk
    # widest LayerNorm row
    x = rnd(33, 2048, dtype=BF16, seed=4)
    g, bb = rnd(2048, seed=5), rnd(2048, seed=6)
    y, _, _ = o.layernorm_fwd(x, g, bb)
    assert nerr(y, ln_ref(x, g, bb)[0]) < 1e-2
    with pytest.raises(RuntimeError):
        o.layernorm_fwd(rnd(4, 2056, dtype=BF16), torch.ones(2056, device=DEV), torch.zeros(2056, device=DEV))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,H,nq,nk,d", [(2, 4, 9, 11, 16), (2, 8, 182, 182, 96), (2, 8, 20, 20, 64)])
def test_attention_probability_dropout_and_lse_gradient(dtype, B, H, nq, nk, d):
    """Dropout on the attention probabilities (transformers' BertSelfAttention inside M4C's MMT) and the gradient
    w.r.t. the returned log-sum-exp (d_lse), against fp64 autograd with the kernel's own keep mask injected."""
    o = ops()
    q, k, v = rnd(B, nq, H * d, dtype=dtype, seed=1), rnd(B, nk, H * d, dtype=dtype, seed=2), rnd(B, nk, H * d, dtype=dtype, seed=3)
    mask = torch.zeros(B, 1, 1, nk, device=DEV)
    mask[0, ..., nk - 3:] = -1e5
    drop = o.DropSpec(p=0.2, seed=77, site=5, step=torch.tensor([9], dtype=torch.int32, device=DEV))
    keep = o.dropout_keep_mask(drop, B * H * nq * nk, DEV).view(B, H, nq, nk).double().cpu() / 0.8

    def ref(qd, kd, vd):
        qh = qd.view(B, nq, H, d).transpose(1, 2)
        kh = kd.view(B, nk, H, d).transpose(1, 2)
        vh = vd.view(B, nk, H, d).transpose(1, 2)
        s = qh @ kh.transpose(-1, -2) / math.sqrt(d) + mask.double().cpu()
        p = torch.softmax(s, -1) * keep
        return (p @ vh).transpose(1, 2).reshape(B, nq, H * d), p, torch.logsumexp(s, -1)
    out, lse, att = o.attention_fwd(q, k, v, mask, H, need_att=True, att_drop=drop)
    qd, kd, vd = (t.double().cpu().detach().clone().requires_grad_(True) for t in (q, k, v))
    ro, rp, rl = ref(qd, kd, vd)
    t = tol(dtype)
    assert nerr(out, ro) < t and nerr(att, rp) < t and nerr(lse, rl) < 1e-2
    d_o = rnd(B, nq, H * d, dtype=dtype, seed=5)
    d_lse = rnd(B, H, nq, seed=6) * 0.3
    ((ro * d_o.double().cpu()).sum() + (rl * d_lse.double().cpu()).sum()).backward()
    dq, dk, dv = o.attention_bwd(d_o, q, k, v, out, lse, mask, H, d_lse=d_lse, att_drop=drop)
    t = t * (3 if dtype == BF16 else 1)
    assert nerr(dq, qd.grad) < t and nerr(dk, kd.grad) < t and nerr(dv, vd.grad) < t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decode_embed_matches_torch_ops(dtype):
    """ovqa_decode_embed against the stateful branch of Decoder.forward written with torch ops (decoders.py:46-66):
    position counter, embedding sum (bit-exact in fp32, its rounding in bf16) and the new mask column."""
    g = torch.Generator().manual_seed(5)
    R, V, D, P = 37, 91, 512, 21
    emb = torch.randn(V, D, generator=g).to(DEV)
    pos = torch.randn(P, D, generator=g).to(DEV)
    tok = torch.randint(0, V, (R,), generator=g).to(DEV)
    tok[3] = 0
    tok[11] = 0
    seq = torch.randint(0, P - 1, (R, 1), generator=g).to(DEV)
    mask = torch.full((R, 32), 7.0, device=DEV)
    seq0 = seq.clone()
    x32, x = ops().decode_embed(tok, emb, pos, seq.view(-1), 0, -1e5, mask, 5, dtype)
    assert torch.equal(seq, seq0 + 1)
    ref = emb[tok] + pos[(seq0 + 1).view(-1)]
    assert torch.equal(x32, ref)
    if dtype == torch.bfloat16:
        assert torch.equal(x, ref.to(dtype))
    else:
        assert x is None
    want = torch.full((R, 32), 7.0, device=DEV)
    want[:, 5] = (tok == 0).float() * -1e5
    assert torch.equal(mask, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [203, 5000])
@pytest.mark.parametrize("beam,cur", [(3, 3), (3, 1), (1, 1), (8, 8), (5, 5)])
def test_beam_step_kernels_match_reference_step(dtype, beam, cur, V):
    """ovqa_beam_candidates + ovqa_beam_commit against ONE step of models/modules/beam_search.py:41-83 written with
    torch ops (log-softmax, candidate scores with finished sequences, full descending sort, gathers)."""
    # (V = 203: unaligned rows, element loads; V = 5000 in bf16: longer than the row a wave keeps in registers)
    g = torch.Generator().manual_seed(beam * 10 + cur)
    b_s, T, t, eos = 6, 9, (0 if cur == 1 else 4), 2
    logits = (torch.randn(b_s * cur, V, generator=g) * 3).to(DEV).to(dtype)
    seq_logprob = (-torch.rand(b_s, cur, generator=g) * 5).to(DEV)
    seq_mask = (torch.rand(b_s, cur, generator=g) > 0.25).float().to(DEV)
    prev = torch.randint(0, V, (b_s * cur,), generator=g).to(DEV)
    prev[1::4] = eos
    out_in = torch.randint(0, V, (b_s, cur, T), generator=g).to(DEV)
    lp_in = -torch.rand(b_s, cur, T, generator=g).to(DEV)
    if t == 0:
        seq_mask.fill_(1.0)
        seq_logprob.zero_()
    # ---- the reference step
    word_logprob = torch.log_softmax(logits.float(), -1).view(b_s, cur, V)
    cand = seq_logprob.unsqueeze(-1) + word_logprob
    m_ref = seq_mask.clone()
    if t > 0:
        m_ref = m_ref * (prev.view(b_s, cur) != eos).float()
        word_logprob = word_logprob * m_ref.unsqueeze(-1)
        old = seq_logprob.unsqueeze(-1).expand_as(cand).contiguous()
        old[:, :, 1:] = -999
        cand = m_ref.unsqueeze(-1) * cand + old * (1 - m_ref.unsqueeze(-1))
    val, idx = torch.sort(cand.view(b_s, -1), dim=-1, descending=True, stable=True)
    val, idx = val[:, :beam], idx[:, :beam]
    sel_ref = idx // V
    words_ref = idx - sel_ref * V
    this_ref = torch.gather(word_logprob.reshape(b_s, -1), 1, idx)
    # ---- the kernels
    k = min(beam, V)
    sm = seq_mask.clone().view(-1)
    vals, i1, wl = ops().beam_candidates(logits, seq_logprob.view(-1).contiguous(), sm, prev if t > 0 else None, eos, k)
    assert torch.equal(sm.view(b_s, cur), m_ref)
    out_out = torch.zeros(b_s, beam, T, dtype=torch.long, device=DEV)
    lp_out = torch.zeros(b_s, beam, T, device=DEV)
    sl_out, sm_out = torch.empty(b_s * beam, device=DEV), torch.empty(b_s * beam, device=DEV)
    sel = torch.empty(b_s, beam, dtype=torch.int32, device=DEV)
    words = torch.empty(b_s * beam, 1, dtype=torch.long, device=DEV)
    ops().beam_commit(vals, i1, wl, sm, (out_in, lp_in), (out_out, lp_out), sl_out, sm_out, sel, words, b_s, cur, k, beam, t)
    assert torch.allclose(sl_out.view(b_s, beam), val, rtol=0, atol=2e-5)
    # (equal scores: any order of the tied candidates is the reference's -- compare where the scores are distinct)
    distinct = torch.ones_like(val, dtype=torch.bool)
    distinct[:, 1:] &= (val[:, 1:] - val[:, :-1]).abs() > 1e-4
    distinct[:, :-1] &= (val[:, 1:] - val[:, :-1]).abs() > 1e-4
    assert distinct.float().mean() > 0.6
    assert torch.equal(sel.long()[distinct], sel_ref[distinct])
    assert torch.equal(words.view(b_s, beam)[distinct], words_ref[distinct])
    assert torch.allclose(lp_out[:, :, t][distinct], this_ref[distinct], rtol=0, atol=2e-5)
    assert torch.equal(out_out[:, :, t], words.view(b_s, beam))
    assert torch.equal(sm_out.view(b_s, beam), torch.gather(m_ref, 1, sel.long()))
    if t > 0:
        sel3 = sel.long().unsqueeze(-1).expand(b_s, beam, t)
        assert torch.equal(out_out[:, :, :t], torch.gather(out_in[:, :, :t], 1, sel3))
        assert torch.equal(lp_out[:, :, :t], torch.gather(lp_in[:, :, :t], 1, sel3))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [203, 4000])
def test_beam_candidates_with_masked_vocabulary_entries(dtype, V):
    """-inf logits (masked words): F.log_softmax gives them -inf and leaves the rest finite; the candidate kernel's online
    log-sum-exp must do the same when a lane's FIRST value is -inf (exp(-inf - -inf) = NaN poisoned the row)."""
    g = torch.Generator().manual_seed(V)
    b_s, beam = 5, 3
    logits = (torch.randn(b_s, V, generator=g) * 3)
    logits[:, :70] = float("-inf")          # every lane's first word (vector and scalar loads alike)
    logits[2, 100:150] = float("-inf")
    logits = logits.to(DEV).to(dtype)
    ref = torch.log_softmax(logits.float(), -1)
    val_ref, idx_ref = torch.topk(ref, beam, dim=-1)
    sm = torch.ones(b_s, device=DEV)
    vals, i1, wl = ops().beam_candidates(logits, torch.zeros(b_s, device=DEV), sm, None, 2, beam)
    assert torch.isfinite(vals).all()
    assert torch.allclose(vals.view(b_s, beam), val_ref, rtol=0, atol=2e-5)
    distinct = (val_ref[:, 1:] - val_ref[:, :-1]).abs().min(dim=1).values > 1e-4
    assert distinct.any() and torch.equal(i1.view(b_s, beam)[distinct], idx_ref[distinct])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M", [64, 192, 1280])
def test_linear_fwd_split3_writes_three_strided_outputs(dtype, M):
    """ovqa_linear_fwd_split3: fc_q / fc_k / fc_v of a decoding step in one launch, k and v into slots of in-place caches
    (row stride = capacity * F), against three separate products."""
    o = ops()
    F, K, cap, n = 512, 512, 21, 7
    x = rnd(M, K, dtype=dtype)
    w = rnd(3 * F, K, dtype=dtype, scale=K ** -0.5, seed=1)
    b = rnd(3 * F, seed=2)
    q = torch.empty(M, F, dtype=dtype, device=DEV)
    kc = torch.full((M, cap, F), 3.0, dtype=dtype, device=DEV)
    vc = torch.full((M, cap, F), 5.0, dtype=dtype, device=DEV)
    o.linear_fwd_split3(x, w, b, (q, kc[:, n], vc[:, n]))
    ref = x.double() @ w.double().t() + b.double()
    assert nerr(q, ref[:, :F]) < tol(dtype)
    assert nerr(kc[:, n], ref[:, F:2 * F]) < tol(dtype)
    assert nerr(vc[:, n], ref[:, 2 * F:]) < tol(dtype)
    kc[:, n], vc[:, n] = 3.0, 5.0  # nothing else was touched
    assert (kc == 3.0).all() and (vc == 5.0).all()
    # the same values as three separate launches of the same kernels
    sep = [o.linear_fwd(x, w[i * F:(i + 1) * F].contiguous(), b[i * F:(i + 1) * F].contiguous()) for i in range(3)]
    assert torch.equal(q, sep[0])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,nq,nk", [(64, 100, 20), (3, 128, 64), (2, 37, 100), (5, 20, 1), (4, 100, 33), (2, 150, 20),
                                     (2, 100, 200)])
def test_attention_q_fwd_equals_projection_plus_attention(dtype, B, nq, nk):
    """ovqa_attention_q_fwd (query projection inside the attention kernel; K / V already projected, as strided views of
    a packed buffer) against ovqa_linear_fwd + ovqa_attention_fwd: q bit-equal, o / lse within the kernels' tolerance,
    and the rounding residual o_lo written."""
    _q_fwd_case(dtype, B, nq, nk, 8, 512)


@pytest.mark.parametrize("B,nq,nk,H,Dm", [(3, 37, 20, 3, 768), (2, 100, 64, 5, 512), (4, 20, 100, 3, 512), (2, 65, 33, 6, 768)])
def test_attention_q_fwd_odd_heads_and_wide_model(B, nq, nk, H, Dm):
    """As above with an odd head count (one head per workgroup: attn_q_fwd_mfma_kernel<., 3, 1>) and d_model = 768 (the
    entry point needs d_model % 64 == 0)."""
    _q_fwd_case(BF16, B, nq, nk, H, Dm)


def _q_fwd_case(dtype, B, nq, nk, H, Dm):
    o_ = ops()
    d = 64
    x = rnd(B, nq, Dm, dtype=dtype)
    w = rnd(H * d, Dm, dtype=dtype, scale=Dm ** -0.5, seed=1)
    b = rnd(H * d, seed=2)
    kv = rnd(B, nk, 3 * 2 * H * d, dtype=dtype, seed=3)  # packed K | V of three layers: slot 1 is ours
    k, v = kv[..., 2 * H * d:3 * H * d], kv[..., 3 * H * d:4 * H * d]
    mask = torch.zeros(B, 1, 1, nk, device=DEV)
    if nk > 3:
        mask[0, :, :, nk - 3:] = -1e5
    lo, lo2 = [], []
    q, o, lse = o_.attention_q_fwd(x, w, b, k, v, mask, H, lo_out=lo)
    if dtype == BF16 and not FORCED_SIMPLE and not NO_FUSED_QKV and nq <= 128 and nk <= 128:
        from openvivqa_amd import _lib
        assert _lib.last_dispatch() == "mfma-fused"  # (longer sequences: the two separate kernels inside the library)
    q2 = o_.linear_fwd(x, w, b)
    o2, lse2, _ = o_.attention_fwd(q2, k, v, mask, H, lo_out=lo2)
    assert torch.equal(q, q2) if dtype == BF16 else nerr(q, q2) < 1e-5
    assert nerr(o, o2) < tol(dtype) and nerr(lse, lse2) < 1e-3
    if dtype == BF16:
        assert len(lo) == 1 and nerr(o.float() + lo[0].float(), o2.float() + lo2[0].float()) < 2e-3
    # fp64 math: the projection (one bf16 rounding + fp32 accumulation), the attention of the stored q (bf16 probabilities
    # in P V: 2^-9 per term, bounded by P |V|), o + o_lo (the fp32 output: the probability term only)
    qr = x.double() @ w.double().t() + b.double()
    assert rel_max(q, qr) < (2 ** -8 if dtype == BF16 else 1e-5)
    ro, rp, _ = att_ref(q, k, v, mask, H)
    vh = v.double().view(B, nk, H, d).transpose(1, 2)
    t = (rp @ vh.abs()).transpose(1, 2).reshape(B, nq, H * d).abs().max().item()
    bar = 2 ** -8 * (ro.abs().max().item() + t) / ro.abs().max().item() if dtype == BF16 else 1e-4
    assert rel_max(o, ro) < bar
    if dtype == BF16:
        assert rel_max(o.double() + lo[0].double(), ro) < bar


@pytest.mark.parametrize("B,nq,nk", [(64, 100, 20), (3, 128, 32), (2, 65, 1), (5, 97, 13), (64, 20, 20), (3, 32, 32), (2, 1, 1),
                                     (4, 17, 29), (2, 50, 20), (64, 100, 100), (3, 128, 128), (2, 97, 100), (2, 100, 97)])
def test_attention_bwd_do_equals_projection_plus_backward(B, nq, nk):
    """ovqa_attention_bwd_do (the fc_o dX product inside the guided-attention backward kernel, from the transposed weight
    copy) against ovqa_linear_bwd_data_wt + ovqa_attention_bwd: same dq, dk, dv."""
    _bwd_do_case(B, nq, nk, 8, 512)


@pytest.mark.parametrize("B,nq,nk,H,Dm", [(3, 100, 20, 3, 768), (2, 128, 100, 3, 512), (4, 20, 20, 6, 768),
                                          (2, 70, 32, 5, 512)])
def test_attention_bwd_do_odd_heads_and_wide_model(B, nq, nk, H, Dm):
    """As above with odd head counts (guided and role-split forms; the single-tile form needs an even H) and d_model = 768
    (the entry point needs d_model % 64 == 0)."""
    _bwd_do_case(B, nq, nk, H, Dm)


def _bwd_do_case(B, nq, nk, H, Dm):
    o_ = ops()
    d = 64
    q = rnd(B, nq, H * d, dtype=BF16)
    kv = rnd(B, nk, 4 * H * d, dtype=BF16, seed=1)  # packed K | V of two layers: slot 1 is ours
    k, v = kv[..., 2 * H * d:3 * H * d], kv[..., 3 * H * d:]
    mask = torch.zeros(B, 1, 1, nk, device=DEV)
    if nk > 3:
        mask[0, :, :, nk - 3:] = -1e5
    lo = []
    o, lse, _ = o_.attention_fwd(q, k, v, mask, H, lo_out=lo)
    dy = rnd(B, nq, Dm, dtype=BF16, seed=2)
    group = rnd(H * d, 4 * Dm, dtype=BF16, scale=Dm ** -0.5, seed=3)  # transposed copies of an adjacency group [in, 4 x out]
    wt = group[:, 3 * Dm:]                                             # fc_o's slice: rows = input features, strided
    dkv1, dkv0 = torch.zeros_like(kv), torch.zeros_like(kv)
    fused_on = not FORCED_SIMPLE and not NO_FUSED_QKV
    # (round 5: 97-128 queries x 97-128 keys -- the image self-attention -- run the role-split backward with the projection
    # inside)
    covered = ((nq > 64 or nq <= 32) and nk <= 32) or (nq > 96 and nk > 96)
    assert o_.attention_bwd_do_ok(dy, wt, q, k, mask, H) == (fused_on and covered)
    if not covered or not fused_on:
        return
    dq1, _, _ = o_.attention_bwd_do(dy, wt, q, k, v, o, lse, mask, H, o_lo=lo[0], dk=dkv1[..., 2 * H * d:3 * H * d],
                                    dv=dkv1[..., 3 * H * d:])
    if not FORCED_SIMPLE and not NO_FUSED_QKV:
        from openvivqa_amd import _lib
        assert _lib.last_dispatch() == "mfma-fused"
    d_o = o_.linear_bwd_data_wt(dy.reshape(B * nq, Dm), wt).view(B, nq, H * d)
    dq0, _, _ = o_.attention_bwd(d_o, q, k, v, o, lse, mask, H, o_lo=lo[0], dk=dkv0[..., 2 * H * d:3 * H * d],
                                 dv=dkv0[..., 3 * H * d:])
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()
    assert rel(dq1, dq0) < 2e-3 and rel(dkv1, dkv0) < 2e-3, (rel(dq1, dq0), rel(dkv1, dkv0))
    # fp64 autograd of the attention with dO = dy wt^T in fp64: relative L2 within two bf16 roundings of the inputs of the
    # last products (dO, and dS / P~ before the MFMA) -- 2 x 2^-8
    qd, kd, vd = (t.double().detach().clone().requires_grad_(True) for t in (q, k, v))
    att_ref(qd, kd, vd, mask, H)[0].backward(dy.double() @ wt.double().t())
    for got, ref in ((dq1, qd.grad), (dkv1[..., 2 * H * d:3 * H * d], kd.grad), (dkv1[..., 3 * H * d:], vd.grad)):
        # (one key: softmax = 1 whatever the scores, dq = dk = 0 exactly; the kernel's cancellation residue is measured
        # against the scale of dv, the gradient of the same magnitude of terms)
        scale = ref if ref.double().norm() > 0 else vd.grad
        e = ((got.double() - ref).norm() / scale.double().norm()).item()
        assert e < 2 * 2 ** -8, e


def test_model_end_entry_points_accept_empty_batches():
    """Empty inputs (a batch of zero samples, as a ragged last batch can produce) are no-ops of the round-5 entry points, like
    those of the older ones; a scatter without tokens still leaves a ZERO table gradient (or the old one when accumulating)."""
    o = ops()
    H, I, T = 512, 512, 5
    w_ih, w_hh = rnd(4 * H, I, dtype=BF16, scale=I ** -0.5), rnd(4 * H, H, dtype=BF16, scale=H ** -0.5, seed=1)
    b0 = torch.zeros(4 * H, device=DEV)
    y, hseq, saved, scratch = o.lstm_fwd(torch.empty(0, I, dtype=BF16, device=DEV), w_ih, w_hh, b0, b0, 0, T)
    assert y.shape == (0, T, H)
    dg, _ = o.lstm_bwd(torch.empty(0, T, H, device=DEV), w_hh, w_hh.t().contiguous(), saved, 0, T, I)
    assert dg.shape == (0, 4 * H)
    table = rnd(11, 24)
    tok = torch.empty(0, T, dtype=torch.int64, device=DEV)
    rows, mask = o.embed_gather(tok, table, time_major=True, want_mask=True, padding_idx=0)
    assert rows.shape == (0, 24) and mask.shape == (0, 1, 1, T)
    dtable = torch.full((11, 24), 7.0, device=DEV)
    o.embed_scatter(tok, rows, dtable, time_major=True, padding_idx=0, accumulate=True)
    assert torch.equal(dtable, torch.full_like(dtable, 7.0))
    o.embed_scatter(tok, rows, dtable, time_major=True, padding_idx=0)
    assert torch.count_nonzero(dtable).item() == 0
    feat = torch.empty(0, 20, 64, dtype=BF16, device=DEV)
    att, pooled = o.pool_fwd(feat, torch.empty(0, 64, dtype=BF16, device=DEV), torch.ones(64, device=DEV), None)
    assert att.shape == (0, 20) and pooled.shape == (0, 64)
    dh, dfeat, part, bpart = o.pool_bwd(feat, torch.empty(0, 64, dtype=BF16, device=DEV), torch.ones(64, device=DEV), att, pooled)
    assert dh.shape == (0, 64) and part.shape == (0, 128)
    assert o.log_softmax_fwd(torch.empty(0, 360, dtype=BF16, device=DEV), 353).shape == (0, 353)
    assert o.dropout_apply(torch.empty(0, 8, device=DEV), o.DropSpec(0.1, 1, 2)).numel() == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,n,tail,d", [(4, 182, 12, 96), (3, 100, 100, 64), (2, 64, 1, 128), (2, 37, 5, 64), (2, 192, 0, 96)])
def test_attention_fwd_prefix_lm_equals_dense_mask(B, n, tail, d):
    """ovqa_attention_fwd_prefix_lm (key-mask row + a causal corner of the last `tail` positions, computed in the kernel) against
    ovqa_attention_fwd on the dense (B, 1, n, n) mask that M4C's MMT.forward builds (mmf_m4c.py:310-340): the same output bits
    (masked probabilities are exactly zero either way)."""
    from openvivqa_amd.utils import generate_sequential_mask
    o_ = ops()
    H = 8
    q, k, v = (rnd(B, n, H * d, dtype=BF16, seed=s) for s in (0, 1, 2))
    row = torch.zeros(B, 1, 1, n, device=DEV)
    row[0, :, :, 3:7] = -10000.0  # (padded keys in front of the decoding positions)
    ext = row.repeat(1, 1, n, 1)
    if tail:
        ext[:, :, -tail:, -tail:] += generate_sequential_mask(tail, device=DEV)
    assert o_.attention_fwd_prefix_lm_ok(q, H) == (not FORCED_SIMPLE)
    if FORCED_SIMPLE:
        return
    want, _, _ = o_.attention_fwd(q, k, v, ext, H, save_lse=False)
    got = o_.attention_fwd_prefix_lm(q, k, v, row, tail, H)
    assert torch.equal(got, want)


def test_stream_helpers_of_the_c_abi():
    """ovqa_stream_create (priority / CU mask) hands back streams that torch can drive: a cast launched on a CU-masked
    stream (the first 64 compute units) and on a high-priority stream gives the values of the default stream."""
    o = ops()
    lo, hi = o.priority_range()
    assert hi <= lo  # (numerically lower = served first)
    x = rnd(4096, 64)
    want = x.to(BF16)
    for st in (o.make_stream(DEV, priority=hi), o.make_stream(DEV, cu_mask=range(64))):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            y = torch.empty(x.shape, dtype=BF16, device=DEV)
            o.cast(x, y)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        assert torch.equal(y, want)


# ---------------------------------------------------------------- LSTM recurrence (ovqa_lstm_fwd / ovqa_lstm_bwd)
def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-12)).item()


def _lstm_ref64(x_tb, w_ih, w_hh, b_ih, b_hh, dy, B, T, round_ops):
    """fp64 math of torch.nn.LSTM's recurrence on time-major rows; ``round_ops``: the recurrent operand h_{t-1} and the
    gradient w.r.t. the pre-activations are rounded to bf16 where the bf16 kernels store them (x and the weights are
    bf16 values already).  Returns y [B,T,H], dgates [T*B,4H] and the gradient w.r.t. x."""
    x = x_tb.double().cpu().requires_grad_(True)
    wi, wh = w_ih.double().cpu(), w_hh.double().cpu()
    H = wh.shape[1]
    xg = (x @ wi.t() + b_ih.double().cpu()).view(T, B, 4 * H)
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    ys, pre = [], []
    for t in range(T):
        hop = h + (h.float().bfloat16().double() - h).detach() if round_ops else h
        g = xg[t] + hop @ wh.t() + b_hh.double().cpu()
        g.retain_grad()
        pre.append(g)
        i, f, gg, o = g.chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        ys.append(h)
    y = torch.stack(ys, 1)
    (y * dy.double().cpu()).sum().backward()
    return y.detach(), torch.cat([p.grad for p in pre], 0), x.grad


@pytest.mark.parametrize("B,T,H,dtype,route", [
    (3, 5, 32, F32, "simple"), (5, 8, 24, F32, "simple"), (4, 6, 32, BF16, "simple"),
    (16, 3, 512, BF16, "mfma"), (64, 20, 512, BF16, "mfma"), (32, 7, 512, BF16, "mfma"), (128, 4, 512, BF16, "mfma"),
    # ragged batches are padded to whole sample groups of 16 by ops.lstm_fwd (the last batch of an epoch), batches larger
    # than the persistent kernels can keep co-resident run as chunks: both stay on the MFMA route
    (24, 4, 512, BF16, "mfma"), (5, 3, 512, BF16, "mfma"), (200, 3, 512, BF16, "mfma"), (64, 20, 512, F32, "simple")])
def test_lstm_fwd_bwd(B, T, H, dtype, route):
    from openvivqa_amd import _lib
    g = torch.Generator().manual_seed(1000 + B * 7 + T)
    s = H ** -0.5
    x = torch.randn(T * B, H, generator=g).to(DEV, dtype)
    w_ih = (torch.rand(4 * H, H, generator=g) * 2 - 1).mul(s).to(DEV, dtype)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1).mul(s).to(DEV, dtype)
    b_ih = (torch.rand(4 * H, generator=g) * 2 - 1).mul(s).to(DEV)
    b_hh = (torch.rand(4 * H, generator=g) * 2 - 1).mul(s).to(DEV)
    dy = torch.randn(B, T, H, generator=g).to(DEV)
    o = ops()
    y, hseq, saved, scratch = o.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, B, T)
    if FORCED_SIMPLE:
        route = "simple"
    assert _lib.last_dispatch() == route
    wt = w_hh.t().contiguous() if dtype == BF16 else None
    dgates, scratch_b = o.lstm_bwd(dy, w_hh, wt, saved, B, T, H)
    assert _lib.last_dispatch() == route
    torch.cuda.synchronize()
    if route == "mfma":  # no hand-off wait of the persistent launches gave up
        assert int(scratch.view(torch.int32)[1000]) == 0 and int(scratch_b.view(torch.int32)[1000]) == 0
        assert o.lstm_status(raise_on_error=False) == 0
    y64, dg64, _ = _lstm_ref64(x, w_ih, w_hh, b_ih, b_hh, dy, B, T, round_ops=dtype == BF16)
    tol = 1e-5 if dtype == F32 else 2e-3  # bf16: a 1-ulp flip of a rounded h_{t-1} moves later steps
    assert nerr(y, y64) < tol, nerr(y, y64)
    assert nerr(hseq[B:].float().view(T, B, H).transpose(0, 1), y64) < (1e-5 if dtype == F32 else 8e-3)
    assert float(hseq[:B].float().abs().max()) == 0.0
    assert rel_l2(dgates.float(), dg64) < (1e-5 if dtype == F32 else 6e-3), rel_l2(dgates.float(), dg64)


@pytest.mark.skipif(FORCED_SIMPLE, reason="the give-up path of the persistent kernels")
def test_lstm_handoff_timeout_reaches_python(monkeypatch):
    """A workgroup of the persistent launch that never runs (OVQA_LSTM_DEBUG_DROP_WG: it exits at once) makes its sample
    group's waits give up after `sweep_limit` sweeps: the eager call raises, the outputs of that group are NaN (so a loss
    would show it), the other sample groups are untouched, and the status word is clear again afterwards."""
    B, T, H = 32, 4, 512
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T * B, H, generator=g).to(DEV, BF16)
    w = [(torch.rand(4 * H, H, generator=g) * 2 - 1).mul(H ** -0.5).to(DEV, BF16) for _ in range(2)]
    b = [(torch.rand(4 * H, generator=g) * 2 - 1).mul(H ** -0.5).to(DEV) for _ in range(2)]
    o = ops()
    y_ok = o.lstm_fwd(x, w[0], w[1], b[0], b[1], B, T)[0]
    assert torch.isfinite(y_ok).all()
    monkeypatch.setenv("OVQA_LSTM_SWEEP_LIMIT", "2000")
    monkeypatch.setenv("OVQA_LSTM_DEBUG_DROP_WG", "1")  # workgroup 0: sample group 0 (two groups: blocks b % 8 < 4)
    with pytest.raises(RuntimeError, match="hand-off wait gave up"):
        o.lstm_fwd(x, w[0], w[1], b[0], b[1], B, T)
    assert o.lstm_status(raise_on_error=False) == 0  # read and cleared by the failing call
    monkeypatch.setenv("OVQA_LSTM_CHECK", "0")
    y_bad = o.lstm_fwd(x, w[0], w[1], b[0], b[1], B, T)[0]
    torch.cuda.synchronize()
    assert torch.isnan(y_bad[:16]).any() and not torch.isnan(y_bad[16:]).any()
    assert torch.equal(y_bad[16:], y_ok[16:])
    assert o.lstm_status(raise_on_error=False) == 2
    monkeypatch.delenv("OVQA_LSTM_DEBUG_DROP_WG")
    monkeypatch.delenv("OVQA_LSTM_SWEEP_LIMIT")
    monkeypatch.setenv("OVQA_LSTM_CHECK", "1")
    assert torch.equal(o.lstm_fwd(x, w[0], w[1], b[0], b[1], B, T)[0], y_ok)


@pytest.mark.skipif(FORCED_SIMPLE, reason="compares the persistent route with the per-step one")
def test_lstm_persistent_equals_per_step_kernels_and_is_deterministic_under_load():
    """The persistent launches against the one-launch-per-step kernels of the same library on the same bf16 operands
    (same arithmetic up to summation order), and run-to-run bitwise determinism under a busy chip (uneven load is where a
    stale or torn read of the in-launch hand-off would show)."""
    B, T, H = 64, 20, 512
    g = torch.Generator().manual_seed(77)
    s = H ** -0.5
    x = torch.randn(T * B, H, generator=g).to(DEV, BF16)
    w_ih = (torch.rand(4 * H, H, generator=g) * 2 - 1).mul(s).to(DEV, BF16)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1).mul(s).to(DEV, BF16)
    b = [(torch.rand(4 * H, generator=g) * 2 - 1).mul(s).to(DEV) for _ in range(2)]
    dy = torch.randn(B, T, H, generator=g).to(DEV)
    wt = w_hh.t().contiguous()

    om = ops()

    def run():
        y, hseq, saved, _ = om.lstm_fwd(x, w_ih, w_hh, b[0], b[1], B, T)
        dg, _ = om.lstm_bwd(dy, w_hh, wt, saved, B, T, H)
        return y, hseq, dg
    # busy neighbours: a chip-filling GEMM stream beside the recurrence (uneven load is where a broken hand-off shows)
    a = torch.randn(4096, 4096, device=DEV, dtype=BF16)
    side = torch.cuda.Stream()
    ref = run()
    for it in range(6):
        with torch.cuda.stream(side):
            for _ in range(4):
                a @ a
        got = run()
        for r, o in zip(ref, got):
            assert torch.equal(r, o), f"iteration {it}: the persistent LSTM is not deterministic"
    torch.cuda.synchronize()
    try:
        import subprocess, sys  # the switch is read once per process: ask a fresh one for the per-step result
        code = ("import torch, json, sys; sys.path.insert(0, %r); from openvivqa_amd import ops\n"
                "d = torch.load(sys.argv[1]); y, hs, sv, _ = ops.lstm_fwd(d['x'], d['w_ih'], d['w_hh'], d['b0'], d['b1'], 64, 20)\n"
                "dg, _ = ops.lstm_bwd(d['dy'], d['w_hh'], None, sv, 64, 20, 512)\n"
                "torch.save({'y': y, 'dg': dg}, sys.argv[2])" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            torch.save({"x": x, "w_ih": w_ih, "w_hh": w_hh, "b0": b[0], "b1": b[1], "dy": dy}, tmp + "/in.pt")
            subprocess.run([sys.executable, "-c", code, tmp + "/in.pt", tmp + "/out.pt"], check=True,
                           env=dict(os.environ, OVQA_FORCE_SIMPLE="1"))
            out = torch.load(tmp + "/out.pt")
    finally:
        pass
    assert nerr(ref[0], out["y"]) < 2e-3
    assert rel_l2(ref[2].float(), out["dg"].float()) < 6e-3


# ---------------------------------------------------------------- the two ends of the model (csrc/model_ends.hip)
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,T,V,W,time_major", [(3, 6, 11, 16, True), (64, 20, 4000, 304, True), (5, 7, 50, 512, False),
                                                 (128, 40, 300, 64, True), (70, 30, 97, 32, False),
                                                 (64, 20, 4000, 512, False), (9, 5, 30, 24, True)])
def test_embed_gather_scatter(dtype, B, T, V, W, time_major):
    """(the last two cases: <bos> at the head of every sample -- up to 64 hits for one table row, read four rows at a time;
    a view of the row gradients that is not 16-byte aligned takes the scalar row reads: the same sums bit for bit)"""
    o = ops()
    g = torch.Generator().manual_seed(B * 100 + T)
    table = torch.randn(V, W, generator=g).to(DEV, dtype)
    tokens = torch.randint(0, V, (B, T), generator=g)
    if W in (512, 24):
        tokens[:, 0] = 1
    tokens[0, -2:] = 0  # padding tokens (index 0)
    tokens[-1] = tokens[0]  # repeated tokens: several rows add into one table row
    tok = tokens.to(DEV)
    rows, mask = o.embed_gather(tok, table, time_major, want_mask=True, padding_idx=0)
    order = tokens.t().reshape(-1) if time_major else tokens.reshape(-1)
    assert torch.equal(rows.cpu(), table.cpu()[order])
    assert torch.equal(mask.cpu(), ((tokens == 0).float() * -10e4).reshape(B, 1, 1, T))
    drows = torch.randn(B * T, W, generator=g).to(DEV, dtype)
    dt = torch.full((V, W), 7.0, device=DEV)  # every row is overwritten: no memset needed
    o.embed_scatter(tok, drows, dt, time_major, padding_idx=0)
    ref = torch.zeros(V, W, dtype=torch.float64)
    keep = order != 0
    ref.index_add_(0, order[keep], drows.double().cpu()[keep])
    assert nerr(dt, ref) < (1e-5 if dtype == F32 else 1e-5)  # fp32 accumulation of the (bf16) rows: exact up to order
    dt2 = dt.clone()
    o.embed_scatter(tok, drows, dt2, time_major, padding_idx=0, accumulate=True)
    assert nerr(dt2, 2 * ref) < 1e-5
    a = torch.empty_like(dt)
    o.embed_scatter(tok, drows, a, time_major, padding_idx=0)
    assert torch.equal(a, dt), "the scatter is not deterministic"
    wide = torch.zeros(B * T, W + 3, device=DEV, dtype=dtype)
    wide[:, 1:W + 1] = drows
    o.embed_scatter(tok, wide[:, 1:W + 1], a.fill_(3.0), time_major, padding_idx=0)
    assert torch.equal(a, dt)


@pytest.mark.parametrize("B,T,D", [(64, 20, 512), (3, 1, 32), (5, 77, 100), (2, 130, 64)])
def test_decoder_inputs_equal_the_reference_mask_and_position_arithmetic(B, T, D):
    """ovqa_decoder_inputs against the torch composition of decoders.py:50-60,66 (generate_padding_mask,
    generate_sequential_mask, generate_self_attention_masks, the masked position ids, pos_emb lookup and add): bit for bit,
    including the sign of the unmasked zeros."""
    from openvivqa_amd.utils import (generate_padding_mask, generate_self_attention_masks, generate_sequential_mask,
                                     sinusoid_encoding_table)
    o = ops()
    g = torch.Generator().manual_seed(B + T)
    tokens = torch.randint(1, 50, (B, T), generator=g)
    for b in range(B):
        n = int(torch.randint(1, T + 1, (1,), generator=g))
        tokens[b, n:] = 0
    tokens[0, 0] = 0  # a padding token in front of words: its row of the mask still opens the causal prefix
    tokens = tokens.to(DEV)
    emb = torch.randn(B, T, D, generator=g).to(DEV)
    pos = sinusoid_encoding_table(T + 3, D, padding_idx=0).to(DEV)
    out, mask = o.decoder_inputs(tokens, emb, pos, 0)
    pad = generate_padding_mask(tokens, 0)
    ref_mask = generate_self_attention_masks(pad, generate_sequential_mask(T, device=DEV))
    seq = torch.arange(1, T + 1, device=DEV).view(1, -1).expand(B, -1).masked_fill(pad.squeeze(1).squeeze(1) != 0, 0)
    assert mask.shape == ref_mask.shape and torch.equal(mask.view(torch.int32), ref_mask.float().view(torch.int32))
    assert torch.equal(out, emb + pos[seq])
    with pytest.raises(RuntimeError, match="position table"):
        o.decoder_inputs(tokens, emb, pos[:T], 0)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_dropout_apply_matches_keep_mask(dtype):
    o = ops()
    n = 1280 * 512 + 3 * 8
    x = rnd(n, dtype=dtype)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = o.DropSpec(p=0.1, seed=1234, site=5, step=step)
    y = o.dropout_apply(x, d)
    keep = o.dropout_keep_mask(d, n, x.device).bool()
    ref = torch.where(keep, x.float() / 0.9, torch.zeros_like(x.float()))
    assert nerr(y, ref) < (1e-6 if dtype == F32 else 4e-3)
    assert 0.08 < 1 - keep.float().mean().item() < 0.12
    assert o.dropout_apply(x, None) is x


def _pool_ref64(feat, hpre, w2, b2, keep, p, dpooled):
    f = feat.double().cpu().requires_grad_(True)
    h = hpre.double().cpu().requires_grad_(True)
    w = w2.double().cpu().requires_grad_(True)
    bb = b2.double().cpu().requires_grad_(True)
    B, N, D = f.shape
    act = torch.relu(h) * (keep.double().cpu().reshape(B * N, D) / (1 - p))
    logit = (act @ w + bb).reshape(B, N)
    att = torch.softmax(logit, 1)
    pooled = (f * att[..., None]).sum(1)
    (pooled * dpooled.double().cpu()).sum().backward()
    return att.detach(), pooled.detach(), f.grad, h.grad, w.grad, bb.grad


@pytest.mark.parametrize("fdt,dtype", [(F32, F32), (BF16, BF16), (F32, BF16)])
@pytest.mark.parametrize("B,N,D,p", [(3, 6, 32, 0.0), (64, 100, 512, 0.1), (64, 20, 512, 0.1), (5, 237, 768, 0.0)])
def test_attention_pool_fwd_bwd(fdt, dtype, B, N, D, p):
    o = ops()
    feat = rnd(B, N, D, dtype=fdt, seed=1)
    hpre = rnd(B * N, D, dtype=dtype, seed=2)
    w2, b2 = rnd(D, scale=D ** -0.5, seed=3), rnd(1, seed=4)
    dpooled = rnd(B, D, dtype=dtype, seed=5)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = o.DropSpec(p=p, seed=99, site=3, step=step) if p > 0 else None
    keep = o.dropout_keep_mask(d, B * N * D, feat.device) if p > 0 else torch.ones(B * N * D, device=DEV)
    att, pooled = o.pool_fwd(feat, hpre, w2, b2, d)
    dh, dfeat, part, bpart = o.pool_bwd(feat, hpre, w2, att, dpooled, d)
    att64, pooled64, gf, gh, gw, gb = _pool_ref64(feat, hpre, w2, b2, keep, p, dpooled)
    t = 1e-5 if dtype == F32 else 1e-2
    assert nerr(att, att64) < 1e-5 and nerr(pooled, pooled64) < t
    # dfeat is only the direct path att * dpooled; the path through fc1 is the caller's dX product
    direct = att64[..., None] * dpooled.double().cpu()[:, None, :]
    assert nerr(dfeat.view(B, N, D), direct) < t
    assert nerr(dh, gh) < t and nerr(part[:, :D].sum(0), gw) < 2e-4
    assert float(part[:, D:].abs().max()) == 0.0 and float(bpart[:, 1:].abs().max()) == 0.0
    assert abs(float(bpart[:, 0].sum()) - float(gb)) < 1e-4


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,n,ld", [(3, 7, 8), (64, 353, 360), (1280, 4000, 4000), (5, 11, 16), (40, 4000, 4096),
                                    (7, 8192, 8192), (3, 1024, 1032), (2, 8200, 8200)])
def test_log_softmax_and_nll(dtype, M, n, ld):
    o = ops()
    g = torch.Generator().manual_seed(M + n)
    x = (torch.randn(M, ld, generator=g) * 3).to(DEV, dtype)
    logp = o.log_softmax_fwd(x, n)
    x64 = x.double().cpu()[:, :n].requires_grad_(True)
    ref = torch.log_softmax(x64, -1)
    assert nerr(logp, ref) < 1e-5
    target = torch.randint(0, n, (M,), generator=g)
    target[0] = 2
    target[-1] = 0  # ignored
    loss = torch.zeros(1, device=DEV)
    dlogp = o.nll_loss(logp, target.to(DEV), ignore_index=0, loss=loss, want_grad=True)
    rl = torch.nn.functional.nll_loss(ref, target, ignore_index=0)
    rl.backward()
    rl = rl.detach()
    assert abs(float(loss) - float(rl)) < 1e-5 * max(1.0, abs(float(rl)))
    dx = o.log_softmax_bwd(dlogp, logp, ld, dtype)
    assert nerr(dx[:, :n], x64.grad) < (1e-6 if dtype == F32 else 1e-3)
    assert ld == n or float(dx[:, n:].float().abs().max()) == 0.0
    sc = torch.full((1,), 0.5, device=DEV)
    d2 = o.nll_loss(logp, target.to(DEV), ignore_index=0, want_grad=True, gscale=sc)
    assert nerr(d2, 0.5 * dlogp) < 1e-7
    loss2 = loss.clone()
    o.nll_loss(logp, target.to(DEV), ignore_index=0, loss=loss2, accumulate=True)
    assert abs(float(loss2) - 2 * float(loss)) < 1e-6 * max(1.0, abs(float(loss)))
