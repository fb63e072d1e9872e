"""Prefix-LM attention as a trainable operation: ovqa_attention_fwd_prefix_lm_train (o, o_lo, lse, dropout on the
probabilities) and ovqa_attention_bwd_prefix_lm (dq, dk, dv) take the mask as a key row + the number of trailing positions
that see each other causally, where ovqa_attention_fwd / _bwd read a dense (B, 1, n, n) tensor per element.

Every row compares with fp64 math on the dense mask under the bars of tests/test_kernel_routes_gpu.py (no tolerance of its
own), is required BIT-IDENTICAL to the dense-mask calls (a masked probability is exactly 0 either way; where the dense-mask
backward of a shape is the role-split kernel, to the per-query-mask form of the two-kernel backward), shows that the bars
see a missing corner (>= 10x, the factor of test_long_prefix_lm_parity) and checks the kernels the calls launch: the
LDS-resident rows the row-mask forms of the forward and of the two-kernel backward -- also where a key-row call without a
tail would take the merged / role-split backward (d = 64, n <= 128) --, the long rows streaming kernels only.
"""
import os

import pytest
import torch

from test_kernel_routes_gpu import BF16, DEV, Sentinel, bar_att, bar_bwd, launched, record, rel_max, rnd
from test_long_attention_gpu import PREFIX_LONG, att_ref, bwd_ref, lse_bar, resident_bwd, resident_fwd

pytestmark = pytest.mark.gpu

B, H = 2, 2
RESIDENT = [(100, 12, 64), (128, 128, 64), (37, 37, 64), (250, 20, 64), (182, 12, 96), (192, 40, 128), (64, 1, 128)]
ROWS = RESIDENT + [(n, tail, d) for (_, n, tail, d) in PREFIX_LONG]
CASES = [pytest.param(n, tail, d, dr, id=f"n{n}-tail{tail}-d{d}{'-drop' if dr else ''}")
         for (n, tail, d) in ROWS for dr in (False, True)]
SWITCHED_OFF = any(os.environ.get(k, "0") == "1" for k in ("OVQA_FORCE_SIMPLE", "OVQA_NO_PREFIX_LM"))
needs_route = pytest.mark.skipif(SWITCHED_OFF, reason="OVQA_FORCE_SIMPLE / OVQA_NO_PREFIX_LM switch the prefix-LM kernels off")


def masks(n, tail):
    """The key row (padded keys in sample 0 and, in the last sample, just in front of the decoding positions) and its dense
    twin with -inf above the corner's diagonal."""
    row = torch.zeros(B, 1, 1, n, device=DEV)
    row[0, :, :, 3:7] = -10000.0
    row[-1, :, :, max(0, n - tail - 9):n - tail] = -10000.0
    dense = row.repeat(1, 1, n, 1)
    dense[:, :, -tail:, -tail:] += torch.full((tail, tail), float("-inf"), device=DEV).triu(1)
    return row, dense


def operands(n, d, tail):
    """q, k, v: row-strided slices of one packed [B, n, 3 H d] projection buffer, and d_o.  The decoding positions attend
    to each other, as a decoder's do: their q and k rows share a component c with c . c / sqrt(d) = 3, so the keys the
    corner hides would hold a large share of a decoding query's probability mass at any n (with independent rows the
    corner's share falls as tail / n, and at 12 of 232 keys the key row alone moves dq by 9x its bar, not 10x)."""
    qkv = rnd(B, n, 3 * H * d, dtype=torch.float32, seed=1)
    c = rnd(H * d, dtype=torch.float32, seed=7).sign() * (3.0 / d ** 0.5) ** 0.5
    qkv[:, n - tail:, :2 * H * d] += c.repeat(2)
    qkv = qkv.to(BF16)
    return qkv[..., :H * d], qkv[..., H * d:2 * H * d], qkv[..., 2 * H * d:], rnd(B, n, H * d, dtype=BF16, seed=5)


def dropout(o_, n, dr):
    if not dr:
        return None, None
    drop = o_.DropSpec(p=0.1, seed=23, site=5, step=torch.tensor([3], dtype=torch.int32, device=DEV))
    return drop, o_.dropout_keep_mask(drop, B * H * n * n, DEV).view(B, H, n, n).double() / 0.9


def nkt_of(n):
    return 1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 6 if n <= 192 else 8  # (launch_fwd_d)


@needs_route
@pytest.mark.parametrize("n,tail,d,dr", CASES)
def test_prefix_lm_train_parity_bits_and_routes(n, tail, d, dr, request):
    from openvivqa_amd import _lib
    from openvivqa_amd import ops as o_
    q, k, v, d_o = operands(n, d, tail)
    row, dense = masks(n, tail)
    drop, keep = dropout(o_, n, dr)
    assert o_.attention_fwd_prefix_lm_ok(q, H)

    lo = []
    (out, lse), flog = launched(lambda: o_.attention_fwd_prefix_lm_train(q, k, v, row, tail, H, att_drop=drop, lo_out=lo))
    fdisp = _lib.last_dispatch()
    sent = Sentinel((B, n, 5 * H * d), BF16)  # dq | gap | dk | gap | dv
    dq_, dk_, dv_ = (sent.view(lambda p, i=i: p[..., 2 * i * H * d:(2 * i + 1) * H * d]) for i in range(3))
    grads, blog = launched(lambda: o_.attention_bwd_prefix_lm(d_o, q, k, v, out, lse, row, tail, H, dq=dq_, dk=dk_, dv=dv_,
                                                              att_drop=drop, o_lo=lo[0]))
    bdisp = _lib.last_dispatch()
    sent.check(*grads)

    # ---- fp64 on the dense mask, under the existing bars
    ro, rp, rpk, vh, rl = att_ref(q, k, v, dense, H, keep)
    bar = bar_att(ro, rpk, vh, B, n, H)
    e = record(request, "o", rel_max(out, ro), bar)
    assert e <= bar, (e, bar)
    e = record(request, "o+o_lo", rel_max(out.double() + lo[0].double(), ro), bar)
    assert e <= bar, (e, bar)
    el = record(request, "lse / bar", ((lse.double() - rl).abs() / lse_bar(rl)).max().item(), 1.0)
    assert el <= 1.0, el
    rq, rk, rv, p, pk = bwd_ref(q, k, v, dense, H, d_o, keep)
    bars = {}
    for name, got, ref in zip(("dq", "dk", "dv"), grads, (rq, rk, rv)):
        bars[name] = bar_bwd(name, ref, q, k, v, d_o, p, pk, dense, H, keep)
        e = record(request, name, rel_max(got, ref), bars[name])
        assert e <= bars[name], (name, e, bars[name])

    # ---- the corner matters: the key row alone moves every result far outside its bar (an empty corner cannot)
    if tail >= 12:
        assert rel_max(att_ref(q, k, v, row, H, keep)[0], ro) >= 10 * bar
        for name, moved, ref in zip(("dq", "dk", "dv"), bwd_ref(q, k, v, row, H, d_o, keep)[:3], (rq, rk, rv)):
            assert rel_max(moved, ref) >= 10 * bars[name], name

    # ---- bit-identical to the dense-mask calls
    lo_d = []
    out_d, lse_d, _ = o_.attention_fwd(q, k, v, dense, H, att_drop=drop, lo_out=lo_d)
    gd, dlog = launched(lambda: o_.attention_bwd(d_o, q, k, v, out_d, lse_d, dense, H, att_drop=drop, o_lo=lo_d[0]))
    drs = "true" if dr else "false"
    twin = ([f"attn_bwd_dq_mfma_kernel<false,{d},{drs}>", f"attn_bwd_dkv_mfma_kernel<false,{d},{drs}>"] if resident_bwd(n, n, d)
            else [f"attn_stream_bwd_dq_kernel<{d},false,{drs}>", f"attn_stream_bwd_dkv_kernel<{d},false,{drs}>"])
    if dlog != twin:
        # d = 64, n <= 128, no dropout: the dense-mask call takes the role-split backward (launch_bwd), which the tail
        # call must not take and which forms its exponent differently (scale and log2e folded into one factor) -- not
        # the same expression, not the same bits.  The per-query-mask twin of the kernels the tail call DID run is reached
        # with a dropout that keeps everything and scales by exactly 1 (p = 2^-40: threshold 0, 1 / (1 - p) == 1.0f).
        assert d == 64 and n <= 128 and not dr and all("_roles_" in x or "_smallk_" in x for x in dlog), (dlog, twin)
        keep_all = o_.DropSpec(p=2.0 ** -40, seed=1, site=1, step=torch.tensor([0], dtype=torch.int32, device=DEV))
        gd, dlog = launched(lambda: o_.attention_bwd(d_o, q, k, v, out_d, lse_d, dense, H, att_drop=keep_all, o_lo=lo_d[0]))
        assert dlog == [f"attn_bwd_dq_mfma_kernel<false,{d},true>", f"attn_bwd_dkv_mfma_kernel<false,{d},true>"], dlog
    for name, a, b in (("o", out, out_d), ("o_lo", lo[0], lo_d[0]), ("lse", lse, lse_d), ("dq", grads[0], gd[0]),
                       ("dk", grads[1], gd[1]), ("dv", grads[2], gd[2])):
        assert torch.equal(a, b), name

    # ---- routes
    if resident_fwd(n, d):
        assert flog == [f"attn_fwd_mfma_kernel<{nkt_of(n)},true,false,{d},{drs}>"], flog
        assert fdisp == "mfma"
    else:
        assert flog == [f"attn_stream_fwd_kernel<{d},true,{drs}>"], flog
        assert fdisp == "mfma-stream"
    if resident_bwd(n, n, d):
        assert blog == [f"attn_bwd_dq_mfma_kernel<true,{d},{drs}>", f"attn_bwd_dkv_mfma_kernel<true,{d},{drs}>"], blog
        assert bdisp == "mfma"
    else:
        assert len(blog) == 2 and all(x.startswith("attn_stream_bwd_") for x in blog), blog
        assert blog == [f"attn_stream_bwd_dq_kernel<{d},true,{drs}>", f"attn_stream_bwd_dkv_tail_kernel<{d},{drs}>"], blog
        assert bdisp == "mfma-stream"


@needs_route
@pytest.mark.parametrize("n,tail,d", [(182, 12, 96), (232, 12, 96)])
def test_prefix_lm_backward_is_deterministic(n, tail, d):
    from openvivqa_amd import ops as o_
    q, k, v, d_o = operands(n, d, tail)
    row, _ = masks(n, tail)
    drop, _ = dropout(o_, n, True)
    lo = []
    out, lse = o_.attention_fwd_prefix_lm_train(q, k, v, row, tail, H, att_drop=drop, lo_out=lo)
    g1 = o_.attention_bwd_prefix_lm(d_o, q, k, v, out, lse, row, tail, H, att_drop=drop, o_lo=lo[0])
    g2 = o_.attention_bwd_prefix_lm(d_o, q, k, v, out, lse, row, tail, H, att_drop=drop, o_lo=lo[0])
    for a, b in zip(g1, g2):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert torch.isfinite(a.float()).all()


def test_prefix_lm_train_errors():
    """fp32 tensors and heads of 80 features are 'unsupported' (-2: the caller passes the dense mask), a tail longer than
    the sequence is a 'bad argument' (-1); nothing is launched."""
    from openvivqa_amd import ops as o_
    n = 40
    row = torch.zeros(B, 1, 1, n, device=DEV)
    for dtype, d, tail, code in ((torch.float32, 64, 4, -2), (BF16, 80, 4, -2), (BF16, 64, n + 1, -1)):
        q = rnd(B, n, H * d, dtype=dtype, seed=1)
        with pytest.raises(RuntimeError, match=f"kernel error {code} in attention_fwd_prefix_lm_train"):
            launched(lambda: o_.attention_fwd_prefix_lm_train(q, q, q, row, tail, H))
        lse = torch.zeros(B, H, n, device=DEV)
        with pytest.raises(RuntimeError, match=f"kernel error {code} in attention_bwd_prefix_lm"):
            o_.attention_bwd_prefix_lm(q, q, q, q, q, lse, row, tail, H)
