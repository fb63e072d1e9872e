"""Dropout on the attention probabilities on the MFMA attention kernels (bf16): forward and two-kernel backward against
fp64 autograd with the library's own keep mask injected, the keep pattern itself, p == 0 and the step counter."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


def ops():
    from openvivqa_amd import ops as o
    return o


def last_dispatch():
    from openvivqa_amd import _lib
    return _lib.last_dispatch()


def nerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g).to(BF16).to(DEV)


def make_mask(kind, B, nq, nk, tail=12):
    """None | key-row mask (B,1,1,nk) with ragged padding | M4C's dense prefix-LM mask (B,1,nq,nk): key padding, and the
    last `tail` positions see each other causally (mmf_m4c.py's extended attention mask)."""
    if kind == "none":
        return None
    row = torch.zeros(B, 1, 1, nk)
    for b in range(B):
        pad = (3 * b + 1) % max(1, nk // 4)  # ragged: a different number of padded keys per sample
        if kind == "row":
            row[b, ..., nk - pad:] = -1e5
        else:  # padded OCR tokens in front of the decoding positions
            row[b, ..., nk - tail - pad:nk - tail] = -1e5
    if kind == "row":
        return row.to(DEV)
    assert nq == nk
    m = row.expand(B, 1, nq, nk).clone()
    i = torch.arange(nq).view(nq, 1)
    j = torch.arange(nk).view(1, nk)
    m[:, :, ((i >= nq - tail) & (j > i))] = -1e5
    return m.contiguous().to(DEV)


def reference(q, k, v, mask, keep, B, H, nq, nk, d):
    qh = q.view(B, nq, H, d).transpose(1, 2)
    kh = k.view(B, nk, H, d).transpose(1, 2)
    vh = v.view(B, nk, H, d).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d)
    if mask is not None:
        s = s + mask.double().cpu()
    p = torch.softmax(s, -1) * keep
    return (p @ vh).transpose(1, 2).reshape(B, nq, H * d), p, torch.logsumexp(s, -1)


SHAPES = [  # (B, H, nq, nk, d, mask)
    (4, 8, 182, 182, 96, "dense"),
    (4, 8, 182, 182, 96, "row"),
    (2, 8, 100, 100, 64, "row"),
    (2, 8, 20, 100, 64, "row"),
    (2, 4, 150, 150, 128, "none"),
    (3, 8, 37, 61, 96, "row"),  # odd n_k: odd rows start on the high half of a pair hash
]


@pytest.mark.parametrize("with_lo", [False, True], ids=["no_o_lo", "o_lo"])
@pytest.mark.parametrize("p_drop", [0.1, 0.5])
@pytest.mark.parametrize("B,H,nq,nk,d,mkind", SHAPES)
def test_mfma_attention_dropout_matches_fp64(B, H, nq, nk, d, mkind, p_drop, with_lo):
    o = ops()
    q, k, v = rnd(B, nq, H * d, seed=1), rnd(B, nk, H * d, seed=2), rnd(B, nk, H * d, seed=3)
    mask = make_mask(mkind, B, nq, nk)
    drop = o.DropSpec(p=p_drop, seed=1234, site=7, step=torch.tensor([5], dtype=torch.int32, device=DEV))
    keep = o.dropout_keep_mask(drop, B * H * nq * nk, DEV).view(B, H, nq, nk).double().cpu() / (1.0 - p_drop)
    lo = [] if with_lo else None
    out, lse, _ = o.attention_fwd(q, k, v, mask, H, att_drop=drop, lo_out=lo)
    assert last_dispatch() == "mfma"
    qd, kd, vd = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    ro, _, rl = reference(qd, kd, vd, mask, keep, B, H, nq, nk, d)
    assert nerr(out, ro) < 1e-2 and nerr(lse, rl) < 1e-2
    d_o = rnd(B, nq, H * d, seed=5)
    (ro * d_o.double().cpu()).sum().backward()
    dq, dk, dv = o.attention_bwd(d_o, q, k, v, out, lse, mask, H, att_drop=drop, o_lo=lo[0] if with_lo else None)
    assert last_dispatch() == "mfma"
    t = 3e-2
    assert nerr(dq, qd.grad) < t and nerr(dk, kd.grad) < t and nerr(dv, vd.grad) < t


@pytest.mark.parametrize("B,H,nq,nk,d", [(2, 8, 182, 182, 96), (3, 8, 37, 61, 96), (2, 8, 100, 100, 64)])
def test_mfma_attention_dropout_zero_pattern_is_the_keep_mask(B, H, nq, nk, d):
    """The MFMA kernel drops exactly the elements ovqa_dropout_keep_mask (and the VALU kernels) drop."""
    o = ops()
    q, k, v = rnd(B, nq, H * d, seed=11), rnd(B, nk, H * d, seed=12), rnd(B, nk, H * d, seed=13)
    drop = o.DropSpec(p=0.3, seed=99, site=3, step=torch.tensor([17], dtype=torch.int32, device=DEV))
    keep = o.dropout_keep_mask(drop, B * H * nq * nk, DEV).view(B, H, nq, nk)
    _, _, att = o.attention_fwd(q, k, v, None, H, need_att=True, att_drop=drop)
    assert last_dispatch() == "mfma"
    assert torch.equal(att == 0, keep == 0)
    qd, kd, vd = (t.double().cpu() for t in (q, k, v))
    _, rp, _ = reference(qd, kd, vd, None, keep.double().cpu() / 0.7, B, H, nq, nk, d)
    assert nerr(att, rp) < 1e-2


@pytest.mark.parametrize("with_lo", [False, True], ids=["no_o_lo", "o_lo"])
def test_mfma_attention_dropout_p0_is_bit_identical_to_none(with_lo):
    o = ops()
    B, H, n, d = 2, 8, 182, 96
    q, k, v = rnd(B, n, H * d, seed=21), rnd(B, n, H * d, seed=22), rnd(B, n, H * d, seed=23)
    mask = make_mask("dense", B, n, n)
    d_o = rnd(B, n, H * d, seed=24)
    step = torch.tensor([2], dtype=torch.int32, device=DEV)
    res = []
    for drop in (None, o.DropSpec(p=0.0, seed=5, site=1, step=step)):
        lo = [] if with_lo else None
        out, lse, _ = o.attention_fwd(q, k, v, mask, H, att_drop=drop, lo_out=lo)
        grads = o.attention_bwd(d_o, q, k, v, out, lse, mask, H, att_drop=drop, o_lo=lo[0] if with_lo else None)
        res.append((out, lse) + tuple(grads))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_mfma_attention_dropout_step_counter():
    """The mask is a function of the device step counter: the same step repeats bit for bit, another step differs."""
    o = ops()
    B, H, n, d = 2, 8, 182, 96
    q, k, v = rnd(B, n, H * d, seed=31), rnd(B, n, H * d, seed=32), rnd(B, n, H * d, seed=33)
    mask = make_mask("row", B, n, n)
    d_o = rnd(B, n, H * d, seed=34)
    step = torch.tensor([7], dtype=torch.int32, device=DEV)
    drop = o.DropSpec(p=0.1, seed=42, site=2, step=step)

    def run():
        lo = []
        out, lse, _ = o.attention_fwd(q, k, v, mask, H, att_drop=drop, lo_out=lo)
        return (out, lse) + tuple(o.attention_bwd(d_o, q, k, v, out, lse, mask, H, att_drop=drop, o_lo=lo[0]))

    first, again = run(), run()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    step.fill_(8)
    other = run()
    assert torch.equal(first[1], other[1])  # lse is that of the undropped probabilities
    for i in (0, 2, 3, 4):
        assert not torch.equal(first[i], other[i])
