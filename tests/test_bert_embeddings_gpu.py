"""ovqa_bert_embeddings_fwd / _bwd against fp64 through the C ABI, fp32 and bf16 output, with guard bands (tests/redzone.py)
around every buffer: values, the exact zeros, accumulation, the mask's bits, run-to-run bits and the refused arguments."""
import sys

import pytest
import torch

from test_kernels_gpu import nerr, tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-12
PAD_COLS = 4        # the tables' row stride is D + 4 floats: strided rows, still 16-byte aligned
SENTINEL = 7.25     # what the columns between the rows of a gradient table hold before and must hold after


@pytest.fixture(autouse=True)
def zones(monkeypatch):
    """Guard bands around everything ``openvivqa_amd.ops`` allocates and around this file's own buffers."""
    import redzone
    rz = redzone.install(monkeypatch, sys.modules[__name__])
    yield rz
    torch.cuda.synchronize()
    rz.check()


def dev(rz, t):
    return rz.guard(t.to(DEV).contiguous(), "input")


def strided(rz, t, fill=float("nan")):
    """``t`` [rows, D] as a view with row stride D + PAD_COLS of a guarded buffer; the columns in between hold ``fill``."""
    rows, D = t.shape
    buf = rz.alloc((rows, D + PAD_COLS), F32, DEV, "table")
    buf.fill_(fill)
    buf[:, :D] = t.to(DEV)
    return buf[:, :D], buf


def make_case(B, T, V, P, D, seed=0):
    """Tokens with a repeated id within and across samples, id 0 (the table's padding row), id V - 1 and the vocabulary's
    padding id; a gradient whose row ``big`` -- one of the repeated id's positions -- is 8 times the others', so that losing
    that one row from any of the sums it enters is far outside the bar (asserted from the fp64 reference below)."""
    g = torch.Generator().manual_seed(1000 * seed + B * T + D)
    R = B * T
    mask_pad = min(2, V - 1)
    tok = torch.randint(min(3, V - 1), V, (R,), generator=g)
    rep = min(5, V - 1)
    big = 0
    if R >= 9:
        tok[0], tok[2], tok[T] = rep, rep, rep      # within sample 0 and in sample 1
        tok[1], tok[3], tok[R - 1], tok[R - 2] = 0, V - 1, mask_pad, mask_pad
    else:
        tok[0] = V - 1
        mask_pad = V - 1
    tok = tok.view(B, T)
    word = torch.randn(V, D, generator=g) * 0.5
    pos = torch.randn(P, D, generator=g) * 0.5
    typ = torch.randn(2, D, generator=g) * 0.5
    gamma = torch.randn(D, generator=g) * 0.2 + 1.0
    beta = torch.randn(D, generator=g) * 0.1
    dy = torch.randn(R, D, generator=g)
    dy[big] *= 8.0
    return dict(tok=tok, word=word, pos=pos, typ=typ, gamma=gamma, beta=beta, dy=dy, mask_pad=mask_pad, big=big)


def reference(c, dy, keep, p):
    """fp64: (y, mean, rstd, gradients of word / pos / typ / gamma / beta, dx rows)."""
    tok = c["tok"]
    B, T = tok.shape
    leaves = [c[k].double().clone().requires_grad_(True) for k in ("word", "pos", "typ", "gamma", "beta")]
    word, pos, typ, gamma, beta = leaves
    x = torch.nn.functional.embedding(tok, word, padding_idx=0) + typ[0] + pos[:T]
    x.retain_grad()
    mu = x.mean(-1, keepdim=True)
    rs = 1 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + EPS)
    y = ((x - mu) * rs * gamma + beta) * keep.double().view(B, T, -1) / (1 - p)
    y.backward(dy.double().view_as(y))
    return (y.detach(), mu.reshape(-1).detach(), rs.reshape(-1).detach(), [t.grad for t in leaves],
            x.grad.reshape(B * T, -1))


SHAPES = [(1, 1, 8, 4, 32), (3, 9, 37, 16, 768), (5, 16, 50, 16, 512)]
CASES = [(s, dt, p) for s in SHAPES for dt in (F32, BF16) for p in (0.0, 0.1)] + [((2, 20, 30522, 512, 768), BF16, 0.1)]


@pytest.mark.parametrize("shape,dtype,p", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_bert_embeddings_fwd_bwd_match_fp64(zones, shape, dtype, p):
    from openvivqa_amd import ops
    from openvivqa_amd.utils import generate_padding_mask
    B, T, V, P, D = shape
    R = B * T
    c = make_case(*shape)
    tok = dev(zones, c["tok"])
    (word, _), (pos, _), (typ, _) = (strided(zones, c[k]) for k in ("word", "pos", "typ"))
    gamma, beta = dev(zones, c["gamma"]), dev(zones, c["beta"])
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    drop = ops.DropSpec(p=p, seed=77, site=5, step=step) if p > 0 else None
    keep = ops.dropout_keep_mask(drop, R * D, DEV).cpu() if p > 0 else torch.ones(R * D)

    def forward():
        return ops.bert_embeddings_fwd(tok, word, pos, typ, gamma, beta, EPS, out_dtype=dtype, drop=drop, want_f32=True,
                                       mask_padding_idx=c["mask_pad"])
    y, y32, mean, rstd, mask = forward()
    dy = c["dy"].to(dtype)
    ry, rmu, rrs, rgrads, rdx = reference(c, dy, keep, p)
    assert nerr(y, ry) < tol(dtype) and nerr(y32, ry) < tol(F32)
    assert nerr(mean, rmu) < 1e-4 and nerr(rstd, rrs) < 1e-4
    assert torch.equal(y32.to(dtype), y)  # the same values, rounded once
    want_mask = generate_padding_mask(c["tok"], c["mask_pad"]).float()
    assert torch.equal(mask.cpu().view(torch.int32), want_mask.view(torch.int32)) and bool((want_mask != 0).any())
    y2 = forward()
    assert all(torch.equal(a, b) for a, b in zip((y, y32, mean, rstd, mask), y2))

    # ---- what the reference itself says about the sums: losing ONE contributing row misses the bar by >= 10x
    rword, rpos, rtyp, rgamma, rbeta = rgrads
    big, t_big, v_big = c["big"], c["big"] % T, int(c["tok"].view(-1)[c["big"]])
    if R > 1:
        assert int((c["tok"] == v_big).sum()) >= 3 and int((c["tok"][0] == v_big).sum()) >= 2  # within and across samples
    for full in (rpos[t_big], rtyp[0], rword[v_big]):
        assert nerr((full - rdx[big])[None], full[None]) >= 10 * tol(dtype)

    # ---- backward: stored, then added to a non-zero initial value
    dyd = dev(zones, dy)
    dgamma, dbeta = dev(zones, torch.full((D,), 0.5)), dev(zones, torch.full((D,), 0.5))
    tabs = [strided(zones, torch.full((n, D), 0.5), fill=SENTINEL) for n in (V, P, 2)]

    def backward(acc):
        return ops.bert_embeddings_bwd(dyd, tok, word, pos, typ, gamma, mean, rstd, tabs[0][0], tabs[1][0], tabs[2][0], dgamma,
                                       dbeta, drop=drop, table_padding_idx=0, accumulate=(acc,) * 5)
    dx = backward(False)
    t = tol(dtype)
    got = [tabs[0][0], tabs[1][0], tabs[2][0], dgamma, dbeta]
    for name, a, b in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), got, rgrads):
        assert nerr(a, b) < t, (name, nerr(a, b))
    assert nerr(dx, rdx) < t
    named = torch.zeros(V, dtype=torch.bool)
    named[c["tok"].view(-1)] = True
    named[0] = False  # the table's padding row: zeros although tokens name it
    assert bool((c["tok"] == 0).any()) or R == 1
    dword = tabs[0][0].cpu()
    assert float(dword[~named].abs().max()) == 0.0 and bool((dword[named].abs().amax(1) > 0).all())
    if P > T:
        assert float(tabs[1][0][T:].abs().max()) == 0.0
    assert float(tabs[2][0][1:].abs().max()) == 0.0
    first = [a.clone() for a in got] + [dx]
    assert all(torch.equal(a, b) for a, b in zip(first, [*got, backward(False)]))  # two runs, the same bits
    backward(True)
    for name, a, b in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), got, first):
        assert torch.equal(a, b + b), name  # x + x is exact: the second run added the same sums to the first's
    for _, buf in tabs:
        assert bool((buf[:, D:] == SENTINEL).all())  # nothing stored between the rows
    # ... and to a value the kernels did not put there
    for a in got:
        a.fill_(0.5)
    backward(True)
    for name, a, b in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), got, rgrads):
        assert nerr(a, b + 0.5) < t, name
    assert bool((tabs[2][0][1:] == 0.5).all()) and bool((tabs[0][0].cpu()[~named] == 0.5).all())
    if P > T:
        assert bool((tabs[1][0][T:] == 0.5).all())


@pytest.mark.parametrize("what,shape", [("T > P", (2, 5, 8, 4, 32)), ("D = 30", (2, 3, 8, 4, 30)), ("D = 1028", (2, 3, 8, 4, 1028))])
def test_bert_embeddings_refuse_bad_arguments_and_write_nothing(zones, what, shape):
    from openvivqa_amd import _lib
    B, T, V, P, D = shape
    lib = _lib.load()
    ld = (D + 3) // 4 * 4
    tok = dev(zones, torch.ones(B, T, dtype=torch.int64))
    word, pos, typ = (zones.alloc((n, ld), F32, DEV).zero_() for n in (V, P, 2))
    gamma, beta = zones.alloc((ld,), F32, DEV).fill_(1), zones.alloc((ld,), F32, DEV).zero_()
    outs = [zones.alloc(s, F32, DEV).fill_(SENTINEL) for s in ((B * T, ld), (B * T, ld), (B * T,), (B * T,), (B, T))]
    y, y32, mean, rstd, mask = outs
    want = -2 if D > 1024 else -1  # OVQA_ERR_UNSUPPORTED, OVQA_ERR_BAD_ARG (include/ovqa_hip.h)
    p = torch.Tensor.data_ptr
    rc = lib.ovqa_bert_embeddings_fwd(_lib.OVQA_F32, p(tok), p(word), ld, V, p(pos), ld, P, p(typ), p(gamma), p(beta), EPS, p(y),
                                      p(y32), p(mean), p(rstd), p(mask), 0, B, T, D, None, None)
    assert rc == want and lib.ovqa_last_error(), (what, rc)
    grads = [zones.alloc(s, F32, DEV).fill_(SENTINEL) for s in ((B * T, ld), (B * T * 3 * ld,), (V, ld), (P, ld), (2, ld), (ld,), (ld,))]
    dx, ws, dword, dpos, dtyp, dgamma, dbeta = grads
    rc = lib.ovqa_bert_embeddings_bwd(_lib.OVQA_F32, p(tok), p(word), ld, V, p(pos), ld, P, p(typ), p(gamma), p(mean), p(rstd),
                                      p(y), p(dx), p(ws), ws.numel(), p(dword), ld, V, 0, 0, p(dpos), ld, P, 0, p(dtyp), ld, 2, 0,
                                      p(dgamma), 0, p(dbeta), 0, B, T, D, None, None)
    assert rc == want and lib.ovqa_last_error(), (what, rc)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs + grads)
