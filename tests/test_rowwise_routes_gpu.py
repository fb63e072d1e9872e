"""Route-table parity of the ROW-WISE kernels that run between the GEMMs -- LayerNorm forward / backward, the attention
pool, log-softmax and the NLL loss -- against fp64 math, by instantiation, through the C ABI.

Style of tests/test_kernel_routes_gpu.py and tests/test_wgrad_routes_gpu.py: references are fp64 torch on the SAME rounded
operands (never another HIP kernel; the dropout keep mask is the counter hash of csrc/common.h written out here), the
launch log must equal the expected instantiation, every output is a view with sentinel bytes around it, every compared
quantity goes through ``parity_record``.

CRITERION: element-wise, not max-normalised.  For every output element

    |got - ref| <= U_out |ref| + (K + 64) 2^-24 T

U_out = 2^-8 for a bf16 output (one rounding of the result) and 0 for fp32; K the length of the reduction behind the
element (a sum of K fp32 terms in any order, then at most 64 further fp32 roundings); T the reference's own expression
evaluated with absolute values -- per kernel:
  * LayerNorm forward  y:      T = max_j (|x| + |mu|) rstd |gamma| + |beta| + |pos|,  K = D
                       mean:   |err| <= (D + 2) 2^-24 mean_j |x|;   rstd: |err| <= (D + 16) 2^-24 rstd
  * LayerNorm backward dx:     T = rstd (|d| + mean_j |d| + |xh| mean_j |d xh|), d = dy gamma, K = D.  (mean_j |d|, not |c1|:
                               c1 = mean_j d is a D-term sum whose error scales with sum |d|; where it cancels, |c1| is no
                               bound on it -- an honest fp32 evaluation measured 1.6 of the bound written with |c1| on the
                               row bf16_x32_dx32_D520_M4096.)
                       dgamma: T_j = sum_m |dy| (|x| + |mean|) rstd, K = M: the M terms summed in fp32 in any order, each
                               term's (x - mean) rstd dy roundings in the 64; under accumulate one more fp32 add,
                               2^-24 (|initial value| + |ref|)
                       dbeta:  integer dy: EXACT
  * pool forward       att:    |err| <= 2^-24 K_att att, K_att = 2 (D + 64) L + (N + 64), L = max_n sum_j |act w2| + |b2|: a
                               logit is a D-term sum (error (D + 64) 2^-24 L at most), a softmax value moves by at most
                               att (|dlogit_n| + sum_m att_m |dlogit_m|) <= 2 att max |dlogit|, and the N-term normaliser
                               and the exponential add (N + 64) 2^-24 att;  pooled: U |ref| + 2^-24 K_att sum_n att |feat|
  * pool backward (att is an INPUT here: the reference's, rounded to fp32)  with A_n = sum_j |feat dpooled|, Abar = sum_n
                       att A_n, K = N + D + 128 (datt a D-term sum, dot an N-term sum of them):
                       dlogit: |err| <= K 2^-24 att_n (A_n + Abar) =: E_n;  dh: U |ref| + E_n |w2| mask;  dfeat (one product):
                       U |ref| + 64 2^-24 |ref|;  dw2 partial: (N + 64 + K) 2^-24 sum_n att_n (A_n + Abar) |act|;
                       sum of the db2 partials: N 2^-24 sum |dlogit| (absolute)
  * log-softmax        logp:   (n + 64) 2^-24 max(max_j |x - max|, |lse|);  dx: U |ref| + (n + 64) 2^-24 (|g| + p sum |g|)
  * NLL                loss:   M 2^-24 sum |logp_t| / cnt;  dlogp: EXACT (-gscale / cnt in fp32 at the targets, 0.0 elsewhere)
The recorded value is max err / bound, the bar 1.0: no headroom factor, no floor.

EVERY BAR SEES A BUG, checked on the reference alone before the kernel's output is looked at: the fp64 reference with
one part left out -- the last live 8-column lane group of a row statistic (LayerNorm), the last row of a column sum
(dgamma), one pool position, the last 8-column block of a log-softmax row, the last target row (NLL) -- exceeds the bound
by at least 10x.  The left-out parts carry weight so that this holds at every shape: +EDGE sigma on the last 8 columns
of x and gamma = EDGE there, the last gradient row LAST_ROW(M) times the others, pool positions N - 1 (and 512 where
N > 512) with the logit that gives them half / a third of the softmax mass, half of the log-softmax mass and a 16-fold
gradient in the last block, a last NLL target row heavy enough for M 2^-24.

EXACT rows of the LayerNorm backward: dy, x, mean small integers, gamma and rstd powers of two, D a power of two, dropout
p = 0.5 (scale 2): every intermediate is exactly representable in fp32 (the test asserts it of the fp64 reference), so
dx (rounded once where the output is bf16), dx_dropped = dx keep 2, dgamma and dbeta must EQUAL the reference.

One row of the forward has x = 100 + N(0, 1), one x = 1000 + N(0, 1): the two-pass variance is pinned by asserting, on
the reference, that a one-pass E[x^2] - E[x]^2 in fp32 misses the reference's rstd by more than the bar.  fp32 inputs
only (bf16 values near 100 are multiples of 0.5 whose squares and sums fp32 holds exactly at small D: the rows are run
but prove nothing there).  The one-pass error is about c^2 2^-24 relative for an offset c while the bar is (D + 16) 2^-24:
the 100 row is asserted up to D = 1032 -- at D = 2048 its miss measured 6.1e-5 against a bar of 1.2e-4 -- the 1000 row at
every D.

NLL targets outside [0, n) (here -1 and n) are treated by the kernel as ignored; the reference masks them the same way.
"""
import math
import os

import pytest
import torch

from test_kernel_routes_gpu import BF16, DEV, EPS32, U, Sentinel, launched, record
from test_wgrad_routes_gpu import assert_exact, values

pytestmark = pytest.mark.gpu
F32 = torch.float32
F64 = torch.float64
TN = {F32: "float", BF16: "bf16"}
UO = {F32: 0.0, BF16: U}
INF = float("inf")
LN_EPS = 1e-5
EDGE = 4.0
ERR_UNSUPPORTED = -2  # include/ovqa_hip.h OVQA_ERR_UNSUPPORTED

# every instantiation of the family: tests/test_rowwise_table_cpu.py checks this list against the symbols of the built
# library, test_every_rowwise_kernel_shows_in_a_launch_log that each one is reached
ALL_ROWWISE = [
    "ln_fwd_kernel<float,float,1,1,4>", "ln_fwd_kernel<float,float,2,1,4>", "ln_fwd_kernel<float,float,4,1,4>",
    "ln_fwd_kernel<bf16,bf16,1,1,4>", "ln_fwd_kernel<bf16,bf16,2,1,4>", "ln_fwd_kernel<bf16,bf16,4,1,4>",
    "ln_fwd_kernel<float,bf16,1,1,4>", "ln_fwd_kernel<float,bf16,2,1,4>", "ln_fwd_kernel<float,bf16,4,1,4>",
    "ln_bwd_kernel<float,float,float,1,4>", "ln_bwd_kernel<float,float,float,2,4>", "ln_bwd_kernel<float,float,float,4,4>",
    "ln_bwd_kernel<float,float,float,1,8>", "ln_bwd_kernel<float,float,float,2,8>", "ln_bwd_kernel<float,float,float,4,8>",
    "ln_bwd_kernel<bf16,bf16,bf16,1,4>", "ln_bwd_kernel<bf16,bf16,bf16,2,4>", "ln_bwd_kernel<bf16,bf16,bf16,4,4>",
    "ln_bwd_kernel<bf16,bf16,bf16,1,8>", "ln_bwd_kernel<bf16,bf16,bf16,2,8>", "ln_bwd_kernel<bf16,bf16,bf16,4,8>",
    "ln_bwd_kernel<bf16,float,bf16,1,4>", "ln_bwd_kernel<bf16,float,bf16,2,4>", "ln_bwd_kernel<bf16,float,bf16,4,4>",
    "ln_bwd_kernel<bf16,float,bf16,1,8>", "ln_bwd_kernel<bf16,float,bf16,2,8>", "ln_bwd_kernel<bf16,float,bf16,4,8>",
    "ln_bwd_kernel<bf16,float,float,1,4>", "ln_bwd_kernel<bf16,float,float,2,4>", "ln_bwd_kernel<bf16,float,float,4,4>",
    "ln_bwd_kernel<bf16,float,float,1,8>", "ln_bwd_kernel<bf16,float,float,2,8>", "ln_bwd_kernel<bf16,float,float,4,8>",
    "pool_fwd_kernel<float,float>", "pool_fwd_kernel<bf16,bf16>", "pool_fwd_kernel<float,bf16>",
    "pool_bwd_kernel<float,float>", "pool_bwd_kernel<bf16,bf16>", "pool_bwd_kernel<float,bf16>",
    "log_softmax_fwd_kernel<float>", "log_softmax_fwd_kernel<bf16>",
    "log_softmax_bwd_kernel<float>", "log_softmax_bwd_kernel<bf16>",
    "log_softmax_fwd_row_kernel<float>", "log_softmax_fwd_row_kernel<bf16>",
    "log_softmax_bwd_row_kernel<float>", "log_softmax_bwd_row_kernel<bf16>",
    "nll_loss_kernel",
]


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
    """A tensor on the device (inside guard bands while the red-zone fixture is active)."""
    return t.to(DEV).contiguous()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def out_view(shape, dtype, pad=8):
    """An output as a view ``pad`` elements into a sentinel-filled parent with ``pad`` more behind it."""
    n = math.prod(shape)
    s = Sentinel((n + 2 * pad,), dtype)
    return s, s.parent[pad:pad + n].view(shape)


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI, one thin caller per entry point (tensors in, launch log out)
# ---------------------------------------------------------------------------------------------------------------------------
def logged(fn):
    """``launched`` with bf16 spelt as in ALL_ROWWISE (a template binding prints as __bf16, a literal argument as bf16)."""
    rc, log = launched(fn)
    return rc, [e.replace("__bf16", "bf16") for e in log]


def k_ln_fwd(x, gamma, beta, pos, y, y32, mean, rstd):
    o, M, D = ops(), x.shape[0], x.shape[1]
    rc, log = logged(lambda: lib().load().ovqa_layernorm_fwd(
        o._DT[y.dtype], o._DT[x.dtype], ptr(x), ptr(gamma), ptr(beta), ptr(pos), 0 if pos is None else pos.shape[0], ptr(y),
        ptr(y32), ptr(mean), ptr(rstd), M, D, LN_EPS, stream()))
    lib().check(rc, "layernorm_fwd")
    return log


def k_ln_bwd(dy, x, gamma, mean, rstd, dx, dxd, dgamma, dbeta, accumulate, drop, ws):
    o, M, D = ops(), x.shape[0], x.shape[1]
    rc, log = logged(lambda: lib().load().ovqa_layernorm_bwd(
        o._DT[dy.dtype], o._DT[dx.dtype], ptr(dy), ptr(x), o._DT[x.dtype], ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dxd),
        ptr(dgamma), ptr(dbeta), M, D, int(accumulate), None if drop is None else drop.c(), ptr(ws), stream()))
    lib().check(rc, "layernorm_bwd")
    return log


def k_bwd_blocks(M, D):
    return lib().load().ovqa_layernorm_bwd_blocks(M, D)


def k_pool_fwd(feat, hpre, w2, b2, att, pooled, pooled32, B, N, D, drop):
    o = ops()
    return logged(lambda: lib().load().ovqa_pool_fwd(
        o._DT[feat.dtype], o._DT[hpre.dtype], ptr(feat), ptr(hpre), ptr(w2), ptr(b2), ptr(att), ptr(pooled), ptr(pooled32), B, N,
        D, None if drop is None else drop.c(), stream()))


def k_pool_bwd(feat, hpre, w2, att, dpooled, dh, dfeat, part, bpart, B, N, D, drop):
    o = ops()
    return logged(lambda: lib().load().ovqa_pool_bwd(
        o._DT[feat.dtype], o._DT[hpre.dtype], ptr(feat), ptr(hpre), ptr(w2), ptr(att), ptr(dpooled), ptr(dh), ptr(dfeat),
        ptr(part), ptr(bpart), B, N, D, None if drop is None else drop.c(), stream()))


def k_lsm_fwd(x, n, out):
    rc, log = logged(lambda: lib().load().ovqa_log_softmax_fwd(ops()._DT[x.dtype], ptr(x), x.stride(0), ptr(out), x.shape[0],
                                                               n, stream()))
    lib().check(rc, "log_softmax_fwd")
    return log


def k_lsm_bwd(g, logp, dx):
    rc, log = logged(lambda: lib().load().ovqa_log_softmax_bwd(ops()._DT[dx.dtype], ptr(g), ptr(logp), ptr(dx), dx.stride(0),
                                                               g.shape[0], g.shape[1], stream()))
    lib().check(rc, "log_softmax_bwd")
    return log


def k_nll(logp, target, loss, dlogp, gscale, ignore_index, accumulate):
    rc, log = logged(lambda: lib().load().ovqa_nll_loss(ptr(logp), ptr(target), ptr(loss), ptr(dlogp), ptr(gscale),
                                                        logp.shape[0], logp.shape[1], ignore_index, int(accumulate), stream()))
    lib().check(rc, "nll_loss")
    return log


def make_drop(p, seed, site, step=3):
    return ops().DropSpec(p=p, seed=seed, site=site, step=rnd(torch.tensor([step], dtype=torch.int32)))


# ---------------------------------------------------------------------------------------------------------------------------
# the dropout keep mask (csrc/common.h: drop_init / drop_pair_hash / drop_keep), in integer torch
# ---------------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def _mul32(h, c):
    """(h * c) mod 2^32 for an int64 tensor / int ``h`` < 2^32, without passing 2^63."""
    return (h * (c & 0xFFFF) + (((h * (c >> 16)) & 0xFFFF) << 16)) & M32


def _fmix32(h):
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def keep_mask(p, seed, site, step, n):
    """fp64 multipliers keep / (1 - p) of the flat element indices 0 .. n - 1 (all ones when p = 0)."""
    if p <= 0:
        return torch.ones(n, dtype=F64, device=DEV)
    key = _fmix32(seed ^ _fmix32((site * 0x9E3779B1 + step * 0x7F4A7C15 + 0x1234567) & M32))
    thresh = int(p * 65536.0 + 0.5)
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    h = _fmix32((idx >> 1) ^ key)
    field = torch.where((idx & 1) == 1, h >> 16, h & 0xFFFF)
    return (field >= thresh).to(F64) / (1.0 - p)


# ---------------------------------------------------------------------------------------------------------------------------
# criterion
# ---------------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 = 0; anything else over 0, and NaN, = inf)."""
    g = got.detach().double()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    err = (g - ref).abs()
    bound = bound.expand_as(err) if torch.is_tensor(bound) else torch.full_like(err, bound)
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, INF)))
    return torch.nan_to_num(r, nan=INF, posinf=INF).max().item()


def within(request, what, got, ref, bound):
    v = record(request, what + " (err / bound)", ratio(got, ref, bound), 1.0)
    assert v <= 1.0, (what, v)
    return v


def sees(what, mutated, ref, bound):
    """On the reference alone: the mutated reference is at least 10 bounds away somewhere."""
    v = ratio(mutated, ref, bound)
    assert v >= 10.0, (what, "the bound does not see the left-out part", v)


def exact(request, what, got, ref):
    record(request, what + " (exact: max |err|)", assert_exact(got, ref, what, 1 << 30), 0.0)


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------------------------------------------------------
def ln_chunks(D):
    return 1 if D <= 512 else 2 if D <= 1024 else 4


def ln_fwd_name(in_dt, out_dt, D):
    return f"ln_fwd_kernel<{TN[in_dt]},{TN[out_dt]},{ln_chunks(D)},1,4>"


def ln_fwd_ref(x, gamma, beta, pos, leave_out_last_group=False):
    xd, g, b = x.double(), gamma.double(), beta.double()
    M, D = xd.shape
    w = torch.ones(D, dtype=F64, device=xd.device)
    if leave_out_last_group:
        w[D - 8:] = 0
    eps = float(torch.tensor(LN_EPS, dtype=F32))
    mu = (xd * w).sum(1) / D
    var = ((xd - mu[:, None]) ** 2 * w).sum(1) / D
    rstd = 1.0 / torch.sqrt(var + eps)
    p = torch.zeros_like(xd) if pos is None else pos.double()[torch.arange(M, device=xd.device) % pos.shape[0]]
    y = (xd - mu[:, None]) * rstd[:, None] * g + b + p
    T = ((xd.abs() + mu.abs()[:, None]) * rstd[:, None] * g.abs() + b.abs() + p.abs()).max(1, keepdim=True).values
    return dict(mean=mu, rstd=rstd, y=y, T=T, absx=xd.abs().mean(1))


def offset_row(D, offset):
    g = torch.Generator().manual_seed(D + int(offset))
    return offset + torch.randn(D, generator=g)


def one_pass_miss(x_row, rstd_ref):
    """|rstd of a one-pass E[x^2] - E[x]^2 in fp32 - the reference's| (NaN where the one-pass variance comes out negative)."""
    x32 = x_row.float()
    m1 = x32.mean()
    return abs((1.0 / torch.sqrt((x32 * x32).mean() - m1 * m1 + LN_EPS)).double().item() - rstd_ref.item())


LN_FWD_PAIRS = [(F32, F32), (BF16, BF16), (F32, BF16)]
LN_FWD_D = [8, 512, 520, 1024, 1032, 2048]


@pytest.mark.parametrize("D", LN_FWD_D)
@pytest.mark.parametrize("in_dt,out_dt", LN_FWD_PAIRS, ids=["f32_f32", "bf16_bf16", "f32_bf16"])
def test_layernorm_fwd_route_parity(request, in_dt, out_dt, D):
    """M = 1 (three waves of the workgroup return at once), 5 (a partial workgroup; rows 3 and 4 are the 1000 + N(0, 1) and
    100 + N(0, 1) rows; once more with save_stats off and no fp32 copy), 37 (10 workgroups: the XCD remap has a remainder; pos_rows = 5)."""
    gamma = rnd(values("gauss", (D,), 2, F32))
    gamma[D - 8:] = EDGE
    beta = rnd(values("gauss", (D,), 3, F32))
    for M, pos_rows, stats, f32 in ((1, 0, True, True), (5, 0, True, True), (5, 0, False, False), (37, 5, True, True)):
        x = values("gauss", (M, D), 10 + M, F32)
        x[:, D - 8:] += EDGE
        if M == 5:
            x[3], x[4] = offset_row(D, 1000.0).to(x.device), offset_row(D, 100.0).to(x.device)
        x = rnd(x.to(in_dt))
        pos = rnd(values("gauss", (pos_rows, D), 4, F32)) if pos_rows else None
        ref, mut = ln_fwd_ref(x, gamma, beta, pos), ln_fwd_ref(x, gamma, beta, pos, True)
        tag = f"M={M} D={D} pos_rows={pos_rows} stats={int(stats)}"
        b_mean, b_rstd = (D + 2) * EPS32 * ref["absx"], (D + 16) * EPS32 * ref["rstd"]
        b_y32 = (D + 64) * EPS32 * ref["T"]
        b_y = UO[out_dt] * ref["y"].abs() + b_y32
        sees(tag + " mean", mut["mean"], ref["mean"], b_mean)
        sees(tag + " rstd", mut["rstd"], ref["rstd"], b_rstd)
        sees(tag + " y", mut["y"], ref["y"], b_y)
        if M == 5 and in_dt == F32:
            for row, what in ((3, "1000 + N(0, 1)"),) + (((4, "100 + N(0, 1)"),) if D <= 1032 else ()):
                miss = one_pass_miss(x[row], ref["rstd"][row])
                assert not miss <= b_rstd[row].item(), (f"a one-pass variance is within the bar on the {what} row", miss)
        s_y, y = out_view((M, D), out_dt)
        s_32, y32 = out_view((M, D), F32) if f32 else (None, None)
        s_m, mean = out_view((M,), F32) if stats else (None, None)
        s_r, rstd = out_view((M,), F32) if stats else (None, None)
        log = k_ln_fwd(x, gamma, beta, pos, y, y32, mean, rstd)
        torch.cuda.synchronize()
        assert log == [ln_fwd_name(in_dt, out_dt, D)], log
        within(request, tag + " y", y, ref["y"], b_y)
        s_y.check(y)
        if f32:
            within(request, tag + " y32", y32, ref["y"], b_y32)
            assert bits_equal(y, y32.to(out_dt)), tag + ": y is not the rounded fp32 copy"
            s_32.check(y32)
        if stats:
            within(request, tag + " mean", mean, ref["mean"], b_mean)
            within(request, tag + " rstd", rstd, ref["rstd"], b_rstd)
            s_m.check(mean)
            s_r.check(rstd)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------
def ln_bwd_waves(M, D):
    """csrc/layernorm.hip layernorm_bwd_waves"""
    return 4 if (M < 4096 or 7 * 2 * D * 4 > 64 * 1024) else 8


def ln_bwd_blocks(M, D):
    """csrc/layernorm.hip layernorm_bwd_blocks"""
    nw = ln_bwd_waves(M, D)
    return max(1, min(512 if nw >= 8 else 1024, (M + nw - 1) // nw))


def ln_bwd_name(triple, M, D):
    return f"ln_bwd_kernel<{TN[triple[0]]},{TN[triple[1]]},{TN[triple[2]]},{ln_chunks(D)},{ln_bwd_waves(M, D)}>"


LN_BWD_TRIPLES = [(F32, F32, F32), (BF16, BF16, BF16), (BF16, F32, BF16), (BF16, F32, F32)]  # (dy, x, dx)
TRIPLE_IDS = ["f32", "bf16", "bf16_x32", "bf16_x32_dx32"]


def last_row_weight(M):
    """The last gradient row against the others: its term must stand 10 bounds out of a column sum whose bound grows
    with (M + 64) 2^-24 M."""
    return 8 if M < 4096 else 1024


def ln_bwd_ref(dy, x, gamma, mean, rstd, leave_out_last_group=False):
    dyd, xd, g = dy.double(), x.double(), gamma.double()
    M, D = xd.shape
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    w = torch.ones(D, dtype=F64, device=xd.device)
    if leave_out_last_group:
        w[D - 8:] = 0
    xh = (xd - mu) * rs
    d = dyd * g
    c1 = (d * w).sum(1, keepdim=True) / D
    c2 = (d * xh * w).sum(1, keepdim=True) / D
    out = dict(dx=rs * (d - c1 - xh * c2))
    if leave_out_last_group:
        return out
    out["T"] = rs * (d.abs() + d.abs().mean(1, keepdim=True) + xh.abs() * (d * xh).abs().mean(1, keepdim=True))
    out["T_c1"] = rs * (d.abs() + c1.abs() + xh.abs() * (d * xh).abs().mean(1, keepdim=True))  # (with |c1|: reported only)
    terms = dyd * xh
    out.update(dgamma=terms.sum(0), dbeta=dyd.sum(0), Tg=(dyd.abs() * (xd.abs() + mu.abs()) * rs).sum(0),
               dgamma_last_row_out=terms[:-1].sum(0))
    return out


def ln_bwd_outputs(M, D, dx_dt, dy_dt, dropped, deferred, init_seed=None):
    outs = dict(dx=out_view((M, D), dx_dt), dxd=out_view((M, D), dy_dt) if dropped else (None, None))
    if deferred:
        blocks = k_bwd_blocks(M, D)
        assert blocks == ln_bwd_blocks(M, D), (M, D, blocks)
        outs.update(ws=out_view((blocks * 2 * D,), F32), dg=(None, None), db=(None, None), blocks=blocks)
    else:
        outs.update(ws=(None, ops().workspace(torch.device(DEV))), dg=out_view((D,), F32), db=out_view((D,), F32))
        for k, name in enumerate(("dg", "db")):
            outs[name][1].copy_(values("int", (D,), init_seed + k, F32))
        outs["init"] = (outs["dg"][1].clone().double(), outs["db"][1].clone().double())
    return outs


def ln_bwd_bounded_case(request, triple, M, D, acc, both_forms=True):
    """Gaussian x, integer dy: dx element-wise, dgamma by columns, dbeta exact; immediate form (accumulate as told over
    non-zero dgamma / dbeta) and deferred form (partials [blocks][2][D] left in ws, summed here in fp64)."""
    dy_dt, x_dt, dx_dt = triple
    x = values("gauss", (M, D), 100 + M % 97, F32)
    x[:, D - 8:] += EDGE
    x = rnd(x.to(x_dt))
    dy = values("int", (M, D), 200 + M % 89, F32)
    dy[M - 1] *= last_row_weight(M)
    dy = rnd(dy.to(dy_dt))
    gamma = rnd(values("gauss", (D,), 5, F32))
    gamma[D - 8:] = EDGE
    xd = x.double()
    mean = rnd(xd.mean(1).float())
    rstd = rnd((1.0 / torch.sqrt(xd.var(1, unbiased=False) + LN_EPS)).float())
    ref = ln_bwd_ref(dy, x, gamma, mean, rstd)
    tag = f"M={M} D={D}"
    b_dx = UO[dx_dt] * ref["dx"].abs() + (D + 64) * EPS32 * ref["T"]
    b_dg0 = (M + 64) * EPS32 * ref["Tg"]
    sees(tag + " dx", ln_bwd_ref(dy, x, gamma, mean, rstd, True)["dx"], ref["dx"], b_dx)
    sees(tag + " dgamma", ref["dgamma_last_row_out"], ref["dgamma"], b_dg0)
    name = ln_bwd_name(triple, M, D)
    # immediate
    o = ln_bwd_outputs(M, D, dx_dt, dy_dt, False, False, init_seed=8)
    log = k_ln_bwd(dy, x, gamma, mean, rstd, o["dx"][1], None, o["dg"][1], o["db"][1], acc, None, o["ws"][1])
    torch.cuda.synchronize()
    assert log == [name, "ln_bwd_reduce_kernel"], log
    ig, ib = o["init"]
    within(request, f"{tag} dx", o["dx"][1], ref["dx"], b_dx)
    # (not a criterion: the same error against the bound written with |c1| in place of mean_j |d|, for the record)
    record(request, f"{tag} dx against the bound with |c1| for mean |d| (reported, not asserted)",
           ratio(o["dx"][1], ref["dx"], UO[dx_dt] * ref["dx"].abs() + (D + 64) * EPS32 * ref["T_c1"]), INF)
    within(request, f"{tag} acc={int(acc)} dgamma", o["dg"][1], ref["dgamma"] + (ig if acc else 0.0),
           b_dg0 + (EPS32 * (ig.abs() + ref["dgamma"].abs()) if acc else 0.0))
    exact(request, f"{tag} acc={int(acc)} dbeta", o["db"][1], ref["dbeta"] + (ib if acc else 0.0))
    for k in ("dx", "dg", "db"):
        o[k][0].check(o[k][1])
    if not both_forms:
        return
    # deferred
    q = ln_bwd_outputs(M, D, dx_dt, dy_dt, False, True)
    log = k_ln_bwd(dy, x, gamma, mean, rstd, q["dx"][1], None, None, None, False, None, q["ws"][1])
    torch.cuda.synchronize()
    assert log == [name], log
    assert bits_equal(q["dx"][1], o["dx"][1]), tag + ": dx of the deferred form differs from the immediate form's"
    part = q["ws"][1].view(q["blocks"], 2, D).double().sum(0)
    within(request, f"{tag} deferred dgamma (fp64 sum of {q['blocks']} partials)", part[0], ref["dgamma"], b_dg0)
    exact(request, f"{tag} deferred dbeta", part[1], ref["dbeta"])
    q["dx"][0].check(q["dx"][1])
    q["ws"][0].check(q["ws"][1])


@pytest.mark.parametrize("D", [8, 520, 1032, 2048])
@pytest.mark.parametrize("triple", LN_BWD_TRIPLES, ids=TRIPLE_IDS)
def test_layernorm_bwd_four_wave_route_parity(request, triple, D):
    """M = 1 (three waves own no row and still take part in the LDS combine), 2, 5 (M % 4 != 0: two workgroups, one
    with a single row), 37."""
    for M in (1, 2, 5, 37):
        assert ln_bwd_waves(M, D) == 4
        ln_bwd_bounded_case(request, triple, M, D, acc=M in (2, 37))


LONG_ROWS = ([(t, D, 4096) for t in range(4) for D in (8, 520, 1032)]       # 8 waves, one row per wave
             + [(t, D, 8704) for t in (0, 1) for D in (8, 520, 1032)]       # 17 rows per workgroup: wave 0 takes 3 rounds
             + [(t, 520, 8704) for t in (2, 3)]
             + [(1, 1176, 9000)])                                           # 4 waves, 1024 workgroups of 8-9 rows: 2-3 rounds


@pytest.mark.parametrize("t,D,M", LONG_ROWS, ids=[f"{TRIPLE_IDS[t]}_D{D}_M{M}" for t, D, M in LONG_ROWS])
def test_layernorm_bwd_long_route_parity(request, t, D, M):
    """The 8-wave form (M >= 4096, D <= 1168) with one and with several rows per wave, every dtype triple at every CHUNKS
    (the mixed triples at M = 4096 for D = 8 and 1032 too: without them four of the 24 forms are never launched), and the
    4-wave form with several rows per wave (M = 9000, D = 1176)."""
    assert ln_bwd_waves(M, D) == (4 if D == 1176 else 8)
    ln_bwd_bounded_case(request, LN_BWD_TRIPLES[t], M, D, acc=(D + M // 4096) % 2 == 1)


@pytest.mark.parametrize("M,D", [(37, 8), (37, 512), (37, 2048), (4096, 1024)])
@pytest.mark.parametrize("triple", LN_BWD_TRIPLES, ids=TRIPLE_IDS)
def test_layernorm_bwd_exact(request, triple, M, D):
    """Integer dy, x, mean; power-of-two gamma, rstd, D; dropout p = 0.5: dx, dx_dropped, dgamma, dbeta EQUAL fp64."""
    dy_dt, x_dt, dx_dt = triple
    dy, x = rnd(values("int", (M, D), 1, dy_dt)), rnd(values("int", (M, D), 2, x_dt))
    pick = lambda n, seed, table: torch.tensor(table, dtype=F32, device=DEV)[
        torch.randint(0, len(table), (n,), generator=torch.Generator().manual_seed(seed)).to(DEV)]
    gamma, rstd, mean = rnd(pick(D, 3, [0.5, 1.0, 2.0])), rnd(pick(M, 4, [0.5, 1.0, 2.0])), rnd(pick(M, 5, [-1.0, 0.0, 1.0]))
    p, seed, site, step = 0.5, 4242, 9, 3
    drop = make_drop(p, seed, site, step)
    ref = ln_bwd_ref(dy, x, gamma, mean, rstd)
    dx64 = ref["dx"]
    assert torch.equal(dx64.float().double(), dx64), "the exact row's dx is not representable in fp32"
    # (the column sums too: at most 4096 terms of |dy xh| <= 3 * 8, multiples of 1 / 2)
    if D >= 64:  # the rounding of a bf16 dx is exercised: many exact values are not bf16 numbers
        assert (dx64.float().to(BF16).double() != dx64).double().mean().item() > 0.25
    keep = keep_mask(p, seed, site, step, M * D).view(M, D)
    tag = f"exact M={M} D={D}"
    for acc in (False, True):
        o = ln_bwd_outputs(M, D, dx_dt, dy_dt, True, False, init_seed=8)
        log = k_ln_bwd(dy, x, gamma, mean, rstd, o["dx"][1], o["dxd"][1], o["dg"][1], o["db"][1], acc, drop, o["ws"][1])
        torch.cuda.synchronize()
        assert log == [ln_bwd_name(triple, M, D), "ln_bwd_reduce_kernel"], log
        ig, ib = o["init"]
        exact(request, f"{tag} dx", o["dx"][1], dx64.float().to(dx_dt).double())
        exact(request, f"{tag} dx_dropped", o["dxd"][1], (dx64 * keep).float().to(dy_dt).double())
        exact(request, f"{tag} acc={int(acc)} dgamma", o["dg"][1], ref["dgamma"] + (ig if acc else 0.0))
        exact(request, f"{tag} acc={int(acc)} dbeta", o["db"][1], ref["dbeta"] + (ib if acc else 0.0))
        for k in ("dx", "dxd", "dg", "db"):
            o[k][0].check(o[k][1])


# ---------------------------------------------------------------------------------------------------------------------------
# attention pool
# ---------------------------------------------------------------------------------------------------------------------------
POOL_TYPES = [(F32, F32), (BF16, BF16), (F32, BF16)]  # (features, activations)
POOL_SHAPES = [(1, 1, 8, 0.0), (2, 7, 520, 0.5), (2, 9, 512, 0.0), (1, 513, 1024, 0.5), (1, 1024, 8, 0.0)]


def heavy_positions(N):
    return [N - 1] + ([512] if N > 512 else [])


def pool_inputs(fdt, dtype, B, N, D, p, seed, site, step):
    feat = rnd(values("gauss", (B, N, D), 1, fdt))
    w2 = rnd(values("gauss", (D,), 3, F32) * D ** -0.5)
    b2 = rnd(values("gauss", (1,), 4, F32))
    dpooled = rnd(values("gauss", (B, D), 5, dtype))
    dm = keep_mask(p, seed, site, step, B * N * D).view(B, N, D)
    h = values("gauss", (B, N, D), 2, F32).double()
    heavy = heavy_positions(N)
    if N > 1:  # the heavy positions get the logit that gives each of them 1 / (1 + len(heavy)) of the softmax mass
        wd = w2.double()
        others = torch.ones(N, dtype=torch.bool, device=h.device)
        others[heavy] = False
        logit = (torch.relu(h) * dm * wd).sum(-1) + b2.double()
        want = torch.logsumexp(logit[:, others], 1).clamp_min(1.0)
        for n in heavy:
            t = h[:, n].abs() * torch.sign(wd) + (wd == 0)
            unit = (torch.relu(t) * dm[:, n] * wd).sum(-1)
            h[:, n] = t * ((want - b2.double()) / unit)[:, None]
        # ... and features along dpooled, so that their datt is as large as it can be
        feat[:, heavy] = feat[:, heavy].abs() * (torch.sign(dpooled.float()) + (dpooled == 0))[:, None].to(fdt)
    hpre = rnd(h.to(dtype).view(B * N, D))
    return feat, hpre, w2, b2, dpooled, dm


def pool_fwd_ref(feat, hpre, w2, b2, dm, leave_out=None):
    B, N, D = feat.shape
    f, h, w = feat.double(), hpre.double().view(B, N, D), w2.double()
    act = torch.relu(h) * dm
    logit = (act * w).sum(-1) + b2.double()
    if leave_out is not None:
        logit = logit.clone()
        logit[:, leave_out] = -INF
    att = torch.softmax(logit, 1)
    pooled = (att[..., None] * f).sum(1)
    L = ((act * w).abs().sum(-1) + b2.double().abs()).max(1, keepdim=True).values
    K_att = 2 * (D + 64) * L + (N + 64)
    return dict(att=att, pooled=pooled, b_att=EPS32 * K_att * att, T_pooled=EPS32 * K_att * (att[..., None] * f.abs()).sum(1),
                act=act)


def pool_bwd_ref(feat, hpre, w2, att32, dpooled, dm, act, leave_out=None):
    B, N, D = feat.shape
    f, h, w, a, dp = feat.double(), hpre.double().view(B, N, D), w2.double(), att32.double(), dpooled.double()
    datt = (f * dp[:, None]).sum(-1)
    A = (f * dp[:, None]).abs().sum(-1)
    live = torch.ones(N, dtype=F64, device=f.device)
    if leave_out is not None:
        live[leave_out] = 0
    dot = (a * datt * live).sum(1, keepdim=True)
    dl = a * (datt - dot) * live
    gate = (h > 0).double() * dm
    K = N + D + 128
    E = K * EPS32 * a * (A + (a * A).sum(1, keepdim=True))
    return dict(dl=dl, dh=dl[..., None] * w * gate, E_dh=E[..., None] * w.abs() * gate, dfeat=a[..., None] * dp[:, None],
                dw2=(dl[..., None] * act).sum(1), b_dw2=(N + 64 + K) / K * (E[..., None] * act.abs()).sum(1),
                db2=dl.sum(), b_db2=N * EPS32 * dl.abs().sum())


@pytest.mark.parametrize("B,N,D,p", POOL_SHAPES, ids=[f"B{B}_N{N}_D{D}_p{p}" for B, N, D, p in POOL_SHAPES])
@pytest.mark.parametrize("fdt,dtype", POOL_TYPES, ids=["f32", "bf16", "f32_feat"])
def test_attention_pool_route_parity(request, fdt, dtype, B, N, D, p):
    """N = 1 and 7 (waves without a row), 9, 513 (a second stripe of the 512-thread softmax loops), 1024 (the LDS array
    limit); D = 8, 512, 520 (a second, short column stripe), 1024 (the limit of the LDS partial array)."""
    seed, site, step = 99, 3, 3
    drop = make_drop(p, seed, site, step) if p > 0 else None
    feat, hpre, w2, b2, dpooled, dm = pool_inputs(fdt, dtype, B, N, D, p, seed, site, step)
    tag = f"B={B} N={N} D={D} p={p}"
    ref = pool_fwd_ref(feat, hpre, w2, b2, dm)
    b_pooled32 = ref["T_pooled"]
    b_pooled = UO[dtype] * ref["pooled"].abs() + b_pooled32
    for n in heavy_positions(N):
        assert N == 1 or ref["att"][:, n].min().item() >= 0.25, (tag, n, ref["att"][:, n])
        mut = pool_fwd_ref(feat, hpre, w2, b2, dm, leave_out=n)
        sees(f"{tag} att without position {n}", mut["att"], ref["att"], ref["b_att"])
        sees(f"{tag} pooled without position {n}", mut["pooled"], ref["pooled"], b_pooled)
    s_att, att = out_view((B, N), F32)
    s_p, pooled = out_view((B, D), dtype)
    s_p32, pooled32 = out_view((B, D), F32)
    rc, log = k_pool_fwd(feat, hpre, w2, b2, att, pooled, pooled32, B, N, D, drop)
    torch.cuda.synchronize()
    assert rc == 0 and log == [f"pool_fwd_kernel<{TN[fdt]},{TN[dtype]}>"], (rc, log)
    within(request, tag + " att", att, ref["att"], ref["b_att"])
    within(request, tag + " att row sums", att.double().sum(1), torch.ones(B, dtype=F64, device=att.device), (N + 64) * EPS32)
    within(request, tag + " pooled", pooled, ref["pooled"], b_pooled)
    within(request, tag + " pooled32", pooled32, ref["pooled"], b_pooled32)
    assert bits_equal(pooled, pooled32.to(dtype))
    for s, v in ((s_att, att), (s_p, pooled), (s_p32, pooled32)):
        s.check(v)
    # backward, from the REFERENCE's attention rounded to fp32
    att32 = rnd(ref["att"].float())
    rb = pool_bwd_ref(feat, hpre, w2, att32, dpooled, dm, ref["act"])
    b_dh = UO[dtype] * rb["dh"].abs() + rb["E_dh"]
    b_dfeat = (UO[dtype] + 64 * EPS32) * rb["dfeat"].abs()
    if N > 1:
        for n in heavy_positions(N):
            mut = pool_bwd_ref(feat, hpre, w2, att32, dpooled, dm, ref["act"], leave_out=n)
            sees(f"{tag} dh without position {n}", mut["dh"], rb["dh"], b_dh)
            sees(f"{tag} dw2 without position {n}", mut["dw2"], rb["dw2"], rb["b_dw2"])
    s_dh, dh = out_view((B * N, D), dtype)
    s_df, dfeat = out_view((B * N, D), dtype)
    s_pt, part = out_view((B, 2 * D), F32)
    s_bp, bpart = out_view((B, 16), F32)
    rc, log = k_pool_bwd(feat, hpre, w2, att32, dpooled, dh, dfeat, part, bpart, B, N, D, drop)
    torch.cuda.synchronize()
    assert rc == 0 and log == [f"pool_bwd_kernel<{TN[fdt]},{TN[dtype]}>"], (rc, log)
    within(request, tag + " dh", dh.view(B, N, D), rb["dh"], b_dh)
    within(request, tag + " dfeat", dfeat.view(B, N, D), rb["dfeat"], b_dfeat)
    within(request, tag + " dw2 partials", part[:, :D], rb["dw2"], rb["b_dw2"])
    assert bits_equal(part[:, D:], torch.zeros_like(part[:, D:])) and bits_equal(bpart[:, 1:], torch.zeros_like(bpart[:, 1:]))
    within(request, tag + " sum of the db2 partials", bpart[:, 0].double().sum(), rb["db2"], rb["b_db2"])
    for s, v in ((s_dh, dh), (s_df, dfeat), (s_pt, part), (s_bp, bpart)):
        s.check(v)


@pytest.mark.parametrize("N,D", [(1025, 8), (2, 1032), (2, 12)])
def test_attention_pool_refuses_what_its_lds_arrays_cannot_hold(N, D):
    """N > 1024, D > 1024, D % 8 != 0: the error code, nothing launched, the outputs untouched."""
    B = 1
    feat, hpre = rnd(torch.zeros(B, N, D)), rnd(torch.zeros(B * N, D))
    w2, b2, dpooled = rnd(torch.zeros(D + 8)), rnd(torch.zeros(1)), rnd(torch.zeros(B, D))
    outs = [out_view(s, F32) for s in ((B, N), (B, D), (B, D), (B * N, D), (B * N, D), (B, 2 * D), (B, 16))]
    att, pooled, pooled32, dh, dfeat, part, bpart = (v for _, v in outs)
    rc, log = k_pool_fwd(feat, hpre, w2, b2, att, pooled, pooled32, B, N, D, None)
    assert rc == ERR_UNSUPPORTED and log == [], (rc, log)
    rc, log = k_pool_bwd(feat, hpre, w2, rnd(torch.ones(B, N) / N), dpooled, dh, dfeat, part, bpart, B, N, D, None)
    assert rc == ERR_UNSUPPORTED and log == [], (rc, log)
    for s, _ in outs:
        s.check()


# ---------------------------------------------------------------------------------------------------------------------------
# log-softmax and NLL
# ---------------------------------------------------------------------------------------------------------------------------
LSM_M = 5
# (id, n, ld, view offset by one element)
LSM_CASES = [("row_1024", 1024, 1024, False), ("row_8192", 8192, 8192, False), ("row_padded", 8184, 8192, False),
             ("wave_7", 7, 8, False), ("n1028", 1028, 1028, False), ("wave_8200", 8200, 8200, False),
             ("wave_unaligned", 1024, 1024, True)]


def lsm_rows(dtype, n, ld, *ptrs):
    """csrc/model_ends.hip lsm_rows"""
    v = 8 if dtype == BF16 else 4
    return 1024 <= n <= 8192 and ld <= 8192 and n % v == 0 and ld % v == 0 and all(p % 16 == 0 for p in ptrs)


def lsm_name(direction, dtype, rows):
    return f"log_softmax_{direction}{'_row' if rows else ''}_kernel<{TN[dtype]}>"


@pytest.mark.parametrize("case", LSM_CASES, ids=[c[0] for c in LSM_CASES])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_log_softmax_route_parity(request, dtype, case):
    rid, n, ld, unaligned = case
    M, blk = LSM_M, min(8, n)
    want_rows = {"row_1024": True, "row_8192": True, "row_padded": True, "wave_7": False, "n1028": dtype == F32,
                 "wave_8200": False, "wave_unaligned": False}[rid]
    xs = values("gauss", (M, ld), 1, F32).double()
    if n > blk:  # the last block carries half of the row's mass
        xs[:, n - blk:n] += (torch.logsumexp(xs[:, :n - blk], 1) - torch.logsumexp(xs[:, n - blk:n], 1))[:, None]
    pad = 1 if unaligned else 8
    flat = rnd(torch.cat([torch.zeros(pad, dtype=F64, device=xs.device), xs.reshape(-1),
                          torch.zeros(pad, dtype=F64, device=xs.device)]).to(dtype))
    x = flat[pad:pad + M * ld].view(M, ld)
    xd = x.double()[:, :n]
    mx = xd.max(1, keepdim=True).values
    lse = torch.logsumexp(xd, 1, keepdim=True)
    ref = xd - lse
    b_fwd = (n + 64) * EPS32 * torch.maximum((xd - mx).abs().max(1, keepdim=True).values, lse.abs())
    mut = xd - (torch.logsumexp(xd[:, :n - blk], 1, keepdim=True) if n > blk else torch.full_like(lse, -INF))
    sees(f"{rid} logp", mut, ref, b_fwd)
    s_o, out = out_view((M, n), F32)
    log = k_lsm_fwd(x, n, out)
    torch.cuda.synchronize()
    assert lsm_rows(dtype, n, ld, x.data_ptr(), out.data_ptr()) == want_rows
    assert log == [lsm_name("fwd", dtype, want_rows)], log
    within(request, f"{rid} logp", out, ref, b_fwd)
    s_o.check(out)
    # backward from the reference's logp rounded to fp32
    logp = rnd(ref.float())
    g = values("gauss", (M, n), 2, F32)
    g[:, n - blk:] = g[:, n - blk:].abs() * 16
    g = rnd(g)
    gd, pr = g.double(), torch.exp(logp.double())
    sg, sabs = gd.sum(1, keepdim=True), gd.abs().sum(1, keepdim=True)
    rdx = gd - pr * sg
    b_bwd = UO[dtype] * rdx.abs() + (n + 64) * EPS32 * (gd.abs() + pr * sabs)
    sees(f"{rid} dx", gd - pr * gd[:, :n - blk].sum(1, keepdim=True), rdx, b_bwd)
    s_dx, dx = out_view((M, ld), dtype, pad=pad)
    log = k_lsm_bwd(g, logp, dx)
    torch.cuda.synchronize()
    assert lsm_rows(dtype, n, ld, dx.data_ptr(), g.data_ptr(), logp.data_ptr()) == want_rows
    assert log == [lsm_name("bwd", dtype, want_rows)], log
    within(request, f"{rid} dx", dx[:, :n], rdx, b_bwd)
    assert bits_equal(dx[:, n:], torch.zeros_like(dx[:, n:])), rid + ": padded columns are not exact zeros"
    s_dx.check(dx)


IGNORE = -100


def nll_ref(logp, target, n, leave_out_last=False):
    t = target.clone()
    t[(t < 0) | (t >= n)] = IGNORE
    live = t != IGNORE
    if leave_out_last:
        live = live.clone()
        live[-1] = False
    picked = logp.double().gather(1, t.clamp(0, n - 1)[:, None])[:, 0] * live
    cnt = int(live.sum())
    return dict(loss=-picked.sum() / cnt if cnt else torch.tensor(float("nan"), dtype=F64, device=logp.device),
                bound=logp.shape[0] * EPS32 * picked.abs().sum() / max(cnt, 1), cnt=cnt, live=live, t=t)


@pytest.mark.parametrize("M,n", [(5, 7), (2049, 8), (16385, 8), (300, 1028)])
def test_nll_loss_route_parity(request, M, n):
    """n = 7: the scalar store path through n % 4 != 0 -- at n = 8 and 1028 through a dlogp that is not 16-byte
    aligned; M = 2049: a second trip of the 2048-row target loop; M = 16385:
    rows_per_wg = 8.  Rows 0 and M - 1 have live targets; the others include ignore_index, -1 and n (all three ignored)."""
    g = torch.Generator().manual_seed(M)
    logp = torch.log_softmax(torch.randn(M, n, generator=g, dtype=F64), 1)
    target = torch.randint(0, n, (M,), generator=g)
    target[1::5], target[2::7], target[3::11] = IGNORE, -1, n
    target[0], target[M - 1] = n - 1, 0
    live = (target >= 0) & (target < n)
    live[M - 1] = False
    others = logp.gather(1, target.clamp(0, n - 1)[:, None])[:, 0].abs() * live
    logp[M - 1, 0] = -(4 * others.sum() / live.sum() + 20 * M * EPS32 * others.sum())  # a last row the bound can see
    logp, target = rnd(logp.float()), rnd(target)
    ref = nll_ref(logp, target, n)
    sees(f"M={M} n={n} loss", nll_ref(logp, target, n, True)["loss"], ref["loss"], ref["bound"])
    tag = f"M={M} n={n}"

    def grad_ref(gs):
        sc = torch.tensor(gs, dtype=F32) * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(ref["cnt"]), dtype=F32))
        want = torch.zeros(M, n, dtype=F32, device=logp.device)
        rows = ref["live"].nonzero()[:, 0]
        want[rows, ref["t"][rows]] = -sc.item()
        return want

    for what, gs, acc, l0, pad in (("plain", None, False, 7.0, 8), ("gscale 0.5", 0.5, False, 7.0, 8),
                                   ("accumulate", None, True, 7.0, 8), ("dlogp off 16-byte alignment", None, False, 7.0, 1)):
        s_l, loss = out_view((1,), F32)
        loss.fill_(l0)
        s_g, dlogp = out_view((M, n), F32, pad=pad)
        assert (dlogp.data_ptr() % 16 == 0) == (pad == 8)  # (pad = 1: scalar stores at n % 4 == 0 as well)
        gscale = None if gs is None else rnd(torch.tensor([gs], dtype=F32))
        log = k_nll(logp, target, loss, dlogp, gscale, IGNORE, acc)
        torch.cuda.synchronize()
        assert log == ["nll_loss_kernel"], log
        want = ref["loss"] + (l0 if acc else 0.0)
        within(request, f"{tag} {what} loss", loss.double()[0], want,
               ref["bound"] + (EPS32 * (abs(l0) + ref["loss"].abs()) if acc else 0.0))
        wg = grad_ref(1.0 if gs is None else gs)
        exact(request, f"{tag} {what} dlogp", dlogp, wg.double())
        assert bits_equal(dlogp, wg), f"{tag} {what}: dlogp differs in its bits (a -0.0?)"
        s_l.check(loss)
        s_g.check(dlogp)
    # the loss alone (one workgroup, no gradient)
    s_l, loss = out_view((1,), F32)
    log = k_nll(logp, target, loss, None, None, IGNORE, False)
    torch.cuda.synchronize()
    assert log == ["nll_loss_kernel"], log
    within(request, f"{tag} loss alone", loss.double()[0], ref["loss"], ref["bound"])
    s_l.check(loss)
    # an all-ignored batch: NaN loss, all-zero gradient
    dead = target.clone()
    dead[ref["live"]] = IGNORE
    s_l, loss = out_view((1,), F32)
    s_g, dlogp = out_view((M, n), F32)
    log = k_nll(logp, dead, loss, dlogp, None, IGNORE, False)
    torch.cuda.synchronize()
    assert log == ["nll_loss_kernel"], log
    assert bool(loss.isnan().all()), loss
    assert bits_equal(dlogp, torch.zeros_like(dlogp))
    s_l.check(loss)
    s_g.check(dlogp)


# ---------------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------------
def expected_names_of_the_parity_rows():
    names = {ln_fwd_name(i, o_, D) for i, o_ in LN_FWD_PAIRS for D in LN_FWD_D}
    names |= {ln_bwd_name(t, M, D) for t in LN_BWD_TRIPLES for D in (8, 520, 1032, 2048) for M in (1, 2, 5, 37)}
    names |= {ln_bwd_name(LN_BWD_TRIPLES[t], M, D) for t, D, M in LONG_ROWS}
    names |= {f"pool_{d}_kernel<{TN[f]},{TN[t]}>" for d in ("fwd", "bwd") for f, t in POOL_TYPES}
    for dt in (F32, BF16):
        for rid, n, ld, unaligned in LSM_CASES:
            rows = lsm_rows(dt, n, ld, 1 if unaligned else 0)
            names |= {lsm_name("fwd", dt, rows), lsm_name("bwd", dt, rows)}
    return names | {"nll_loss_kernel"}


def test_the_parity_rows_name_every_rowwise_kernel():
    assert len(set(ALL_ROWWISE)) == len(ALL_ROWWISE) == 48
    assert expected_names_of_the_parity_rows() == set(ALL_ROWWISE)


def test_every_rowwise_kernel_shows_in_a_launch_log():
    """Each entry of ALL_ROWWISE by the smallest call that reaches it (zeros in, nothing compared)."""
    z = lambda shape, dt=F32: rnd(torch.zeros(shape, dtype=dt))
    seen = []
    ws = ops().workspace(torch.device(DEV))
    for D in (8, 520, 1032):
        for i, o_ in LN_FWD_PAIRS:
            seen += k_ln_fwd(z((1, D), i), z(D), z(D), None, z((1, D), o_), None, None, None)
        for dy_dt, x_dt, dx_dt in LN_BWD_TRIPLES:
            for M in (1, 4096):
                seen += k_ln_bwd(z((M, D), dy_dt), z((M, D), x_dt), z(D), z(M), z(M), z((M, D), dx_dt), None, None, None, False,
                                 None, ws)
    for f, t in POOL_TYPES:
        rc, log = k_pool_fwd(z((1, 1, 8), f), z((1, 8), t), z(8), None, z((1, 1)), z((1, 8), t), None, 1, 1, 8, None)
        assert rc == 0
        seen += log
        rc, log = k_pool_bwd(z((1, 1, 8), f), z((1, 8), t), z(8), z((1, 1)), z((1, 8), t), z((1, 8), t), z((1, 8), t), z((1, 16)),
                             z((1, 16)), 1, 1, 8, None)
        assert rc == 0
        seen += log
    for dt in (F32, BF16):
        for n in (8, 1024):
            seen += k_lsm_fwd(z((1, n), dt), n, z((1, n)))
            seen += k_lsm_bwd(z((1, n)), z((1, n)), z((1, n), dt))
    seen += k_nll(z((1, 8)), rnd(torch.zeros(1, dtype=torch.int64)), z(1), None, None, IGNORE, False)
    torch.cuda.synchronize()
    assert set(seen) == set(ALL_ROWWISE), {"never launched": sorted(set(ALL_ROWWISE) - set(seen)),
                                           "not in the list": sorted(set(seen) - set(ALL_ROWWISE))}
