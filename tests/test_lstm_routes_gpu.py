"""LSTM recurrence kernels (csrc/lstm.hip), step by step against fp64, by the form that runs.

Two routes: the persistent pair ``lstm_fwd_persistent_kernel`` / ``lstm_bwd_persistent_kernel`` (bf16, I = H = 512, whole
sample groups of 16; route "mfma") and one launch per time step of ``lstm_step_fwd_simple<T>`` / ``lstm_step_bwd_simple<T>``
(everything else and the fp32 mode; route "simple").  Each persistent launch has ``lstm_sentinel_fill_kernel`` in front
of it (the 0xFF fill of the exchange buffer).  ALL_LSTM is the literal kernel list; tests/test_lstm_table_cpu.py checks it
against the kernel symbols of the built library.

The reference is STEP-LOCAL ("teacher-forced"): step t is recomputed in fp64 from the exact values the kernel itself
produced for step t - 1 (forward: its ``hseq[t]`` and its saved c_{t-1}; backward: its saved gates, its own ``dgates[t+1]``
for the recurrent term, the carried dc in fp64 inside the reference).  One bf16 flip of h_{t-1} then no longer moves every
later step, and the bars are those of the number formats:

  forward   i, f, g, o, c_t (decoded from ``saved``) and y[:, t]: ``rel_max`` per (step, quantity) <= tol(F32) = 1e-4;
            hseq[t+1] and y_lp are y[:, t] cast to the compute dtype, bit for bit; block 0 of hseq is exactly zero.
  backward  dgates[t] elementwise: |got - ref| <= U |ref| + tol(F32) s_t, U = 2^-8 for bf16 (the half-ulp of the stored
            value; 0 for fp32), s_t = max(max |dh_t|, max |dc_t|) of the reference over the step.

Every bar is first shown to see a realistic bug (``assert_bars_see_bugs``), in fp64 on the row's own inputs along the
free-running fp64 trajectory, no kernel value involved: a K step of h W_hh left out, a stale h or c, b_hh left out (forward,
each moves h_t by >= 10 bars at every t >= 1); 32 columns of gate g left out of dgates[t+1] W_hh, the dc carry dropped, a
stale c in d_f (backward, each >= 10 bars elementwise; the same columns of each other gate: more than one bar).  Where a shape has no 32-wide K step (H <= 32) a quarter of the
reduction is left out instead.  The free-running comparison of tests/test_kernels_gpu.py (``_lstm_ref64``, its bars) stays
as a second, coarse check.

``saved`` is decoded by one function per route with the layout quoted from the kernel (``decode_persistent``,
``decode_simple``); a padded / chunked batch chunk by chunk.  Every persistent row runs behind a decoy call of the same
shape on other inputs whose outputs are freed first, so that the caching allocator hands the real call blocks that hold
a previous call's h / dgates / saved values: a consumer that read them would not be bit-identical to anything.
"""
import os

import pytest
import torch

from test_kernels_gpu import BF16, DEV, F32, FORCED_SIMPLE, _lstm_ref64, nerr, rel_l2, tol

pytestmark = pytest.mark.gpu

LH = 512        # hidden (and input) size of the persistent kernels
NUB = LH // 16  # workgroups per sample group
U_BF16 = 2.0 ** -8  # bf16 keeps 8 significand bits: a correctly rounded value is within 2^-8 relative
BAR = tol(F32)
Q = ("i", "f", "g", "o", "c")

ALL_LSTM = [
    "lstm_fwd_persistent_kernel", "lstm_bwd_persistent_kernel", "lstm_sentinel_fill_kernel",
    "lstm_step_fwd_simple<bf16>", "lstm_step_fwd_simple<float>",
    "lstm_step_bwd_simple<bf16>", "lstm_step_bwd_simple<float>",
]


def ops():
    from openvivqa_amd import ops as o
    return o


def rnd(*shape, dtype=F32, scale=1.0, seed=0, uniform=False, device=None):
    g = torch.Generator().manual_seed(seed + sum(shape))
    r = torch.rand(*shape, generator=g) * 2 - 1 if uniform else torch.randn(*shape, generator=g)
    return (r * scale).to(dtype).to(device or DEV)


@pytest.fixture(autouse=True)
def _red_zones(request, monkeypatch):
    """Guard bands (tests/redzone.py) around what ops allocates and what this module's rnd() makes, as in the kernel tests.
    Yields the RedZone (None when switched off): the decoy calls check and release their buffers through it."""
    if os.environ.get("OVQA_TEST_REDZONE", "1") == "0" or not torch.cuda.is_available():
        yield None
        return
    import redzone
    rz = redzone.install(monkeypatch, request.module)
    yield rz
    torch.cuda.synchronize()
    rz.check()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def record(request, what, value, bar):
    from conftest import parity_record
    return parity_record(request.node.nodeid, what, value, bar)


def _d(t):
    return t.detach().double().cpu()


def rel_max(a, ref):
    """max |a - ref| / max |ref| (the reference's own scale, no floor); NaN when either side holds one."""
    a, ref = _d(a), _d(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return ((a - ref).abs().max() / ref.abs().max()).item()


# ---------------------------------------------------------------------------------------------------- inputs
class Case:
    """One row's operands.  ``x`` is [T*B, I] time-major, a column view of a [T*B, ldx] buffer when ldx > I."""

    def __init__(self, B, T, I, H, dtype, dy_dtype=F32, ldx=None, seed=0, kind="plain", device=None, x_offset=0):
        self.B, self.T, self.I, self.H, self.dtype, self.kind = B, T, I, H, dtype, kind
        s = H ** -0.5
        xs, ws = (3.0, 4.0) if kind == "scaled" else (1.0, 1.0)  # saturation row: weights x 4, inputs x 3
        self.x = rnd(T * B, I, dtype=dtype, scale=xs, seed=seed, device=device)
        if (ldx or I) > I:  # the same values, as a column view of a wider buffer
            wide = rnd(T * B, ldx, dtype=dtype, seed=seed + 6, device=device)
            wide[:, x_offset:x_offset + I].copy_(self.x)
            self.x = wide[:, x_offset:x_offset + I]
        self.w_ih = rnd(4 * H, I, dtype=dtype, scale=s * ws, seed=seed + 1, uniform=True, device=device)
        self.w_hh = rnd(4 * H, H, dtype=dtype, scale=s * ws, seed=seed + 2, uniform=True, device=device)
        b_ih = rnd(4 * H, scale=s, seed=seed + 3, uniform=True, device="cpu")
        if kind == "biased":  # saturation row: +-100 on eight units of every gate
            units = torch.linspace(0, H - 1, 8).long()
            for gate in range(4):
                for k, u in enumerate(units.tolist()):
                    b_ih[gate * H + u] += 100.0 if (k + gate) % 2 == 0 else -100.0
        self.b_ih = rnd(4 * H, seed=seed + 3, device=device).copy_(b_ih)
        self.b_hh = rnd(4 * H, scale=s, seed=seed + 4, uniform=True, device=device)
        self.dy = rnd(B, T, H, dtype=dy_dtype, seed=seed + 5, device=device)

    def wt(self, ldwt=None):
        """The transposed bf16 copy of W_hh [H, 4H], rows strided by ``ldwt`` (None in fp32 mode)."""
        if self.dtype != BF16:
            return None
        H = self.H
        buf = rnd(H, ldwt or 4 * H, dtype=BF16, seed=99, device=self.w_hh.device)
        view = buf[:, :4 * H] if (ldwt or 4 * H) > 4 * H else buf
        view.copy_(self.w_hh.t())
        return view


# ---------------------------------------------------------------------------------------------------- fp64 steps
def fwd_step64(xt, h_in, c_in, wi, wh, bi, bh):
    """One step of torch.nn.LSTM's cell in fp64 (gate order i, f, g, o) -> dict of i, f, g, o, c, h [B, H]."""
    pre = xt @ wi.t() + bi + h_in @ wh.t() + bh
    i, f, g, o = pre.chunk(4, -1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_in + i * g
    return dict(i=i, f=f, g=g, o=o, c=c, h=o * torch.tanh(c))


def bwd_step64(dy_t, dg_next, wh, i, f, g, o, c, cp, carry, cp_df=None):
    """One step of the backward recurrence in fp64: dgates [B, 4H] (columns gate*H + unit), dh, dc, the carried dc * f.
    ``dg_next`` = dgates of step t + 1 (None at the last step); ``cp_df``: another c_{t-1} for d_f alone (planted bug)."""
    dh = dy_t if dg_next is None else dy_t + dg_next @ wh
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc) + carry
    dg = torch.cat([dc * g * i * (1 - i), dc * (cp if cp_df is None else cp_df) * f * (1 - f), dc * i * (1 - g * g),
                    dh * tc * o * (1 - o)], -1)
    return dg, dh, dc, dc * f


def bwd_bar(ref, dh, dc, u):
    return u * ref.abs() + BAR * max(dh.abs().max().item(), dc.abs().max().item())


def _operands64(case):
    T, B = case.T, case.B
    return (_d(case.x).view(T, B, case.I), _d(case.w_ih), _d(case.w_hh), _d(case.b_ih), _d(case.b_hh),
            _d(case.dy).transpose(0, 1))  # dy [T, B, H], in the values of the dtype the kernel reads


def _round(t, dtype):
    return t.to(dtype).double() if dtype != F32 else t


def kcut(H):
    """Columns a planted 'short reduction' leaves out: one 32-wide MFMA K step, or a quarter of a reduction that has none."""
    return 32 if H > 32 else max(1, H // 4)


_SEEN = {}


def assert_bars_see_bugs(case, key=None):
    """Each bar against each planted bug, in fp64 along the free-running trajectory of the row's own inputs (h and dgates
    rounded to the compute dtype where the kernels store them).  Returns the minima over the steps, in bars; shared between
    rows of equal inputs."""
    if key is not None and key in _SEEN:
        return _SEEN[key]
    x, wi, wh, bi, bh, dy = _operands64(case)
    T, B, H, k = case.T, case.B, case.H, kcut(case.H)
    zero = torch.zeros(B, H, dtype=torch.float64)
    hs, cs, st = [zero], [zero], []  # hs[t] = operand of step t (h_{t-1}), cs[t] = c_{t-1}
    worst = {n: float("inf") for n in ("fwd K step", "fwd stale h", "fwd no b_hh", "fwd stale c",
                                       "bwd K step", "bwd no carry", "bwd stale c")}
    for t in range(T):
        ref = fwd_step64(x[t], hs[t], cs[t], wi, wh, bi, bh)
        if t >= 1:
            short = hs[t].clone()
            short[:, H - k:] = 0
            bugs = {"fwd K step": fwd_step64(x[t], short, cs[t], wi, wh, bi, bh),
                    "fwd stale h": fwd_step64(x[t], hs[t - 1], cs[t], wi, wh, bi, bh),
                    "fwd no b_hh": fwd_step64(x[t], hs[t], cs[t], wi, wh, bi, 0 * bh),
                    "fwd stale c": fwd_step64(x[t], hs[t], cs[t - 1], wi, wh, bi, bh)}
            for name, bug in bugs.items():
                moved = rel_max(bug["h"], ref["h"])
                assert moved >= 10 * BAR, (name, t, moved)
                worst[name] = min(worst[name], moved / BAR)
        st.append(ref)
        hs.append(_round(ref["h"], case.dtype))
        cs.append(ref["c"])
    u = U_BF16 if case.dtype == BF16 else 0.0
    dg_next, carry = None, zero
    for t in reversed(range(T)):
        s = st[t]
        args = (s["i"], s["f"], s["g"], s["o"], s["c"], cs[t])
        ref, dh, dc, carry_out = bwd_step64(dy[t], dg_next, wh, *args, carry)
        bar = bwd_bar(ref, dh, dc, u)
        bugs = {}
        if t < T - 1:
            for gate in range(4):
                short = dg_next.clone()
                short[:, gate * H + H - k:(gate + 1) * H] = 0
                bugs[f"bwd K step/{gate}"] = bwd_step64(dy[t], short, wh, *args, carry)[0]
            bugs["bwd no carry"] = bwd_step64(dy[t], dg_next, wh, *args, zero)[0]
        if t >= 1:
            bugs["bwd stale c"] = bwd_step64(dy[t], dg_next, wh, *args, carry, cp_df=cs[t - 1])[0]
        for name, bug in bugs.items():
            ratio = ((bug - ref).abs() / bar).max().item()
            if name.startswith("bwd K step/") and name != "bwd K step/2":
                # the 10 x is asked of ONE gate: g, wave 2's, whose gradient dc i (1 - g^2) is the largest of the four (d_f
                # carries a factor c_{t-1}, d_o a factor tanh c: in bf16 their lost columns show at 5 .. 30 bars).  The
                # other three must still leave the bar, i.e. fail the comparison
                assert ratio > 1, (name, t, ratio)
                continue
            assert ratio >= 10, (name, t, ratio)
            worst[name.split("/")[0]] = min(worst[name.split("/")[0]], ratio)
        dg_next, carry = _round(ref, case.dtype), carry_out
    if key is not None:
        _SEEN[key] = worst
    return worst


# ---------------------------------------------------------------------------------------------------- ``saved``
def wg_role(b, nsg):
    """csrc/lstm.hip ``wg_role``: block -> (sample group, unit block)."""
    if nsg <= 8 and 8 % nsg == 0:
        per, xcd, idx = 8 // nsg, b % 8, b // 8
        return xcd // per, idx * per + xcd % per
    return b // NUB, b % NUB


def decode_persistent(saved, B, T):
    """``float* saved;  // [T][nwg][5][256]: i, f, g, o (post-activation), c_t of the workgroup's lanes``; block b is
    (sg, ub) = wg_role(b, B / 16); thread tid = w*64 + q*16 + n holds sample sg*16 + n, unit ub*16 + w*4 + q
    (``const int unit = ub * 16 + w * 4 + q;  // this lane's hidden unit; its sample is sg * 16 + n``).  -> [5, T, B, 512]."""
    nsg = B // 16
    nwg = nsg * NUB
    f = saved.view(torch.float32).cpu()[:T * nwg * 5 * 256].view(T, nwg, 5, 256)
    tid = torch.arange(256)
    w, q, n = tid >> 6, (tid >> 4) & 3, tid & 15
    out = torch.full((5, T, B, LH), float("nan"))
    for b in range(nwg):
        sg, ub = wg_role(b, nsg)
        out[:, :, sg * 16 + n, ub * 16 + w * 4 + q] = f[:, b].permute(1, 0, 2)
    return out


def decode_simple(saved, B, T, H):
    """``saved = post-activation gates [T*B][4H] fp32 followed by c [T*B][H] fp32`` -> [5, T, B, H]."""
    f = saved.view(torch.float32).cpu()
    gates = f[:T * B * 4 * H].view(T, B, 4, H).permute(2, 0, 1, 3)
    c = f[T * B * 4 * H:T * B * 5 * H].view(1, T, B, H)
    return torch.cat([gates, c], 0)


def decode_saved(saved, route, B, T, H):
    """i, f, g, o, c as [5, T, B, H] fp32 on the CPU; an ``ops.LstmChunks`` is decoded chunk by chunk with B = bp."""
    one = (lambda s, b: decode_persistent(s, b, T)) if route == "mfma" else (lambda s, b: decode_simple(s, b, T, H))
    if isinstance(saved, list):
        return torch.cat([one(sc, bp)[:, :, :b1 - b0] for b0, b1, bp, sc in saved], 2)
    return one(saved, B)


def decode_mock(saved, H):
    """tests/mock_ops.lstm_fwd: [T, B, 5H] = i, f, g, o, c side by side."""
    T, B = saved.shape[:2]
    return saved.view(T, B, 5, H).permute(2, 0, 1, 3).float()


# ---------------------------------------------------------------------------------------------------- the checker
def check_forward(case, y, hseq, dec, y_lp=None, rec=None):
    """Every step from the implementation's own h_{t-1} (hseq[t]) and c_{t-1} (decoded ``saved``)."""
    x, wi, wh, bi, bh, _ = _operands64(case)
    T, B, H = case.T, case.B, case.H
    hs, dec64, y64 = _d(hseq).view(T + 1, B, H), _d(dec), _d(y)
    assert float(hs[0].abs().max()) == 0.0, "block 0 of hseq must be exactly zero"
    worst = dict.fromkeys(Q + ("y",), 0.0)
    for t in range(T):
        ref = fwd_step64(x[t], hs[t], dec64[4, t - 1] if t else torch.zeros(B, H, dtype=torch.float64), wi, wh, bi, bh)
        for qi, name in enumerate(Q):
            e = rel_max(dec64[qi, t], ref[name])
            assert e <= BAR, (name, t, e)
            worst[name] = max(worst[name], e)
        e = rel_max(y64[:, t], ref["h"])
        assert e <= BAR, ("y", t, e)
        worst["y"] = max(worst["y"], e)
    yc = y.detach().cpu()
    assert torch.equal(hseq.detach().cpu().view(T + 1, B, H)[1:].transpose(0, 1), yc.to(hseq.dtype)), "hseq[t+1] != cast(y[:, t])"
    if y_lp is not None:
        assert y_lp.dtype == case.dtype and torch.equal(y_lp.detach().cpu(), yc.to(case.dtype)), "y_lp != cast(y)"
    if rec:
        for name, e in worst.items():
            rec(f"fwd step-local {name}", e, BAR)
    return worst


def check_backward(case, dec, dgates, rec=None):
    """Every step from the decoded ``saved``, dy as read, and the implementation's own dgates[t+1]."""
    _, _, wh, _, _, dy = _operands64(case)
    T, B, H = case.T, case.B, case.H
    assert dgates.dtype == case.dtype
    u = U_BF16 if dgates.dtype == BF16 else 0.0
    dg, dec64 = _d(dgates).view(T, B, 4 * H), _d(dec)
    zero = torch.zeros(B, H, dtype=torch.float64)
    carry, worst = zero, 0.0
    for t in reversed(range(T)):
        ref, dh, dc, carry = bwd_step64(dy[t], dg[t + 1] if t < T - 1 else None, wh, *dec64[:5, t],
                                        dec64[4, t - 1] if t else zero, carry)
        ratio = ((dg[t] - ref).abs() / bwd_bar(ref, dh, dc, u)).max().item()
        assert ratio <= 1.0, ("dgates", t, ratio)
        worst = max(worst, ratio)
    if rec:
        rec("bwd step-local dgates err/bar", worst, 1.0)
    return worst


def check_saturation(case, hseq, dec, dgates):
    """Gates the fp64 step rounds to 0 / 1 / +-1 in fp32 -- with a factor 2 to spare, so that an error of a few ulp in the
    fast exponential cannot decide the rounding: 1 - |v| <= 2^-26, v <= 2^-151 -- must be exactly there, and their dgates
    exactly zero.  -> the number of saturated gate values."""
    x, wi, wh, bi, bh, _ = _operands64(case)
    T, B, H = case.T, case.B, case.H
    hs, dec64, dg = _d(hseq).view(T + 1, B, H), _d(dec), _d(dgates).view(T, B, 4, H)
    for name, t in (("hseq", hseq), ("saved", dec), ("dgates", dgates)):
        assert torch.isfinite(t.float()).all(), name
    count = 0
    for t in range(T):
        ref = fwd_step64(x[t], hs[t], dec64[4, t - 1] if t else torch.zeros(B, H, dtype=torch.float64), wi, wh, bi, bh)
        for qi, name in enumerate(Q[:4]):
            r, got = ref[name], dec64[qi, t]
            for const, where in ((1.0, 1 - r <= 2.0 ** -26), (-1.0, 1 + r <= 2.0 ** -26), (0.0, r.abs() <= 2.0 ** -151)):
                if name != "g" and const < 0 or name == "g" and const == 0:
                    continue
                assert bool((got[where] == const).all()), (name, t, const)
                assert bool((dg[t, :, qi][where] == 0).all()), ("dgates of a saturated gate", name, t, const)
                count += int(where.sum())
    return count


# ---------------------------------------------------------------------------------------------------- running a row
def run_lstm(case, want_lp, wt, route, chunks=1):
    """ops.lstm_fwd + ops.lstm_bwd; asserts the route and the launches (skipped under OVQA_FORCE_SIMPLE) and, on the
    persistent route, both scratch status words and the process status word."""
    from openvivqa_amd import _lib
    o, B, T, H = ops(), case.B, case.T, case.H
    _lib.launch_log_clear()
    res = o.lstm_fwd(case.x, case.w_ih, case.w_hh, case.b_ih, case.b_hh, B, T, want_lp=want_lp)
    got_route, log_f = _lib.last_dispatch(), _lib.launch_log()
    y, hseq, saved, scratch = res[:4]
    _lib.launch_log_clear()
    dgates, scratch_b = o.lstm_bwd(case.dy, case.w_hh, wt, saved, B, T, case.I)
    log_b = _lib.launch_log()
    assert _lib.last_dispatch() == got_route, "forward and backward of one sequence took different routes"
    torch.cuda.synchronize()
    if not FORCED_SIMPLE:
        assert got_route == route
        t = "bf16" if case.dtype == BF16 else "float"
        if route == "mfma":
            assert log_f == ["lstm_sentinel_fill_kernel", "lstm_fwd_persistent_kernel"] * chunks, log_f
            assert log_b == ["lstm_sentinel_fill_kernel", "lstm_bwd_persistent_kernel"] * chunks, log_b
        else:
            assert log_f == [f"lstm_step_fwd_simple<{t}>"] * T, log_f
            assert log_b == [f"lstm_step_bwd_simple<{t}>"] * T, log_b
    if got_route == "mfma":  # no hand-off wait of the persistent launches gave up
        assert int(scratch.view(torch.int32)[1000]) == 0 and int(scratch_b.view(torch.int32)[1000]) == 0
        assert o.lstm_status(raise_on_error=False) == 0
    return dict(y=y, hseq=hseq, saved=saved, dgates=dgates, y_lp=res[4] if want_lp else None, route=got_route)


def with_decoy(rz, make_case, run):
    """A call of the same shape on other inputs first; its buffers (outputs, saved, scratch) are checked and released
    before the real call allocates."""
    keep = list(rz.live) if rz is not None else []
    run(make_case(1000))
    torch.cuda.synchronize()
    if rz is not None:
        rz.check()
        rz.live.extend(keep)


def check_row(request, case, out, coarse=True):
    rec = lambda what, v, bar: record(request, what, v, bar)
    dec = decode_saved(out["saved"], out["route"], case.B, case.T, case.H)
    assert torch.isfinite(dec).all(), "saved holds a value no lane wrote, or a NaN"
    check_forward(case, out["y"], out["hseq"], dec, out["y_lp"], rec)
    check_backward(case, dec, out["dgates"], rec)
    if coarse:  # free-running fp64, the bars of tests/test_kernels_gpu.py::test_lstm_fwd_bwd
        B, T, H, lo = case.B, case.T, case.H, case.dtype == BF16
        y64, dg64, _ = _lstm_ref64(case.x, case.w_ih, case.w_hh, case.b_ih, case.b_hh, case.dy.float(), B, T, round_ops=lo)
        e = [nerr(out["y"], y64), nerr(out["hseq"][B:].float().view(T, B, H).transpose(0, 1), y64),
             rel_l2(out["dgates"].float(), dg64)]
        for what, v, bar in zip(("free-running y", "free-running hseq", "free-running dgates"), e,
                                (2e-3, 8e-3, 6e-3) if lo else (1e-5, 1e-5, 1e-5)):
            rec(what, v, bar)
            assert v < bar, (what, v)
    return dec


def max_batch():
    from openvivqa_amd import _lib
    return int(_lib.load().ovqa_lstm_persistent_max_batch())


def _needs_groups(B):
    """Skip -- never pass -- a persistent row whose sample groups this device cannot keep co-resident."""
    if not FORCED_SIMPLE and -(-B // 16) * 16 > max_batch():
        pytest.skip(f"{-(-B // 16)} sample groups need {-(-B // 16) * NUB} CUs, the device has {cus()}")


def _persistent_row(request, rz, B, T, dy_dtype=BF16, want_lp=True, ldx=LH, ldwt=4 * LH, chunks=1, kind="plain", coarse=True):
    make = lambda seed: Case(B, T, LH, LH, BF16, dy_dtype, ldx=ldx, seed=seed, kind=kind)
    if kind == "plain":
        record(request, "planted bugs, min over steps", min(assert_bars_see_bugs(
            Case(B, T, LH, LH, BF16, dy_dtype, device="cpu"), key=(B, T, dy_dtype)).values()), 10.0)
    case = make(0)
    wt = case.wt(ldwt)
    with_decoy(rz, make, lambda c: run_lstm(c, want_lp, c.wt(ldwt), "mfma", chunks))
    out = run_lstm(case, want_lp, wt, "mfma", chunks)
    return case, out, check_row(request, case, out, coarse)


# ---------------------------------------------------------------------------------------------------- persistent rows
@pytest.mark.parametrize("B,T", [(16, 1), (16, 2), (32, 3), (64, 20), (112, 2), (128, 2), (5, 3), (24, 2)])
def test_persistent_rows(request, _red_zones, B, T):
    """One, two, seven and eight sample groups, T = 1 (no hand-off, cprev = 0) and T = 2 (no t + 2 prefetch), the workload
    shape, and ragged batches padded to whole groups; dy bf16 and want_lp as functional._LSTM calls the kernels."""
    _needs_groups(B)
    _persistent_row(request, _red_zones, B, T)


def test_persistent_chunked_batch(request, _red_zones):
    """max_batch + 8 samples: one full chunk and one padded chunk of a single group."""
    B = max_batch() + 8
    _persistent_row(request, _red_zones, B, 2, chunks=1 if FORCED_SIMPLE else 2)


@pytest.mark.parametrize("ldwt", [4 * LH, 4 * LH + 8])
@pytest.mark.parametrize("ldx", [LH, LH + 8])
@pytest.mark.parametrize("want_lp", [False, True], ids=["no_lp", "lp"])
@pytest.mark.parametrize("dy_dtype", [F32, BF16], ids=["dy32", "dy16"])
@pytest.mark.parametrize("B", [16, 48])
def test_persistent_arguments_crossed(request, _red_zones, B, dy_dtype, want_lp, ldx, ldwt):
    """One group and three groups (wg_role's else-branch) at T = 3 under every combination of the arguments the C ABI takes:
    dy fp32 / bf16, with / without the bf16 twin of y, x rows and W_hh^T rows contiguous or strided."""
    _needs_groups(B)
    _persistent_row(request, _red_zones, B, 3, dy_dtype, want_lp, ldx, ldwt)


# ---------------------------------------------------------------------------------------------------- per-step rows
SIMPLE_ROWS = [(3, 5, 32, 32, F32), (5, 8, 40, 24, F32), (2, 2, 24, 40, F32), (4, 1, 16, 8, F32),
               (3, 5, 32, 32, BF16), (5, 8, 40, 24, BF16), (2, 2, 24, 40, BF16), (4, 1, 16, 8, BF16), (3, 4, 512, 256, BF16)]


@pytest.mark.parametrize("want_lp", [False, True], ids=["no_lp", "lp"])
@pytest.mark.parametrize("dy_dtype", [F32, BF16], ids=["dy32", "dy16"])
@pytest.mark.parametrize("B,T,I,H,dtype", SIMPLE_ROWS)
def test_per_step_rows(request, B, T, I, H, dtype, dy_dtype, want_lp):
    """The per-step kernels with I != H (both ways round), B * H not a multiple of the block, T = 1 and 2, x rows strided."""
    record(request, "planted bugs, min over steps", min(assert_bars_see_bugs(
        Case(B, T, I, H, dtype, dy_dtype, device="cpu"), key=(B, T, I, H, dtype, dy_dtype)).values()), 10.0)
    case = Case(B, T, I, H, dtype, dy_dtype, ldx=I + (1 if dtype == F32 else 8))
    out = run_lstm(case, want_lp, case.wt(), "simple")
    check_row(request, case, out)


# ---------------------------------------------------------------------------------------------------- saturation
@pytest.mark.parametrize("kind", ["scaled", "biased"])
@pytest.mark.parametrize("B,T,H,dtype", [(16, 3, 512, BF16), (3, 5, 32, BF16), (3, 5, 32, F32)])
def test_saturated_gates(request, _red_zones, B, T, H, dtype, kind):
    """``scaled``: weights x 4 and inputs x 3 (pre-activations of some tens); ``biased``: +-100 on b_ih of eight units of
    every gate (exp overflows to inf inside the fast sigmoid / tanh).  Everything finite, the step-local bars hold, the
    saturated gates are exactly 0 / 1 / +-1 and their gradients exactly 0.  (The free-running comparison is left out: its
    bars are for the unit-scale operands of the other rows.)"""
    if H == LH:
        _needs_groups(B)
        case, out, dec = _persistent_row(request, _red_zones, B, T, kind=kind, coarse=False)
    else:
        case = Case(B, T, H, H, dtype, BF16, kind=kind)
        out = run_lstm(case, True, case.wt(), "simple")
        dec = check_row(request, case, out, coarse=False)
    assert torch.isfinite(out["y"]).all()
    n = check_saturation(case, out["hseq"], dec, out["dgates"])
    # biased: per (step, sample) the 16 gate values at +100 and the four g at -100 (sigmoid(-100) = 3.7e-44 is still an fp32
    # denormal: not "rounded to 0", though the fast form gives exactly 0 there, which the step-local bar accepts)
    assert n >= (T * B * 20 if kind == "biased" else 1), n


# ---------------------------------------------------------------------------------------------------- state between calls
def test_graph_replays_on_new_inputs_equal_eager(_red_zones):
    """lstm_fwd + lstm_bwd at (16, 3) captured once (a linear graph, one stream) and replayed on two other inputs copied into
    the static buffers: each replay equals the eager call on those inputs bit for bit -- the sentinel fill and every
    hand-off are part of the graph, nothing is left over from the capture or the previous replay."""
    B, T = 16, 3
    o = ops()
    cases = [Case(B, T, LH, LH, BF16, BF16, seed=s) for s in (0, 50, 90)]
    wt = cases[0].wt()

    def call(x, dy):
        y, hseq, saved, _, y_lp = o.lstm_fwd(x, cases[0].w_ih, cases[0].w_hh, cases[0].b_ih, cases[0].b_hh, B, T, want_lp=True)
        dg, _ = o.lstm_bwd(dy, cases[0].w_hh, wt, saved, B, T, LH)
        return y, hseq, saved, y_lp, dg
    eager = [[t.clone() for t in call(c.x, c.dy)] for c in cases]
    torch.cuda.synchronize()
    assert not torch.equal(eager[1][0], eager[2][0])
    x_s, dy_s = cases[0].x.clone(), cases[0].dy.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        static = call(x_s, dy_s)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for c, want in zip(cases[1:], eager[1:]):
        x_s.copy_(c.x)
        dy_s.copy_(c.dy)
        g.replay()
        torch.cuda.synchronize()
        for name, got, w in zip(("y", "hseq", "saved", "y_lp", "dgates"), static, want):
            assert torch.equal(got, w), f"{name}: the replay differs from the eager call"
    if not FORCED_SIMPLE:
        assert o.lstm_status(raise_on_error=False) == 0


# ---------------------------------------------------------------------------------------------------- loud errors
@pytest.mark.skipif(FORCED_SIMPLE, reason="the argument checks of the persistent route")
def test_persistent_route_rejects_what_it_cannot_index():
    """bf16, H = 512: x rows that are not 16-byte aligned (ldx = 516, or a base 8 bytes off) and W_hh^T rows with
    ldwt = 2052 raise; the call does not fall back to the per-step kernels."""
    from openvivqa_amd import _lib
    B, T, o = 16, 2, ops()
    case = Case(B, T, LH, LH, BF16, BF16)
    args = (case.w_ih, case.w_hh, case.b_ih, case.b_hh, B, T)
    _lib.launch_log_clear()
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        o.lstm_fwd(Case(B, T, LH, LH, BF16, ldx=LH + 4).x, *args)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        o.lstm_fwd(Case(B, T, LH, LH, BF16, ldx=LH + 8, x_offset=4).x, *args)
    assert _lib.launch_log() == []
    saved = o.lstm_fwd(case.x, *args)[2]
    _lib.launch_log_clear()
    with pytest.raises(RuntimeError, match="transposed w_hh copy"):
        o.lstm_bwd(case.dy, case.w_hh, case.wt(4 * LH + 4), saved, B, T, LH)
    assert _lib.launch_log() == []
