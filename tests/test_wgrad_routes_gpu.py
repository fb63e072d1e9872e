"""Route-table parity of the PARAMETER-gradient kernels against fp64 math: the weight-gradient GEMMs (single, grouped
register-staged, grouped direct-to-LDS, the plain-store branch of the fused dW + Adam kernel, the VALU fallback), the bias
gradient (``colsum_bf16_kernel``) and the LayerNorm dgamma / dbeta partial reduces.  tests/test_adam_gpu.py has the optimiser.

Style of tests/test_kernel_routes_gpu.py: every row names the entry point, the shape and the kernel the launch log must
show; references are fp64 torch on the same operands (never another HIP kernel); every compared quantity goes through
``parity_record``.

Two inputs per row, two kinds of bar:
  * INTEGER operands in [-3, 3] (and integer initial dw / db on accumulate rows): every product and every partial sum, in
    any order, is an integer below 9 * 11648 + 3 < 2^24, so fp32 accumulation is exact whatever the order of the K loop and
    of the atomics: the outputs must EQUAL the fp64 reference.  This sees a lost row, a tile computed twice under
    accumulate, a wrong tile origin, at any M.
  * GAUSSIAN operands (N(0, 1) rounded to bf16): ``bar_gemm`` of the routes module with the reduction length M in place of
    K and an fp32 output -- (M + 64) 2^-24 max(sum |dy x|, max |ref|) / max |ref|, worst case, no headroom factor.  This
    sees precision lost on the way (an intermediate rounded to bf16).  The worst-case bound grows with M while real error
    does not: on the rows in SENS_ROWS (M <= 448; every MFMA form has one) the test asserts FROM THE REFERENCE ALONE that
    (a) the reference with its last reduction row left out and (b) the reference rounded to bf16 each differ from the full
    reference by >= 10 bars; rows with M > 1280 carry the Gaussian check as a coarse guard and rely on the integer input.
db (the wgrad epilogue's column sums and ``ovqa_bias_grad``) gets the same two inputs, the bar with sum |dy| in place of the
products.

The grouped entry points are driven through the C ABI with device tables built HERE (hand-made tile lists: -1 padding
first, last and in between, tiles in reverse order, the problems' tiles interleaved) as well as with the table
``WgradQueue.tile_table`` emits: the kernels' contract is the table.  All dw / db of one grouped launch sit back to back in
ONE parent buffer with sentinel bytes between them (``Sentinel``).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_kernel_routes_gpu import (BF16, DEV, FORCED_SIMPLE, Sentinel, bar_gemm, check_route, launched, record,
                                    rel_max)

pytestmark = pytest.mark.gpu
F32 = torch.float32

# the kernels of the family: tests/test_wgrad_table_cpu.py checks this list against the symbols of the built library,
# test_every_kernel_of_the_family_shows_in_a_launch_log below that each one is reached
ALL_KERNELS = [
    "gemm_bf16_wgrad_kernel",
    "gemm_bf16_grouped_wgrad_kernel",
    "gemm_bf16_grouped_wgrad_glds_kernel<2>",
    "gemm_bf16_grouped_wgrad_adam_kernel",
    "colsum_bf16_kernel",
    "adam_kernel<float>",
    "adam_kernel<bf16>",
    "adam_tiled_kernel<float>",
    "adam_tiled_kernel<bf16>",
    "ln_bwd_reduce_kernel",
    "ln_bwd_grouped_reduce_kernel",
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


def values(kind, shape, seed, dtype=BF16):
    """``int``: integers in [-3, 3]; ``gauss``: N(0, 1).  Generated on the device (a 40000 x 4000 operand would take longer
    to upload than to test), deterministic for a seed."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "int":
        return torch.randint(-3, 4, shape, generator=g, device=DEV).to(dtype)
    return torch.randn(shape, generator=g, device=DEV).to(dtype)


def operand(kind, M, C_, seed, sliced, dtype=BF16):
    """[M, C_] operand; ``sliced``: a column slice of a wider buffer (ld = C_ + 24, starting 16 bytes into the rows: the
    packed q | k | v case -- base pointer 16-byte aligned but not at the allocation's start)."""
    if not sliced:
        return rnd(values(kind, (M, C_), seed, dtype))
    parent = rnd(values(kind, (M, C_ + 24), seed, dtype))
    return parent[:, 8:8 + C_]


def assert_exact(got, ref, what, tile=128):
    """Equality, not closeness; a failure names the first wrong element, its tile and how many there are."""
    g = got.detach().double()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    if torch.equal(g, ref):
        return 0.0
    bad = (g != ref) | g.isnan()
    idx = bad.nonzero()[0].tolist()
    where = tuple(idx)
    msg = (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact fp64 result; first at {where} "
           f"(tile {tuple(i // tile for i in where)}): got {g[where].item()!r}, expected {ref[where].item()!r}")
    if g.dim() == 2:
        tiles = sorted({(int(r) // tile, int(c) // tile) for r, c in bad.nonzero()[:4096].tolist()})
        msg += f"; tiles touched (first 4096 elements): {tiles[:32]}"
    raise AssertionError(msg)


def wgrad_reference(dy, x, want_sens):
    dyd, xd = dy.double(), x.double()
    ref = dyd.t() @ xd
    out = dict(dw=ref, absprod=dyd.abs().t() @ xd.abs(), db=dyd.sum(0), absdy=dyd.abs().sum(0))
    if want_sens:
        out["dw_last_row_out"] = dyd[:-1].t() @ xd[:-1]
        out["db_last_row_out"] = dyd[:-1].sum(0)
    return out


# (id, M, N, K, sliced operands, single-product entry too).  Problem i of a launch runs with accumulate bits i % 4 and
# without db where i % 5 == 4, so that every launch has all four combinations and a NULL db.
WGRAD_SHAPES = [
    ("m1_8x2048", 1, 8, 2048, False),          # one reduction row; a sliver of a tile along N
    ("m37_48x40", 37, 48, 40, True),           # ragged M, shorter than one 64-deep step; SENS row of the ragged-M forms
    ("m37_2048x8", 37, 2048, 8, False),        # a sliver of a tile along K
    ("m64_72x40", 64, 72, 40, False),          # exactly one step, partial tiles
    ("m64_8x2048", 64, 8, 2048, True),
    ("m64_2048x8", 64, 2048, 8, False),
    ("m65_304x264", 65, 304, 264, False),      # one row into the second step; partial tiles both ways
    ("m192_304x264", 192, 304, 264, True),     # odd number of 64-row steps through the two-buffer ring
    ("m192_768x384", 192, 768, 384, False),    # SENS row of the direct-to-LDS forms
    ("m192_128x128", 192, 128, 128, False),    # exactly one tile
    ("m64_3072x768", 64, 3072, 768, False),
    ("m192_768x3072", 192, 768, 3072, True),
    ("m448_1536x512", 448, 1536, 512, False),
    ("m6400_512x512", 6400, 512, 512, False),  # the MCAN row count
    ("m6400_768x3072", 6400, 768, 3072, True),
    ("m11648_5000x768", 11648, 5000, 768, False),  # the M4C row count and classifier: the last N tile has 8 rows
    ("m11648_3072x768", 11648, 3072, 768, False),
]
SENS_ROWS = {"m37_48x40", "m192_768x384"}
FORMS = {
    # form -> (kernel, admits the row)
    "single": ("gemm_bf16_wgrad_kernel", lambda M: True),
    "grouped0": ("gemm_bf16_grouped_wgrad_kernel", lambda M: True),
    "grouped1": ("gemm_bf16_grouped_wgrad_glds_kernel<2>", lambda M: M % 64 == 0),
    "adam_plain": ("gemm_bf16_grouped_wgrad_adam_kernel", lambda M: M % 64 == 0),
}


def rows_of(form):
    return [r for r in WGRAD_SHAPES if FORMS[form][1](r[1])]


def test_every_form_has_a_sensitive_gaussian_row():
    for form in FORMS:
        sens = [r for r in rows_of(form) if r[0] in SENS_ROWS]
        assert sens and all(r[1] <= 448 for r in sens), form


def check_outputs(request, rid, kind, M, flags, ref, init_dw, init_db, dw, db):
    """dw / db of one problem against the fp64 reference (plus the initial values under accumulate)."""
    acc_w, acc_b = flags & 1, (flags >> 1) & 1
    want_dw = ref["dw"] + (init_dw.double() if acc_w else 0.0)
    want_db = None if db is None else ref["db"] + (init_db.double() if acc_b else 0.0)
    if kind == "int":
        record(request, f"{rid} dw (integer operands: max |err|)", assert_exact(dw, want_dw, f"{rid} dw"), 0.0)
        if db is not None:
            record(request, f"{rid} db (integer operands: max |err|)", assert_exact(db, want_db, f"{rid} db", 1 << 30), 0.0)
        return
    refmax = want_dw.abs().max().item()
    absprod = (ref["absprod"] + (init_dw.double().abs() if acc_w else 0.0)).max().item()
    bar = bar_gemm(absprod, refmax, M, bf16_out=False)
    err = record(request, f"{rid} dw", rel_max(dw, want_dw), bar)
    assert err < bar, (rid, "dw", err, bar)
    if rid in SENS_ROWS:
        assert M <= 448
        full = ref["dw"]
        s_row = rel_max(ref["dw_last_row_out"], full)
        s_bf16 = rel_max(full.to(BF16).double(), full)
        plain_bar = bar_gemm(ref["absprod"].max().item(), full.abs().max().item(), M, bf16_out=False)
        assert s_row >= 10 * plain_bar and s_bf16 >= 10 * plain_bar, (rid, s_row, s_bf16, plain_bar)
    if db is not None:
        bmax = want_db.abs().max().item()
        babs = (ref["absdy"] + (init_db.double().abs() if acc_b else 0.0)).max().item()
        bbar = bar_gemm(babs, bmax, M, bf16_out=False)
        berr = record(request, f"{rid} db", rel_max(db, want_db), bbar)
        assert berr < bbar, (rid, "db", berr, bbar)
        if rid in SENS_ROWS:
            pb = bar_gemm(ref["absdy"].max().item(), ref["db"].abs().max().item(), M, bf16_out=False)
            s_row = rel_max(ref["db_last_row_out"], ref["db"])
            s_bf16 = rel_max(ref["db"].to(BF16).double(), ref["db"])
            assert s_row >= 10 * pb and s_bf16 >= 10 * pb, (rid, "db", s_row, s_bf16, pb)


class Outputs:
    """dw / db of several problems back to back in ONE parent buffer, 8 sentinel floats in front of, between and behind
    them; accumulate targets are initialised with values of the row's kind."""

    def __init__(self, kind, specs):
        """specs: [(N, K, flags, has_db)]"""
        total, offs = 8, []
        for N, K, flags, has_db in specs:
            o_dw = total
            total += N * K + 8
            o_db = None
            if has_db:
                o_db = total
                total += N + 8
            offs.append((o_dw, o_db))
        self.sent = Sentinel((total,), F32)
        self.dw, self.db, self.init_dw, self.init_db = [], [], [], []
        for i, ((N, K, flags, has_db), (o_dw, o_db)) in enumerate(zip(specs, offs)):
            dw = self.sent.parent[o_dw:o_dw + N * K].view(N, K)
            db = self.sent.parent[o_db:o_db + N] if has_db else None
            # initial values everywhere (a non-accumulating problem must overwrite them)
            dw.copy_(values(kind, (N, K), 900 + i, F32))
            if db is not None:
                db.copy_(values(kind, (N,), 950 + i, F32))
            self.dw.append(dw)
            self.db.append(db)
            self.init_dw.append(dw.clone())
            self.init_db.append(None if db is None else db.clone())

    def check_gaps(self):
        self.sent.check(*[v for v in self.dw + self.db if v is not None])


def device_image(problems, tiles, targets=None):
    """Problem array | int4 tile table (16-byte aligned) | Adam targets, as one device byte buffer built here."""
    _lib = lib()
    probs = (_lib.WgradProblem * len(problems))(*problems)
    pb = bytes(probs)
    pb += b"\0" * ((-len(pb)) % 16)
    tb = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 4)).tobytes()
    assert len(tb) % 16 == 0
    gb = b"" if targets is None else bytes((_lib.AdamTarget * len(targets))(*targets))
    buf = rnd(torch.frombuffer(bytearray(pb + tb + gb), dtype=torch.uint8))
    assert buf.data_ptr() % 16 == 0
    return buf, len(pb), len(pb) + len(tb), len(tb) // 16


PAD = (-1, -1, -1, -1)


def all_tiles(shapes):
    return [[(i, c, r, 0) for c in range(-(-N // 128)) for r in range(-(-K // 128))] for i, (M, N, K) in enumerate(shapes)]


def hand_made_tiles(shapes):
    """Every tile once, but nothing else as ``WgradQueue.flush`` would emit it: each problem's tiles in REVERSE order, the
    problems INTERLEAVED round-robin, padding entries first (3), last (2) and after every 5th tile; the length is not a
    multiple of 8."""
    per = [list(reversed(t)) for t in all_tiles(shapes)]
    out, k = [PAD] * 3, 0
    while any(per):
        for t in per:
            if t:
                out.append(t.pop(0))
                k += 1
                if k % 5 == 0:
                    out.append(PAD)
    return out + [PAD] * 2


def run_grouped(form, problems, tiles):
    o, _lib = ops(), lib()
    buf, toff, goff, n_tiles = device_image(
        problems, tiles, [_lib.AdamTarget() for _ in problems] if form == "adam_plain" else None)
    base = buf.data_ptr()
    if form == "adam_plain":
        consts = _lib.AdamConsts(1e-3, 0.9, 0.98, 1e-8, 0.0, 1.0, None, None)
        call = lambda: _lib.check(_lib.load().ovqa_grouped_linear_bwd_weight_adam(
            o.OVQA_BF16, base, base + toff, n_tiles, base + goff, C.addressof(consts), stream()), "grouped_wgrad_adam")
    else:
        call = lambda: _lib.check(_lib.load().ovqa_grouped_linear_bwd_weight(
            o.OVQA_BF16, base, base + toff, n_tiles, 1 if form == "grouped1" else 0, stream()), "grouped_wgrad")
    _, log = launched(call)
    torch.cuda.synchronize()
    return log, buf


def refuse_under_forced_simple(form):
    """OVQA_FORCE_SIMPLE=1: the fused entry point has no fallback and says so."""
    if form == "adam_plain" and FORCED_SIMPLE:
        o, _lib = ops(), lib()
        consts = _lib.AdamConsts(1e-3, 0.9, 0.98, 1e-8, 0.0, 1.0, None, None)
        dummy = rnd(torch.zeros(256, dtype=torch.uint8))
        rc = _lib.load().ovqa_grouped_linear_bwd_weight_adam(o.OVQA_BF16, dummy.data_ptr(), dummy.data_ptr() + 64, 1,
                                                             dummy.data_ptr() + 128, C.addressof(consts), stream())
        assert rc != 0
        pytest.skip("ovqa_grouped_linear_bwd_weight_adam refuses under OVQA_FORCE_SIMPLE=1 (asserted)")


@pytest.mark.parametrize("table", ["hand_made", "queue"])
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("form", ["grouped0", "grouped1", "adam_plain"])
def test_grouped_wgrad_route_parity(request, form, kind, table):
    """Every admissible row of WGRAD_SHAPES as the problems of ONE launch."""
    refuse_under_forced_simple(form)
    _lib = lib()
    rows = rows_of(form)
    if table == "queue":  # the emitted table once more on the short rows (the hand-made one carries the long ones)
        rows = [r for r in rows if r[1] <= 448]
    specs = [(N, K, i % 4, i % 5 != 4) for i, (rid, M, N, K, sl) in enumerate(rows)]
    outs = Outputs(kind, specs)
    operands, problems = [], []
    for i, (rid, M, N, K, sl) in enumerate(rows):
        dy, x = operand(kind, M, N, 10 + i, sl), operand(kind, M, K, 50 + i, sl)
        if form != "grouped0":
            assert M % 64 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and dy.stride(0) % 8 == 0
        operands.append((dy, x))
        db = outs.db[i]
        problems.append(_lib.WgradProblem(dy.data_ptr(), x.data_ptr(), outs.dw[i].data_ptr(),
                                          None if db is None else db.data_ptr(), dy.stride(0), x.stride(0), M, N, K,
                                          specs[i][2]))
    shapes = [(M, N, K) for _, M, N, K, _ in rows]
    tiles = hand_made_tiles(shapes) if table == "hand_made" else ops().WgradQueue.tile_table(shapes)
    log, _keep = run_grouped(form, problems, tiles)
    for i, (rid, M, N, K, sl) in enumerate(rows):
        ref = wgrad_reference(*operands[i], rid in SENS_ROWS)
        check_outputs(request, rid, kind, M, specs[i][2], ref, outs.init_dw[i], outs.init_db[i], outs.dw[i], outs.db[i])
        del ref
    outs.check_gaps()
    check_route(log, [FORMS[form][0]])


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("row", WGRAD_SHAPES, ids=[r[0] for r in WGRAD_SHAPES])
def test_single_wgrad_route_parity(request, row, kind):
    """ovqa_linear_bwd_weight, bf16, mfma_linear_bwd_weight_supported (N, K, lddy, ldx multiples of 8, M >= 1)."""
    o = ops()
    rid, M, N, K, sl = row
    i = [r[0] for r in WGRAD_SHAPES].index(rid)
    flags, has_db = i % 4, i % 5 != 4
    outs = Outputs(kind, [(N, K, flags, has_db)])
    dy, x = operand(kind, M, N, 10 + i, sl), operand(kind, M, K, 50 + i, sl)
    _, log = launched(lambda: o.linear_bwd_weight(dy, x, outs.dw[0], outs.db[0], accumulate=bool(flags & 1),
                                                  accumulate_db=bool(flags & 2)))
    torch.cuda.synchronize()
    ref = wgrad_reference(dy, x, rid in SENS_ROWS)
    check_outputs(request, rid, kind, M, flags, ref, outs.init_dw[0], outs.init_db[0], outs.dw[0], outs.db[0])
    outs.check_gaps()
    check_route(log, ["gemm_bf16_wgrad_kernel"])


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("dtype,M,N,K", [(F32, 37, 50, 29), (F32, 192, 128, 64), (BF16, 37, 50, 32), (BF16, 65, 48, 29),
                                         (BF16, 192, 52, 36)],
                         ids=["f32_37x50x29", "f32_192x128x64", "bf16_N50", "bf16_K29", "bf16_N52_K36"])
def test_valu_fallback_wgrad_parity(request, dtype, M, N, K, kind):
    """fp32, and bf16 with N or K not a multiple of 8: simple_linear_bwd_weight (OVQA_FALLBACK), no MFMA kernel in the log."""
    o = ops()
    for flags, has_db in ((0, True), (1, True), (2, True), (3, False)):
        outs = Outputs(kind, [(N, K, flags, has_db)])
        dy, x = operand(kind, M, N, 3, False, dtype), operand(kind, M, K, 4, False, dtype)
        _, log = launched(lambda: o.linear_bwd_weight(dy, x, outs.dw[0], outs.db[0], accumulate=bool(flags & 1),
                                                      accumulate_db=bool(flags & 2)))
        torch.cuda.synchronize()
        assert lib().last_dispatch() == "simple"
        assert not [e for e in log if "wgrad" in e], log
        ref = wgrad_reference(dy, x, False)
        check_outputs(request, f"fallback acc{flags}", kind, M, flags, ref, outs.init_dw[0], outs.init_db[0], outs.dw[0],
                      outs.db[0])
        outs.check_gaps()


def test_wgrad_queue_builds_the_same_launch(request):
    """Through ``ops.WgradQueue`` (what the modules use): form 1 when every M is a multiple of 64, form 0 otherwise."""
    o = ops()
    for rows, kernel in (([r for r in WGRAD_SHAPES if r[1] in (64, 192)], "gemm_bf16_grouped_wgrad_glds_kernel<2>"),
                         ([r for r in WGRAD_SHAPES if r[1] <= 192], "gemm_bf16_grouped_wgrad_kernel")):
        specs = [(N, K, i % 4, i % 5 != 4) for i, (rid, M, N, K, sl) in enumerate(rows)]
        outs = Outputs("int", specs)
        q = o.WgradQueue()
        operands = []
        for i, (rid, M, N, K, sl) in enumerate(rows):
            dy, x = operand("int", M, N, 10 + i, sl), operand("int", M, K, 50 + i, sl)
            operands.append((dy, x))
            q.add(dy, x, outs.dw[i], bool(specs[i][2] & 1), outs.db[i], bool(specs[i][2] & 2))
        _, log = launched(q.finish)
        torch.cuda.synchronize()
        for i, (rid, M, N, K, sl) in enumerate(rows):
            check_outputs(request, f"queue {rid}", "int", M, specs[i][2], wgrad_reference(*operands[i], False),
                          outs.init_dw[i], outs.init_db[i], outs.dw[i], outs.db[i])
        outs.check_gaps()
        if FORCED_SIMPLE:
            continue
        assert log == [kernel], log


# ---------------------------------------------------------------------------------------------------------------------------
# ovqa_bias_grad / colsum_bf16_kernel
# ---------------------------------------------------------------------------------------------------------------------------
BIAS_M = [1, 3, 4, 13, 16, 17, 63, 64, 65, 6400, 40000]
BIAS_N = [8, 504, 512, 520, 4000]


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("M", BIAS_M)
def test_bias_grad_parity(request, M, kind):
    """Both row loops of the kernel (4 loads in flight while m + 12 < m1, then one) and their hand-over; more than 512
    slabs' worth of rows (M = 40000: rows_per_slab = 79 > 64); N below, at and above one 512-column workgroup; lddy > N;
    accumulate on and off over a non-zero db."""
    o = ops()
    for j, N in enumerate(BIAS_N):
        sl = j % 2 == 1
        dy = operand(kind, M, N, 7 + j, sl)
        dyd = dy.double()
        ref, absdy = dyd.sum(0), dyd.abs().sum(0)
        for acc in (False, True):
            sent = Sentinel((N + 16,), F32)
            db = sent.parent[8:8 + N]
            db.copy_(values(kind, (N,), 70 + j, F32))
            init = db.clone().double()
            _, log = launched(lambda: o.bias_grad(dy, db, accumulate=acc))
            torch.cuda.synchronize()
            want = ref + (init if acc else 0.0)
            what = f"db M={M} N={N} ld={dy.stride(0)} acc={int(acc)}"
            if kind == "int":
                record(request, what + " (integer operands: max |err|)", assert_exact(db, want, what, 1 << 30), 0.0)
            else:
                bar = bar_gemm((absdy + (init.abs() if acc else 0.0)).max().item(), want.abs().max().item(), M, bf16_out=False)
                err = record(request, what, rel_max(db, want), bar)
                assert err < bar, (what, err, bar)
                if M in (13, 65) and not acc:  # the bar sees a lost row and a bf16 intermediate (from the reference alone)
                    s_row, s_bf16 = rel_max(dyd[:-1].sum(0), ref), rel_max(ref.to(BF16).double(), ref)
                    assert s_row >= 10 * bar and s_bf16 >= 10 * bar, (what, s_row, s_bf16, bar)
            sent.check(db)
            assert log == ["colsum_bf16_kernel"], log


def test_bias_grad_of_no_rows():
    """M = 0 (an empty batch slice): db is zeroed, or left alone under accumulate, as ovqa_linear_bwd_weight does; nothing
    is launched (the kernel's slab count would be 0)."""
    o, _lib = ops(), lib()
    dy = rnd(torch.zeros(1, 512, dtype=BF16))  # a valid pointer; no row of it is read
    for acc in (0, 1):
        sent = Sentinel((512 + 16,), F32)
        db = sent.parent[8:8 + 512]
        db.copy_(values("int", (512,), 5, F32) + 0.5)
        init = db.clone()
        _, log = launched(lambda: _lib.check(_lib.load().ovqa_bias_grad(o.OVQA_BF16, dy.data_ptr(), 512, db.data_ptr(), 0, 512,
                                                                        acc, stream()), "bias_grad"))
        torch.cuda.synchronize()
        assert torch.equal(db, init if acc else torch.zeros_like(db))
        sent.check(db)
        assert log == [], log


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm dgamma / dbeta: the grouped partial reduce on hand-made partials, the immediate reduce behind ovqa_layernorm_bwd
# ---------------------------------------------------------------------------------------------------------------------------
def run_partial_reduce(request, tag, specs, max_D=None):
    """specs: [(blocks, D, accumulate, out1 is NULL)]: integer partials [blocks][2][D] in [-3, 3] (sums of at most 1024 of
    them: exact in fp32 in any order), the outputs of all problems in one parent buffer with sentinels behind each."""
    o, _lib = ops(), lib()
    total, offs = 8, []
    for blocks, D, acc, no1 in specs:
        offs.append((total, None if no1 else total + D + 8))
        total += (D + 8) * (1 if no1 else 2)
    sent = Sentinel((total,), F32)
    probs, parts, outs = [], [], []
    for i, ((blocks, D, acc, no1), (o0, o1)) in enumerate(zip(specs, offs)):
        part = rnd(values("int", (blocks, 2, D), 20 + i, F32))
        out0 = sent.parent[o0:o0 + D]
        out1 = None if no1 else sent.parent[o1:o1 + D]
        for k, out in enumerate((out0, out1)):
            if out is not None:
                out.copy_(values("int", (D,), 40 + 2 * i + k, F32))
        parts.append(part)
        outs.append((out0, out1, out0.clone(), None if no1 else out1.clone()))
        probs.append(_lib.ReduceProblem(part.data_ptr(), out0.data_ptr(), None if no1 else out1.data_ptr(), blocks, D,
                                        int(acc), 0))
    table = rnd(torch.frombuffer(bytearray(bytes((_lib.ReduceProblem * len(probs))(*probs))), dtype=torch.uint8))
    mD = max(s[1] for s in specs) if max_D is None else max_D
    _, log = launched(lambda: _lib.check(_lib.load().ovqa_grouped_partial_reduce(
        table.data_ptr(), len(probs), max(s[0] for s in specs), mD, stream()), "grouped_partial_reduce"))
    torch.cuda.synchronize()
    views = []
    for (blocks, D, acc, no1), part, (out0, out1, i0, i1) in zip(specs, parts, outs):
        s = part.double().sum(0)
        for k, (out, init) in enumerate(((out0, i0), (out1, i1))):
            if out is None:
                continue
            want = s[k] + (init.double() if acc else 0.0)
            what = f"{tag} blocks={blocks} D={D} acc={int(acc)} out{k}"
            record(request, what + " (integer partials: max |err|)", assert_exact(out, want, what, 1 << 30), 0.0)
            views.append(out)
    sent.check(*views)
    assert log == ["ln_bwd_grouped_reduce_kernel"], log


def test_grouped_partial_reduce_exact(request):
    # problems of different blocks and D in one launch: max_D = 2048 is larger than most problems' D -- their surplus
    # workgroups must store nothing (the sentinels behind each output); out1 NULL; accumulate on and off
    run_partial_reduce(request, "mixed", [(1, 8, 0, False), (2, 504, 1, False), (511, 512, 0, True), (512, 1176, 1, False),
                                          (1024, 2048, 0, False), (3, 8, 1, True), (1024, 512, 1, False)])
    for blocks in (1, 2, 511, 512, 1024):
        run_partial_reduce(request, "alone", [(blocks, D, acc, False) for acc, D in enumerate((504, 1176))])
    run_partial_reduce(request, "one small problem under a large max_D", [(2, 8, 0, False)], max_D=2048)


def test_two_uses_of_one_output_go_to_successive_launches(request):
    """``WgradQueue._flush_reduces``: problems of one launch must not share an output (plain stores); the second use of a
    LayerNorm in a pass goes to a second launch and adds to what the first stored."""
    o = ops()
    D = 512
    sent = Sentinel((4 * (D + 8) + 8,), F32)
    g0, b0, g1, b1 = (sent.parent[8 + k * (D + 8):8 + k * (D + 8) + D] for k in range(4))
    p = [rnd(values("int", (blocks, 2, D), 60 + i, F32)) for i, blocks in enumerate((5, 64, 17))]
    q = o.WgradQueue()
    q.add_reduce(p[0], 5, D, g0, b0, accumulate=False)
    q.add_reduce(p[1], 64, D, g1, b1, accumulate=False)
    q.add_reduce(p[2], 17, D, g0, b0, accumulate=True)
    _, log = launched(q.finish)
    torch.cuda.synchronize()
    s = [t.double().sum(0) for t in p]
    for what, got, want in (("dgamma used twice", g0, s[0][0] + s[2][0]), ("dbeta used twice", b0, s[0][1] + s[2][1]),
                            ("dgamma used once", g1, s[1][0]), ("dbeta used once", b1, s[1][1])):
        record(request, what + " (integer partials: max |err|)", assert_exact(got, want, what, 1 << 30), 0.0)
    sent.check(g0, b0, g1, b1)
    assert log == ["ln_bwd_grouped_reduce_kernel"] * 2, log


@pytest.mark.parametrize("M,D", [(37, 512), (6400, 512), (1280, 1176), (300, 2048)])
def test_layernorm_bwd_immediate_reduce(request, M, D):
    """ovqa_layernorm_bwd with dgamma / dbeta given: ln_bwd_reduce_kernel sums the row-slab partials right away.  dy holds
    integers in [-3, 3]: dbeta = sum_m dy is exact.  dgamma = sum_m dy (x - mean) rstd against fp64 on the SAME fp32 mean /
    rstd, bar: M terms summed in fp32 in any order plus the few roundings of (x - mean) rstd dy per term (``bar_gemm``'s
    64).  The log names the row kernel in front of it (``form``: its CHUNKS and waves per workgroup; tests/
    test_rowwise_routes_gpu.py has its parity)."""
    o = ops()
    form = {(37, 512): "1,4", (6400, 512): "1,8", (1280, 1176): "4,4", (300, 2048): "4,4"}[(M, D)]
    dy = rnd(values("int", (M, D), 1))
    x = rnd(values("gauss", (M, D), 2))
    gamma = rnd(values("gauss", (D,), 3, F32))
    xd = x.double()
    mean = rnd(xd.mean(-1).float())
    rstd = rnd((1.0 / torch.sqrt(xd.var(-1, unbiased=False) + 1e-5)).float())
    xhat = (xd - mean.double()[:, None]) * rstd.double()[:, None]
    terms = dy.double() * xhat
    for acc in (False, True):
        sent = Sentinel((2 * (D + 8) + 8,), F32)
        dg, dbt = sent.parent[8:8 + D], sent.parent[16 + D:16 + 2 * D]
        dg.copy_(values("int", (D,), 8, F32))
        dbt.copy_(values("int", (D,), 9, F32))
        ig, ib = dg.clone().double(), dbt.clone().double()
        _, log = launched(lambda: o.layernorm_bwd(dy, x, gamma, mean, rstd, dg, dbt, accumulate=acc))
        torch.cuda.synchronize()
        record(request, f"dbeta acc={int(acc)} (integer dy: max |err|)",
               assert_exact(dbt, dy.double().sum(0) + (ib if acc else 0.0), "dbeta", 1 << 30), 0.0)
        want = terms.sum(0) + (ig if acc else 0.0)
        bar = bar_gemm((terms.abs().sum(0) + (ig.abs() if acc else 0.0)).max().item(), want.abs().max().item(), M,
                       bf16_out=False)
        err = record(request, f"dgamma acc={int(acc)}", rel_max(dg, want), bar)
        assert err < bar, (err, bar)
        sent.check(dg, dbt)
        assert log == [f"ln_bwd_kernel<__bf16,__bf16,__bf16,{form}>", "ln_bwd_reduce_kernel"], log


def test_every_kernel_of_the_family_shows_in_a_launch_log():
    """Each entry of ALL_KERNELS by the smallest call that reaches it."""
    if FORCED_SIMPLE:
        pytest.skip("route checks are skipped under OVQA_FORCE_SIMPLE=1")
    o, _lib = ops(), lib()
    seen = []
    dy, x = rnd(values("int", (64, 128), 1)), rnd(values("int", (64, 128), 2))
    dw = rnd(torch.zeros(128, 128))
    seen += launched(lambda: o.linear_bwd_weight(dy, x, dw))[1]
    prob = [_lib.WgradProblem(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), None, 128, 128, 64, 128, 128, 0)]
    for form in ("grouped0", "grouped1", "adam_plain"):
        log, _keep = run_grouped(form, prob, [(0, 0, 0, 0)])
        seen += log
    db = rnd(torch.zeros(128))
    seen += launched(lambda: o.bias_grad(dy, db))[1]
    n = 64 * 64
    step = rnd(torch.ones(1, dtype=torch.int32))
    tile = rnd(torch.frombuffer(bytearray(bytes(_lib.AdamTile(0, 64, 64, 0, 0, (C.c_int32 * 2)(0, 0)))), dtype=torch.uint8))
    for gdt in (F32, BF16):
        p, g, m, v = (rnd(values("gauss", (n,), 3 + k, F32)) for k in range(4))
        g, v = g.to(gdt), v.abs()
        sh, sht = rnd(torch.zeros(n, dtype=BF16)), rnd(torch.zeros(n, dtype=BF16))
        seen += launched(lambda: o.adam_step(p, g, m, v, sh, 1e-3, step))[1]
        seen += launched(lambda: o.adam_step_tiled(p, g, m, v, sh, sht, tile, 1, n, n, 1e-3, step))[1]
    part = rnd(values("int", (2, 2, 8), 9, F32))
    out = rnd(torch.zeros(16))
    tab = rnd(torch.frombuffer(bytearray(bytes(_lib.ReduceProblem(part.data_ptr(), out.data_ptr(), out.data_ptr() + 32, 2, 8,
                                                                  0, 0))), dtype=torch.uint8))
    seen += launched(lambda: _lib.check(_lib.load().ovqa_grouped_partial_reduce(tab.data_ptr(), 1, 2, 8, stream()), "reduce"))[1]
    xs = rnd(values("gauss", (8, 64), 10))
    ones = rnd(torch.ones(8))
    seen += launched(lambda: o.layernorm_bwd(rnd(values("int", (8, 64), 11)), xs, rnd(torch.ones(64)), ones, ones,
                                             rnd(torch.zeros(64)), rnd(torch.zeros(64))))[1]
    torch.cuda.synchronize()
    # (the row kernel in front of ln_bwd_reduce_kernel belongs to the family of tests/test_rowwise_routes_gpu.py)
    want = set(ALL_KERNELS) | {"ln_bwd_kernel<__bf16,__bf16,__bf16,1,4>"}
    assert set(seen) == want, {"never launched": sorted(want - set(seen)), "not in the list": sorted(set(seen) - want)}
