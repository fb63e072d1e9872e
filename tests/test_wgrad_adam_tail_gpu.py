"""The Adam tail of ``gemm_bf16_grouped_wgrad_adam_kernel`` where its schedule makes it fragile: the optimiser state of a tile
is loaded ahead of its use (part of it from inside the last K step), under a workgroup-uniform ``fused`` condition, and the
transposed shadow is gathered from a swizzled LDS image.  tests/test_adam_gpu.py has the arithmetic (every hyper-parameter
row against fp64); this file has the launch shapes that file does not single out:

  * tile tables whose FIRST tiles belong to unfused problems (NULL targets) and whose last to fused ones, and the reverse: a
    state load issued under the wrong condition reads through a NULL pointer or is missing;
  * fused problems with M = 64 (ONE K step: the hook inside the last K step runs in the first) next to M = 6400;
  * padding entries (-1) in front of, between and behind the real ones;
  * three consecutive steps on the same state (moments carried, the device step counter advanced), eager and replayed from
    a captured graph;
  * every element of every arena holds a value of its own, so that an element of the transposed shadow (or of any array)
    that lands in the wrong place cannot hide behind an equal neighbour.

Expected values: (a) the separate path -- form-1 grouped dW into a gradient arena, then ``ovqa_adam_step_tiled`` -- on copies
of the same state, bit for bit in all five arenas; (b) operands are integers, so the gradient is exact and exp_avg,
exp_avg_sq and the update are held against the fp64 Adam of tests/test_adam_gpu.py with that module's bars; (c) the exact
identities shadow == bf16(param), shadow_t == shadow.t(); (d) nothing outside the fused problems' elements changes, the dw
buffer of a fused problem stays as it was, unfused dw / db are exact.  Every buffer sits between the guard bands of
tests/redzone.py."""
import ctypes as C
import os

import pytest
import torch

from test_adam_gpu import HP, Arena, check_adam
from test_kernel_routes_gpu import BF16, DEV, FORCED_SIMPLE, launched
from test_wgrad_routes_gpu import PAD, all_tiles, assert_exact, device_image, values, wgrad_reference

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(autouse=True)
def _red_zones(request, monkeypatch):
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


# fused problems (name, M, N, K): each is a whole matrix of the arena (its transposed copy is [K, N], ld_transposed = N)
FUSED = [("m64_wide", 64, 128, 384), ("m6400", 6400, 256, 128), ("m64_tall", 64, 384, 128), ("m192", 192, 128, 128)]
# unfused problems of the same launch (name, M, N, K, accumulate bits, has db): NULL targets
UNFUSED = [("u_72x40", 64, 72, 40, 0, True), ("u_acc", 192, 128, 256, 1, False), ("u_m6400", 6400, 128, 128, 2, True)]
MATS = {f[0]: (f[2], f[3]) for f in FUSED}
ORDERS = ["unfused_first", "fused_first", "padded"]


def tile_table(order, n_fused, shapes):
    per = all_tiles(shapes)
    fused = [t for p in per[:n_fused] for t in p]
    unfused = [t for p in per[n_fused:] for t in p]
    if order == "unfused_first":
        return unfused + fused
    if order == "fused_first":
        return fused + unfused
    out = [PAD, PAD]  # padded: fused and unfused alternate, a padding entry behind every real one, three in front and behind
    a, b = list(fused), list(unfused)
    while a or b:
        for src in (a, b):
            if src:
                out += [src.pop(0), PAD]
    return [PAD] + out + [PAD] * 2


def distinct_state(n):
    """p, m, v of n <= 2^18 elements, no two elements of an array equal (all exactly representable); p is a scrambled
    permutation of multiples of 2^-10 in [-128, 128), so that neighbours in either direction of a tile differ in the bf16
    shadow as well."""
    assert n <= 1 << 18
    i = torch.arange(n, dtype=torch.int64)
    p = (((i * 40503) % (1 << 18)) - (1 << 17)).double() * 2.0 ** -10  # (40503 is odd: a bijection on [0, 2^18))
    m = (i.double() - n // 2) * 2.0 ** -22
    v = (i.double() + 1) * 2.0 ** -20
    p, m, v = p.float(), m.float(), v.float()
    for x in (p, m, v):
        assert x.unique().numel() == n
    return rnd(p), rnd(m), rnd(v)


def byte_pattern(n, dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    pat = (torch.arange(n * size, dtype=torch.int64) * 37 + 11) % 251
    return rnd(pat.to(torch.uint8)).view(dtype)


class Launch:
    """One fused launch over FUSED + UNFUSED with the tile table of ``order``, built through the C ABI."""

    def __init__(self, order, hp, t0):
        o, _lib = ops(), lib()
        self.hp, self.ar = hp, Arena(MATS)
        ar = self.ar
        p, m, v = distinct_state(ar.n)
        self.S = dict(p=p, m=m, v=v, sh=byte_pattern(ar.n, BF16), sht=byte_pattern(ar.n, BF16))
        self.shapes = [(f[1], f[2], f[3]) for f in FUSED] + [(u[1], u[2], u[3]) for u in UNFUSED]
        self.flags = [0] * len(FUSED) + [u[4] for u in UNFUSED]
        self.operands, self.dw, self.db, problems, targets = [], [], [], [], []
        for i, (M, N, K) in enumerate(self.shapes):
            dy, x = rnd(values("int", (M, N), 300 + i)), rnd(values("int", (M, K), 400 + i))
            dw = rnd(values("int", (N, K), 500 + i, F32))
            has_db = i >= len(FUSED) and UNFUSED[i - len(FUSED)][5] or i == 1
            db = rnd(values("int", (N,), 600 + i, F32)) if has_db else None
            self.operands.append((dy, x))
            self.dw.append(dw)
            self.db.append(db)
            problems.append(_lib.WgradProblem(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(),
                                              dy.stride(0), x.stride(0), M, N, K, self.flags[i]))
            if i < len(FUSED):
                e = ar.off[FUSED[i][0]]
                targets.append(_lib.AdamTarget(p.data_ptr() + 4 * e, m.data_ptr() + 4 * e, v.data_ptr() + 4 * e,
                                               self.S["sh"].data_ptr() + 2 * e, self.S["sht"].data_ptr() + 2 * e, N))
            else:
                targets.append(_lib.AdamTarget())
        self.init_dw = [x.clone() for x in self.dw]
        self.init_db = [None if x is None else x.clone() for x in self.db]
        self.problems = problems
        tiles = tile_table(order, len(FUSED), self.shapes)
        assert sorted(t for t in tiles if t != PAD) == sorted(t for p_ in all_tiles(self.shapes) for t in p_)
        self.buf, toff, goff, n_tiles = device_image(problems, tiles, targets)
        self.step = rnd(torch.tensor([t0], dtype=torch.int32))
        self.consts = _lib.AdamConsts(hp.lr, hp.b1, hp.b2, hp.eps, hp.wd, hp.gs, None, self.step.data_ptr())
        base = self.buf.data_ptr()
        self.rc_call = lambda: _lib.load().ovqa_grouped_linear_bwd_weight_adam(
            o.OVQA_BF16, base, base + toff, n_tiles, base + goff, C.addressof(self.consts), stream())

    def run(self):
        lib().check(self.rc_call(), "grouped_linear_bwd_weight_adam")

    def region(self, i):
        name, M, N, K = FUSED[i]
        lo = self.ar.off[name]
        return slice(lo, lo + N * K)


class Separate:
    """The same steps as two launches each, on copies of a Launch's initial state."""

    def __init__(self, L):
        o, _lib = ops(), lib()
        self.L, ar = L, L.ar
        self.B = {k: x.clone() for k, x in L.S.items()}
        self.grad = rnd(torch.zeros(ar.n))
        problems = []
        for i, f in enumerate(FUSED):
            pr = L.problems[i]
            problems.append(_lib.WgradProblem(pr.dy, pr.x, self.grad.data_ptr() + 4 * ar.off[f[0]], None, pr.lddy, pr.ldx,
                                              pr.M, pr.N, pr.K, 0))
        self.buf, self.toff, _, self.n_tiles = device_image(problems, o.WgradQueue.tile_table(L.shapes[:len(FUSED)]))
        tiles = ar.tiles()
        self.n_adam = len(tiles)
        self.table = rnd(torch.frombuffer(bytearray(bytes((_lib.AdamTile * len(tiles))(*tiles))), dtype=torch.uint8))
        self.step = L.step.clone()

    def run(self):
        o, _lib, L, B = ops(), lib(), self.L, self.B
        _lib.check(_lib.load().ovqa_grouped_linear_bwd_weight(o.OVQA_BF16, self.buf.data_ptr(), self.buf.data_ptr() + self.toff,
                                                              self.n_tiles, 1, stream()), "grouped_linear_bwd_weight")
        n = L.ar.n
        o.adam_step_tiled(B["p"], self.grad, B["m"], B["v"], B["sh"], B["sht"], self.table, self.n_adam, n - 20, n - 20,
                          L.hp.lr, self.step, betas=(L.hp.b1, L.hp.b2), eps=L.hp.eps, weight_decay=L.hp.wd, grad_scale=L.hp.gs)


def refuse_if_forced_simple(L):
    if FORCED_SIMPLE:
        assert L.rc_call() != 0
        pytest.skip("ovqa_grouped_linear_bwd_weight_adam refuses under OVQA_FORCE_SIMPLE=1 (asserted)")


def check_step(request, tag, L, B, old, t, refs):
    """One step of the fused launch: against fp64 Adam on the exact gradient (``old``: the state before the step), the
    shadows' identities, untouched elements, and bit-equality with the separate path's arenas ``B``."""
    S, ar = L.S, L.ar
    inside = torch.zeros(ar.n, dtype=torch.bool, device=DEV)
    for i, (name, M, N, K) in enumerate(FUSED):
        sl = L.region(i)
        inside[sl] = True
        st_old = [old["p"][sl], refs[i]["dw"].reshape(-1), old["m"][sl], old["v"][sl]]
        check_adam(request, f"{tag} {name}", L.hp, t, st_old, (S["p"][sl], S["m"][sl], S["v"][sl]), S["sh"][sl])
        assert torch.equal(S["sht"][sl].view(K, N), S["sh"][sl].view(N, K).t()), f"{tag} {name}: transposed shadow != shadow.t()"
        assert torch.equal(L.dw[i], L.init_dw[i]), f"{tag} {name}: the fp32 gradient of a fused problem reached its dw buffer"
    for k in ("p", "m", "v", "sh", "sht"):
        a, b = S[k].view(torch.int32 if k in "pmv" else torch.int16), old[k].view(torch.int32 if k in "pmv" else torch.int16)
        assert torch.equal(a[~inside], b[~inside]), f"{tag}: arena {k} changed outside the fused problems' elements"
        diff = int((S[k].view(a.dtype) != B[k].view(a.dtype)).sum())
        assert diff == 0, f"{tag}: arena {k}: the fused launch and grouped dW + tiled Adam differ in {diff} elements"


def check_unfused_and_db(L, refs, steps):
    """dw / db of the unfused problems and db of fused ones after ``steps`` identical launches (integer operands: exact)."""
    for i, (M, N, K) in enumerate(L.shapes):
        acc_w, acc_b = L.flags[i] & 1, (L.flags[i] >> 1) & 1
        if i >= len(FUSED):
            want = refs[i]["dw"] * (steps if acc_w else 1) + (L.init_dw[i].double() if acc_w else 0.0)
            assert_exact(L.dw[i], want, f"{UNFUSED[i - len(FUSED)][0]} dw")
        if L.db[i] is not None:
            want = refs[i]["db"] * (steps if acc_b else 1) + (L.init_db[i].double() if acc_b else 0.0)
            assert_exact(L.db[i], want, f"problem {i} db", 1 << 30)


@pytest.mark.parametrize("order", ORDERS)
def test_tail_against_separate_path_and_fp64(request, order):
    """One step at t = 2 (moments non-zero) with weight decay and a gradient scale, per tile-table order."""
    hp, t = HP(wd=0.01, gs=0.25), 2
    L = Launch(order, hp, t)
    refuse_if_forced_simple(L)
    old = {k: x.clone() for k, x in L.S.items()}
    sep = Separate(L)
    _, log = launched(L.run)
    torch.cuda.synchronize()
    assert log == ["gemm_bf16_grouped_wgrad_adam_kernel"], log
    sep.run()
    torch.cuda.synchronize()
    refs = [wgrad_reference(dy, x, False) for dy, x in L.operands]
    check_step(request, order, L, sep.B, old, t, refs)
    check_unfused_and_db(L, refs, 1)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("order", ORDERS)
def test_three_steps_on_the_same_state(request, order, graph):
    """Steps t = 1, 2, 3 on the same arenas: the moments of a step are the next one's input, the device step counter is
    advanced in front of every launch (inside the captured graph when replayed)."""
    hp = HP(wd=0.01)
    L = Launch(order, hp, 0)
    refuse_if_forced_simple(L)
    sep = Separate(L)
    refs = [wgrad_reference(dy, x, False) for dy, x in L.operands]

    def one_step():
        L.step.add_(1)
        L.run()
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            one_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    for t in (1, 2, 3):
        old = {k: x.clone() for k, x in L.S.items()}
        if graph:
            g.replay()
        else:
            one_step()
        sep.step.add_(1)
        sep.run()
        torch.cuda.synchronize()
        assert int(L.step.item()) == t
        check_step(request, f"{order} t={t}", L, sep.B, old, t, refs)
    check_unfused_and_db(L, refs, 3)
