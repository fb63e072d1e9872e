"""Route-table parity: every MFMA GEMM and attention kernel INSTANTIATION against fp64 math, by the route that reaches it.

The bf16 hot path is a dispatcher (csrc/gemm_mfma.hip ``launch<PK, QK, Epi>()``, csrc/attention_mfma.hip ``launch_*``) that
picks an instantiation by shape, stride, alignment and CU count.  Each row below names the entry point and arguments, the
instantiation the launch log (``ovqa_launch_log``, ABI 11) must show, and the dispatch predicate that sends the shape there.
The expected GEMM form is recomputed from a Python copy of the predicates (``gemm_form``), with the device's own CU count:
a row whose intended tier the device's CU count does not reach is SKIPPED with the count in the reason, never passed.

References are fp64 math on the same bf16-rounded operands (never another HIP kernel).  Bars are normalised by the
reference's own scale (no max(1, .) floor) and derived from the output format (``bar_gemm`` / ``bar_att``); every row also
shows that its bar sees a realistic bug: the reference with its last 64-deep K step (GEMM) or last 32-key tile (attention)
left out differs from the full one by at least 10x the bar.  Outputs that are views into a larger buffer are checked for
stores into the gaps (``Sentinel``): tests/redzone.py only guards the two ends of an allocation.

Pairs of (tier, epilogue) that no entry point can reach:
  * k-major P (``linear_bwd_data``) x any epilogue but MEpiBwdData: only ovqa_linear_bwd_data launches with PK = true.
  * 256-tile / skinny / 16-wave 128 x 128 x MEpiBwdData from ``linear_bwd_data``: those tiers need !PK (launch(): ``if
    constexpr (!QK && !PK)``); ``linear_bwd_data_wt`` reaches them instead.
  * register-staged via ``wide_ok == false`` x MEpiBiasRes32 / MEpiBiasSplit3: both entry points pass wide_ok = true (their
    outputs must be 16-byte aligned with ld % 8 == 0, checked in api.hip); they reach the register-staged form by K % 64 only.
  * gemm_bf16_glds_kernel<false, false, Epi, 4, 8, 32, 128> and <false, false, Epi, 3, 8, 64, 128> for every Epi (the 8-wave
    tiny / small tiers with a row-major P): compiled because launch()'s ``if constexpr (!QK)`` block is instantiated for
    PK = false too, but never launched there -- for !PK the ``if constexpr (!QK && !PK)`` block above it returns on the
    same tiny_c / small_c predicates (64 x 32 on 4 waves, 16-wave 128 x 128).  UNREACHABLE_INSTANTIATIONS lists them; the
    CPU test tests/test_kernel_routes_cpu.py checks ALL + UNREACHABLE against the kernel symbols of the built library.
  * attn_fwd_mfma_kernel<8, ., ., 96 | 128, .>: launch_fwd_d returns OVQA_ERR_UNSUPPORTED (n_k > 192 with d > 64).
  * attn_bwd_roles / smallk x dropout and x d != 64: launch_bwd sends both to the two-kernel form.
  * attn_qkv_fwd x square masks / need_att / dropout: mfma_attention_qkv_supported excludes them (library's two-kernel route).
Prefix-LM forward (ovqa_attention_fwd_prefix_lm) runs the same attn_fwd_mfma_kernel<NKT, true, false, D, false> forms with a
causal corner computed in the kernel: its rows (test_attention_fwd_prefix_lm_route_parity) compare with fp64 on the dense
mask.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
U = 2.0 ** -8  # bf16 has 8 significand bits (7 stored): one ulp at 1.0 is 2^-7, a correctly rounded value is within U relative
EPS32 = 2.0 ** -24

FORCED_SIMPLE = os.environ.get("OVQA_FORCE_SIMPLE", "0") == "1"
NO_FUSED_QKV = os.environ.get("OVQA_NO_FUSED_QKV", "0") == "1"
NO_FUSED_Q = os.environ.get("OVQA_NO_FUSED_Q", "0") == "1"
NO_FUSED_DO = os.environ.get("OVQA_NO_FUSED_DO", "0") == "1"
NO_PREFIX_LM = os.environ.get("OVQA_NO_PREFIX_LM", "0") == "1"
T256_ON = os.environ.get("OVQA_GEMM_T256", "1") not in ("0",)
ROUTES_DEFAULT = not (FORCED_SIMPLE or NO_FUSED_QKV or NO_FUSED_Q or NO_FUSED_DO or NO_PREFIX_LM)


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


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def record(request, what, value, bar):
    from conftest import parity_record
    return parity_record(request.node.nodeid, what, value, bar)


def rel_max(a, ref):
    """max |a - ref| / max |ref|: normalised by the reference's own scale, no floor."""
    a, ref = a.detach().double(), ref.detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    s = ref.abs().max().item()
    assert s > 0
    return ((a - ref).abs().max() / s).item()


def launched(fn):
    """Run ``fn`` and return (its result, the instantiations it launched on this thread)."""
    from openvivqa_amd import _lib
    _lib.launch_log_clear()
    out = fn()
    return out, _lib.launch_log()


def check_route(log, expect, off=False):
    """The launch log names exactly the expected instantiations.  Under the library's A/B switches (``off``, or a 256-tile
    row with OVQA_GEMM_T256=0) the parity checks above have run and the route check is reported as SKIPPED."""
    if off or not ROUTES_DEFAULT or (not T256_ON and any("ovqa_t256" in e for e in expect)):
        pytest.skip(f"parity checked; route check skipped under the library's A/B switches (expected {list(expect)}, "
                    f"ran {log})")
    assert log == list(expect), (log, expect)


class Sentinel:
    """A parent buffer filled with a byte pattern; after the call every byte outside the child view must be unchanged."""

    def __init__(self, shape, dtype):
        n = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        pat = (torch.arange(n, dtype=torch.int64) * 37 + 11) % 251
        self.parent = pat.to(torch.uint8).to(DEV).view(dtype).view(shape)
        self.before = self.parent.clone()

    def view(self, fn):
        return fn(self.parent)

    def check(self, *views):
        torch.cuda.synchronize()
        idx = torch.arange(self.parent.numel(), device=DEV)
        inside = torch.zeros(self.parent.numel(), dtype=torch.bool, device=DEV)
        for v in views:
            off = v.storage_offset() - self.parent.storage_offset()
            inside[torch.as_strided(idx, v.shape, v.stride(), off).reshape(-1)] = True
        a = self.parent.reshape(-1).view(torch.uint8 if self.parent.element_size() == 1 else torch.int16
                                         if self.parent.element_size() == 2 else torch.int32)
        b = self.before.reshape(-1).view(a.dtype)
        bad = (~inside) & (a != b)
        assert not bool(bad.any()), f"{int(bad.sum())} elements outside the output view changed (first at {int(bad.nonzero()[0])})"


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: a copy of launch()'s predicates (csrc/gemm_mfma.hip) -> the instantiation a product reaches
# ---------------------------------------------------------------------------------------------------------------------------
BT, BK = 128, 64


def owned_rows(tiles_r, tiles_c, C, per_cu, ncu):
    slots, tiles = ncu * per_cu, tiles_r * tiles_c
    if tiles % slots == 0:
        return 0
    rounds = (tiles + slots - 1) // slots
    n_c = rounds * slots // tiles_r
    if n_c <= tiles_c:
        return 0
    step = (C + n_c - 1) // n_c
    return step if 64 <= step < BT else 0


def gemm_form(PK, epi, R, C, K, wide_ok, ldp, ldq, ncu, t256=True):
    """(tier label, instantiation, detail) of launch<PK, false, epi>(R, C, K) on ``ncu`` CUs."""
    cdiv = lambda a, b: (a + b - 1) // b
    pk = "true" if PK else "false"
    wide_epi = True  # every epilogue launch() takes is kWide (MEpiWgrad* use their own kernels)
    tiles_r, tiles_c = cdiv(R, BT), cdiv(C, BT)
    glds = K % BK == 0 and (PK or not wide_epi or wide_ok)
    small_c = glds and tiles_r * tiles_c <= 320
    wide_enough = tiles_r * cdiv(C, 128) >= 128
    tiny_c = small_c and tiles_r * cdiv(C, 64) <= 330 and (R <= 1024 or not wide_enough)
    if not PK:
        if t256 and glds and K >= 1024 and R % 8 == 0 and ldp < (1 << 22) and ldq < (1 << 22):
            tr, tc = cdiv(R, 256), cdiv(C, 256)
            tiles = tr * tc
            rounds = cdiv(tiles, ncu)
            if tiles * 4 >= rounds * ncu * 3:
                group = 4 if (tiles >= 2 * ncu and tr >= 8 and tc >= 8) else 0
                return "t256", f"ovqa_t256::kernel<{epi},3>", dict(tiles=tiles, tiles_c=tc, group_c=group)
        if glds and C <= 128 and K % 32 == 0 and K <= 2048 and R % 4 == 0:
            nk = K // 32
            s = 1 if nk <= 16 else 2 if nk <= 32 else 4
            return f"skinny{s}", f"gemm_bf16_skinny_kernel<{epi},{s}>", {}
        if tiny_c:
            return "tiny64x32", f"gemm_bf16_glds_kernel<false,false,{epi},4,4,32,64>", {}
        if small_c:
            return "w16", f"gemm_bf16_glds_kernel<false,false,{epi},3,16,128,128>", dict(
                owned=owned_rows(tiles_r, tiles_c, C, 1, ncu))
    if tiny_c:
        return "tiny", f"gemm_bf16_glds_kernel<{pk},false,{epi},4,8,32,128>", {}
    if small_c:
        return "small", f"gemm_bf16_glds_kernel<{pk},false,{epi},3,8,64,128>", {}
    if glds:
        return "nbuf2", f"gemm_bf16_glds_kernel<{pk},false,{epi},2,8,128,128>", {}
    return "regs", f"gemm_bf16_kernel<{pk},false,{epi}>", {}


# entry points: epilogue variants they can reach, the launch() operands they map to
ENTRY_EPIS = {
    "fwd": ["bias", "nobias", "gelu_preact", "gelu_drop", "residual", "residual_drop"],
    "res32": ["plain", "lnref", "drop"],
    "split3": ["bias"],
    "bwd_wt": ["plain", "gelu_drop", "addend_alias"],
    "bwd": ["plain", "gelu_drop", "addend_alias"],
}
EPI_STRUCT = {("fwd", "bias"): "MEpiBias", ("fwd", "nobias"): "MEpiBias", ("fwd", "gelu_preact"): "MEpiBiasGelu",
              ("fwd", "gelu_drop"): "MEpiBiasGelu", ("fwd", "residual"): "MEpiBiasResidual",
              ("fwd", "residual_drop"): "MEpiBiasResidual"}


def epi_struct(entry, epi):
    return EPI_STRUCT.get((entry, epi)) or {"res32": "MEpiBiasRes32", "split3": "MEpiBiasSplit3", "bwd_wt": "MEpiBwdData",
                                            "bwd": "MEpiBwdData"}[entry]


# (id, entry, M, N, K, intended tier, extra, why).  M = activation rows, N = output features of fwd / res32 / split3 (3 F),
# reduction length of bwd / bwd_wt; K = reduction of fwd, output features (input features of the layer) of bwd / bwd_wt.
# launch() sees R = N (fwd) or K (bwd), C = M, reduction K (fwd) or N (bwd).  Tile counts below are for 256 CUs.
GEMM_ROWS = [
    ("t256_g0_ragged", "fwd", 6000, 2000, 1024, "t256", {},
     "K >= 1024, 8 x 24 = 192 tiles fill 3/4 of a 256-CU round; < 512 tiles: plain raster (group_c 0); R 2000 and C 6000 "
     "ragged in their last 256 tile; 16 K steps"),
    ("t256_g4_remap", "fwd", 12500, 3000, 1088, "t256", {},
     "12 x 49 = 588 tiles (3 rounds, >= 3/4 full): grouped raster (group_c 4) with tiles_c % 4 = 1 (a short last group), "
     "588 % 8 = 4 (XCD remap with a remainder), ragged R and C, 17 K steps"),
    ("t256_res32", "res32", 6000, 2000, 1024, "t256", {}, "as t256_g0_ragged, fp32 residual epilogue"),
    ("t256_res32_g4", "res32", 12500, 3000, 1088, "t256", {}, "as t256_g4_remap, fp32 residual epilogue"),
    ("t256_split3", "split3", 6000, 2016, 1024, "t256", {"slots": True},
     "3 F = 2016: 8 x 24 tiles; the three outputs are column blocks of one wider buffer (gaps between them)"),
    ("t256_bwd_wt", "bwd_wt", 6000, 1024, 2000, "t256", {},
     "dX from the transposed weight: R = 2000 input features, C = 6000, reduction 1024"),
    ("skinny1", "fwd", 17, 4000, 512, "skinny1", {}, "C = 17 <= 128 rows, K / 32 = 16 <= 16"),
    ("skinny2", "fwd", 100, 512, 1024, "skinny2", {}, "C = 100, K / 32 = 32; 2 x 1 256-tiles are far from a round"),
    ("skinny4", "fwd", 64, 768, 2048, "skinny4", {}, "C = 64, K / 32 = 64 > 32"),
    ("skinny_res32", "res32", 40, 512, 512, "skinny1", {}, "C = 40 rows"),
    ("skinny_bwd_wt", "bwd_wt", 64, 512, 768, "skinny1", {}, "dX of 64 rows: R = 768, C = 64, reduction 512"),
    ("tiny64x32", "fwd", 1280, 512, 512, "tiny64x32", {}, "4 x 10 128-tiles <= 320, 4 x 20 64-wide <= 330, R = 512 <= 1024"),
    ("tiny64x32_res32", "res32", 1280, 512, 512, "tiny64x32", {}, "as tiny64x32"),
    ("tiny64x32_bwd_wt", "bwd_wt", 1280, 2048, 512, "tiny64x32", {}, "R = 512, C = 1280, reduction 2048 (K < 1024? no: t256 "
     "needs >= 192 256-tiles, this has 10)"),
    ("tiny64x32_split3", "split3", 1280, 768, 512, "tiny64x32", {"slots": True}, "3 F = 768: 6 x 10 tiles, 6 x 20 <= 330"),
    ("w16_owned", "fwd", 1280, 2048, 512, "w16", {"owned": True},
     "16 x 10 = 160 <= 320 tiles; R = 2048 > 1024 with 160 >= 128 tiles leaves the tiny tier; 160 of 256 slots -> owned "
     "c steps of 80 rows"),
    ("w16_full", "fwd", 2048, 2048, 512, "w16", {"owned": False}, "16 x 16 = 256 tiles = one whole round: no owned rows"),
    ("w16_res32_owned", "res32", 6400, 512, 512, "w16", {"owned": True}, "4 x 50 = 200 tiles, 4 x 100 > 330: owned steps of 100"),
    ("w16_bwd_wt", "bwd_wt", 6400, 2048, 512, "w16", {"owned": True}, "R = 512, C = 6400: 4 x 50 tiles"),
    ("kmajor_tiny", "bwd", 640, 2048, 512, "tiny", {}, "k-major P (dX from the [N, K] weight): R = 512, 4 x 5 tiles"),
    ("kmajor_small", "bwd", 1280, 512, 2048, "small", {}, "R = 2048, C = 1280: 160 tiles, R > 1024 and >= 128 tiles"),
    ("kmajor_nbuf2", "bwd", 6400, 512, 2048, "nbuf2", {}, "16 x 50 = 800 > 320 tiles"),
    ("nbuf2", "fwd", 6400, 2048, 512, "nbuf2", {}, "16 x 50 = 800 > 320 tiles, K = 512 < 1024"),
    ("nbuf2_res32", "res32", 6400, 2048, 512, "nbuf2", {}, "as nbuf2"),
    ("nbuf2_bwd_wt", "bwd_wt", 6400, 512, 2048, "nbuf2", {}, "R = 2048, C = 6400, reduction 512"),
    ("regs_k520", "fwd", 300, 768, 520, "regs", {}, "K % 64 != 0: the register-staged kernel"),
    ("regs_res32_k520", "res32", 300, 768, 520, "regs", {}, "K % 64 != 0"),
    ("regs_ld516", "fwd", 1280, 512, 512, "regs", {"ld": 516},
     "out= view with ld % 8 != 0: wide_ok == false for a kWide epilogue -> no direct-to-LDS form"),
    ("regs_bwd_wt_ld", "bwd_wt", 1280, 512, 512, "regs", {"ld": 516}, "dx view with ld % 8 != 0"),
    ("kmajor_regs", "bwd", 300, 520, 768, "regs", {}, "reduction N = 520: K % 64 != 0 with a k-major P"),
    # split3 goes through the whole ladder (mfma_linear_fwd_split3_supported: F % 8, K % 8); skinny1 is the greedy
    # decoding step's fused K | V projection (64 rows)
    ("split3_skinny1", "split3", 64, 1536, 512, "skinny1", {"slots": True}, "C = 64 rows, K / 32 = 16"),
    ("split3_skinny2", "split3", 100, 768, 1024, "skinny2", {"slots": True}, "C = 100, K / 32 = 32"),
    ("split3_skinny4", "split3", 64, 768, 2048, "skinny4", {"slots": True}, "C = 64, K / 32 = 64"),
    ("split3_w16", "split3", 1280, 3072, 512, "w16", {"slots": True, "owned": False},
     "3 F = 3072: 24 x 10 = 240 <= 320 tiles, 24 x 20 > 330 leaves the tiny tier; 256 / 24 = 10 c tiles: no owned steps"),
    ("split3_nbuf2", "split3", 6400, 1536, 512, "nbuf2", {"slots": True}, "12 x 50 = 600 > 320 tiles"),
    ("split3_regs", "split3", 300, 768, 520, "regs", {"slots": True}, "K % 64 != 0"),
    ("res32_skinny2", "res32", 40, 512, 1024, "skinny2", {}, "C = 40, K / 32 = 32"),
    ("res32_skinny4", "res32", 40, 512, 2048, "skinny4", {}, "C = 40, K / 32 = 64"),
    ("bwd_wt_skinny2", "bwd_wt", 64, 1024, 768, "skinny2", {}, "dX of 64 rows, reduction 1024"),
    ("bwd_wt_skinny4", "bwd_wt", 64, 2048, 768, "skinny4", {}, "dX of 64 rows, reduction 2048"),
]


def gemm_operands(entry, M, N, K, extra):
    """launch() arguments (R, C, K, wide_ok, ldp, ldq) of an entry point's product."""
    ld = extra.get("ld")
    wide_ok = ld is None or ld % 8 == 0
    if entry in ("fwd", "res32", "split3"):
        return False, N, M, K, wide_ok, K, K
    if entry == "bwd_wt":
        return False, K, M, N, wide_ok, N, N
    return True, K, M, N, True, K, N


def expected_gemm(row, epi):
    rid, entry, M, N, K, tier, extra, why = row
    PK, R, C, KK, wide_ok, ldp, ldq = gemm_operands(entry, M, N, K, extra)
    ncu = cus()
    got_tier, inst, det = gemm_form(PK, epi_struct(entry, epi), R, C, KK, wide_ok, ldp, ldq, ncu)
    if got_tier != tier:
        pytest.skip(f"{rid}: on {ncu} CUs this product lands on {got_tier}, not {tier} (the row is for 256 CUs)")
    if "owned" in extra and bool(det.get("owned")) != extra["owned"]:
        pytest.skip(f"{rid}: on {ncu} CUs owned_rows = {det.get('owned')} (the row is for 256 CUs)")
    if rid == "t256_g4_remap" or rid == "t256_res32_g4":
        if not (det["group_c"] == 4 and det["tiles_c"] % 4 and det["tiles"] % 8):
            pytest.skip(f"{rid}: on {ncu} CUs {det} (grouped raster with a short group and a partial XCD needs 256 CUs)")
    if rid in ("t256_g0_ragged", "t256_res32") and det["group_c"] != 0:
        pytest.skip(f"{rid}: on {ncu} CUs group_c = {det['group_c']}")
    return [inst]


def bar_gemm(absprod_max, ref_max, K, bf16_out=True):
    """Bar of a GEMM output, normalised by max |ref| (worst-case bounds, no headroom factor):
      * accumulation: K bf16 x bf16 products (exact in fp32) summed in fp32 in any order: |err| <= K 2^-24 sum_k |x_k w_k|
        (gamma_K);
      * epilogue: at most 64 further fp32 roundings of values no larger than max(sum_k |x_k w_k|, max |ref|) -- bias add,
        the erf-based GELU / GELU', the dropout scale, the residual add, the LayerNorm recomputed from saved statistics;
      * a bf16 output is rounded once more: <= 2^-8 |y| <= U max |ref|.
    Bar = U (bf16 outputs only) + (K + 64) 2^-24 max(sum |x w|, max |ref|) / max |ref|."""
    return (U if bf16_out else 0.0) + (K + 64) * EPS32 * max(absprod_max, ref_max) / ref_max


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def run_gemm(entry, epi, M, N, K, extra, o):
    """Run one entry point; return (outputs to check [(name, got, ref, absprod, bf16_out, ref_dropped)], views, call)."""
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    drop = o.DropSpec(p=0.25, seed=77, site=5, step=step)
    ld = extra.get("ld")
    kd = min(64, K if entry in ("fwd", "res32", "split3") else N)
    if entry in ("fwd", "res32", "split3"):
        x, w = rnd(M, K, dtype=BF16), rnd(N, K, dtype=BF16, scale=K ** -0.5, seed=1)
        b = rnd(N, seed=2)
        xd, wd = x.double(), w.double()
        prod = xd @ wd.t()
        prod_drop = xd[:, :K - kd] @ wd[:, :K - kd].t()
        absprod = (xd.abs() @ wd.abs().t()).max().item()
    if entry == "fwd":
        keep = o.dropout_keep_mask(drop, M * N, DEV).view(M, N).double() / 0.75
        res = rnd(M, N, dtype=BF16, seed=3)
        sent, y = None, None
        if ld is not None:
            sent = Sentinel((M, ld), BF16)
            y = sent.view(lambda p: p[:, :N])
        bias = None if epi == "nobias" else b
        bd = 0 if bias is None else b.double()
        if epi in ("bias", "nobias"):
            call = lambda: o.linear_fwd(x, w, bias, out=y)
            f = lambda p: p + bd
        elif epi == "gelu_preact":
            call = lambda: o.linear_fwd(x, w, b, o.EPI_BIAS_GELU, want_preact=True, out=y)
            f = lambda p: gelu(p + bd)
        elif epi == "gelu_drop":
            call = lambda: o.linear_fwd(x, w, b, o.EPI_BIAS_GELU, drop=drop, out=y)
            f = lambda p: gelu(p + bd) * keep
        elif epi == "residual":
            call = lambda: o.linear_fwd(x, w, b, o.EPI_BIAS_RESIDUAL, residual=res, out=y)
            f = lambda p: p + bd + res.double()
        else:
            call = lambda: o.linear_fwd(x, w, b, o.EPI_BIAS_RESIDUAL, residual=res, drop=drop, out=y)
            f = lambda p: res.double() + (p + bd) * keep
        out, log = launched(call)
        checks = []
        if epi == "gelu_preact":
            yv, pre = out
            checks.append(("preact", pre, prod + bd, absprod, True, prod_drop + bd))
            checks.append(("y", yv, f(prod), absprod, True, f(prod_drop)))
        else:
            checks.append(("y", out, f(prod), absprod, True, f(prod_drop)))
        views = [] if sent is None else [(sent, [checks[-1][1]])]
        return checks, views, log
    if entry == "res32":
        keep = o.dropout_keep_mask(drop, M * N, DEV).view(M, N).double() / 0.75
        if epi == "lnref":
            prev = rnd(M, N, scale=2.0, seed=4) + 0.3
            g, be = rnd(N, seed=5) * 0.2 + 1.0, rnd(N, seed=6) * 0.1
            _, _, mean, rstd = o.layernorm_fwd(prev, g, be, 1e-5, out_dtype=BF16, want_f32=True)
            pd = prev.double()
            mu, var = pd.mean(-1, keepdim=True), pd.var(-1, unbiased=False, keepdim=True)
            rres = (pd - mu) / torch.sqrt(var + 1e-5) * g.double() + be.double()
            res = o.LnRef(prev, mean, rstd, g, be, 1e-5)
        else:
            res = rnd(M, N, scale=2.0, seed=4)
            rres = res.double()
        d = drop if epi == "drop" else None
        kk = keep if epi == "drop" else 1.0
        out, log = launched(lambda: o.linear_fwd_res32(x, w, b, res, drop=d))
        ref = rres + (prod + b.double()) * kk
        refd = rres + (prod_drop + b.double()) * kk
        # (an LnRef residual is recomputed in fp32 from the saved statistics: a few eps32 of its own scale more, covered
        # by the 16 eps term of bar_gemm)
        return [("pre32", out, ref, absprod, False, refd)], [], log
    if entry == "split3":
        F = N // 3
        gap = 8
        sent = Sentinel((M, 3 * F + 3 * gap), BF16)
        outs = [sent.view(lambda p, i=i: p[:, i * (F + gap):i * (F + gap) + F]) for i in range(3)]
        _, log = launched(lambda: o.linear_fwd_split3(x, w, b, outs))
        ref, refd = prod + b.double(), prod_drop + b.double()
        checks = [(f"y{i}", outs[i], ref[:, i * F:(i + 1) * F], absprod, True, refd[:, i * F:(i + 1) * F]) for i in range(3)]
        return checks, [(sent, outs)], log
    # dX: dy [M, N] (N = reduction), w [N, K]
    dy, w = rnd(M, N, dtype=BF16), rnd(N, K, dtype=BF16, scale=N ** -0.5, seed=1)
    dyd, wd = dy.double(), w.double()
    prod, prod_drop = dyd @ wd, dyd[:, :N - kd] @ wd[:N - kd]
    absprod = (dyd.abs() @ wd.abs()).max().item()
    pre = rnd(M, K, dtype=BF16, seed=7)
    keep = o.dropout_keep_mask(drop, M * K, DEV).view(M, K).double() / 0.75
    wt = w.t().contiguous()
    sent, dx = None, None
    if ld is not None:
        sent = Sentinel((M, ld), BF16)
        dx = sent.view(lambda p: p[:, :K])
    fn = o.linear_bwd_data_wt if entry == "bwd_wt" else o.linear_bwd_data
    wop = wt if entry == "bwd_wt" else w
    if epi == "plain":
        out, log = launched(lambda: fn(dy, wop, out=dx))
        f = lambda p: p
    elif epi == "gelu_drop":
        out, log = launched(lambda: fn(dy, wop, preact=pre, drop=drop, out=dx))
        f = lambda p: p * keep * gelu_grad(pre.double())
    else:
        base = rnd(M, K, dtype=BF16, seed=8)
        if dx is None:
            dx = base.clone()
        else:
            dx.copy_(base)
            sent.before.copy_(sent.parent)
        out, log = launched(lambda: fn(dy, wop, out=dx, addend=dx))  # the addend aliases the output
        f = lambda p: p + base.double()
    views = [] if sent is None else [(sent, [out])]
    return [("dx", out, f(prod), absprod, True, f(prod_drop))], views, log


GEMM_CASES = [pytest.param(r, e, id=f"{r[0]}-{e}") for r in GEMM_ROWS for e in ENTRY_EPIS[r[1]]
              if not (r[2] * r[3] * r[4] > 2e10 and e not in (ENTRY_EPIS[r[1]][0], ENTRY_EPIS[r[1]][-1]))]


@pytest.mark.parametrize("row,epi", GEMM_CASES)
def test_gemm_route_parity(row, epi, request):
    rid, entry, M, N, K, tier, extra, why = row
    expect = expected_gemm(row, epi)
    o = ops()
    checks, views, log = run_gemm(entry, epi, M, N, K, extra, o)
    red = N if entry in ("bwd", "bwd_wt") else K
    for name, got, ref, absprod, bf16_out, ref_dropped in checks:
        rmax = ref.abs().max().item()
        bar = bar_gemm(absprod, rmax, red, bf16_out)
        e = record(request, f"{rid}/{epi}/{name}", rel_max(got, ref), bar)
        assert e <= bar, (rid, epi, name, e, bar)
        # the bar sees a dropped pipeline stage: the last 64-deep K step left out moves the result by >= 10 bars
        sens = rel_max(ref_dropped, ref)
        assert sens >= 10 * bar, (rid, name, sens, bar)
    for sent, vs in views:
        sent.check(*vs)
    check_route(log, expect)


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def att_ref(q, k, v, mask, H, keep=None, drop_keys=0):
    """fp64 attention; ``drop_keys`` masks out the last keys (the 'lost key tile' of the sensitivity check)."""
    B, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    dk, dv = q.shape[2] // H, v.shape[2] // H
    qh = q.double().view(B, nq, H, dk).transpose(1, 2)
    kh = k.double().view(B, nk, H, dk).transpose(1, 2)
    vh = v.double().view(B, nk, H, dv).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dk)
    if mask is not None:
        s = s + mask.double()
    if drop_keys:
        s = s.clone()
        s[..., nk - drop_keys:] = float("-inf")
    p = torch.softmax(s, -1)
    pk = p if keep is None else p * keep
    o = (pk @ vh).transpose(1, 2).reshape(B, nq, H * dv)
    return o, p, pk, vh, torch.logsumexp(s, -1)


def lost_tile(nk):
    return 32 if nk > 32 else max(1, nk // 2)


def bar_att(o_ref, pk, vh, B, nq, H):
    """Bar of a bf16 attention output o = P~ V, normalised by max |o| (worst-case bound, no headroom factor).  Each
    probability carries the fp32 softmax's error (exp, a running max, a sum of n_k terms, the 1 / l scale: <= (n_k + 8) 2^-24
    relative) and is then rounded to bf16 for the P V product (<= 2^-8 relative): |err_i| <= (U + (n_k + 8) 2^-24)
    sum_j |p~_ij| |v_j|; the fp32 accumulation of the products adds n_k 2^-24 of the same sum; o is rounded once
    (<= U |o_i|).  Bar = (U max|o| + (U + (2 n_k + 8) 2^-24) T) / max|o|, T = max_i sum_j |p~_ij| |v_j|."""
    t = (pk @ vh.abs()).transpose(1, 2).reshape(B, nq, -1).abs().max().item()
    m = o_ref.abs().max().item()
    nk = pk.shape[-1]
    return (U * m + (U + (2 * nk + 8) * EPS32) * t) / m


def make_mask(kind, B, nq, nk, seed=4):
    if kind == "key":
        m = torch.zeros(B, 1, 1, nk, device=DEV)
        m[0, ..., nk - max(1, nk // 4):] = -1e5
        return m
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, 1, nq, nk, generator=g) < 0.2).float() * -1e5
    m[..., 0] = 0  # every query sees at least one key
    return m.to(DEV)


def attention_fwd_into(q, k, v, mask, H, o, lo, need_att=False, drop=None):
    """ovqa_attention_fwd with o and its rounding residual o_lo written into caller views of one packed buffer (row stride
    ldo shared, as the C ABI defines it); returns (lse, att)."""
    import ctypes as C
    from openvivqa_amd import _lib
    o_ = ops()
    B, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    dk, dv = q.shape[2] // H, v.shape[2] // H
    assert o.stride() == lo.stride() and o.stride(-1) == 1
    lse = torch.empty(B, H, nq, dtype=torch.float32, device=DEV)
    att = torch.empty(B, H, nq, nk, dtype=q.dtype, device=DEV) if need_att else None
    m, sb, sh, sq = o_._mask_strides(mask, B, H, nq, nk)
    _lib.check(_lib.load().ovqa_attention_fwd(
        o_._dt(q), o_._p(q), o_._rows(q)[0], o_._p(k), o_._rows(k)[0], o_._p(v), o_._rows(v)[0], o_._p(m), sb, sh, sq,
        o_._p(o), o_._rows(o)[0], o_._p(lse), o_._p(att), o_._p(lo), B, H, nq, nk, dk, dv, 1.0 / math.sqrt(dk),
        o_._drop(drop), o_._stream()), "attention_fwd")
    return lse, att


ATT_FWD_NK = {1: 20, 2: 64, 4: 100, 6: 160, 8: 250}
ATT_FWD_CASES = [pytest.param(nkt, d, mk, att, dr, id=f"nkt{nkt}-d{d}-{mk}{'-att' if att else ''}{'-drop' if dr else ''}")
                 for nkt in (1, 2, 4, 6, 8) for d in (64, 96, 128) if not (nkt == 8 and d != 64)
                 for mk in ("key", "square") for att in (False, True) for dr in (False, True)]


@pytest.mark.parametrize("nkt,d,mk,need_att,dr", ATT_FWD_CASES)
def test_attention_fwd_route_parity(nkt, d, mk, need_att, dr, request):
    """attn_fwd_mfma_kernel<NKT, ROWMASK, WANT_ATT, D, DROP>: NKT = ceil(n_k / 32) in {1, 2, 4, 6, 8} (launch_fwd_d), a key
    row (ROWMASK) or a square mask, the probabilities written or not, dropout on the probabilities or not."""
    o_ = ops()
    B, H, nq, nk = 2, 2, 40, ATT_FWD_NK[nkt]
    q, k, v = rnd(B, nq, H * d, dtype=BF16, seed=1), rnd(B, nk, H * d, dtype=BF16, seed=2), rnd(B, nk, H * d, dtype=BF16, seed=3)
    mask = make_mask(mk, B, nq, nk)
    drop, keep = None, None
    if dr:
        drop = o_.DropSpec(p=0.2, seed=31, site=9, step=torch.tensor([2], dtype=torch.int32, device=DEV))
        keep = o_.dropout_keep_mask(drop, B * H * nq * nk, DEV).view(B, H, nq, nk).double() / 0.8
    sent = Sentinel((B, nq, 3 * H * d), BF16)  # o | gap | o_lo in one packed buffer
    out, lo = sent.view(lambda p: p[..., :H * d]), sent.view(lambda p: p[..., 2 * H * d:])
    (lse, att), log = launched(lambda: attention_fwd_into(q, k, v, mask, H, out, lo, need_att=need_att, drop=drop))
    sent.check(out, lo)
    ro, rp, rpk, vh, rl = att_ref(q, k, v, mask, H, keep)
    bar = bar_att(ro, rpk, vh, B, nq, H)
    e = record(request, "o", rel_max(out, ro), bar)
    assert e <= bar, (e, bar)
    e = record(request, "o+o_lo", rel_max(out.double() + lo.double(), ro), bar)  # the fp32 output: within the p~ term
    assert e <= bar, (e, bar)
    ro2 = att_ref(q, k, v, mask, H, keep, drop_keys=lost_tile(nk))[0]
    assert rel_max(ro2, ro) >= 10 * bar
    # lse: fp32 log-sum-exp of fp32 scores of bf16 operands: scores carry <= d * 2^-24 * sum|q||k| * scale; bar 1e-5 absolute
    # relative to max|lse| plus that term is far below a lost tile (checked by the o bar above)
    el = record(request, "lse", rel_max(lse, rl), 1e-4)
    assert el <= 1e-4
    if need_att:
        ea = record(request, "att", rel_max(att, rpk.float().double()), U)
        assert ea <= U  # one bf16 rounding of fp32 probabilities (x keep / (1 - p)): U / 2 relative, bar U
    rm = "true" if mk == "key" else "false"
    check_route(log, [f"attn_fwd_mfma_kernel<{nkt},{rm},{'true' if need_att else 'false'},{d},{'true' if dr else 'false'}>"])


PREFIX_ROWS = [(2, 100, 12, 64), (2, 182, 12, 96), (2, 64, 1, 128), (2, 37, 37, 64), (1, 250, 20, 64)]


@pytest.mark.parametrize("B,n,tail,d", PREFIX_ROWS, ids=[f"n{r[1]}-tail{r[2]}-d{r[3]}" for r in PREFIX_ROWS])
def test_attention_fwd_prefix_lm_route_parity(B, n, tail, d, request):
    """ovqa_attention_fwd_prefix_lm: the key-mask row plus a causal corner among the last ``tail`` positions, computed in
    attn_fwd_mfma_kernel<NKT, true, false, D, false>, against fp64 attention on the dense mask (mmf_m4c.py:310-340)."""
    o_ = ops()
    H = 2
    q, k, v = (rnd(B, n, H * d, dtype=BF16, seed=s) for s in (1, 2, 3))
    row = torch.zeros(B, 1, 1, n, device=DEV)
    row[0, :, :, 3:7] = -10000.0
    dense = row.repeat(1, 1, n, 1)
    if tail:
        dense[:, :, -tail:, -tail:] += torch.full((tail, tail), float("-inf"), device=DEV).triu(1)
    if not o_.attention_fwd_prefix_lm_ok(q, H):
        pytest.skip("parity and route need the prefix-LM kernel, which OVQA_FORCE_SIMPLE / OVQA_NO_PREFIX_LM switch off")
    out, log = launched(lambda: o_.attention_fwd_prefix_lm(q, k, v, row, tail, H))
    ro, _, rpk, vh, _ = att_ref(q, k, v, dense, H)
    bar = bar_att(ro, rpk, vh, B, n, H)
    e = record(request, "o", rel_max(out, ro), bar)
    assert e <= bar, (e, bar)
    assert rel_max(att_ref(q, k, v, dense, H, drop_keys=lost_tile(n))[0], ro) >= 10 * bar
    nkt = 1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 6 if n <= 192 else 8  # (launch_fwd_d)
    check_route(log, [f"attn_fwd_mfma_kernel<{nkt},true,false,{d},false>"])


def bwd_ref(q, k, v, mask, H, d_o, keep=None, drop_keys=0):
    qd, kd, vd = (t.double().detach().clone().requires_grad_(True) for t in (q, k, v))
    o, p, pk, vh, _ = att_ref(qd, kd, vd, mask, H, keep, drop_keys)
    o.backward(d_o.double())
    return qd.grad, kd.grad, vd.grad, p.detach(), pk.detach()


def bar_bwd(name, ref, q, k, v, d_o, p, pk, mask, H, keep):
    """Bars of dq / dk / dv (bf16), normalised by max |ref| (worst-case rounding bound).  The last contraction of each runs
    on bf16 operands: dV = P~^T dO (P~ rounded: <= 2^-8 |p~| per term), dQ = scale dS K and dK = scale dS^T Q (dS = P (dP -
    delta) rounded to bf16: <= 2^-8 |dS| per term), then the output is rounded once (<= U |ref|).  Bar = U (max|ref| +
    max T) / max|ref| with T the same contraction of absolute values.  dP and delta are fp32 sums of exact products (delta
    from o + o_lo) and P is recomputed in fp32 from the saved lse: their relative errors are O(n 2^-24), two orders below
    U, and enter dS at most with the weight of |dS| terms themselves -- not bounded separately (measured worst: 0.5 of the
    bar)."""
    B, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    d = q.shape[2] // H
    qh = q.double().view(B, nq, H, d).transpose(1, 2)
    kh = k.double().view(B, nk, H, d).transpose(1, 2)
    vh = v.double().view(B, nk, H, d).transpose(1, 2)
    doh = d_o.double().view(B, nq, H, d).transpose(1, 2)
    if name == "dv":
        t = pk.transpose(-1, -2) @ doh.abs()
    else:
        dp = doh @ vh.transpose(-1, -2)
        if keep is not None:
            dp = dp * keep
        delta = (p * dp).sum(-1, keepdim=True)
        ds = (p * (dp - delta)).abs() / math.sqrt(d)
        t = ds @ kh.abs() if name == "dq" else ds.transpose(-1, -2) @ qh.abs()
    m = ref.abs().max().item()
    return U * (m + t.abs().max().item()) / m


# (id, B, H, nq, nk, d, mask kind, dropout, expected instantiations, why)
ATT_BWD_ROWS = [
    ("roles_4x4_dma", 2, 2, 100, 100, 64, "key", False, ["attn_bwd_roles_mfma_kernel<4,4,true,0,true>"],
     "32 < n_k <= 128, n_q <= 128, 4 x 4 tiles, key row: the unrolled direct-to-LDS form"),
    ("roles_4x4_square", 2, 2, 100, 100, 64, "square", False, ["attn_bwd_roles_mfma_kernel<4,4,false,0,false>"],
     "4 x 4 tiles with a square mask"),
    ("roles_generic_key", 2, 2, 70, 50, 64, "key", False, ["attn_bwd_roles_mfma_kernel<0,0,true,0,false>"], "3 x 2 tiles"),
    ("roles_generic_square", 2, 2, 128, 40, 64, "square", False, ["attn_bwd_roles_mfma_kernel<0,0,false,0,false>"], "4 x 2 tiles"),
    ("smallk_w1g2_key", 2, 2, 20, 20, 64, "key", False, ["attn_bwd_smallk_mfma_kernel<true,1,2>"],
     "n_k <= 32, one query tile, B H = 4: (4 + 3) / 4 < 256 -> two problems per workgroup"),
    ("smallk_w1g2_square", 2, 2, 20, 20, 64, "square", False, ["attn_bwd_smallk_mfma_kernel<false,1,2>"], "as above"),
    ("smallk_w1g4_key", 128, 8, 20, 20, 64, "key", False, ["attn_bwd_smallk_mfma_kernel<true,1,4>"],
     "B H = 1024 >= 1021: four single-tile problems per workgroup"),
    ("smallk_w1g4_square", 128, 8, 20, 20, 64, "square", False, ["attn_bwd_smallk_mfma_kernel<false,1,4>"], "as above"),
    ("smallk_w2_key", 3, 2, 50, 32, 64, "key", False, ["attn_bwd_smallk_mfma_kernel<true,2,2>"], "two query tiles"),
    ("smallk_w2_square", 3, 2, 50, 32, 64, "square", False, ["attn_bwd_smallk_mfma_kernel<false,2,2>"], "two query tiles"),
    ("smallk_w4_key", 2, 3, 70, 13, 64, "key", False, ["attn_bwd_smallk_mfma_kernel<true,4,1>"], "three (-> four) tiles"),
    ("smallk_w4_square", 2, 2, 128, 20, 64, "square", False, ["attn_bwd_smallk_mfma_kernel<false,4,1>"], "four tiles"),
    ("two_d64_drop_key", 2, 2, 40, 50, 64, "key", True,
     ["attn_bwd_dq_mfma_kernel<true,64,true>", "attn_bwd_dkv_mfma_kernel<true,64,true>"], "dropout: the two-kernel form"),
    ("two_d64_long_square", 1, 2, 150, 160, 64, "square", False,
     ["attn_bwd_dq_mfma_kernel<false,64,false>", "attn_bwd_dkv_mfma_kernel<false,64,false>"], "n_k > 128"),
    ("two_d96_key", 2, 2, 40, 50, 96, "key", False,
     ["attn_bwd_dq_mfma_kernel<true,96,false>", "attn_bwd_dkv_mfma_kernel<true,96,false>"], "d = 96"),
    ("two_d96_drop_square", 2, 2, 40, 50, 96, "square", True,
     ["attn_bwd_dq_mfma_kernel<false,96,true>", "attn_bwd_dkv_mfma_kernel<false,96,true>"], "d = 96 with dropout"),
    ("two_d128_square", 2, 2, 40, 50, 128, "square", False,
     ["attn_bwd_dq_mfma_kernel<false,128,false>", "attn_bwd_dkv_mfma_kernel<false,128,false>"], "d = 128"),
    ("two_d128_drop_key", 2, 2, 40, 50, 128, "key", True,
     ["attn_bwd_dq_mfma_kernel<true,128,true>", "attn_bwd_dkv_mfma_kernel<true,128,true>"], "d = 128 with dropout"),
    ("two_d64_key", 2, 2, 150, 20, 64, "key", False,
     ["attn_bwd_dq_mfma_kernel<true,64,false>", "attn_bwd_dkv_mfma_kernel<true,64,false>"], "n_k <= 32 but n_q > 128"),
    ("two_d64_drop_square", 2, 2, 40, 50, 64, "square", True,
     ["attn_bwd_dq_mfma_kernel<false,64,true>", "attn_bwd_dkv_mfma_kernel<false,64,true>"], "dropout, square mask"),
    ("two_d96_drop_key", 2, 2, 40, 50, 96, "key", True,
     ["attn_bwd_dq_mfma_kernel<true,96,true>", "attn_bwd_dkv_mfma_kernel<true,96,true>"], "d = 96, dropout"),
    ("two_d96_square", 2, 2, 40, 50, 96, "square", False,
     ["attn_bwd_dq_mfma_kernel<false,96,false>", "attn_bwd_dkv_mfma_kernel<false,96,false>"], "d = 96"),
    ("two_d128_key", 2, 2, 40, 50, 128, "key", False,
     ["attn_bwd_dq_mfma_kernel<true,128,false>", "attn_bwd_dkv_mfma_kernel<true,128,false>"], "d = 128"),
    ("two_d128_drop_square", 2, 2, 40, 50, 128, "square", True,
     ["attn_bwd_dq_mfma_kernel<false,128,true>", "attn_bwd_dkv_mfma_kernel<false,128,true>"], "d = 128, dropout"),
]


def run_att_bwd(row, o_):
    rid, B, H, nq, nk, d, mk, dr, expect, why = row
    q = rnd(B, nq, H * d, dtype=BF16, seed=1)
    kv = rnd(B, nk, 3 * H * d, dtype=BF16, seed=2)  # packed K | V | spare: k, v strided views
    k, v = kv[..., :H * d], kv[..., H * d:2 * H * d]
    mask = make_mask(mk, B, nq, nk)
    drop, keep = None, None
    if dr:
        drop = o_.DropSpec(p=0.2, seed=41, site=3, step=torch.tensor([5], dtype=torch.int32, device=DEV))
        keep = o_.dropout_keep_mask(drop, B * H * nq * nk, DEV).view(B, H, nq, nk).double() / 0.8
    lo = []
    out, lse, _ = o_.attention_fwd(q, k, v, mask, H, att_drop=drop, lo_out=lo)
    d_o = rnd(B, nq, H * d, dtype=BF16, seed=5)
    sent = Sentinel((B, nk, 3 * H * d), BF16)  # dk | dv written into a packed buffer
    dkv = (sent.view(lambda p: p[..., :H * d]), sent.view(lambda p: p[..., H * d:2 * H * d]))
    (dq, dk, dv), log = launched(lambda: o_.attention_bwd(d_o, q, k, v, out, lse, mask, H, dk=dkv[0], dv=dkv[1],
                                                          att_drop=drop, o_lo=lo[0]))
    sent.check(dk, dv)
    return (q, k, v, mask, H, d_o, keep), (dq, dk, dv), log


@pytest.mark.parametrize("row", [pytest.param(r, id=r[0]) for r in ATT_BWD_ROWS])
def test_attention_bwd_route_parity(row, request):
    o_ = ops()
    args, grads, log = run_att_bwd(row, o_)
    q, k, v, mask, H, d_o, keep = args
    rq, rk, rv, p, pk = bwd_ref(q, k, v, mask, H, d_o, keep)
    for name, got, ref in zip(("dq", "dk", "dv"), grads, (rq, rk, rv)):
        bar = bar_bwd(name, ref, q, k, v, d_o, p, pk, mask, H, keep)
        e = record(request, name, rel_max(got, ref), bar)
        assert e <= bar, (row[0], name, e, bar)
    nk = k.shape[1]
    rq2 = bwd_ref(q, k, v, mask, H, d_o, keep, drop_keys=lost_tile(nk))[0]
    assert rel_max(rq2, rq) >= 10 * bar_bwd("dq", rq, q, k, v, d_o, p, pk, mask, H, keep)
    check_route(log, row[8])


# qkv_fwd: (id, B, n, H, d_model, expected, why)
QKV_ROWS = [
    ("qkv_32x2_k64", 4, 20, 8, 512, "attn_qkv_fwd_mfma_kernel<32,2,true,64,4>",
     "n <= 32 and ceil(B / 4) H = 8 < 256: two samples per workgroup, d_model % 64 == 0: K steps of 64"),
    ("qkv_32x2_k32", 4, 20, 8, 544, "attn_qkv_fwd_mfma_kernel<32,2,true,32,4>", "as above with d_model % 64 = 32"),
    ("qkv_32x4", 128, 20, 8, 512, "attn_qkv_fwd_mfma_kernel<32,4,true,32,4>", "ceil(128 / 4) 8 = 256: four samples"),
    ("qkv_64x4", 7, 49, 4, 544, "attn_qkv_fwd_mfma_kernel<64,4,true,32,4>", "33-64 positions"),
    ("qkv_128x1_k64", 3, 100, 4, 512, "attn_qkv_fwd_mfma_kernel<128,1,true,64,2>", "65-128 positions, d_model % 64 == 0"),
    ("qkv_128x2_k32", 3, 100, 4, 544, "attn_qkv_fwd_mfma_kernel<128,2,true,32,4>", "65-128 positions, d_model % 64 = 32"),
]


@pytest.mark.parametrize("row", [pytest.param(r, id=r[0]) for r in QKV_ROWS])
def test_attention_qkv_fwd_route_parity(row, request):
    rid, B, n, H, Dm, expect, why = row
    o_ = ops()
    d = 64
    x = rnd(B, n, Dm, dtype=BF16, seed=1)
    w = rnd(3 * H * d, Dm, dtype=BF16, scale=Dm ** -0.5, seed=2)
    b = rnd(3 * H * d, scale=0.1, seed=3)
    mask = make_mask("key", B, n, n)
    (qkv, out, lse), log = launched(lambda: o_.attention_qkv_fwd(x, w, b, mask, H))
    xd, wd = x.double(), w.double()
    ref = xd @ wd.transpose(0, 1) + b.double()
    refd = xd[..., :Dm - 64] @ wd[:, :Dm - 64].t() + b.double()
    absprod = (xd.abs() @ wd.abs().t()).max().item()
    bar = bar_gemm(absprod, ref.abs().max().item(), Dm)
    e = record(request, "qkv", rel_max(qkv, ref), bar)
    assert e <= bar and rel_max(refd, ref) >= 10 * bar
    hd = H * d
    q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
    ro, _, rpk, vh, _ = att_ref(q, k, v, mask, H)  # attention of the STORED projections
    bar = bar_att(ro, rpk, vh, B, n, H)
    e = record(request, "o", rel_max(out, ro), bar)
    assert e <= bar and rel_max(att_ref(q, k, v, mask, H, drop_keys=lost_tile(n))[0], ro) >= 10 * bar
    check_route(log, [expect], off=NO_FUSED_QKV)


# q_fwd: (id, B, nq, nk, H, d_model)
Q_ROWS = [(f"q_nkt{t}_nh{nh}_dm{dm}", B, nq, nk, H, dm, t, nh)
          for (t, nk) in ((1, 20), (2, 50), (4, 100)) for (nh, H) in ((2, 4), (1, 3)) for dm in (512, 768)
          for (B, nq) in ((3, 37),)]


@pytest.mark.parametrize("row", [pytest.param(r, id=r[0]) for r in Q_ROWS])
def test_attention_q_fwd_route_parity(row, request):
    """attn_q_fwd_mfma_kernel<NKT, 3, NH>: NKT from n_k (<= 32, <= 64, else 4), two heads per workgroup where H is even,
    one where it is odd; d_model 512 and 768 (the entry point needs d_model % 64 == 0)."""
    rid, B, nq, nk, H, Dm, nkt, nh = row
    o_ = ops()
    d = 64
    x = rnd(B, nq, Dm, dtype=BF16)
    w = rnd(H * d, Dm, dtype=BF16, scale=Dm ** -0.5, seed=1)
    b = rnd(H * d, seed=2)
    kv = rnd(B, nk, 3 * H * d, dtype=BF16, seed=3)
    k, v = kv[..., H * d:2 * H * d], kv[..., 2 * H * d:]
    mask = make_mask("key", B, nq, nk)
    import ctypes as C
    from openvivqa_amd import _lib
    sent = Sentinel((B, nq, 5 * H * d), BF16)  # q | gap | o | gap | o_lo
    q = sent.view(lambda p: p[..., :H * d])
    out, lo0 = sent.view(lambda p: p[..., 2 * H * d:3 * H * d]), sent.view(lambda p: p[..., 4 * H * d:])
    lse = torch.empty(B, H, nq, dtype=torch.float32, device=DEV)
    m, sb, sh, _ = o_._mask_strides(mask, B, H, nq, nk)
    call = lambda: _lib.check(_lib.load().ovqa_attention_q_fwd(
        o_._dt(x), o_._p(x), Dm, o_._p(w), o_._p(b), o_._p(q), 5 * H * d, o_._p(k), o_._rows(k)[0], o_._p(v),
        o_._rows(v)[0], o_._p(m), sb, sh, o_._p(out), 5 * H * d, o_._p(lse), o_._p(lo0), B, H, nq, nk, Dm, d, 1.0 / 8.0,
        o_._stream()), "attention_q_fwd")
    _, log = launched(call)
    sent.check(q, out, lo0)
    lo = [lo0]
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t() + b.double()
    absprod = (xd.abs() @ wd.abs().t()).max().item()
    bar = bar_gemm(absprod, ref.abs().max().item(), Dm)
    e = record(request, "q", rel_max(q, ref), bar)
    assert e <= bar and rel_max(xd[..., :Dm - 64] @ wd[:, :Dm - 64].t() + b.double(), ref) >= 10 * bar
    ro, _, rpk, vh, _ = att_ref(q, k, v, mask, H)
    bar = bar_att(ro, rpk, vh, B, nq, H)
    e = record(request, "o", rel_max(out, ro), bar)
    assert e <= bar and rel_max(att_ref(q, k, v, mask, H, drop_keys=lost_tile(nk))[0], ro) >= 10 * bar
    # o + o_lo carries the fp32 output: within the p~ rounding term alone
    e = record(request, "o+o_lo", rel_max(out.double() + lo[0].double(), ro), bar)
    assert e <= bar
    check_route(log, [f"attn_q_fwd_mfma_kernel<{nkt},3,{nh}>"], off=NO_FUSED_QKV or NO_FUSED_Q)


# bwd_do: (id, B, nq, nk, H, d_model, expected)
DO_ROWS = [
    ("do_roles", 2, 100, 100, 4, 512, "attn_bwd_roles_mfma_kernel<4,4,true,3,true>", "97-128 x 97-128: role-split"),
    ("do_roles_dm768_h3", 2, 128, 97, 3, 768, "attn_bwd_roles_mfma_kernel<4,4,true,3,true>", "odd H, d_model 768"),
    ("do_single", 4, 20, 20, 4, 512, "attn_bwd_do_smallk1_mfma_kernel<4>", "<= 32 queries, even H"),
    ("do_single_dm768", 3, 32, 13, 2, 768, "attn_bwd_do_smallk1_mfma_kernel<4>", "d_model 768"),
    ("do_guided", 3, 100, 20, 4, 512, "attn_bwd_do_smallk_mfma_kernel<3,1>", "65-128 queries, <= 32 keys"),
    ("do_guided_h3_dm768", 2, 70, 32, 3, 768, "attn_bwd_do_smallk_mfma_kernel<3,1>", "odd H, d_model 768"),
]


@pytest.mark.parametrize("row", [pytest.param(r, id=r[0]) for r in DO_ROWS])
def test_attention_bwd_do_route_parity(row, request):
    rid, B, nq, nk, H, Dm, expect, why = row
    o_ = ops()
    d = 64
    q = rnd(B, nq, H * d, dtype=BF16)
    kv = rnd(B, nk, 2 * H * d, dtype=BF16, seed=1)
    k, v = kv[..., :H * d], kv[..., H * d:]
    mask = make_mask("key", B, nq, nk)
    lo = []
    out, lse, _ = o_.attention_fwd(q, k, v, mask, H, lo_out=lo)
    dy = rnd(B, nq, Dm, dtype=BF16, seed=2)
    group = rnd(H * d, 2 * Dm, dtype=BF16, scale=Dm ** -0.5, seed=3)
    wt = group[:, Dm:]  # strided transposed weight [H d, d_model]
    fused = o_.attention_bwd_do_ok(dy, wt, q, k, mask, H)
    assert fused or not ROUTES_DEFAULT, "the row's shape must be covered by the fused form"
    sent = Sentinel((B, nk, 3 * H * d), BF16)
    dk_, dv_ = sent.view(lambda p: p[..., :H * d]), sent.view(lambda p: p[..., 2 * H * d:])
    if fused:
        call = lambda: o_.attention_bwd_do(dy, wt, q, k, v, out, lse, mask, H, dk=dk_, dv=dv_, o_lo=lo[0])
    else:  # (the A/B switches: the separate fc_o dX product + attention backward the library's callers run instead)
        call = lambda: o_.attention_bwd(o_.linear_bwd_data_wt(dy.reshape(B * nq, Dm), wt).view(B, nq, H * d), q, k, v,
                                        out, lse, mask, H, dk=dk_, dv=dv_, o_lo=lo[0])
    (dq, dk, dv), log = launched(call)
    sent.check(dk, dv)
    d_o = (dy.double() @ wt.double().t())  # fp64 fc_o dX
    rq, rk, rv, p, pk = bwd_ref(q, k, v, mask, H, d_o)
    for name, got, ref in zip(("dq", "dk", "dv"), (dq, dk, dv), (rq, rk, rv)):
        # dO is formed inside the kernel and rounded to bf16 once more before the attention products: twice the bar of
        # the plain backward
        bar = 2 * bar_bwd(name, ref, q, k, v, d_o, p, pk, mask, H, None)
        e = record(request, name, rel_max(got, ref), bar)
        assert e <= bar, (rid, name, e, bar)
    rq2 = bwd_ref(q, k, v, mask, H, d_o, drop_keys=lost_tile(nk))[0]
    assert rel_max(rq2, rq) >= 10 * 2 * bar_bwd("dq", rq, q, k, v, d_o, p, pk, mask, H, None)
    check_route(log, [expect], off=NO_FUSED_DO or not fused)


# compiled, never launched (module docstring: the !PK 8-wave tiny / small tiers)
UNREACHABLE_INSTANTIATIONS = sorted(f"gemm_bf16_glds_kernel<false,false,{e},{t}>" for e in (
    "MEpiBias", "MEpiBiasGelu", "MEpiBiasResidual", "MEpiBiasRes32", "MEpiBiasSplit3", "MEpiBwdData")
    for t in ("4,8,32,128", "3,8,64,128"))


# ---------------------------------------------------------------------------------------------------------------------------
# completeness: every instantiation the launch sites of gemm_mfma.hip (launch()), gemm_tile256.h and attention_mfma.hip can
# launch, as a literal list.  A new kernel form without a route row fails here.
# ---------------------------------------------------------------------------------------------------------------------------
ALL_INSTANTIATIONS = sorted("""
ovqa_t256::kernel<MEpiBias,3>
ovqa_t256::kernel<MEpiBiasGelu,3>
ovqa_t256::kernel<MEpiBiasResidual,3>
ovqa_t256::kernel<MEpiBiasRes32,3>
ovqa_t256::kernel<MEpiBiasSplit3,3>
ovqa_t256::kernel<MEpiBwdData,3>
gemm_bf16_skinny_kernel<MEpiBias,1>
gemm_bf16_skinny_kernel<MEpiBias,2>
gemm_bf16_skinny_kernel<MEpiBias,4>
gemm_bf16_skinny_kernel<MEpiBiasGelu,1>
gemm_bf16_skinny_kernel<MEpiBiasGelu,2>
gemm_bf16_skinny_kernel<MEpiBiasGelu,4>
gemm_bf16_skinny_kernel<MEpiBiasResidual,1>
gemm_bf16_skinny_kernel<MEpiBiasResidual,2>
gemm_bf16_skinny_kernel<MEpiBiasResidual,4>
gemm_bf16_skinny_kernel<MEpiBiasRes32,1>
gemm_bf16_skinny_kernel<MEpiBiasRes32,2>
gemm_bf16_skinny_kernel<MEpiBiasRes32,4>
gemm_bf16_skinny_kernel<MEpiBiasSplit3,1>
gemm_bf16_skinny_kernel<MEpiBiasSplit3,2>
gemm_bf16_skinny_kernel<MEpiBiasSplit3,4>
gemm_bf16_skinny_kernel<MEpiBwdData,1>
gemm_bf16_skinny_kernel<MEpiBwdData,2>
gemm_bf16_skinny_kernel<MEpiBwdData,4>
gemm_bf16_glds_kernel<false,false,MEpiBias,4,4,32,64>
gemm_bf16_glds_kernel<false,false,MEpiBiasGelu,4,4,32,64>
gemm_bf16_glds_kernel<false,false,MEpiBiasResidual,4,4,32,64>
gemm_bf16_glds_kernel<false,false,MEpiBiasRes32,4,4,32,64>
gemm_bf16_glds_kernel<false,false,MEpiBiasSplit3,4,4,32,64>
gemm_bf16_glds_kernel<false,false,MEpiBwdData,4,4,32,64>
gemm_bf16_glds_kernel<false,false,MEpiBias,3,16,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasGelu,3,16,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasResidual,3,16,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasRes32,3,16,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasSplit3,3,16,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBwdData,3,16,128,128>
gemm_bf16_glds_kernel<true,false,MEpiBwdData,4,8,32,128>
gemm_bf16_glds_kernel<true,false,MEpiBwdData,3,8,64,128>
gemm_bf16_glds_kernel<true,false,MEpiBwdData,2,8,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBias,2,8,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasGelu,2,8,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasResidual,2,8,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasRes32,2,8,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBiasSplit3,2,8,128,128>
gemm_bf16_glds_kernel<false,false,MEpiBwdData,2,8,128,128>
gemm_bf16_kernel<false,false,MEpiBias>
gemm_bf16_kernel<false,false,MEpiBiasGelu>
gemm_bf16_kernel<false,false,MEpiBiasResidual>
gemm_bf16_kernel<false,false,MEpiBiasRes32>
gemm_bf16_kernel<false,false,MEpiBiasSplit3>
gemm_bf16_kernel<false,false,MEpiBwdData>
gemm_bf16_kernel<true,false,MEpiBwdData>
""".split() + [f"attn_fwd_mfma_kernel<{t},{rm},{a},{d},{dr}>" for t in (1, 2, 4, 6, 8) for d in (64, 96, 128)
               if not (t == 8 and d != 64) for rm in ("true", "false") for a in ("true", "false")
               for dr in ("true", "false")] + """
attn_bwd_roles_mfma_kernel<4,4,true,0,true>
attn_bwd_roles_mfma_kernel<4,4,false,0,false>
attn_bwd_roles_mfma_kernel<0,0,true,0,false>
attn_bwd_roles_mfma_kernel<0,0,false,0,false>
attn_bwd_smallk_mfma_kernel<true,1,2>
attn_bwd_smallk_mfma_kernel<false,1,2>
attn_bwd_smallk_mfma_kernel<true,1,4>
attn_bwd_smallk_mfma_kernel<false,1,4>
attn_bwd_smallk_mfma_kernel<true,2,2>
attn_bwd_smallk_mfma_kernel<false,2,2>
attn_bwd_smallk_mfma_kernel<true,4,1>
attn_bwd_smallk_mfma_kernel<false,4,1>
attn_qkv_fwd_mfma_kernel<32,2,true,64,4>
attn_qkv_fwd_mfma_kernel<32,2,true,32,4>
attn_qkv_fwd_mfma_kernel<32,4,true,32,4>
attn_qkv_fwd_mfma_kernel<64,4,true,32,4>
attn_qkv_fwd_mfma_kernel<128,1,true,64,2>
attn_qkv_fwd_mfma_kernel<128,2,true,32,4>
attn_q_fwd_mfma_kernel<1,3,1>
attn_q_fwd_mfma_kernel<1,3,2>
attn_q_fwd_mfma_kernel<2,3,1>
attn_q_fwd_mfma_kernel<2,3,2>
attn_q_fwd_mfma_kernel<4,3,1>
attn_q_fwd_mfma_kernel<4,3,2>
attn_bwd_roles_mfma_kernel<4,4,true,3,true>
attn_bwd_do_smallk1_mfma_kernel<4>
attn_bwd_do_smallk_mfma_kernel<3,1>
""".split() + [f"attn_bwd_{p}_mfma_kernel<{rm},{d},{dr}>" for p in ("dq", "dkv") for rm in ("true", "false")
               for d in (64, 96, 128) for dr in ("true", "false")])


def test_route_table_reaches_every_instantiation():
    """One call per table row (fresh inputs, no reference math): the union of the logged instantiations equals the literal
    list above -- every form the launch sites can take has a route row, and every row reaches what it says.  Independent
    of test order (it runs the rows itself)."""
    if not ROUTES_DEFAULT or not T256_ON:
        pytest.skip("route checks hold on the default library paths only")
    if cus() != 256:
        pytest.skip(f"the GEMM tiers of the table are laid out for 256 CUs; this device has {cus()}")
    o = ops()
    seen = set()
    for r in GEMM_ROWS:
        for e in ENTRY_EPIS[r[1]]:
            if r[2] * r[3] * r[4] > 2e10 and e not in (ENTRY_EPIS[r[1]][0], ENTRY_EPIS[r[1]][-1]):
                continue
            seen.update(run_gemm(r[1], e, r[2], r[3], r[4], r[6], o)[2])
    for p in ATT_FWD_CASES:
        nkt, d, mk, need_att, dr = p.values
        B, H, nq, nk = 1, 1, 8, ATT_FWD_NK[nkt]
        q, k, v = rnd(B, nq, H * d, dtype=BF16), rnd(B, nk, H * d, dtype=BF16, seed=1), rnd(B, nk, H * d, dtype=BF16, seed=2)
        drop = o.DropSpec(p=0.2, seed=1, site=1, step=None) if dr else None
        seen.update(launched(lambda: o.attention_fwd(q, k, v, make_mask(mk, B, nq, nk), H, need_att=need_att,
                                                     att_drop=drop))[1])
    for r in ATT_BWD_ROWS:
        seen.update(run_att_bwd(r, o)[2])
    for rid, B, n, H, Dm, expect, why in QKV_ROWS:
        x, w = rnd(B, n, Dm, dtype=BF16), rnd(3 * H * 64, Dm, dtype=BF16, scale=Dm ** -0.5, seed=1)
        seen.update(launched(lambda: o.attention_qkv_fwd(x, w, rnd(3 * H * 64, seed=2), None, H))[1])
    for rid, B, nq, nk, H, Dm, nkt, nh in Q_ROWS:
        x, w = rnd(B, nq, Dm, dtype=BF16), rnd(H * 64, Dm, dtype=BF16, scale=Dm ** -0.5, seed=1)
        k, v = rnd(B, nk, H * 64, dtype=BF16, seed=2), rnd(B, nk, H * 64, dtype=BF16, seed=3)
        seen.update(launched(lambda: o.attention_q_fwd(x, w, rnd(H * 64, seed=4), k, v, None, H))[1])
    for rid, B, nq, nk, H, Dm, expect, why in DO_ROWS:
        q, k, v = (rnd(B, n_, H * 64, dtype=BF16, seed=s_) for n_, s_ in ((nq, 1), (nk, 2), (nk, 3)))
        out, lse, _ = o.attention_fwd(q, k, v, None, H)
        dy, wt = rnd(B, nq, Dm, dtype=BF16, seed=4), rnd(H * 64, Dm, dtype=BF16, scale=Dm ** -0.5, seed=5)
        seen.update(launched(lambda: o.attention_bwd_do(dy, wt, q, k, v, out, lse, None, H))[1])
    seen = {s for s in seen if "mfma_kernel" in s or "gemm_bf16" in s or "ovqa_t256" in s}
    assert sorted(seen) == ALL_INSTANTIATIONS, (sorted(set(ALL_INSTANTIATIONS) - seen), sorted(seen - set(ALL_INSTANTIATIONS)))
