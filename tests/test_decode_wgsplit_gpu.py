"""Single-query decode attention with the keys split ACROSS workgroups (ovqa_attention_decode_split).

Two launches: attn_decode_part_kernel on a grid of (row group, head) x slices, every workgroup writing its slice's
(maximum, sum, unnormalised o) into a workspace, then attn_decode_merge_kernel, one wave per (row, head).  The slice plan is
chunk = ceil(n / splits) rounded up to 64 keys, slices = ceil(n / chunk); one slice is the unsplit call, bit for bit.

Bars and reference are those of test_long_decode_gpu.py: ``rel_max`` = max |out - ref| / max |ref| against fp64 softmax
attention on the same operands (a mask added in fp32, as the model does), bf16 2^-7, fp32 tol(F32) = 1e-4.  The merge across
workgroups applies the formulas of the merge across the four waves of a workgroup one level up, so the bars are the same.
Shapes are a handful of (row, head) problems: two cache rows, H = 2 (H = 3 for the odd head count).

Every (n, splits) pair sits on one boundary of the plan:
  65 / 4    chunk 64,  2 slices: the last slice is one key
  128 / 2   chunk 64,  2 slices: two exact slices, one 16-key pass per wave
  129 / 2   chunk 128, 2 slices: the last slice is one key, three of its waves idle
  513 / 8   chunk 128, 5 slices: the last slice is one key
  1100 / 2  chunk 576, 2 slices: windowed slices (more than 512 keys), the second of 524 keys
  2049 / 8  chunk 320, 7 slices: the last slice has 129 keys
  2049 / 32 chunk 128, 17 slices: many slices
"""
import os

import pytest
import torch

from test_kernels_gpu import BF16, DEV, F32, rel_max
from test_long_decode_gpu import bar, ref_decode
from test_long_decode_gpu import rnd as _plain_rnd

pytestmark = pytest.mark.gpu

SWITCHES_DEFAULT = "OVQA_DECODE_SPLIT_MIN" not in os.environ and "OVQA_DECODE_GROUP_MAX" not in os.environ
# (n, splits, chunk, slices)
PAIRS = [(65, 4, 64, 2), (128, 2, 64, 2), (129, 2, 128, 2), (513, 8, 128, 5), (1100, 2, 576, 2), (2049, 8, 320, 7),
         (2049, 32, 128, 17)]
PAIR_IDS = [f"n{n}-s{s}" for n, s, _, _ in PAIRS]
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])


def rnd(*shape, **kw):  # (this module's name for it: the red-zone fixture wraps the module's own ``rnd``)
    return _plain_rnd(*shape, **kw)


def caches(Bc, Lmax, F, dtype):
    return rnd(Bc, Lmax, F, dtype=dtype, seed=2), rnd(Bc, Lmax, F, dtype=dtype, seed=3)


@pytest.fixture(autouse=True)
def _red_zones(request, monkeypatch):
    """Guard bands (tests/redzone.py) around what ops allocates -- the workspace among it -- and what rnd() makes."""
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


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def tname(dtype):
    return "float" if dtype == F32 else "__bf16"


def part_group(group, R):
    """Queries per wave of the part kernel: the largest divisor of the group that is at most 4, or 1."""
    if 2 <= group <= 8 and R % group == 0:
        for g in (4, 3, 2):
            if group % g == 0:
                return g
    return 1


def expected_split_log(dtype, d, n, splits, group, R):
    chunk = (-(-n // splits) + 63) // 64 * 64
    assert -(-n // chunk) > 1
    t = tname(dtype)
    win = "true" if chunk > 512 else "false"
    return [f"attn_decode_part_kernel<{t},{d},{part_group(group, R)},{win}>", f"attn_decode_merge_kernel<{t},{d}>"]


def split_decode(q, kc, vc, n, H, splits, mask=None, group=1, out=None, workspace=None):
    """ops.attention_decode(..., splits): the call must dispatch "decode-split" and launch exactly the part kernel the
    documented rule names, then the merge."""
    _lib = lib()
    _lib.launch_log_clear()
    o = ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group, out=out, splits=splits, workspace=workspace)
    assert _lib.last_dispatch() == "decode-split"
    if SWITCHES_DEFAULT:
        want = expected_split_log(q.dtype, q.shape[-1] // H, n, splits, group, q.shape[0])
        assert _lib.launch_log() == want, (_lib.launch_log(), want)
    return o


def pad_mask(R, Lmax, n):
    """Padded tails and heads (-1e5), different per row, as test_long_decode_gpu.check_row."""
    mask = torch.zeros(R, Lmax, device=DEV)
    mask[1 % R, n - max(1, n // 5):] = -1e5
    mask[R - 1, :max(1, n // 3)] = -1e5
    return mask


def check(dtype, group, H, d, n, splits):
    Bc = 2
    R, F, Lmax = Bc * group, H * d, n + 9
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, Lmax, F, dtype)
    b = bar(dtype)
    # no mask, into a strided output between sentinel columns
    buf = torch.full((R, 3 * F), 7.0, dtype=dtype, device=DEV)
    split_decode(q.view(R, F), kc, vc, n, H, splits, group=group, out=buf[:, F:2 * F])
    assert bool((buf[:, :F] == 7.0).all()) and bool((buf[:, 2 * F:] == 7.0).all()), "sentinel columns changed"
    e = rel_max(buf[:, F:2 * F], ref_decode(q, kc, vc, n, H, None, group))
    print(f"no mask: group {group} H {H} d {d} n {n} splits {splits}: {e:.3e} (bar {b:.3e})")
    assert e < b, ("no mask", group, H, e, b)
    # a padding mask
    mask = pad_mask(R, Lmax, n)
    out = split_decode(q, kc, vc, n, H, splits, mask=mask, group=group)
    assert out.shape == q.shape and out.dtype == dtype
    e = rel_max(out.reshape(R, F), ref_decode(q, kc, vc, n, H, mask, group))
    print(f"pad mask: group {group} H {H} d {d} n {n} splits {splits}: {e:.3e} (bar {b:.3e})")
    assert e < b, ("mask", group, H, e, b)


# -------------------------------------------------------------------------------------------------------------------------
# 1. against fp64
# -------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_split_against_fp64(dtype, d, pair):
    """No mask (strided output) and a padding mask, each at H = 2 and at the odd head count H = 3; on d = 64 the groups
    {1, 3, 4, 5, 8} (5 reads per row, 8 runs as two waves of four), elsewhere group 1."""
    n, splits, chunk, slices = pair
    assert ops().decode_split_slices(n, splits) == slices and (-(-n // splits) + 63) // 64 * 64 == chunk
    for group in ([1, 3, 4, 5, 8] if d == 64 else [1]):
        for H in (2, 3):
            check(dtype, group, H, d, n, splits)


# -------------------------------------------------------------------------------------------------------------------------
# 2. planted keys: a lost slice, or a lost end of one, must show
# -------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_split_planted_key(dtype, d, pair):
    """One boosted key j* (+8 in every query's mask row) at the first key of the last slice, at the last key overall and at
    the last key of slice 0.  First, in fp64 on the test's own inputs: removing j* moves the tensor by >= 10 bars and
    every (row, head) by more than one bar.  Only then the kernel is compared."""
    n, splits, chunk, slices = pair
    Bc, group, H = 2, 3, 2
    R, F = Bc * group, H * d
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, n + 3, F, dtype)
    b = bar(dtype)
    for js in sorted({(slices - 1) * chunk, n - 1, chunk - 1}):
        mask = torch.zeros(R, n + 3, device=DEV)
        mask[:, js] = 8.0
        ref = ref_decode(q, kc, vc, n, H, mask, group)
        lost = ref_decode(q, kc, vc, n, H, mask, group, drop=js)
        scale = ref.abs().max()
        per = ((ref - lost).abs().reshape(R, H, d).amax(-1) / scale)
        assert rel_max(lost, ref) >= 10 * b, (js, rel_max(lost, ref))  # the bar sees a lost j* ten times over ...
        assert per.min().item() > b, (js, per.min().item())            # ... and in every (row, head)
        out = split_decode(q, kc, vc, n, H, splits, mask=mask, group=group)
        e = rel_max(out.reshape(R, F), ref)
        print(f"planted {js}: d {d} n {n} splits {splits}: {e:.3e} (bar {b:.3e})")
        assert e < b, (js, e, b)
        got = ((out.reshape(R, F).double().cpu() - ref).abs().reshape(R, H, d).amax(-1) / scale)
        assert got.max().item() < b, (js, got.max().item())


# -------------------------------------------------------------------------------------------------------------------------
# 3. masked slices
# -------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("pair", [PAIRS[3], PAIRS[4], PAIRS[5]], ids=[PAIR_IDS[3], PAIR_IDS[4], PAIR_IDS[5]])
def test_split_masked_slices(dtype, pair):
    """Row 0: every key of slice 1 carries -1e5 while the other slices are live (its record has a finite maximum near -1e5
    and drops out by underflow).  Row 1: every key carries -1e5 (finite): uniform over the n keys.  Row 2: only slice 0
    is live.  Row 3: only the last slice is live."""
    n, splits, chunk, slices = pair
    Bc, H, d = 4, 2, 64
    R, F = Bc, H * d
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, n + 5, F, dtype)
    q[1] = 0  # the fully masked row: equal scores, exactly uniform over its n keys
    mask = torch.zeros(R, n + 5, device=DEV)
    mask[0, chunk:min(2 * chunk, n)] = -1e5
    mask[1, :] = -1e5
    mask[2, chunk:] = -1e5
    mask[3, :(slices - 1) * chunk] = -1e5
    out = split_decode(q, kc, vc, n, H, splits, mask=mask).reshape(R, F)
    assert bool(torch.isfinite(out.float()).all())
    ref = ref_decode(q, kc, vc, n, H, mask, 1)
    b = bar(dtype)
    scale = ref.abs().max()
    for r in range(R):  # row by row, each against the tensor's scale
        e = ((out[r].double().cpu() - ref[r]).abs().max() / scale).item()
        print(f"masked slices row {r}: n {n} splits {splits}: {e:.3e} (bar {b:.3e})")
        assert e < b, (r, e, b)
    uni = vc[1, :n].double().mean(0).cpu()
    assert ((out[1].double().cpu() - uni).abs().max() / uni.abs().max()).item() < b
    # the row with a dead slice gives what the same row gives without that slice's keys
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[chunk:min(2 * chunk, n)] = False
    alive = ref_decode(q[:1], kc[:1, :n][:, keep], vc[:1, :n][:, keep], int(keep.sum()), H, None, 1)
    assert ((out[0].double().cpu() - alive[0]).abs().max() / alive.abs().max()).item() < b


# -------------------------------------------------------------------------------------------------------------------------
# 4. forms
# -------------------------------------------------------------------------------------------------------------------------
def _operands(dtype, group, H, d, n, Bc=2):
    R, F = Bc * group, H * d
    q = rnd(R, 1, F, dtype=dtype, seed=1)
    kc, vc = caches(Bc, n + 2, F, dtype)
    return q, kc, vc, pad_mask(R, n + 2, n)


@DTYPES
@pytest.mark.parametrize("n,splits", [(617, 1), (40, 4), (64, 32), (2049, 1)])
def test_one_slice_is_the_unsplit_call(dtype, n, splits):
    """splits = 1, or a plan of one slice: the existing instantiation, dispatch "decode", the same bits."""
    from test_long_decode_gpu import expected_form
    _lib = lib()
    H, d, group = 2, 64, 3
    q, kc, vc, mask = _operands(dtype, group, H, d, n)
    assert ops().decode_split_slices(n, splits) == 1
    plain = ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group)
    _lib.launch_log_clear()
    out = ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group, splits=splits)
    assert _lib.last_dispatch() == "decode"
    if SWITCHES_DEFAULT:
        assert _lib.launch_log() == [expected_form(dtype, d, n, group, q.shape[0], H)], _lib.launch_log()
    assert torch.equal(out, plain)


@DTYPES
@pytest.mark.parametrize("n", [40, 237, 617, 2049])
@pytest.mark.parametrize("group", [1, 3])
def test_automatic_rule_runs_what_it_names(dtype, n, group):
    """splits = 0: the launches are those of the splits that ovqa_attention_decode_auto_splits returns for the call."""
    from test_long_decode_gpu import expected_form
    _lib = lib()
    H, d = 2, 64
    q, kc, vc, mask = _operands(dtype, group, H, d, n)
    R = q.shape[0]
    auto = _lib.load().ovqa_attention_decode_auto_splits(R, H, group, n, d, 0 if dtype == F32 else 1)
    assert 1 <= auto <= min(32, max(1, n // 64)), auto
    _lib.launch_log_clear()
    out = ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group, splits=0)
    if ops().decode_split_slices(n, auto) == 1:
        assert _lib.last_dispatch() == "decode"
        want = [expected_form(dtype, d, n, group, R, H)]
    else:
        assert _lib.last_dispatch() == "decode-split"
        want = expected_split_log(dtype, d, n, auto, group, R)
    if SWITCHES_DEFAULT:
        assert _lib.launch_log() == want, (_lib.launch_log(), want)
    assert torch.equal(out, ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group, splits=auto))
    assert rel_max(out.reshape(R, H * d), ref_decode(q, kc, vc, n, H, mask, group)) < bar(dtype)


def test_automatic_rule_leaves_a_full_chip_alone():
    """problems >= 2 * CUs: one launch already fills the chip twice (launch_decode's own criterion): never split."""
    L = lib().load()
    H = 8
    R = -(-2 * cus() // H)
    for n in (237, 617, 2048, 1 << 20):
        for dt in (0, 1):
            assert L.ovqa_attention_decode_auto_splits(R, H, 1, n, 64, dt) == 1
            assert L.ovqa_attention_decode_auto_splits(4 * R, H, 4, n, 64, dt) == 1  # four beams share a workgroup
    for n in (1, 63, 64, 127):  # and never more than n / 64 slices, whatever the batch
        assert L.ovqa_attention_decode_auto_splits(1, H, 1, n, 64, 1) <= max(1, n // 64)


# -------------------------------------------------------------------------------------------------------------------------
# 5. buffers
# -------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[4], PAIRS[6]], ids=[PAIR_IDS[0], PAIR_IDS[4], PAIR_IDS[6]])
def test_workspace_bounds(dtype, pair):
    n, splits, _, _ = pair
    _lib = lib()
    H, d, group = 3, 64, 3
    q, kc, vc, mask = _operands(dtype, group, H, d, n)
    R, F = q.shape[0], H * d
    need = ops().decode_split_workspace_bytes(R, H, n, d, splits)
    raw = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = split_decode(q, kc, vc, n, H, splits, mask=mask, group=group, workspace=raw[:need])
    torch.cuda.synchronize()
    assert bool((raw[need:] == 0xA5).all()), "the workspace's sentinel changed"
    assert torch.equal(out, split_decode(q, kc, vc, n, H, splits, mask=mask, group=group))
    assert rel_max(out.reshape(R, F), ref_decode(q, kc, vc, n, H, mask, group)) < bar(dtype)
    # one byte too small, or off the 16-byte grid: refused before anything is launched
    for ws in (raw[:need - 1], raw[1:need + 1]):
        _lib.launch_log_clear()
        with pytest.raises(RuntimeError, match="workspace"):
            ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group, splits=splits, workspace=ws)
        assert _lib.launch_log() == []
    _lib.launch_log_clear()
    rc = _lib.load().ovqa_attention_decode_split(
        0 if dtype == F32 else 1, q.data_ptr(), q.stride(0), kc.data_ptr(), kc.stride(1), vc.data_ptr(), vc.stride(1),
        kc.stride(0), group, None, 0, out.data_ptr(), out.stride(0), R, H, n, d, 0.125, splits, None, need, None)
    assert rc == -1 and _lib.launch_log() == []  # OVQA_ERR_BAD_ARG: a NULL workspace


# -------------------------------------------------------------------------------------------------------------------------
# 6. determinism and graphs
# -------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("pair", [PAIRS[3], PAIRS[4]], ids=[PAIR_IDS[3], PAIR_IDS[4]])
def test_split_is_deterministic_and_replays_from_a_graph(dtype, pair):
    n, splits, _, _ = pair
    H, d, group = 2, 64, 3
    q, kc, vc, mask = _operands(dtype, group, H, d, n)
    R = q.shape[0]
    first = split_decode(q, kc, vc, n, H, splits, mask=mask, group=group)
    assert torch.equal(first, split_decode(q, kc, vc, n, H, splits, mask=mask, group=group))
    ws = torch.empty(ops().decode_split_workspace_bytes(R, H, n, d, splits), dtype=torch.uint8, device=DEV)
    out = torch.zeros_like(q)
    call = lambda: ops().attention_decode(q, kc, vc, n, H, mask=mask, group=group, out=out, splits=splits, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for trial in range(2):
        q.copy_(_plain_rnd(*q.shape, dtype=dtype, seed=10 + trial))  # refilled in place: the graph reads the same memory
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = split_decode(q, kc, vc, n, H, splits, mask=mask, group=group)
        assert torch.equal(out, eager), trial
        assert rel_max(out.reshape(R, H * d), ref_decode(q, kc, vc, n, H, mask, group)) < bar(dtype)


# -------------------------------------------------------------------------------------------------------------------------
# 7. modules: OVQA_DECODE_WG_SPLIT
# -------------------------------------------------------------------------------------------------------------------------
NE, T_STEPS = 200, 6


def _vocab(max_len, size):
    class Vocab:
        max_answer_length, padding_idx, bos_idx, eos_idx = max_len, 0, 1, 2

        def __len__(self):
            return size
    return Vocab()


def _small_decoder():
    import openvivqa_amd.modules as M
    from openvivqa_amd.config import ConfigNode, attention_config
    att = lambda **kw: attention_config(d_model=128, head=2, d_key=64, d_value=64, d_ff=256, **kw)
    cfg = ConfigNode(dict(
        ARCHITECTURE="Decoder", D_MODEL=128, LAYERS=1,
        ATTENTION=dict(SELF_ATTENTION=att(can_be_stateful=True), ENC_ATTENTION=att()),
        TEXT_EMBEDDING=dict(ARCHITECTURE="UsualEmbedding", D_MODEL=128, D_EMBEDDING=64, WORD_EMBEDDING=None,
                            WORD_EMBEDDING_CACHE=None, DROPOUT=0.1)))
    torch.manual_seed(31)
    dec = M.Decoder(cfg, _vocab(T_STEPS, 60)).to(DEV).eval()
    with torch.no_grad():
        dec.fc.weight.mul_(6.0)  # spread the vocabulary distribution: fewer near-ties between candidates
    return dec


def _encoder_features():
    from openvivqa_amd.utils import generate_padding_mask
    enc = torch.randn(1, NE, 128, generator=torch.Generator().manual_seed(4))
    enc[0, 180:] = 0  # padded: the last slice of the encoder attention's keys is masked in part
    enc = enc.to(DEV)
    return enc, generate_padding_mask(enc, 0)


def _steps(dec, toks, enc, emask, beam):
    """Teacher-forced stateful steps on ``toks`` [beam, T]: every step's output and its attention launches."""
    _lib = lib()
    outs, logs = [], []
    with torch.no_grad(), dec.statefulness(beam):
        for t in range(toks.shape[1]):
            _lib.launch_log_clear()
            outs.append(dec(toks[:, t:t + 1], enc, emask, encoder_group=beam))
            logs.append([e for e in _lib.launch_log() if "attn_" in e])
    return torch.cat(outs, 1), logs


@pytest.mark.parametrize("beam", [1, 3])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_decoder_with_the_switch(dtype, beam, monkeypatch):
    """A small Decoder (L = 1, d_model 128, H = 2) over 200 encoder positions, B = 1.  OVQA_DECODE_WG_SPLIT=4 cuts the
    encoder attention's 200 keys into 4 slices of 64 (the self-attention's few keys stay one slice).  fp32: the search
    returns the tokens it returns with the switch off.  bf16: every step, replayed on the tokens of the run with the switch
    off, stays within the module bar of the suite (rel-L2 1e-2) of that run's step."""
    import openvivqa_amd as A
    from openvivqa_amd.beam import GraphedBeamSearch
    from test_blocks_gpu import rel_l2
    A.set_compute_dtype(dtype)
    try:
        monkeypatch.delenv("OVQA_DECODE_WG_SPLIT", raising=False)
        dec = _small_decoder()
        enc, emask = _encoder_features()
        search = GraphedBeamSearch(dec, 1, T_STEPS, 1, -1, beam)  # (eos unreachable)
        tok_off, lp_off = search(enc, emask, use_graph=False)
        toks = tok_off[:1].reshape(1, -1).expand(beam, -1).contiguous()
        step_off, log_off = _steps(dec, toks, enc, emask, beam)
        t = tname(dtype)
        G = beam if beam <= 4 else 1
        if SWITCHES_DEFAULT:  # unset: what a step launches today
            assert all(l == [f"attn_decode_kernel<{t},64,1,false,false>", f"attn_decode_kernel<{t},64,{G},true,false>"]
                       for l in log_off), log_off
        monkeypatch.setenv("OVQA_DECODE_WG_SPLIT", "0")
        assert _steps(dec, toks, enc, emask, beam)[1] == log_off
        monkeypatch.setenv("OVQA_DECODE_WG_SPLIT", "4")
        tok_on, lp_on = search(enc, emask, use_graph=False)
        step_on, log_on = _steps(dec, toks, enc, emask, beam)
        if SWITCHES_DEFAULT:
            assert all(l == [f"attn_decode_kernel<{t},64,1,false,false>", f"attn_decode_part_kernel<{t},64,{G},false>",
                             f"attn_decode_merge_kernel<{t},64>"] for l in log_on), log_on
        e = rel_l2(step_on, step_off)
        print(f"switch on against off, {t} beam {beam}: step outputs rel-L2 {e:.3e}")
        if dtype == F32:
            assert torch.equal(tok_on, tok_off), (tok_on, tok_off)
            assert e < 1e-4 and rel_l2(lp_on, lp_off) < 1e-4
        else:
            assert e < 1e-2
        monkeypatch.setenv("OVQA_DECODE_WG_SPLIT", "auto")
        step_auto, _ = _steps(dec, toks, enc, emask, beam)
        assert rel_l2(step_auto, step_off) < (1e-4 if dtype == F32 else 1e-2)
    finally:
        A.set_compute_dtype(BF16)
