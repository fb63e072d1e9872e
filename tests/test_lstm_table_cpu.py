"""The LSTM table of tests/test_lstm_routes_gpu.py, without a GPU: its step-local fp64 checker, bars and planted bugs on
the CPU emulation of the kernel arithmetic (tests/mock_ops.lstm_fwd / lstm_bwd: fp32 math, h and dgates rounded where
the kernels store them) -- the proof that the reference alone stays inside the bars and that every planted bug leaves
them --, the ``saved`` decoders against synthetic tensors built lane by lane from the layouts csrc/lstm.hip documents, the
Python copy of ``wg_role``, and the literal kernel list against the kernel symbols of the built library."""
import shutil
import subprocess

import pytest
import torch

import mock_ops
import test_lstm_routes_gpu as L
from test_rowwise_table_cpu import ARG, SYMBOL

BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(16, 4, 512, 512), (5, 8, 40, 24)]


def _mock_run(case):
    B, T, H = case.B, case.T, case.H
    y, hseq, saved, _, y_lp = mock_ops.lstm_fwd(case.x, case.w_ih, case.w_hh, case.b_ih, case.b_hh, B, T, want_lp=True)
    dgates, _ = mock_ops.lstm_bwd(case.dy, case.w_hh, None, saved, B, T, case.I)
    return y, hseq, L.decode_mock(saved, H), y_lp, dgates


@pytest.mark.parametrize("dy_dtype", [F32, BF16], ids=["dy32", "dy16"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,T,I,H", SHAPES)
def test_emulation_passes_the_step_local_checker(B, T, I, H, dtype, dy_dtype):
    case = L.Case(B, T, I, H, dtype, dy_dtype, device="cpu")
    y, hseq, dec, y_lp, dgates = _mock_run(case)
    fwd = L.check_forward(case, y, hseq, dec, y_lp)
    bwd = L.check_backward(case, dec, dgates)
    print(f"step-local on the emulation {(B, T, I, H)} {dtype}: forward {max(fwd.values()):.1e} (bar {L.BAR:.0e}), "
          f"backward err/bar {bwd:.2f}")
    assert max(fwd.values()) <= 0.1 * L.BAR  # (fp32 libm against fp64: the margin of the bar is for the fast intrinsics)
    assert bwd > 0.5 if dtype == BF16 else bwd < 0.1  # bf16: the half-ulp of the format is what fills the bar


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,T,I,H", SHAPES)
def test_every_planted_bug_exceeds_its_factor(B, T, I, H, dtype):
    worst = L.assert_bars_see_bugs(L.Case(B, T, I, H, dtype, device="cpu"))
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v < float("inf") for v in worst.values())  # (every bug had a step to show at)


@pytest.mark.parametrize("B,T,I,H,dtype,dy_dtype", [(b, t, i, h, d, dd) for (b, t, i, h, d) in L.SIMPLE_ROWS for dd in (F32, BF16)]
                         + [(b, t, 512, 512, BF16, dd) for (b, t) in ((16, 2), (16, 3), (48, 3), (5, 3)) for dd in (F32, BF16)])
def test_planted_bugs_at_the_small_rows_of_the_gpu_table(B, T, I, H, dtype, dy_dtype):
    """The rows' own inputs need no device: the >= 10 x assertions of the smallest GPU rows, here as well."""
    L.assert_bars_see_bugs(L.Case(B, T, I, H, dtype, dy_dtype, device="cpu"))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_checker_sees_one_wrong_element_and_one_wrong_step(dtype):
    """What the whole-tensor norms of the free-running test let through: one (sample, unit) of one step, 1e-3 off."""
    case = L.Case(5, 8, 40, 24, dtype, device="cpu")
    y, hseq, dec, y_lp, dgates = _mock_run(case)
    bad = dec.clone()
    bad[4, 3, 2, 7] *= 1 + 1e-3  # c_3 of sample 2, unit 7
    with pytest.raises(AssertionError):
        L.check_forward(case, y, hseq, bad, y_lp)
    bad_y = y.clone()
    bad_y[1, 5, 11] += 1e-3
    with pytest.raises(AssertionError):
        L.check_forward(case, bad_y, hseq, dec, None)
    bad_h = hseq.clone()
    bad_h.view(9, 5, 24)[0, 0, 0] = 1e-3  # block 0 must be exactly zero
    with pytest.raises(AssertionError, match="block 0"):
        L.check_forward(case, y, bad_h, dec, y_lp)
    bad_g = dgates.clone().view(8, 5 * 96)
    bad_g[2, bad_g[2].abs().argmax()] *= 1.03  # one gate gradient of step 2 (its largest), three percent
    with pytest.raises(AssertionError, match="dgates"):
        L.check_backward(case, dec, bad_g.view(40, 96))
    nan = dgates.clone()
    nan[7, 5] = float("nan")
    with pytest.raises(AssertionError):
        L.check_backward(case, dec, nan)


# ---------------------------------------------------------------------------------------------------- ``saved``
def _encode_persistent(vals):
    """[5, T, B, 512] -> the persistent kernels' ``saved``, written as the forward kernel does: workgroup (sg, ub), wave w,
    lane l = q*16 + n stores its five values at ((t * nwg + block) * 5 + k) * 256 + tid."""
    _, T, B, _ = vals.shape
    nsg = B // 16
    nwg = nsg * L.NUB
    out = torch.full((T, nwg, 5, 256), float("nan"))
    for block in range(nwg):
        sg, ub = L.wg_role(block, nsg)
        for tid in range(256):
            w, l = tid >> 6, tid & 63
            n, q = l & 15, l >> 4
            out[:, block, :, tid] = vals[:, :, sg * 16 + n, ub * 16 + w * 4 + q].t()
    return out.reshape(-1).view(torch.uint8)


def _encode_simple(vals):
    _, T, B, H = vals.shape
    gates = vals[:4].permute(1, 2, 0, 3).reshape(-1)  # [T*B][4H], column gate*H + unit
    return torch.cat([gates, vals[4].reshape(-1)]).view(torch.uint8)


@pytest.mark.parametrize("nsg", [1, 2, 3, 5, 8])
def test_saved_decoders_round_trip(nsg):
    B, T = nsg * 16, 2
    vals = torch.arange(5 * T * B * 512, dtype=torch.float32).view(5, T, B, 512)  # every element its own value
    assert torch.equal(L.decode_persistent(_encode_persistent(vals), B, T), vals)
    small = vals[:, :, :nsg + 2, :24].contiguous()
    assert torch.equal(L.decode_simple(_encode_simple(small), nsg + 2, T, 24), small)
    assert torch.equal(L.decode_saved(_encode_simple(small), "simple", nsg + 2, T, 24), small)


def test_saved_of_a_chunked_batch_is_decoded_chunk_by_chunk():
    """ops.LstmChunks: [(b0, b1, bp, saved)]; each chunk's block has B = bp, its first b1 - b0 samples are the batch's."""
    from openvivqa_amd.ops import LstmChunks
    T, B = 2, 40
    vals = torch.arange(5 * T * B * 512, dtype=torch.float32).view(5, T, B, 512)
    chunks = LstmChunks()
    for b0, b1, bp in ((0, 32, 32), (32, 40, 16)):
        padded = torch.full((5, T, bp, 512), -1.0)
        padded[:, :, :b1 - b0] = vals[:, :, b0:b1]
        chunks.append((b0, b1, bp, _encode_persistent(padded)))
    assert torch.equal(L.decode_saved(chunks, "mfma", B, T, 512), vals)


@pytest.mark.parametrize("nsg", range(1, 9))
def test_wg_role_copy_is_a_bijection(nsg):
    roles = [L.wg_role(b, nsg) for b in range(nsg * L.NUB)]
    assert sorted(roles) == [(sg, ub) for sg in range(nsg) for ub in range(L.NUB)]
    if 8 % nsg == 0:  # the 32 workgroups of a sample group share 8 / nsg XCDs (blocks b and b + 8 share one)
        for sg in range(nsg):
            assert len({b % 8 for b, r in enumerate(roles) if r[0] == sg}) == 8 // nsg


# ---------------------------------------------------------------------------------------------------- kernel list
def _lstm_kernel_names(lib_path):
    """The host-side handles ``lstm_*`` of the anonymous namespace, written as the launch log writes an instantiation
    (mangled names decoded as in tests/test_rowwise_table_cpu.py)."""
    out = subprocess.run(["nm", lib_path], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split()
        m = SYMBOL.match(parts[-1]) if parts else None
        if not m:
            continue
        n, rest = int(m.group(1)), parts[-1][m.end():]
        name, rest = rest[:n], rest[n:]
        if not name.startswith("lstm_"):
            continue
        if rest.startswith("I"):
            args, pos = [], 1
            while rest[pos] != "E":
                a = ARG.match(rest, pos)
                if a is None:
                    args.append("?" + rest[pos:])
                    break
                args.append({"DF16b": "bf16", "f": "float"}.get(a.group(0), a.group(1)))
                pos = a.end()
            name += "<%s>" % ",".join(args)
        names.add(name)
    return names


def test_lstm_kernel_list_equals_the_library_kernel_symbols():
    from openvivqa_amd import build as B
    if shutil.which("nm") is None:
        pytest.skip("nm (binutils) is not installed: the kernel symbols cannot be listed")
    B.build(verbose=False)
    names = _lstm_kernel_names(B.LIB)
    listed = set(L.ALL_LSTM)
    assert len(listed) == len(L.ALL_LSTM) == 7  # 2 persistent + their sentinel fill + 4 per-step
    assert names == listed, {"compiled, in no list": sorted(names - listed), "listed, not compiled": sorted(listed - names)}
    assert sum(1 for n in names if "persistent" in n) == 2 and sum(1 for n in names if n.startswith("lstm_step_")) == 4
