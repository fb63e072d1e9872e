"""Host side of the prefix-LM training route, on the CPU with the torch-math stand-ins of tests/mock_ops.py: the mask
helper and its hint, the multimodal transformer's forward + backward staying on the dense mask where the kernels are not
there (mock_ops.attention_fwd_prefix_lm_ok is False: no new ``ops`` entry may be reached), and the two C signatures."""
import ctypes as C

import pytest
import torch

import mock_ops
from golden_cases import hip_namespace, run_case

NEW_OPS = ("attention_fwd_prefix_lm_train", "attention_bwd_prefix_lm")


def test_prefix_lm_mask_values_and_hint():
    from openvivqa_amd.utils import MASK_VALUE, generate_sequential_mask, prefix_lm_mask
    B, n, tail = 3, 11, 4
    row = torch.zeros(B, 1, 1, n)
    row[1, ..., 2:5] = MASK_VALUE
    ext = prefix_lm_mask(row, tail)
    assert ext.shape == (B, 1, n, n) and ext.dtype == torch.float32
    for b in range(B):
        for i in range(n):
            for j in range(n):
                corner = i >= n - tail and j >= n - tail
                want = (MASK_VALUE if j > i else 0.0) if corner else float(row[b, 0, 0, j])
                assert float(ext[b, 0, i, j]) == want, (b, i, j)
    assert torch.equal(ext[:, :, -tail:, -tail:], generate_sequential_mask(tail).expand(B, 1, tail, tail))
    hint_row, hint_tail = ext._ovqa_prefix_lm
    assert hint_tail == tail and torch.equal(hint_row, row) and hint_row.dtype == torch.float32
    # the hint belongs to that tensor object: conversions and copies do not carry it (the dense route, silently)
    for other in (ext.double(), ext.clone(), ext + 0, ext.to(torch.float32, copy=True)):
        assert getattr(other, "_ovqa_prefix_lm", None) is None
    assert ext.to(torch.float32) is ext  # (what BertLayer does to its mask: a no-op on fp32 keeps the hint)
    # no corner: the repeated row, and the hint says so
    e0 = prefix_lm_mask(row, 0)
    assert torch.equal(e0, row.repeat(1, 1, n, 1)) and e0._ovqa_prefix_lm[1] == 0
    # a (B, H, 1, n) row is not a key row per sample: no hint
    assert getattr(prefix_lm_mask(torch.zeros(B, 2, 1, n), tail), "_ovqa_prefix_lm", None) is None


class _Recording:
    """mock_ops with every attribute access recorded (getattr on a name it lacks raises, as on the module)."""

    def __init__(self):
        self.seen = set()

    def __getattr__(self, name):
        self.seen.add(name)
        return getattr(mock_ops, name)


@pytest.fixture
def recording_ops(monkeypatch):
    import openvivqa_amd as A
    import openvivqa_amd.functional as Fn
    import openvivqa_amd.modules.embeddings as emb
    import openvivqa_amd.runtime as rt
    import openvivqa_amd.train as tr
    rec = _Recording()
    for mod in (Fn, rt, tr, emb):
        monkeypatch.setattr(mod, "ops", rec)

    def build_arena_cpu(module, device=None, compute_dtype=None):
        params = list(module.parameters())
        return rt.ParamArena(rt.collect_groups(module), params[0].device, compute_dtype or rt.get_compute_dtype())
    monkeypatch.setattr(rt, "build_arena", build_arena_cpu)
    monkeypatch.setattr(rt, "step_tensor", lambda device: torch.zeros(1, dtype=torch.int32))
    A.set_compute_dtype(torch.float32)
    yield rec
    A.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("opt_in", ["0", "1"])
def test_mmt_forward_backward_stays_on_the_dense_mask_on_the_mock(recording_ops, monkeypatch, opt_in):
    """The golden multimodal-transformer case, forward + backward with gradients enabled: the mask carries the hint, the
    gate (ops.attention_fwd_prefix_lm_ok, False on the mock) is asked, and neither new entry is touched -- with the opt-in
    set or not; results equal, bit for bit, those of a run whose mask carries no hint."""
    import openvivqa_amd.modules.mmt as mmt
    monkeypatch.setenv("OVQA_PREFIX_LM_TRAIN", opt_in)
    assert not hasattr(mock_ops, NEW_OPS[0]) and not hasattr(mock_ops, NEW_OPS[1])
    hinted = []
    real = mmt.prefix_lm_mask

    def spy(row, tail):
        ext = real(row, tail)
        hinted.append(getattr(ext, "_ovqa_prefix_lm", None) is not None)
        return ext
    monkeypatch.setattr(mmt, "prefix_lm_mask", spy)
    _, outs, gin, gw, _ = run_case(hip_namespace(), "G13_mmt")
    assert hinted and all(hinted)
    assert "attention_fwd_prefix_lm_ok" in recording_ops.seen and "attention_fwd" in recording_ops.seen
    assert "attention_bwd" in recording_ops.seen
    assert not recording_ops.seen & {*NEW_OPS, "attention_fwd_prefix_lm"}, recording_ops.seen

    monkeypatch.setattr(mmt, "prefix_lm_mask", lambda row, tail: real(row, tail).clone())  # the same values, no hint
    _, outs2, gin2, gw2, _ = run_case(hip_namespace(), "G13_mmt")
    for a, b in ((outs, outs2), (gin, gin2), (gw, gw2)):
        assert a.keys() == b.keys()
        for k in a:
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), k


def test_lib_table_holds_the_two_signatures():
    from openvivqa_amd import _lib
    vp, i64, f32, dp = C.c_void_p, C.c_int64, C.c_float, C.POINTER(_lib.Dropout)
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "ovqa_attention_fwd_prefix_lm" in v)
    assert _lib.ABI_VERSION == 12
    fwd = table["ovqa_attention_fwd_prefix_lm_train"]
    # the inference entry's arguments, then o_lo after lse and att_drop in front of the stream
    base = list(table["ovqa_attention_fwd_prefix_lm"])
    assert fwd == base[:14] + [vp] + base[14:19] + [dp, vp]
    bwd = table["ovqa_attention_bwd_prefix_lm"]
    assert bwd == ([C.c_int] + [vp, i64] * 5 + [vp, vp] + [vp, i64, i64, i64] + [vp, i64] * 3 + [vp] + [i64] * 4
                   + [f32, dp, vp])
