"""bench.py --dump-outputs on the host: the budget, the fixed sample, float32 files, and training dumps that do not depend
on how the parameter arena is laid out (so that two builds can be compared output for output)."""
import copy
import os

import numpy as np
import torch
from torch import nn

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_budget_sample_and_repeatability(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.tensor([2.5]), "tokens": torch.arange(12).reshape(3, 4),
              "big": torch.randn(9_000_000, generator=g),
              "wide": torch.randn(3_000, 4_000, generator=g, dtype=torch.float64)}  # 48M float32 elements in all: over budget
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["big", "loss", "tokens", "wide"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)  # same positions, same values, every run
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET
    # arrays that fit are written whole, in their own shape
    assert np.array_equal(a["loss"], [2.5]) and np.array_equal(a["tokens"], np.arange(12, dtype=np.float32).reshape(3, 4))
    # the larger ones are samples OF them that use the budget: at least a quarter of it each
    for k in ("big", "wide"):
        src = arrays[k].float().reshape(-1).numpy()
        assert a[k].ndim == 1 and a[k].size < src.size and a[k].nbytes >= bench.DUMP_BUDGET // 4
        assert np.isin(a[k], src).all()


def test_training_dump_does_not_depend_on_the_arena_layout():
    """The same weights and moments in two arenas of different grouping (an adjacency group of two matrices against one
    group per parameter: the ragged 353 x 300 matrix is then zero-padded to 360 x 320) dump identically."""
    from openvivqa_amd import runtime as rt
    from openvivqa_amd.train import FlatAdam
    torch.manual_seed(3)
    m1 = nn.ModuleDict({"a": nn.Linear(300, 353), "b": nn.Linear(300, 24), "c": nn.LayerNorm(24)})
    m2 = copy.deepcopy(m1)
    a, b, c = m1["a"], m1["b"], m1["c"]
    ar1 = rt.ParamArena([[a.weight, b.weight], [a.bias], [b.bias], [c.weight], [c.bias]], torch.device("cpu"), torch.float32)
    ar2 = rt.ParamArena([[p] for p in reversed(list(m2.parameters()))], torch.device("cpu"), torch.float32)
    assert ar2.is_padded(m2["a"].weight) and not ar1.is_padded(a.weight)
    assert ar1.numel != ar2.numel  # the flat buffers differ in size and order
    loss = torch.tensor([1.25])
    outs = []
    for m, ar in ((m1, ar1), (m2, ar2)):
        opt = FlatAdam(ar)
        for i, (_, p) in enumerate(m.named_parameters()):
            ar._slice(opt.exp_avg, p).copy_(p.detach() * 0.5 + i)
        outs.append(bench.training_outputs(m, ar, opt, loss))
    n = sum(p.numel() for p in m1.parameters())
    assert outs[0]["params"].numel() == outs[0]["adam_exp_avg"].numel() == n
    for k in ("loss", "params", "adam_exp_avg"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(outs[0]["params"][:353 * 300], m1["a"].weight.detach().reshape(-1))
