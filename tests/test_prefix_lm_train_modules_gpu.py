"""M4C training through the prefix-LM attention route (OVQA_PREFIX_LM_TRAIN=1): the multimodal transformer's mask reaches the
attention kernels as a key row + the number of decoding positions, forward and backward, instead of the dense (B, 1, S, S)
tensor.  The route is a faster path to the same bits: loss, scores and every gradient tensor of a forward + backward are
torch.equal between fresh processes with the route on, with OVQA_NO_PREFIX_LM=1 (which wins over the opt-in) and with no
switch at all (the dense mask, as before), at S = 182 (LDS-resident kernels) and S = 232 (streaming kernels), in training
mode (dropout 0.1 at every site) and in eval mode with gradients enabled; the launch logs show which kernels each ran."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCED_SIMPLE = os.environ.get("OVQA_FORCE_SIMPLE", "0") == "1"
ARMS = {"route": {"OVQA_PREFIX_LM_TRAIN": "1", "OVQA_NO_PREFIX_LM": "0"},
        "off": {"OVQA_PREFIX_LM_TRAIN": "1", "OVQA_NO_PREFIX_LM": "1"},
        "default": {"OVQA_PREFIX_LM_TRAIN": "0", "OVQA_NO_PREFIX_LM": "0"}}
LAYERS = 4


def _child(mode, env_extra, *args):
    env = dict(os.environ, OVQA_REQUIRE_MFMA="1")
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, *map(str, args)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def expected_kernels(S, train, rowmask):
    """The attention instantiations of the MMT layers (heads of 96): LDS-resident at S = 182, streaming at S = 232."""
    rm, dr = ("true" if rowmask else "false"), ("true" if train else "false")
    if S <= 192:
        return ({f"attn_fwd_mfma_kernel<6,{rm},false,96,{dr}>"},
                {f"attn_bwd_dq_mfma_kernel<{rm},96,{dr}>", f"attn_bwd_dkv_mfma_kernel<{rm},96,{dr}>"})
    dkv = f"attn_stream_bwd_dkv_tail_kernel<96,{dr}>" if rowmask else f"attn_stream_bwd_dkv_kernel<96,false,{dr}>"
    return {f"attn_stream_fwd_kernel<96,{rm},{dr}>"}, {f"attn_stream_bwd_dq_kernel<96,{rm},{dr}>", dkv}


@pytest.mark.skipif(FORCED_SIMPLE, reason="OVQA_REQUIRE_MFMA has no meaning under OVQA_FORCE_SIMPLE")
@pytest.mark.parametrize("n_ocr", [50, 100], ids=["S182-resident", "S232-streaming"])
def test_m4c_forward_backward_is_bit_identical_on_both_routes(n_ocr, tmp_path):
    S = 20 + 100 + n_ocr + 12
    res = {}
    for arm, env in ARMS.items():
        _child("fwdbwd", env, n_ocr, tmp_path / f"{arm}.pt")
        res[arm] = torch.load(tmp_path / f"{arm}.pt")
    for mode in ("train", "eval"):
        a = res["route"][mode]
        for other in ("off", "default"):
            b = res[other][mode]
            assert torch.equal(a["loss"], b["loss"]), (mode, other, a["loss"], b["loss"])
            assert torch.equal(a["scores"], b["scores"]), (mode, other)
            assert a["grads"].keys() == b["grads"].keys() and len(a["grads"]) > 50
            for k in a["grads"]:
                assert torch.equal(a["grads"][k], b["grads"][k]), (mode, other, k)
        assert torch.isfinite(a["loss"]).all() and all(torch.isfinite(g).all() for g in a["grads"].values())
        # the launch logs: the row-mask forms with the route on, the per-query-mask forms otherwise, once per layer
        for arm, rowmask in (("route", True), ("off", False), ("default", False)):
            fwd, bwd = expected_kernels(S, mode == "train", rowmask)
            r = res[arm][mode]
            assert set(r["fwd_log"]) == fwd and len(r["fwd_log"]) == LAYERS, (mode, arm, r["fwd_log"])
            assert set(r["bwd_log"]) == bwd and len(r["bwd_log"]) == 2 * LAYERS, (mode, arm, r["bwd_log"])
    for log in (res["route"]["train"]["fwd_log"] + res["route"]["train"]["bwd_log"]):  # no per-query-mask dropout form
        assert "<false,96,true>" not in log and "<96,false,true>" not in log and ",false,false,96,true>" not in log, log


@pytest.mark.skipif(FORCED_SIMPLE, reason="the prefix-LM kernels are off under OVQA_FORCE_SIMPLE")
def test_m4c_graphed_train_steps_equal_eager_on_the_route(tmp_path):
    """Three hipGraph-replayed TrainSteps (B = 4, S = 182) against three eager steps, route on, each in a fresh process: the
    same losses and the same fp32 master weights, bit for bit; the graph captured the row-mask kernels.  Dropout is off, as
    in the graph-against-eager tests of tests/test_train_gpu.py: with dropout on the two modes of TrainStep draw different
    masks from the second step on, on either route."""
    res = {}
    for name, use_graph in (("graph", 1), ("eager", 0)):
        _child("steps", ARMS["route"], use_graph, tmp_path / f"{name}.pt", 0)
        res[name] = torch.load(tmp_path / f"{name}.pt")
    g, e = res["graph"], res["eager"]
    assert g["captured"] and not e["captured"]
    assert g["losses"] == e["losses"] and len(g["losses"]) == 3 and all(x == x for x in g["losses"]), (g["losses"], e["losses"])
    assert torch.equal(g["master"], e["master"])
    assert "attn_fwd_mfma_kernel<6,true,false,96,false>" in g["log"], g["log"]
    assert "attn_bwd_dkv_mfma_kernel<true,96,false>" in e["log"], e["log"]
    assert not any("<false,96," in x or ",false,false,96," in x for x in g["log"] + e["log"]), (g["log"], e["log"])


def test_prefix_lm_mask_equals_the_mask_mmt_built_before():
    """utils.prefix_lm_mask(row, tail), value for value, against the construction MMT._extended_mask held before it called
    the helper (repeat the row over the queries, SET the corner to generate_sequential_mask); the hint names the row."""
    from openvivqa_amd.modules.mmt import MMT
    from openvivqa_amd.utils import MASK_VALUE, generate_sequential_mask, prefix_lm_mask
    dev = torch.device("cuda", 0)
    B, steps = 3, 12
    tm, om, cm = (torch.zeros(B, 1, 1, n, device=dev) for n in (20, 100, 50))
    tm[1, ..., 13:] = MASK_VALUE
    om[2, ..., 90:] = MASK_VALUE
    cm[0, ..., 44:] = MASK_VALUE
    dec_emb = torch.zeros(B, steps, 8, device=dev)
    mask = torch.cat([tm, om, cm, torch.zeros(B, 1, 1, steps, device=dev)], dim=-1).float()
    S = mask.size(-1)
    want = mask.repeat(1, 1, S, 1)
    want[:, :, -steps:, -steps:] = generate_sequential_mask(steps, device=dev)
    for got in (prefix_lm_mask(mask, steps), MMT._extended_mask(tm, om, cm, steps, dec_emb)):
        assert got.dtype == torch.float32 and got.shape == (B, 1, S, S) and torch.equal(got, want)
        row, tail = got._ovqa_prefix_lm
        assert tail == steps and torch.equal(row, mask)
        assert getattr(got.to(torch.float64), "_ovqa_prefix_lm", None) is None  # (a conversion drops the hint)


# ---------------------------------------------------------------------------------------------------------------------------
def _fwdbwd(m, forward, inputs, tgt, loss_fn):
    from openvivqa_amd import _lib
    _lib.launch_log_clear()
    scores = forward(*inputs)
    loss = loss_fn(scores, tgt)
    torch.cuda.synchronize()
    fwd = _lib.launch_log()
    _lib.launch_log_clear()
    with torch.autograd.set_multithreading_enabled(False):  # (backward on the logging thread)
        loss.backward()
    torch.cuda.synchronize()
    bwd = _lib.launch_log()
    assert len(fwd) < 256 and len(bwd) < 256, (len(fwd), len(bwd))  # (the log keeps the first 256 launches)
    grads = {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
    return {"loss": loss.detach().float().cpu(), "scores": scores.detach().float().cpu(), "grads": grads,
            "fwd_log": [e for e in fwd if e.startswith("attn_")], "bwd_log": [e for e in bwd if e.startswith("attn_")]}


def _child_main(mode, args):
    sys.path.insert(0, ROOT)
    import openvivqa_amd as A
    from openvivqa_amd import _lib
    from openvivqa_amd.models.mmf_m4c import M4CLoss, M4CTrainModel, synthetic_batch
    A.set_compute_dtype(torch.bfloat16)
    A.manual_seed(17)
    torch.manual_seed(17)
    dev = torch.device("cuda", 0)
    V, B = 300, 4
    loss_fn = M4CLoss(0)
    if mode == "fwdbwd":
        n_ocr, out = int(args[0]), args[1]
        m = M4CTrainModel(V).to(dev).train()
        inputs, tgt = synthetic_batch(B, V, dev, seed=8, n_ocr=n_ocr)
        res = {"train": _fwdbwd(m, m, inputs, tgt, loss_fn)}
        # eval mode with gradients enabled, on a second model (fresh gradient buffers).  The model's own eval forward is the
        # greedy decode under no_grad: the teacher-forced pass of its training forward, by hand.
        torch.manual_seed(18)
        m = M4CTrainModel(V).to(dev).eval()

        def teacher_forced(txt, tm, reg, box, f1, f2, f3, ocr_box, ans):
            obj, om, ocr, cm = m.encode(reg, box, f1, f2, f3, ocr_box)
            r = m.mmt(txt_emb=txt, txt_mask=tm, obj_emb=obj, obj_mask=om, ocr_emb=ocr, ocr_mask=cm,
                      fixed_ans_emb=m.classifier.weight, prev_inds=ans)
            return m.scores(r, cm)
        res["eval"] = _fwdbwd(m, teacher_forced, inputs, tgt, loss_fn)
        torch.save(res, out)
        return
    from openvivqa_amd.train import TrainStep
    use_graph, out, dropout = bool(int(args[0])), args[1], bool(int(args[2]))
    inputs, tgt = synthetic_batch(B, V, dev, seed=8)
    m = M4CTrainModel(V).to(dev).train()
    if not dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    ts = TrainStep(m, lambda *x: loss_fn(m(*x), tgt), lr=2e-4, betas=(0.9, 0.98), use_graph=use_graph)
    _lib.launch_log_clear()
    with torch.autograd.set_multithreading_enabled(False):
        losses = [float(ts.step(*inputs)) for _ in range(3)]
    torch.cuda.synchronize()
    torch.save({"losses": losses, "master": ts.arena.master.detach().cpu().clone(), "captured": bool(ts.captured),
                "log": sorted(set(e for e in _lib.launch_log() if e.startswith("attn_")))}, out)


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2:])
