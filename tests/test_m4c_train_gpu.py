"""M4C training (BASELINE configs[3]): the teacher-forced M4CTrainModel + M4CLoss under TrainStep against the oracle's
torch.optim.Adam trajectory, the same dropout masks on the MFMA and the VALU attention kernels, the training step on the
MFMA kernels only, and a falling loss."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _RefM4C(torch.nn.Module):
    """The reference's training forward (mmf_m4c.py:135-235) in plain torch on the oracle's MMT / OcrPtrNet, with the
    reference's parameter names."""

    def __init__(self, V, cfg):
        import oracle as O
        super().__init__()
        L, LN = torch.nn.Linear, torch.nn.LayerNorm
        self.linear_obj_feat_to_mmt_in, self.linear_obj_bbox_to_mmt_in = L(1024, 768), L(4, 768)
        self.obj_feat_layer_norm, self.obj_bbox_layer_norm = LN(768), LN(768)
        self.linear_ocr_feat_to_mmt_in, self.linear_ocr_bbox_to_mmt_in = L(812, 768), L(4, 768)
        self.ocr_feat_layer_norm, self.ocr_bbox_layer_norm, self.ocr_text_layer_norm = LN(768), LN(768), LN(768)
        self.mmt = O.OracleMMT(cfg)
        head = O.OracleM4CDecodingHead(768, V)
        self.ocr_ptr_net, self.classifier = head.ocr_ptr_net, head.classifier

    def forward(self, txt, txt_mask, reg, box, f1, f2, f3, ocr_box, prev):
        import torch.nn.functional as F
        from openvivqa_amd.utils import generate_padding_mask
        obj = self.obj_feat_layer_norm(self.linear_obj_feat_to_mmt_in(reg)) + \
            self.obj_bbox_layer_norm(self.linear_obj_bbox_to_mmt_in(box))
        feat = torch.cat([F.normalize(f1, dim=-1), F.normalize(f2, dim=-1), F.normalize(f3, dim=-1)], dim=-1)
        ocr = self.ocr_feat_layer_norm(self.linear_ocr_feat_to_mmt_in(feat)) + \
            self.ocr_bbox_layer_norm(self.linear_ocr_bbox_to_mmt_in(ocr_box))
        obj_mask, ocr_mask = generate_padding_mask(reg, 0).float(), generate_padding_mask(feat, 0).float()
        res = self.mmt(txt, txt_mask, obj, obj_mask, ocr, ocr_mask, self.classifier.weight, prev)
        dec = res["mmt_dec_output"]
        return torch.cat([self.classifier(dec), self.ocr_ptr_net(dec, res["mmt_ocr_output"], ocr_mask)], dim=-1)


@pytest.mark.parametrize("use_graph", [False, True])
def test_m4c_two_training_steps_match_oracle(use_graph):
    """fp32, dropout off, B=4, |V|=300: losses and post-step weights -- classifier.weight, which is also the answer table
    the decoding positions embed, included -- follow torch.optim.Adam on the oracle."""
    import openvivqa_amd as A
    from openvivqa_amd.models.mmf_m4c import M4CLoss, M4CTrainModel, m4c_mmt_config, synthetic_batch
    from openvivqa_amd.train import TrainStep
    V, B = 300, 4
    cfg = m4c_mmt_config()
    torch.manual_seed(31)
    ref = _RefM4C(V, cfg)
    w0 = {k: v.clone() for k, v in ref.state_dict().items()}
    ref.eval()  # dropout off
    inputs, tgt = synthetic_batch(B, V, "cpu", seed=4)
    nll = torch.nn.NLLLoss(ignore_index=0)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.9, 0.98))

    def ref_loss():
        s = ref(*inputs)
        return nll(torch.log_softmax(s, -1).reshape(-1, s.shape[-1]), tgt.reshape(-1))
    import oracle as O
    ref_losses = [O.oracle_train_step(None, ref_loss, opt) for _ in range(2)]

    A.set_compute_dtype(torch.float32)
    try:
        dev = torch.device("cuda", 0)
        m = M4CTrainModel(V)
        m.load_state_dict(w0)
        m = m.to(dev).train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        loss_fn, tg = M4CLoss(0), tgt.to(dev)
        ts = TrainStep(m, lambda *x: loss_fn(m(*x), tg), lr=1e-3, betas=(0.9, 0.98), use_graph=use_graph,
                       compute_dtype=torch.float32)
        batch = tuple(t.to(dev) for t in inputs)
        losses = [float(ts.step(*batch)) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        A.set_compute_dtype(torch.bfloat16)
    assert max(abs(a - b) for a, b in zip(losses, ref_losses)) < 2e-4, (losses, ref_losses)
    sd = m.state_dict()
    num = den = 0.0
    for k, v in ref.state_dict().items():
        if k.endswith("attention.self.key.bias"):
            continue  # analytically zero gradient: Adam turns rounding noise into +-lr steps
        d = (sd[k].cpu().double() - v.double()).abs()
        assert d.max().item() < 1e-3, (k, d.max().item())
        upd = v.double() - w0[k].double()
        num += ((sd[k].cpu().double() - w0[k].double()) - upd).pow(2).sum().item()
        den += upd.pow(2).sum().item()
    assert den > 0 and (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5
    cu = (sd["classifier.weight"].cpu().double() - w0["classifier.weight"].double())
    cr = ref.state_dict()["classifier.weight"].double() - w0["classifier.weight"].double()
    assert ((cu - cr).norm() / cr.norm()).item() < 1e-2


def _child(mode, env_extra, out):
    env = dict(os.environ)
    env.update(env_extra)
    out = str(out)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return out, r.stdout


def test_m4c_dropout_masks_agree_on_mfma_and_valu_attention(tmp_path):
    """One bf16 training-mode forward + backward, dropout 0.1 at every site, in two fresh processes: default routing
    (MFMA attention) and OVQA_FORCE_SIMPLE=1 (VALU kernels).  Same masks -> loss, scores and every gradient agree to
    bf16 accuracy; a different attention mask would be off by O(0.1)."""
    a, _ = _child("fwdbwd", {"OVQA_FORCE_SIMPLE": "0"}, tmp_path / "mfma.pt")
    b, _ = _child("fwdbwd", {"OVQA_FORCE_SIMPLE": "1"}, tmp_path / "simple.pt")
    ra, rb = torch.load(a), torch.load(b)
    assert ra["dispatch"] == "mfma" and rb["dispatch"] == "simple"

    def rel(x, y):
        return ((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30)).item()
    assert rel(ra["loss"], rb["loss"]) < 2e-2 and rel(ra["scores"], rb["scores"]) < 2e-2
    assert ra["grads"].keys() == rb["grads"].keys() and len(ra["grads"]) > 50
    for k in ra["grads"]:
        if k.endswith("attention.self.key.bias") or k == "ocr_text_layer_norm.weight" or k == "ocr_text_layer_norm.bias":
            continue  # analytically zero (rounding noise only) / unused by the forward
        assert rel(ra["grads"][k], rb["grads"][k]) < 2e-2, (k, rel(ra["grads"][k], rb["grads"][k]))


def test_m4c_training_step_runs_on_mfma_kernels_only(tmp_path):
    """B=64, S=182, dropout on: three graphed bf16 TrainSteps with OVQA_REQUIRE_MFMA=1 (a bf16 call that would fall back
    to the VALU kernels raises) complete with finite losses."""
    _, out = _child("require", {"OVQA_REQUIRE_MFMA": "1"}, tmp_path / "unused")
    losses = json.loads(out.strip().splitlines()[-1])["losses"]
    assert len(losses) == 3 and all(torch.isfinite(torch.tensor(losses)))


def test_m4c_training_reduces_loss_bf16():
    """30 hipGraph-replayed bf16 steps on one fixed batch (dropout on at every site): the loss goes down."""
    import openvivqa_amd as A
    from openvivqa_amd.models.mmf_m4c import M4CLoss, M4CTrainModel, synthetic_batch
    from openvivqa_amd.train import TrainStep
    A.set_compute_dtype(torch.bfloat16)
    A.manual_seed(5)
    torch.manual_seed(5)
    dev = torch.device("cuda", 0)
    V = 300
    m = M4CTrainModel(V).to(dev).train()
    inputs, tgt = synthetic_batch(8, V, dev, seed=6)
    loss_fn = M4CLoss(0)
    ts = TrainStep(m, lambda *x: loss_fn(m(*x), tgt), lr=2e-4, betas=(0.9, 0.98), use_graph=True)
    losses = [float(ts.step(*inputs)) for _ in range(30)]
    assert all(map(lambda v: v == v, losses))
    assert sum(losses[-5:]) / 5 < 0.8 * sum(losses[:5]) / 5, losses


def _child_main(mode, out):
    sys.path.insert(0, ROOT)
    import openvivqa_amd as A
    from openvivqa_amd import _lib
    from openvivqa_amd.models.mmf_m4c import M4CLoss, M4CTrainModel, synthetic_batch
    A.set_compute_dtype(torch.bfloat16)
    A.manual_seed(17)
    torch.manual_seed(17)
    dev = torch.device("cuda", 0)
    if mode == "fwdbwd":
        V = 300
        m = M4CTrainModel(V).to(dev).train()
        inputs, tgt = synthetic_batch(4, V, dev, seed=8)
        scores = m(*inputs)
        loss = M4CLoss(0)(scores, tgt)
        loss.backward()
        torch.cuda.synchronize()
        # which kernel family an attention call with dropout runs on in this process: mfma / simple
        from openvivqa_amd import ops
        q = torch.zeros(1, 182, 768, dtype=torch.bfloat16, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.attention_fwd(q, q, q, None, 8, att_drop=ops.DropSpec(p=0.1, seed=1, site=1, step=step))
        dispatch = _lib.last_dispatch()
        grads = {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
        torch.save({"loss": loss.detach().float().cpu(), "scores": scores.detach().float().cpu(), "grads": grads,
                    "dispatch": dispatch}, out)
    else:
        from openvivqa_amd.train import TrainStep
        V = 5000
        m = M4CTrainModel(V).to(dev).train()
        inputs, tgt = synthetic_batch(64, V, dev, seed=9)
        loss_fn = M4CLoss(0)
        ts = TrainStep(m, lambda *x: loss_fn(m(*x), tgt), lr=1e-4, betas=(0.9, 0.98), use_graph=True)
        losses = [float(ts.step(*inputs)) for _ in range(3)]
        torch.cuda.synchronize()
        print(json.dumps({"losses": losses}))


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
