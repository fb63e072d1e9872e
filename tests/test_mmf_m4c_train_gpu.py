"""Training the whole MMF_M4C (TextBert inside the step) under TrainStep: int64 question tokens in, the whole step in one
hipGraph, Adam over the word / position / token-type tables through the flat path.  The reference is torch.optim.Adam on
tests/text_bert_ref.py + test_m4c_train_gpu._RefM4C, with the bars of test_m4c_two_training_steps_match_oracle."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B, TEXT_LAYERS = 300, 4, 2
TABLES = tuple("text_bert.embeddings." + n + "_embeddings.weight" for n in ("word", "position", "token_type"))


def _ref_class():
    from test_m4c_train_gpu import _RefM4C
    from text_bert_ref import RefTextBert

    class RefWhole(_RefM4C):
        """mmf_m4c.py:128-141, 204-235 in plain torch, with the reference's parameter names."""

        def __init__(self, num_choices, cfg, tb_cfg):
            super().__init__(num_choices, cfg)
            self.text_bert = RefTextBert(tb_cfg)

        def forward(self, tokens, txt_mask, *rest):
            return super().forward(self.text_bert(tokens, txt_mask), txt_mask, *rest)
    return RefWhole


@functools.lru_cache(maxsize=None)
def reference_run(text_vocab):
    """(initial weights, weights after two Adam steps, the two losses, inputs, targets) of the plain-torch model -- computed
    once per table size and shared by the tests below."""
    import oracle as O
    from openvivqa_amd.models.mmf_m4c import m4c_mmt_config, synthetic_batch, text_bert_config
    torch.manual_seed(31)
    ref = _ref_class()(V, m4c_mmt_config(), text_bert_config(768, TEXT_LAYERS, 8, vocab_size=text_vocab))
    with torch.no_grad():  # BERT's initialisation of the text encoder (the tables at torch's N(0, 1) would swamp the rest)
        for p in ref.text_bert.parameters():
            if p.dim() == 2:
                p.normal_(0, 0.02)
        ref.text_bert.embeddings.word_embeddings.weight[0].zero_()
    w0 = {k: v.clone() for k, v in ref.state_dict().items()}
    ref.eval()  # dropout off
    inputs, tgt = synthetic_batch(B, V, "cpu", seed=4, question_vocab=text_vocab)
    nll = torch.nn.NLLLoss(ignore_index=0)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.9, 0.98))

    def ref_loss():
        s = ref(*inputs)
        return nll(torch.log_softmax(s, -1).reshape(-1, s.shape[-1]), tgt.reshape(-1))
    losses = [O.oracle_train_step(None, ref_loss, opt) for _ in range(2)]
    return w0, {k: v.clone() for k, v in ref.state_dict().items()}, losses, inputs, tgt


@functools.lru_cache(maxsize=None)
def hip_run(text_vocab, use_graph):
    """(losses, weights on the host) after two fp32 TrainStep steps of MMF_M4C from the reference's initial weights."""
    import openvivqa_amd as A
    from openvivqa_amd.builders.model_builder import build_model
    from openvivqa_amd.models.mmf_m4c import M4CLoss
    from openvivqa_amd.train import TrainStep
    from test_text_bert_modules_gpu import ITEM_KEYS, _Vocab, m4c_config
    w0, _, _, inputs, tgt = reference_run(text_vocab)
    A.set_compute_dtype(torch.float32)
    try:
        dev = torch.device("cuda", 0)
        m = build_model(m4c_config(TEXT_LAYERS, text_vocab), _Vocab(V))
        m.load_state_dict(w0)
        m = m.to(dev).train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        loss_fn, tg = M4CLoss(0), tgt.to(dev)
        ts = TrainStep(m, lambda *x: loss_fn(m(dict(zip(ITEM_KEYS, x)))["scores"], tg), lr=1e-3, betas=(0.9, 0.98),
                       use_graph=use_graph, compute_dtype=torch.float32)
        batch = tuple(t.to(dev) for t in inputs)
        assert batch[0].dtype == torch.int64
        losses = [float(ts.step(*batch)) for _ in range(2)]
        torch.cuda.synchronize()
        ts.check_device_status()
        return losses, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    finally:
        A.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("text_vocab,use_graph", [(1000, False), (1000, True), (30522, True)])
def test_mmf_m4c_two_training_steps_match_oracle(text_vocab, use_graph):
    """fp32, dropout off, B = 4, |V| = 300, 2 TextBert layers: losses and post-step weights -- the word, position and
    token-type tables among them -- follow torch.optim.Adam on the plain-torch model."""
    w0, ref_sd, ref_losses, _, _ = reference_run(text_vocab)
    losses, sd = hip_run(text_vocab, use_graph)
    assert max(abs(a - b) for a, b in zip(losses, ref_losses)) < 2e-4, (losses, ref_losses)
    assert set(sd) == set(ref_sd) and all(k in sd for k in TABLES)
    num = den = 0.0
    for k, v in ref_sd.items():
        if k.endswith("attention.self.key.bias"):
            continue  # analytically zero gradient: Adam turns rounding noise into +-lr steps
        d = (sd[k].double() - v.double()).abs()
        assert d.max().item() < 1e-3, (k, d.max().item())
        upd = v.double() - w0[k].double()
        num += ((sd[k].double() - w0[k].double()) - upd).pow(2).sum().item()
        den += upd.pow(2).sum().item()
    assert den > 0 and (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5
    for k in TABLES + ("classifier.weight",):
        cu, cr = sd[k].double() - w0[k].double(), ref_sd[k].double() - w0[k].double()
        assert cr.norm() > 0 and ((cu - cr).norm() / cr.norm()).item() < 1e-2, k
    word = "text_bert.embeddings.word_embeddings.weight"
    assert torch.equal(sd[word][0], w0[word][0]) and float(sd[word][0].abs().max()) == 0.0  # the padding row never moves


def test_mmf_m4c_graph_steps_equal_eager_steps():
    """Without dropout the captured step and the eager step are the same kernels on the same data: the same bits."""
    le, se = hip_run(1000, False)
    lg, sg = hip_run(1000, True)
    assert le == lg, (le, lg)
    diff = [k for k in se if not torch.equal(se[k], sg[k])]
    assert not diff, diff


def test_mmf_m4c_bf16_training_on_mfma_kernels_reduces_loss(tmp_path):
    """A fresh process under OVQA_REQUIRE_MFMA=1 (a bf16 call that would fall back to the VALU kernels raises): ten graphed
    bf16 steps, dropout 0.1 at every site, 4 TextBert layers, on one batch -- the loss ends lower than it began and the
    device status word is clean."""
    env = dict(os.environ, OVQA_REQUIRE_MFMA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    losses = json.loads(r.stdout.strip().splitlines()[-1])["losses"]
    assert len(losses) == 10 and all(v == v for v in losses)
    assert losses[-1] < losses[0], losses


def _child_main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import openvivqa_amd as A
    from openvivqa_amd.builders.model_builder import build_model
    from openvivqa_amd.models.mmf_m4c import M4CLoss, synthetic_batch
    from openvivqa_amd.train import TrainStep
    from test_text_bert_modules_gpu import ITEM_KEYS, _Vocab, m4c_config
    A.set_compute_dtype(torch.bfloat16)
    A.manual_seed(23)
    torch.manual_seed(23)
    dev = torch.device("cuda", 0)
    m = build_model(m4c_config(4, 1000), _Vocab(V)).train()
    inputs, tgt = synthetic_batch(8, V, dev, seed=6, question_vocab=1000)
    loss_fn = M4CLoss(0)
    ts = TrainStep(m, lambda *x: loss_fn(m(dict(zip(ITEM_KEYS, x)))["scores"], tgt), lr=2e-4, betas=(0.9, 0.98), use_graph=True)
    losses = [float(ts.step(*inputs)) for _ in range(10)]
    torch.cuda.synchronize()
    ts.check_device_status()
    print(json.dumps({"losses": losses}))


if __name__ == "__main__":
    _child_main()
