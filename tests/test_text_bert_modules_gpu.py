"""``modules.mmt.TextBert`` against tests/text_bert_ref.py (fp32 and bf16: output and every parameter gradient, the three
embedding tables included), and ``MMF_M4C`` in evaluation mode against ``M4CTrainModel`` fed with TextBert's own output."""
import pytest
import torch

from test_blocks_gpu import EMU_GRAD_BAR, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(params=[F32, BF16], ids=["fp32", "bf16"])
def mode(request):
    import openvivqa_amd as A
    A.set_compute_dtype(request.param)
    yield request.param
    A.set_compute_dtype(BF16)


def test_text_bert_matches_plain_torch_reference(mode):
    """Hidden 768, 8 heads of 96, 2 layers, 1000 words, B = 4, T = 20, two samples padded.  fp32: rel-L2 2e-5 on the output,
    2e-4 on every gradient (the bars of tests/test_blocks_gpu.py's MMT test).  bf16: 1e-2 on the output against the fp32
    reference, every gradient against the reference in bf16-emulation mode through conftest.grad_close at EMU_GRAD_BAR."""
    import oracle as O
    from conftest import grad_close, parity_record as rec
    from openvivqa_amd.models.mmf_m4c import text_bert_config
    from openvivqa_amd.modules.mmt import TextBert
    from openvivqa_amd.utils import generate_padding_mask
    from text_bert_ref import RefTextBert
    cfg = text_bert_config(768, 2, 8, vocab_size=1000)
    torch.manual_seed(12)
    ref = RefTextBert(cfg).eval()
    with torch.no_grad():
        for n, p in ref.named_parameters():  # BERT's initialisation, with biases and LayerNorm parameters that are not trivial
            if p.dim() == 2:
                p.normal_(0, 0.02)
            elif n.endswith("LayerNorm.weight"):
                p.uniform_(0.8, 1.2)
            else:
                p.normal_(0, 0.05)
        ref.embeddings.word_embeddings.weight[0].zero_()
    hip = TextBert(cfg)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to(DEV).eval()
    g = torch.Generator().manual_seed(13)
    tok = torch.randint(1, 1000, (4, 20), generator=g)
    tok[0, 3] = tok[0, 7] = tok[2, 5] = 17  # a word repeated within and across samples
    tok[1, 14:] = 0
    tok[3, 9:] = 0
    mask = generate_padding_mask(tok, 0).float()
    w = torch.randn(4, 20, 768, generator=g)

    out_h = hip(tok.to(DEV), mask.to(DEV))
    (out_h.float() * w.to(DEV)).sum().backward()
    with torch.no_grad():  # the mask out of the embeddings launch, and the same output through it
        out_e, mask_e = hip.encode(tok.to(DEV), 0)
    assert torch.equal(mask_e.cpu().view(torch.int32), mask.view(torch.int32)) and torch.equal(out_e, out_h.detach())

    def ref_pass(emulate):
        ref.zero_grad(set_to_none=True)
        with O.emulate_bf16(emulate):
            out = ref(tok, mask)
            (out * w).sum().backward()
        return out.detach(), {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}
    out_r, g32 = ref_pass(False)
    tag = f"text_bert[{'fp32' if mode == F32 else 'bf16'}]"
    tol_f = 2e-5 if mode == F32 else 1e-2
    e = rec(tag, "out vs fp32 reference", rel_l2(out_h, out_r), tol_f)
    assert e < tol_f, e
    gh = {k: p.grad for k, p in hip.named_parameters()}
    assert set(g32) == set(gh) and all(v is not None for v in gh.values())
    assert float(gh["embeddings.word_embeddings.weight"][0].abs().max()) == 0.0        # the table's padding row
    assert float(gh["embeddings.position_embeddings.weight"][20:].abs().max()) == 0.0  # positions no token stands at
    assert float(gh["embeddings.token_type_embeddings.weight"][1:].abs().max()) == 0.0
    bad = []
    if mode == F32:
        for k in g32:
            if not k.endswith("self.key.bias") and not rec(tag, f"dW[{k}] vs fp32 reference", rel_l2(gh[k], g32[k]), 2e-4) < 2e-4:
                bad.append((k, rel_l2(gh[k], g32[k])))
    else:
        _, gemu = ref_pass(True)
        for k in g32:
            if k.endswith("self.key.bias"):
                continue  # analytically zero: rounding noise on both sides
            e, fmt = rec(tag, f"dW[{k}] vs emulation", rel_l2(gh[k], gemu[k]), EMU_GRAD_BAR), rel_l2(gemu[k], g32[k])
            if not grad_close(e, fmt, EMU_GRAD_BAR, tag, "dW/" + k):
                bad.append((k, e, fmt))
    assert not bad, bad


class _Vocab:
    padding_idx, bos_idx, eos_idx, max_answer_length = 0, 1, 2, 12

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def m4c_config(text_layers, vocab_size, mmt_layers=4, mmt_hidden=768):
    """The MODEL keys of the reference's mmf_m4c.yaml that MMF_M4C reads, TextBert sized for a test."""
    from openvivqa_amd.config import ConfigNode
    return ConfigNode(dict(
        ARCHITECTURE="MMF_M4C", DEVICE="cuda",
        MMT=dict(HIDDEN_SIZE=mmt_hidden, NUM_HIDDEN_LAYERS=mmt_layers, NUM_ATTENTION_HEADS=8),
        TEXT_BERT=dict(HIDDEN_SIZE=768, NUM_HIDDEN_LAYERS=text_layers, NUM_ATTENTION_HEADS=12, LOAD_PRETRAINED=False,
                       FREEZE_WEIGHTS=True, PRETRAINED_NAME="bert-base-uncased", VOCAB_SIZE=vocab_size),
        OBJECT_EMBEDDING=dict(D_FEATURE=1024, DROPOUT=0.1), OCR_EMBEDDING=dict(D_FEATURE=812, DROPOUT=0.1),
        OCR_PTR_NET=dict(HIDDEN_SIZE=mmt_hidden, QUERY_KEY_SIZE=768)))


ITEM_KEYS = ("question_tokens", "txt_mask", "region_features", "region_boxes", "ocr_fasttext_features", "ocr_rec_features",
             "ocr_det_features", "ocr_boxes", "answer_tokens")


def test_mmf_m4c_eval_equals_train_model_fed_with_text_bert_output():
    """bf16, greedy decode: the registered model is M4CTrainModel behind TextBert and nothing else -- bit for bit."""
    import openvivqa_amd as A
    from openvivqa_amd.builders.model_builder import build_model
    from openvivqa_amd.models.mmf_m4c import M4CTrainModel, m4c_mmt_config, synthetic_batch
    A.set_compute_dtype(BF16)
    A.manual_seed(3)
    torch.manual_seed(3)
    V = 300
    m = build_model(m4c_config(2, 1000, mmt_layers=2), _Vocab(V)).eval()
    base = M4CTrainModel(V, m4c_mmt_config(768, 2, 8), ptr_query_key_size=768)
    missing, unexpected = base.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("text_bert.")})
    assert missing == [] and unexpected == []
    base = base.to(DEV).eval()
    inputs, _ = synthetic_batch(4, V, DEV, seed=11, question_vocab=1000)
    items = dict(zip(ITEM_KEYS, inputs))
    with torch.no_grad():
        scores = m(items)["scores"]
        txt_emb, txt_mask = m.encode_text(items["question_tokens"])
        assert torch.equal(txt_mask, items["txt_mask"])  # (by value: the batch's own mask holds +0.0 where unmasked)
        want = base(txt_emb, txt_mask, *inputs[2:8], max_iter=12, bos_idx=1, eos_idx=2)
    assert scores.shape[0] == 4 and scores.shape[2] == V + 50 and bool(torch.isfinite(scores).all())
    assert torch.equal(scores, want)


def test_mmf_m4c_projects_text_bert_output_into_a_narrower_mmt():
    """MMT hidden 512 (8 heads of 64) behind the 768-wide TextBert: ``text_bert_out_linear`` is an nn.Linear (mmf_m4c.py:62-71)
    on the HIP GEMM.  A bf16 training forward + backward gives finite scores and loss, and gradients that reach the
    projection and, through TextBert, the rows of the word table the questions name."""
    import openvivqa_amd as A
    from openvivqa_amd.builders.model_builder import build_model
    from openvivqa_amd.models.mmf_m4c import M4CLoss, synthetic_batch
    A.set_compute_dtype(BF16)
    A.manual_seed(4)
    torch.manual_seed(4)
    V = 300
    m = build_model(m4c_config(1, 1000, mmt_layers=1, mmt_hidden=512), _Vocab(V)).train()
    assert isinstance(m.text_bert_out_linear, torch.nn.Linear)
    inputs, tgt = synthetic_batch(4, V, DEV, seed=12, question_vocab=1000)
    scores = m(dict(zip(ITEM_KEYS, inputs)))["scores"]
    loss = M4CLoss(0)(scores, tgt)
    loss.backward()
    torch.cuda.synchronize()
    assert tuple(scores.shape) == (4, 12, V + 50) and bool(torch.isfinite(loss))
    gw, word = m.text_bert_out_linear.weight.grad, m.text_bert.embeddings.word_embeddings.weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    named = torch.zeros(1000, dtype=torch.bool, device=DEV)
    named[inputs[0].view(-1)] = True
    named[0] = False
    assert bool((word[named].abs().amax(1) > 0).all()) and float(word[~named].abs().max()) == 0.0
