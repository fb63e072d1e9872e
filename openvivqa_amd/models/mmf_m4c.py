"""M4C's training forward (BASELINE configs[3]) on the product's blocks: models/mmf_m4c.py:100-235 without the text encoder.

``M4CTrainModel(txt_emb, txt_mask, region_features, region_boxes, ocr_fasttext, ocr_rec, ocr_det, ocr_boxes,
answer_tokens)`` returns the scores (B, T, |V| + n_ocr) of the teacher-forced decoding positions:
  object encoding   LN(Linear 1024->768)(feat) + LN(Linear 4->768)(box), dropout          (:135-154)
  OCR encoding      F.normalize of fasttext (300) | rec (256) | det (256) -> 812, same form (:156-199)
  masks             (B,1,1,N) additive padding masks of all-zero feature rows (generate_padding_mask(.., 0))
  body              MMT with prev_inds = answer_tokens (:230-233); every attention call applies dropout to its
                    probabilities in training (BertConfig's attention_probs_dropout_prob), on the MFMA kernels
  scores            classifier(dec) || OcrPtrNet(dec, ocr)                                 (:221-229)

The reference's TextBert is trained with the rest of the model (nothing there freezes it: ``FREEZE_WEIGHTS`` is never
read): ``MMF_M4C`` below puts it in front.  ``M4CTrainModel`` itself takes TextBert's output ``txt_emb`` (B x 20 x 768) and
the question mask (B,1,1,20) as inputs.  Parameter names are the reference's
(``linear_obj_feat_to_mmt_in``, ``mmt.*``, ``ocr_ptr_net.*``, ``classifier.*``, ...): a reference checkpoint loads once its
``text_bert.*`` keys are dropped.  Not registered under ``MMF_M4C``: it is not the whole reference model -- the class
``MMF_M4C`` is.

``classifier.weight`` is also the fixed answer table the decoding positions embed (``fixed_ans_emb``, :216), so in
training it receives two gradients: the classifier product's (stored eagerly, Fn.linear(eager_wgrad=True)) and, added to
it by autograd later in the same backward pass, the one through PrevPredEmbeddings' answer LayerNorm and row gather.

Evaluation mode delegates to ``M4CDecodingHead.greedy_decode`` (the graphed decode lives in ``GraphedGreedyDecode``).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

from .. import functional as Fn
from .. import runtime as rt
from ..builders.model_builder import META_ARCHITECTURE
from ..losses import NLLLoss
from ..modules.mmt import MMT, M4CDecodingHead, TextBert, load_text_bert_weights
from ..modules.pointer import OcrPtrNet
from ..utils import generate_padding_mask


def m4c_mmt_config(hidden_size=768, num_hidden_layers=4, num_attention_heads=8, hidden_dropout_prob=0.1,
                   attention_probs_dropout_prob=0.1):
    """BertConfig(hidden_size, num_hidden_layers, num_attention_heads) with transformers' defaults for the rest
    (mmf_m4c.py:28-31): intermediate 4 x hidden, LayerNorm eps 1e-12, both dropout probabilities 0.1."""
    return SimpleNamespace(hidden_size=hidden_size, num_hidden_layers=num_hidden_layers,
                           num_attention_heads=num_attention_heads, intermediate_size=4 * hidden_size, layer_norm_eps=1e-12,
                           hidden_dropout_prob=hidden_dropout_prob, attention_probs_dropout_prob=attention_probs_dropout_prob,
                           hidden_act="gelu")


class M4CTrainModel(nn.Module):
    def __init__(self, num_choices: int, mmt_config=None, obj_feature=1024, ocr_feature=812, obj_dropout=0.1,
                 ocr_dropout=0.1, ptr_query_key_size=None):
        super().__init__()
        cfg = mmt_config if mmt_config is not None else m4c_mmt_config()
        d = cfg.hidden_size
        self.mmt_config = cfg
        self.linear_obj_feat_to_mmt_in = nn.Linear(obj_feature, d)
        self.linear_obj_bbox_to_mmt_in = nn.Linear(4, d)
        self.obj_feat_layer_norm = nn.LayerNorm(d)  # (nn.LayerNorm's eps 1e-5, not BERT's)
        self.obj_bbox_layer_norm = nn.LayerNorm(d)
        self.obj_drop = nn.Dropout(obj_dropout)
        self.linear_ocr_feat_to_mmt_in = nn.Linear(ocr_feature, d)
        self.linear_ocr_bbox_to_mmt_in = nn.Linear(4, d)
        self.ocr_feat_layer_norm = nn.LayerNorm(d)
        self.ocr_bbox_layer_norm = nn.LayerNorm(d)
        self.ocr_text_layer_norm = nn.LayerNorm(d)  # built and unused by the reference (a checkpoint carries it)
        self.ocr_drop = nn.Dropout(ocr_dropout)
        self.mmt = MMT(cfg)
        self.ocr_ptr_net = OcrPtrNet(d, ptr_query_key_size)
        self.classifier = nn.Linear(d, num_choices)
        self._sites = [rt.new_dropout_site() for _ in range(2)]

    def _encode(self, feat, box, lin_f, ln_f, lin_b, ln_b, drop, site):
        """dropout(LN(lin_f(feat)) + LN(lin_b(box))): GEMMs, LayerNorms and dropout on the HIP kernels (the sum is a
        torch add)."""
        arena = rt.ensure_arena(self)
        T = arena.compute_dtype
        a = Fn.prologue(Fn.linear(feat.to(T), lin_f, arena), ln_f, None, arena, T)
        b = Fn.prologue(Fn.linear(box.to(T), lin_b, arena), ln_b, None, arena, T)
        return Fn.dropout(a + b, rt.dropout_spec(drop.p, site, self.training, a.device))

    def encode(self, region_features, region_boxes, ocr_fasttext, ocr_rec, ocr_det, ocr_boxes):
        """(obj_emb, obj_mask, ocr_emb, ocr_mask).  mmf_m4c.py:135-199."""
        obj = self._encode(region_features, region_boxes, self.linear_obj_feat_to_mmt_in, self.obj_feat_layer_norm,
                           self.linear_obj_bbox_to_mmt_in, self.obj_bbox_layer_norm, self.obj_drop, self._sites[0])
        ocr_feat = torch.cat([F.normalize(ocr_fasttext, dim=-1), F.normalize(ocr_rec, dim=-1),
                              F.normalize(ocr_det, dim=-1)], dim=-1)
        ocr = self._encode(ocr_feat, ocr_boxes, self.linear_ocr_feat_to_mmt_in, self.ocr_feat_layer_norm,
                           self.linear_ocr_bbox_to_mmt_in, self.ocr_bbox_layer_norm, self.ocr_drop, self._sites[1])
        return (obj, generate_padding_mask(region_features, 0).float(), ocr,
                generate_padding_mask(ocr_feat, 0).float())

    def scores(self, mmt_results, ocr_mask):
        """classifier(dec) || OcrPtrNet(dec, ocr): mmf_m4c.py:221-229 (also what greedy decoding calls)."""
        dec, ocr = mmt_results["mmt_dec_output"], mmt_results["mmt_ocr_output"]
        arena = rt.ensure_arena(self)
        fixed = Fn.linear(dec.to(arena.compute_dtype), self.classifier, arena, eager_wgrad=True)
        return torch.cat([fixed.float(), self.ocr_ptr_net(dec, ocr, ocr_mask).float()], dim=-1)

    def forward(self, txt_emb, txt_mask, region_features, region_boxes, ocr_fasttext, ocr_rec, ocr_det, ocr_boxes,
                answer_tokens=None, max_iter=12, bos_idx=1, eos_idx=2):
        obj, obj_mask, ocr, ocr_mask = self.encode(region_features, region_boxes, ocr_fasttext, ocr_rec, ocr_det,
                                                   ocr_boxes)
        if not self.training:
            scores, _, _ = M4CDecodingHead.greedy_decode(self, self.mmt, txt_emb, txt_mask, obj, obj_mask, ocr, ocr_mask,
                                                         max_iter, bos_idx, eos_idx)
            return scores
        res = self.mmt(txt_emb=txt_emb, txt_mask=txt_mask, obj_emb=obj, obj_mask=obj_mask, ocr_emb=ocr,
                       ocr_mask=ocr_mask, fixed_ans_emb=self.classifier.weight, prev_inds=answer_tokens)
        return self.scores(res, ocr_mask)


def text_bert_config(hidden_size=768, num_hidden_layers=12, num_attention_heads=8, vocab_size=30522):
    """BertConfig(hidden_size, num_hidden_layers, num_attention_heads) of the text encoder (mmf_m4c.py:49-51) with
    transformers' defaults for the rest: 30522 words, 512 positions, 2 token types, pad_token_id 0, initializer_range 0.02."""
    cfg = m4c_mmt_config(hidden_size, num_hidden_layers, num_attention_heads)
    cfg.vocab_size, cfg.max_position_embeddings, cfg.type_vocab_size = vocab_size, 512, 2
    cfg.pad_token_id, cfg.initializer_range = 0, 0.02
    return cfg


@META_ARCHITECTURE.register()
class MMF_M4C(M4CTrainModel):
    """The reference's whole ``MMF_M4C(config, vocab)`` (models/mmf_m4c.py:21-256), built from the reference's config keys
    (``MMT.*``, ``TEXT_BERT.*``, ``OBJECT_EMBEDDING.*``, ``OCR_EMBEDDING.*``, ``OCR_PTR_NET.*``): ``M4CTrainModel``'s
    encodings, multimodal transformer and heads behind a trained ``text_bert`` (``modules.mmt.TextBert``), so a training step
    runs TextBert forward and backward and Adam over its 30522 x 768 word table, as the reference's does.

    ``forward(items)`` reads ``question_tokens``, ``region_features``, ``region_boxes``, ``ocr_fasttext_features``,
    ``ocr_rec_features``, ``ocr_det_features``, ``ocr_boxes`` and (training) ``answer_tokens`` and returns
    ``{"scores": ...}``: teacher-forced in training (:231-235), the greedy decode in evaluation -- TextBert runs ONCE per call
    there (the reference recomputes it in every pass with the same result).

    Kept quirks: TextBert's head count is ``MMT.NUM_ATTENTION_HEADS``, not ``TEXT_BERT.NUM_ATTENTION_HEADS`` (:51);
    ``text_bert_out_linear`` is ``nn.Identity`` when the MMT's hidden size is 768 and an ``nn.Linear`` otherwise (:62-71).
    ``TEXT_BERT.FREEZE_WEIGHTS`` is ignored, as the reference ignores it: nothing there reads the key, and the optimiser is
    built over ``model.parameters()``.  ``TEXT_BERT.LOAD_PRETRAINED`` never touches a network: ``PRETRAINED_NAME`` must be a
    local torch state dict (``modules.mmt.load_text_bert_weights``).  One key the reference does not have,
    ``TEXT_BERT.VOCAB_SIZE`` (default 30522), sizes the word table."""

    def __init__(self, config, vocab):
        mmt, tb = config.MMT, config.TEXT_BERT
        super().__init__(len(vocab), m4c_mmt_config(mmt.HIDDEN_SIZE, mmt.NUM_HIDDEN_LAYERS, mmt.NUM_ATTENTION_HEADS),
                         obj_feature=config.OBJECT_EMBEDDING.D_FEATURE, ocr_feature=config.OCR_EMBEDDING.D_FEATURE,
                         obj_dropout=config.OBJECT_EMBEDDING.DROPOUT, ocr_dropout=config.OCR_EMBEDDING.DROPOUT,
                         ptr_query_key_size=config.OCR_PTR_NET.QUERY_KEY_SIZE)
        self.config, self.vocab = config, vocab
        self.d_model = mmt.HIDDEN_SIZE
        self.device = torch.device(config.DEVICE)
        self.max_iter = vocab.max_answer_length
        self.text_bert_config = text_bert_config(tb.HIDDEN_SIZE, tb.NUM_HIDDEN_LAYERS, mmt.NUM_ATTENTION_HEADS,
                                                 tb["VOCAB_SIZE"] if "VOCAB_SIZE" in tb else 30522)
        self.text_bert = TextBert(self.text_bert_config)
        if tb.LOAD_PRETRAINED:
            load_text_bert_weights(self.text_bert, tb.PRETRAINED_NAME)
        self.text_bert_out_linear = nn.Identity() if mmt.HIDDEN_SIZE == 768 else nn.Linear(tb.HIDDEN_SIZE, mmt.HIDDEN_SIZE)

    def encode_text(self, question_tokens):
        """(txt_emb, txt_mask): mmf_m4c.py:128-141, 204-207."""
        out, txt_mask = self.text_bert.encode(question_tokens, self.vocab.padding_idx)
        if isinstance(self.text_bert_out_linear, nn.Linear):
            arena = rt.ensure_arena(self)
            out = Fn.linear(out.to(arena.compute_dtype), self.text_bert_out_linear, arena)
        return out, txt_mask

    def forward(self, items):
        def item(name):
            return items[name] if isinstance(items, dict) else getattr(items, name)
        txt_emb, txt_mask = self.encode_text(item("question_tokens"))
        feats = [item(k) for k in ("region_features", "region_boxes", "ocr_fasttext_features", "ocr_rec_features",
                                   "ocr_det_features", "ocr_boxes")]
        scores = M4CTrainModel.forward(self, txt_emb, txt_mask, *feats,
                                       answer_tokens=item("answer_tokens") if self.training else None,
                                       max_iter=self.max_iter, bos_idx=self.vocab.bos_idx, eos_idx=self.vocab.eos_idx)
        return {"scores": scores}


class M4CLoss(nn.Module):
    """NLLLoss(ignore_index = padding_idx)(log_softmax(scores), shifted-right answers): tasks/training_mmf_task.py:101-108,
    log_softmax over the |V| + n_ocr scores and the loss on the HIP kernels."""

    def __init__(self, padding_idx: int = 0):
        super().__init__()
        self.nll = NLLLoss(ignore_index=padding_idx)

    def forward(self, scores, shifted_right_answer_tokens):
        logp = Fn.log_softmax(scores)
        return self.nll(logp.view(-1, logp.shape[-1]), shifted_right_answer_tokens.reshape(-1))


def synthetic_batch(B, num_choices, device, seed=0, T=12, n_txt=20, n_obj=100, n_ocr=50, d=768, dtype=torch.float32,
                    question_vocab=None):
    """Seeded inputs of configs[3]'s shapes with padding: some regions / OCR tokens are all-zero rows, some question
    positions are masked, some answers end early (padding_idx 0 after them).  Returns (inputs, targets): ``inputs`` =
    (txt_emb, txt_mask, region_features, region_boxes, ocr_fasttext, ocr_rec, ocr_det, ocr_boxes, answer_tokens) with
    answer_tokens = <bos> a_1 .. a_{T-1}; ``targets`` = a_1 .. a_T (the shifted-right answers).

    ``question_vocab`` = N: the first input is ``question_tokens`` (int64 B x n_txt, ids in [1, N), padding id 0 from where
    ``txt_mask`` masks) instead of ``txt_emb`` -- what ``MMF_M4C`` reads; every other tensor is the default batch's."""
    from ..utils import MASK_VALUE
    g = torch.Generator().manual_seed(seed)
    txt = torch.randn(B, n_txt, d, generator=g)
    txt_mask = torch.zeros(B, 1, 1, n_txt)
    reg, box = torch.randn(B, n_obj, 1024, generator=g).abs(), torch.rand(B, n_obj, 4, generator=g)
    f1, f2, f3 = (torch.randn(B, n_ocr, n, generator=g) for n in (300, 256, 256))
    ocr_box = torch.rand(B, n_ocr, 4, generator=g)
    ans = torch.randint(3, num_choices + n_ocr - 16, (B, T + 1), generator=g)  # (copies of unpadded OCR tokens only)
    ans[:, 0] = 1
    for b in range(B):
        if b % 2:
            txt_mask[b, ..., n_txt - 2 - b % 7:] = MASK_VALUE
            reg[b, n_obj - 10 - b % 13:] = 0
            box[b, n_obj - 10 - b % 13:] = 0
            for f in (f1, f2, f3, ocr_box):
                f[b, n_ocr - 5 - b % 11:] = 0
            ans[b, 4 + b % (T - 4):] = 0
    if question_vocab is not None:
        q = torch.randint(1, question_vocab, (B, n_txt), generator=torch.Generator().manual_seed(seed + 7919))
        q[txt_mask[:, 0, 0] != 0] = 0
        txt = q
    inputs = [t.to(device) for t in (txt, txt_mask, reg, box, f1, f2, f3, ocr_box)]
    if question_vocab is None:
        inputs[0] = inputs[0].to(dtype)
    return tuple(inputs) + (ans[:, :-1].contiguous().to(device),), ans[:, 1:].contiguous().to(device)
