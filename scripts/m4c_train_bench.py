"""M4C training step (BASELINE configs[3]) on one GPU: samples/s of M4CTrainModel + M4CLoss under TrainStep.

Workload: B=64, T=12 decoding positions (S = 20 + 100 + 50 + 12 = 182), |V| = 5000, 100 regions with boxes, 50 OCR tokens,
dropout 0.1 at every site (the attention probabilities included), bf16, the whole step (forward, loss, backward, Adam
(0.9, 0.98)) replayed from one hipGraph.  Synthetic seeded inputs with padded regions / OCR rows / answer positions.
Prints one JSON line.  Needs the GPU: there is no fallback.

    python scripts/m4c_train_bench.py [--steps 100] [--warmup 20] [--batch 64] [--text-bert LAYERS]

``--text-bert 0`` (the default) is the run above.  ``--text-bert 4`` / ``12``: the reference's WHOLE step -- the registered
``MMF_M4C`` with that many TextBert layers (30522 x 768 word table, 20 question tokens) trained inside the step -- and, next to
it, the BERT-embeddings op alone (forward + backward, B x 20 tokens) beside the stock composition F.embedding x 3 + add +
F.layer_norm + F.dropout on the same tensors: device events, the median of 5 windows.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def gflop_per_step(B, T=12, V=5000, n_txt=20, n_obj=100, n_ocr=50, d=768, ff=3072, layers=4, text_layers=0):
    """Algorithmic GFLOP of one training step: 3 x (forward) -- backward = 2 x forward -- over B samples.  Forward per
    sample: the MMT pass (per position and layer the four d x d projections and the two d x ff FFN products, plus scores
    and weighted sum over S positions: BASELINE.md section 3's 10.71 GF at S = 182), the object / OCR encoders (1024 -> d,
    812 -> d) and the heads (classifier d -> V and the pointer's two d x d projections and scores on T positions)."""
    S = n_txt + n_obj + n_ocr + T
    mmt = S * layers * (2 * (4 * d * d + 2 * d * ff) + 4 * S * d)
    enc = 2 * n_obj * 1024 * d + 2 * n_ocr * 812 * d
    heads = 2 * T * d * V + 2 * (T + n_ocr) * d * d + 2 * T * n_ocr * d
    text = n_txt * text_layers * (2 * (4 * d * d + 2 * d * ff) + 4 * n_txt * d)  # TextBert over the question tokens
    return 3 * B * (mmt + enc + heads + text) / 1e9


class _Vocab:
    padding_idx, bos_idx, eos_idx, max_answer_length = 0, 1, 2, 12

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


ITEM_KEYS = ("question_tokens", "txt_mask", "region_features", "region_boxes", "ocr_fasttext_features", "ocr_rec_features",
             "ocr_det_features", "ocr_boxes", "answer_tokens")


def whole_model_config(text_layers):
    """The keys of the reference's configs/mmf_m4c.yaml that MMF_M4C reads (no pretrained weights: nothing is downloaded)."""
    from openvivqa_amd.config import ConfigNode
    return ConfigNode(dict(
        ARCHITECTURE="MMF_M4C", DEVICE="cuda", MMT=dict(HIDDEN_SIZE=768, NUM_HIDDEN_LAYERS=4, NUM_ATTENTION_HEADS=8),
        TEXT_BERT=dict(HIDDEN_SIZE=768, NUM_HIDDEN_LAYERS=text_layers, NUM_ATTENTION_HEADS=12, LOAD_PRETRAINED=False),
        OBJECT_EMBEDDING=dict(D_FEATURE=1024, DROPOUT=0.1), OCR_EMBEDDING=dict(D_FEATURE=812, DROPOUT=0.1),
        OCR_PTR_NET=dict(HIDDEN_SIZE=768, QUERY_KEY_SIZE=768)))


def median_window_us(fn, iters=50, windows=5):
    """Median over ``windows`` of the device-event time of ``iters`` back-to-back calls, per call, in microseconds."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(times)[len(times) // 2]


def embeddings_op_vs_stock(model, tokens, seed):
    """(ours, stock) microseconds of forward + backward of the BERT embeddings at the model's own tables, fp32 in, bf16 out:
    the op of this package (4 launches) and the stock torch composition (its autograd included)."""
    import torch.nn.functional as F
    from openvivqa_amd import ops
    emb = model.text_bert.embeddings
    word, pos, typ = (m.weight.detach() for m in (emb.word_embeddings, emb.position_embeddings, emb.token_type_embeddings))
    gamma, beta = emb.LayerNorm.weight.detach(), emb.LayerNorm.bias.detach()
    B, T = tokens.shape
    D = gamma.shape[0]
    dev = tokens.device
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    drop = ops.DropSpec(p=0.1, seed=seed, site=1, step=step)
    dy = torch.randn(B, T, D, device=dev).to(torch.bfloat16)
    grads = [torch.zeros_like(t) for t in (word, pos, typ, gamma, beta)]

    def ours():
        _, _, mean, rstd, _ = ops.bert_embeddings_fwd(tokens, word, pos, typ, gamma, beta, 1e-12, out_dtype=torch.bfloat16,
                                                      drop=drop, want_f32=True, mask_padding_idx=0)
        ops.bert_embeddings_bwd(dy, tokens, word, pos, typ, gamma, mean, rstd, *grads, drop=drop, table_padding_idx=0)
    leaves = [t.clone().requires_grad_(True) for t in (word, pos, typ, gamma, beta)]
    position_ids, type_ids = torch.arange(T, device=dev)[None].expand(B, T), torch.zeros_like(tokens)

    def stock():
        w, p, t, g, b = leaves
        x = F.embedding(tokens, w, padding_idx=0) + F.embedding(type_ids, t) + F.embedding(position_ids, p)
        y = F.dropout(F.layer_norm(x, (D,), g, b, 1e-12), 0.1, True).to(torch.bfloat16)
        for leaf in leaves:
            leaf.grad = None
        y.backward(dy)
    return median_window_us(ours), median_window_us(stock)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--text-bert", type=int, default=0, metavar="LAYERS",
                    help="0: M4CTrainModel on given text features (default); N > 0: MMF_M4C with N TextBert layers")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("m4c_train_bench: needs the GPU (no CPU fallback)")
    import openvivqa_amd as A
    from openvivqa_amd.models.mmf_m4c import M4CLoss, M4CTrainModel, synthetic_batch
    from openvivqa_amd.train import TrainStep
    V, T, B = 5000, 12, args.batch
    dev = torch.device("cuda", 0)
    A.set_compute_dtype(torch.bfloat16)
    A.manual_seed(args.seed)
    torch.manual_seed(args.seed)
    loss_fn = M4CLoss(0)
    if args.text_bert > 0:
        from openvivqa_amd.builders.model_builder import build_model
        model = build_model(whole_model_config(args.text_bert), _Vocab(V)).train()
        inputs, tgt = synthetic_batch(B, V, dev, seed=args.seed + 1, T=T, question_vocab=30522)
        ts = TrainStep(model, lambda *x: loss_fn(model(dict(zip(ITEM_KEYS, x)))["scores"], tgt), lr=1e-4, betas=(0.9, 0.98),
                       use_graph=True)
    else:
        model = M4CTrainModel(V).to(dev).train()
        inputs, tgt = synthetic_batch(B, V, dev, seed=args.seed + 1, T=T)
        ts = TrainStep(model, lambda *x: loss_fn(model(*x), tgt), lr=1e-4, betas=(0.9, 0.98), use_graph=True)
    for _ in range(max(1, args.warmup)):
        ts.step(*inputs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = ts.step(*inputs)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    answer_tokens = int((tgt != 0).sum())
    gf = gflop_per_step(B, T=T, V=V, text_layers=args.text_bert)
    extra = {}
    if args.text_bert > 0:
        ours, stock = embeddings_op_vs_stock(model, inputs[0], args.seed)
        extra = {"text_bert_layers": args.text_bert, "parameters": sum(p.numel() for p in model.parameters()),
                 "bert_embeddings_fwd_bwd_us": round(ours, 1), "stock_composition_fwd_bwd_us": round(stock, 1)}
    print(json.dumps({
        "metric": "M4C training step (configs[3]), bf16, whole-step hipGraph, 1 GPU" +
                  (", TextBert trained inside the step" if args.text_bert > 0 else ""),
        **extra,
        "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(B / dt, 1),
        "answer_tokens_per_s": round(answer_tokens / dt, 1), "algorithmic_gflop_per_step": round(gf, 1),
        "step_frac_of_bf16_peak": round(gf / dt / 1e3 / 2500.0, 4), "loss": round(float(loss), 4),
        "steps": args.steps, "warmup": args.warmup,
        "config": {"B": B, "T": T, "S": 182, "V": V, "n_obj": 100, "n_ocr": 50, "dropout": 0.1,
                   "optimizer": "Adam(0.9, 0.98)", "seed": args.seed}}))


if __name__ == "__main__":
    main()
