"""M4C training step (BASELINE configs[3]) on one GPU: samples/s of M4CTrainModel + M4CLoss under TrainStep.

Workload: B=64, T=12 decoding positions (S = 20 + 100 + 50 + 12 = 182), |V| = 5000, 100 regions with boxes, 50 OCR tokens,
dropout 0.1 at every site (the attention probabilities included), bf16, the whole step (forward, loss, backward, Adam
(0.9, 0.98)) replayed from one hipGraph.  Synthetic seeded inputs with padded regions / OCR rows / answer positions.
Prints one JSON line.  Needs the GPU: there is no fallback.

    python scripts/m4c_train_bench.py [--steps 100] [--warmup 20] [--batch 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def gflop_per_step(B, T=12, V=5000, n_txt=20, n_obj=100, n_ocr=50, d=768, ff=3072, layers=4):
    """Algorithmic GFLOP of one training step: 3 x (forward) -- backward = 2 x forward -- over B samples.  Forward per
    sample: the MMT pass (per position and layer the four d x d projections and the two d x ff FFN products, plus scores
    and weighted sum over S positions: BASELINE.md section 3's 10.71 GF at S = 182), the object / OCR encoders (1024 -> d,
    812 -> d) and the heads (classifier d -> V and the pointer's two d x d projections and scores on T positions)."""
    S = n_txt + n_obj + n_ocr + T
    mmt = S * layers * (2 * (4 * d * d + 2 * d * ff) + 4 * S * d)
    enc = 2 * n_obj * 1024 * d + 2 * n_ocr * 812 * d
    heads = 2 * T * d * V + 2 * (T + n_ocr) * d * d + 2 * T * n_ocr * d
    return 3 * B * (mmt + enc + heads) / 1e9


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
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
    model = M4CTrainModel(V).to(dev).train()
    inputs, tgt = synthetic_batch(B, V, dev, seed=args.seed + 1, T=T)
    loss_fn = M4CLoss(0)
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
    gf = gflop_per_step(B, T=T, V=V)
    print(json.dumps({
        "metric": "M4C training step (configs[3]), bf16, whole-step hipGraph, 1 GPU",
        "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(B / dt, 1),
        "answer_tokens_per_s": round(answer_tokens / dt, 1), "algorithmic_gflop_per_step": round(gf, 1),
        "step_frac_of_bf16_peak": round(gf / dt / 1e3 / 2500.0, 4), "loss": round(float(loss), 4),
        "steps": args.steps, "warmup": args.warmup,
        "config": {"B": B, "T": T, "S": 182, "V": V, "n_obj": 100, "n_ocr": 50, "dropout": 0.1,
                   "optimizer": "Adam(0.9, 0.98)", "seed": args.seed}}))


if __name__ == "__main__":
    main()
