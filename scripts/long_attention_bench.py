"""Long-sequence attention on the MI355X: the streaming MFMA kernels (csrc/attention_stream.hip) against the VALU kernels
(OVQA_FORCE_SIMPLE routing is per process, so the VALU column comes from a child run with it set), the unfused torch
composition (bmm -> softmax -> bmm, bf16) and torch's scaled_dot_product_attention, forward and backward separately.

Times are PER CALL: device events around `--iters` Python-level calls (each allocates its outputs) after `--warmup` calls,
median of `--reps` windows -- not kernel time from a kernel trace.  FLOPs: the products the algorithm needs, 4 B H n_q n_k d
forward and 8 B H n_q n_k d backward (dQ, dK, dV, dP; the recomputed S not counted); the per-call rate's share of the bf16
dense peak (2.5 PFLOP/s).  Masks: "key" = one key-padding row per sample (the kernels' key-row form), "dense" = M4C
training's (B, 1, S, S) mask (key row + causal corner of the 12 decoding positions: the per-query-mask form), "prefix" =
the same mask given as the key row + tail 12 (ovqa_attention_fwd_prefix_lm_train / ovqa_attention_bwd_prefix_lm: the
key-row form with the corner computed; there is no VALU form); the torch yardsticks run without a mask.  Each time is
the median of the windows, ``*_us_range`` their minimum and maximum.  Prints one JSON line per shape.
  python scripts/long_attention_bench.py [--only m4c_train,s182,s232] [--no-yardsticks] [--out profiles/long_attention_bench.jsonl]"""
import argparse
import json
import math
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BF16 = 2.5e15
# (name, B, H, d, nq, nk, dropout, mask)
SHAPES = [
    ("self_577_d64_key", 64, 8, 64, 577, 577, 0.0, "key"),
    ("guided_577x20_d64_key", 64, 8, 64, 577, 20, 0.0, "key"),
    ("s232_d96_drop_key", 64, 8, 96, 232, 232, 0.1, "key"),
    ("m4c_train_232_d96_drop_dense", 64, 8, 96, 232, 232, 0.1, "dense"),
    ("m4c_train_232_d96_drop_prefix", 64, 8, 96, 232, 232, 0.1, "prefix"),
    ("s182_d96_drop_key", 64, 8, 96, 182, 182, 0.1, "key"),
    ("m4c_train_182_d96_drop_dense", 64, 8, 96, 182, 182, 0.1, "dense"),
    ("m4c_train_182_d96_drop_prefix", 64, 8, 96, 182, 182, 0.1, "prefix"),
    ("self_1024_d128_key", 64, 8, 128, 1024, 1024, 0.0, "key"),
    ("self_300_d64_key", 64, 8, 64, 300, 300, 0.0, "key"),
]


def timed(fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    RANGES.append((min(out), max(out)))
    return sorted(out)[len(out) // 2]


RANGES = []  # (min, max) of the windows of every timed() call, in call order
TAIL = 12


def ours(B, H, d, nq, nk, p, mk, warmup, iters, reps, res=None):
    """(fwd us, bwd us, fwd route, bwd route); with ``res`` (a dict) the forward's numbers land there before the backward
    runs, so a backward the kernels refuse still leaves the forward timed."""
    from openvivqa_amd import _lib, ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, nq, H * d, device=dev, generator=g).bfloat16()
    k = torch.randn(B, nk, H * d, device=dev, generator=g).bfloat16()
    v = torch.randn(B, nk, H * d, device=dev, generator=g).bfloat16()
    mask = torch.zeros(B, 1, 1, nk, device=dev)
    mask[1::2, ..., nk - nk // 8:] = -1e5
    if mk == "dense":
        mask = mask.repeat(1, 1, nq, 1)
        mask[:, :, -TAIL:, -TAIL:] += torch.full((TAIL, TAIL), float("-inf"), device=dev).triu(1)
    drop = ops.DropSpec(p=p, seed=1, site=1, step=torch.zeros(1, dtype=torch.int32, device=dev)) if p > 0 else None
    lo = []
    if mk == "prefix":
        def fwd(lo_out):
            return ops.attention_fwd_prefix_lm_train(q, k, v, mask, TAIL, H, att_drop=drop, lo_out=lo_out)

        def bwd():
            return ops.attention_bwd_prefix_lm(d_o, q, k, v, o, lse, mask, TAIL, H, dq=dq, dk=dk, dv=dv, att_drop=drop,
                                               o_lo=lo[0])
    else:
        def fwd(lo_out):
            return ops.attention_fwd(q, k, v, mask, H, att_drop=drop, lo_out=lo_out)

        def bwd():
            return ops.attention_bwd(d_o, q, k, v, o, lse, mask, H, dq=dq, dk=dk, dv=dv, att_drop=drop, o_lo=lo[0])
    o, lse = fwd(lo)[:2]
    fwd_route = _lib.last_dispatch()
    tf = timed(lambda: fwd([]), warmup, iters, reps)
    if res is not None:
        res.update(fwd_us=tf, fwd_route=fwd_route)
    d_o = torch.randn_like(q)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    bwd()
    bwd_route = _lib.last_dispatch()
    tb = timed(bwd, warmup, iters, reps)
    return tf, tb, fwd_route, bwd_route


def torch_forms(B, H, d, nq, nk, p, warmup, iters, reps):
    import torch.nn.functional as F
    dev = "cuda"
    q = torch.randn(B, H, nq, d, device=dev, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, H, nk, d, device=dev, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, H, nk, d, device=dev, dtype=torch.bfloat16, requires_grad=True)
    scale = 1.0 / math.sqrt(d)

    def unfused():
        s = torch.matmul(q, k.transpose(-1, -2)) * scale
        a = torch.softmax(s, -1)
        if p > 0:
            a = F.dropout(a, p)
        return torch.matmul(a, v)

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, dropout_p=p)
    res = {}
    for name, fn in (("unfused", unfused), ("sdpa", sdpa)):
        try:
            res[name + "_fwd_us"] = timed(lambda: fn(), warmup, iters, reps)
            out = fn()
            g = torch.randn_like(out)
            t_all = timed(lambda: torch.autograd.grad(fn(), (q, k, v), g), warmup, iters, reps)
            res[name + "_bwd_us"] = t_all - res[name + "_fwd_us"]
        except Exception as e:  # (a form torch does not run for this shape is reported, not skipped silently)
            res[name + "_error"] = f"{type(e).__name__}: {e}"[:200]
    return res


def valu_child(args):
    env = dict(os.environ, OVQA_FORCE_SIMPLE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--valu-only", "--warmup", str(args.warmup),
                        "--iters", str(args.iters), "--reps", str(args.reps)] + (["--only", args.only] if args.only else []),
                       env=env, capture_output=True, text=True, timeout=600)
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            j = json.loads(line)
            out[j["shape"]] = j
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--valu-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated substrings: the shapes whose name holds one of them")
    ap.add_argument("--no-yardsticks", action="store_true", help="skip the VALU child and the torch forms")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    if args.only:
        SHAPES[:] = [r for r in SHAPES if any(x in r[0] for x in args.only.split(","))]
    if args.valu_only:
        for name, B, H, d, nq, nk, p, mk in SHAPES:
            res = {}
            row = {"shape": name}
            try:
                tf, tb, fr, br = ours(B, H, d, nq, nk, p, mk, args.warmup, args.iters, args.reps, res)
                row.update(valu_fwd_us=tf, valu_bwd_us=tb, valu_routes=[fr, br])
            except Exception as e:
                if "fwd_us" in res:
                    row.update(valu_fwd_us=res["fwd_us"], valu_routes=[res["fwd_route"]])
                row["valu_error"] = f"{type(e).__name__}: {e}"[:200]
            print(json.dumps(row), flush=True)
        return
    valu = {} if args.no_yardsticks else valu_child(args)
    lines = []
    for name, B, H, d, nq, nk, p, mk in SHAPES:
        del RANGES[:]
        tf, tb, fr, br = ours(B, H, d, nq, nk, p, mk, args.warmup, args.iters, args.reps)
        (f_lo, f_hi), (b_lo, b_hi) = RANGES[0], RANGES[1]
        ff, fb = 4.0 * B * H * nq * nk * d, 8.0 * B * H * nq * nk * d
        row = {"shape": name, "B": B, "H": H, "d": d, "nq": nq, "nk": nk, "dropout": p, "mask": mk, "routes": [fr, br],
               "timing": "per call (device events around Python-level calls)",
               "fwd_us_per_call": round(tf, 2), "bwd_us_per_call": round(tb, 2),
               "fwd_us_range": [round(f_lo, 2), round(f_hi, 2)], "bwd_us_range": [round(b_lo, 2), round(b_hi, 2)],
               "fwd_tflops_per_call": round(ff / tf / 1e6, 1), "bwd_tflops_per_call": round(fb / tb / 1e6, 1),
               "fwd_per_call_frac_peak": round(ff / (tf * 1e-6) / PEAK_BF16, 4),
               "bwd_per_call_frac_peak": round(fb / (tb * 1e-6) / PEAK_BF16, 4)}
        row.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in valu.get(name, {}).items() if k != "shape"})
        if not args.no_yardsticks:
            row.update({k: (round(v, 2) if isinstance(v, float) else v)
                        for k, v in torch_forms(B, H, d, nq, nk, p, args.warmup, args.iters, args.reps).items()})
        if "valu_fwd_us" in row:
            row["speedup_fwd_vs_valu"] = round(row["valu_fwd_us"] / tf, 2)
        if "valu_bwd_us" in row:
            row["speedup_bwd_vs_valu"] = round(row["valu_bwd_us"] / tb, 2)
        if "unfused_fwd_us" in row and "unfused_bwd_us" in row:
            row["speedup_fwdbwd_vs_unfused"] = round((row["unfused_fwd_us"] + row["unfused_bwd_us"]) / (tf + tb), 2)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
