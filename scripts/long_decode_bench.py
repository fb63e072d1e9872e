"""Single-query decode attention over long key lists on the MI355X (csrc/attention_decode.hip).

  --kernel   ``ops.attention_decode`` alone: n in {237, 512, 577, 617, 1024, 2048} x B in {1, 8, 64} x beam in {1, 3, 5},
             H = 8, d = 64, bf16, a key-padding mask row per query.  ``--calls`` launches are captured into one hipGraph
             (rotating over ``--sets`` K / V cache sets, so that B = 64 does not replay out of the 256 MB last-level
             cache); the graph is replayed ``--iters`` times between device events, median of ``--reps`` windows ->
             microseconds per launch.  Bytes: the K and V rows of every sample once (beams share them when the kernel does,
             ``--ungrouped`` times the same queries with a cache row per beam instead, bytes still counted once per sample)
             plus the mask rows; share of the 8 TB/s HBM figure that bench.py's ``roofline_decode`` uses.
  --decoder  the ``decode`` workload's model (Decoder L = 3, d_model 512, H = 8, dff 2048, 4000 words, T = 20) over
             ``--positions`` encoder positions (617 = 577 ViT patches + 40 question tokens), B = 64, beams 1, 3 and 5, the
             whole decode replayed from one hipGraph: tokens/s and ms per decode.

``--splits 1 auto 8 --rounds 3``: the key split across workgroups (``ovqa_attention_decode_split``) against the unsplit call,
both in this build, alternated round by round in one process; a row per value with the range of its rounds' medians.

``--tree DIR`` imports the package from another checkout (with its own built library), e.g. the parent commit, so that
both sides of a comparison are measured by the same script, alternated on one box.  One JSON line per row.
  python scripts/long_decode_bench.py --kernel [--out profiles/r09_long_decode_bench.jsonl]
  python scripts/long_decode_bench.py --decoder --tree ../parent_checkout --tag parent"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

PEAK_HBM = 8.0e12
KERNEL_N = [237, 512, 577, 617, 1024, 2048]
KERNEL_B = [1, 8, 64]
BEAMS = [1, 3, 5]


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def kernel_row(ops, n, B, beam, H, d, a):
    """One row per value of ``--splits``.  Several values are ALTERNATED in this process: every round times each value's
    graph in turn (``--reps`` windows, their median), ``--rounds`` rounds; a row reports the median of its rounds' medians
    and their range, the spread a difference between two values has to beat."""
    dev, F = "cuda", H * d
    g = torch.Generator(device=dev).manual_seed(0)
    R = B * beam
    q = torch.randn(R, 1, F, device=dev, generator=g).bfloat16()
    rows_kv, group = (R, 1) if a.ungrouped else (B, beam)  # --ungrouped: a cache row per beam, every row reads for itself
    sets = [(torch.randn(rows_kv, n, F, device=dev, generator=g).bfloat16(),
             torch.randn(rows_kv, n, F, device=dev, generator=g).bfloat16()) for _ in range(a.sets)]
    mask = torch.zeros(R, n, device=dev)
    mask[:, n - n // 8:] = -1e5
    out = torch.empty_like(q)
    graphs, info = [], []
    for sp in a.splits:
        kw, row = {}, {}
        if sp != "1":  # (splits = 1 is the call without the keyword: a tree from before the split can run it)
            splits = 0 if sp == "auto" else int(sp)
            kw = {"splits": splits, "workspace": torch.empty(max(16, ops.decode_split_workspace_bytes(R, H, n, d, splits)),
                                                             dtype=torch.uint8, device=dev)}
            if splits == 0:
                from openvivqa_amd import _lib
                splits = int(_lib.load().ovqa_attention_decode_auto_splits(R, H, group, n, d, 1))
            row = {"splits": sp, "splits_used": splits, "slices": ops.decode_split_slices(n, splits)}
        elif len(a.splits) > 1:
            row = {"splits": "1", "splits_used": 1, "slices": 1}

        def calls(kw=kw):
            for i in range(a.calls):
                k, v = sets[i % a.sets]
                ops.attention_decode(q, k, v, n, H, mask=mask, group=group, out=out, **kw)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            calls()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            calls()
        for _ in range(a.warmup):
            graph.replay()
        torch.cuda.synchronize()
        graphs.append(graph)
        info.append(row)
    rounds = [[] for _ in a.splits]
    for _ in range(a.rounds):
        for i, graph in enumerate(graphs):
            us = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / (a.iters * a.calls))
            us.sort()
            rounds[i].append(us)
    kv_bytes = B * n * F * 2 * 2  # K and V of every sample once, bf16
    nbytes = kv_bytes + R * n * 4
    rows = []
    for row, rs in zip(info, rounds):
        meds = sorted(us[len(us) // 2] for us in rs)
        med = statistics.median(meds)
        row.update({"us_per_launch": round(med, 2), "us_min": round(min(us[0] for us in rs), 2),
                    "us_max": round(max(us[-1] for us in rs), 2), "bytes": nbytes,
                    "frac_of_hbm_peak": round(nbytes / (med * 1e-6) / PEAK_HBM, 4)})
        if a.rounds > 1:
            row.update({"rounds": a.rounds, "round_medians_us": [round(m, 2) for m in meds]})
        rows.append(row)
    return rows


def run_kernel(a):
    from openvivqa_amd import ops
    for n in (a.n or KERNEL_N):
        for B in (a.batch or KERNEL_B):
            for beam in (a.beam or BEAMS):
                base = {"mode": "kernel", "tag": a.tag, "n": n, "B": B, "beam": beam, "H": 8, "d": 64, "dtype": "bf16",
                        "ungrouped": bool(a.ungrouped)}
                try:
                    rows = kernel_row(ops, n, B, beam, 8, 64, a)
                except RuntimeError as exc:  # (a library that refuses the shape: the row says so)
                    rows = [{"error": str(exc)[:160]}]
                for row in rows:
                    emit(dict(base, **row), a.out)


def run_decoder(a):
    import openvivqa_amd as A
    from openvivqa_amd.beam import GraphedBeamSearch
    from openvivqa_amd.config import ConfigNode, attention_config
    from openvivqa_amd.utils import generate_padding_mask
    T, NE, V, L, D, B = 20, a.positions, 4000, 3, 512, 64
    dev = "cuda"

    class Vocab:
        max_answer_length, padding_idx, bos_idx, eos_idx = T, 0, 1, 2

        def __len__(self):
            return V
    cfg = ConfigNode(dict(
        ARCHITECTURE="Decoder", D_MODEL=D, LAYERS=L,
        ATTENTION=dict(SELF_ATTENTION=attention_config(can_be_stateful=True), ENC_ATTENTION=attention_config()),
        TEXT_EMBEDDING=dict(ARCHITECTURE="UsualEmbedding", D_MODEL=D, D_EMBEDDING=300, WORD_EMBEDDING=None,
                            WORD_EMBEDDING_CACHE=None, DROPOUT=0.1)))
    A.set_compute_dtype(torch.bfloat16)
    for beam in (a.beam or BEAMS):
        torch.manual_seed(0)
        dec = A.build_decoder(cfg, Vocab()).to(dev).eval()
        g = torch.Generator().manual_seed(0)
        enc = torch.randn(B, NE, D, generator=g)
        ne = torch.randint(NE - 37, NE + 1, (B,), generator=g)
        enc[torch.arange(NE)[None, :] >= ne[:, None]] = 0
        enc = enc.to(dev)
        emask = generate_padding_mask(enc, 0)
        search = GraphedBeamSearch(dec, B, T, 1, -1, beam)  # eos unreachable: every batch costs the same
        row = {"mode": "decoder", "tag": a.tag, "positions": NE, "B": B, "beam": beam, "T": T, "dtype": "bf16"}
        try:
            for _ in range(max(1, a.warmup)):
                search(enc, emask)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    tokens, logp = search(enc, emask)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            med = statistics.median(ms)
            row.update({"ms_per_decode": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                        "tokens_per_s": round(B * T / (med * 1e-3), 1),
                        "checksum": round(float(logp.double().sum()), 4)})
        except RuntimeError as exc:
            row["error"] = str(exc)[:160]
        emit(row, a.out)
        del search, dec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--decoder", action="store_true")
    ap.add_argument("--tree", default=None, help="checkout to import openvivqa_amd from (default: this one)")
    ap.add_argument("--tag", default="change")
    ap.add_argument("--out", default=None)
    ap.add_argument("--positions", type=int, default=617)
    ap.add_argument("--n", type=int, nargs="*")
    ap.add_argument("--batch", type=int, nargs="*")
    ap.add_argument("--beam", type=int, nargs="*")
    ap.add_argument("--ungrouped", action="store_true",
                    help="--kernel: group = 1 on caches gathered per beam (the route of a group without a shared form)")
    ap.add_argument("--splits", nargs="*", default=["1"],
                    help="--kernel: 1 (the unsplit call), auto (the library's rule) or N slices of the keys across "
                         "workgroups; several values are alternated in one process")
    ap.add_argument("--rounds", type=int, default=1, help="--kernel: alternated rounds per value of --splits")
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not (a.kernel or a.decoder):
        ap.error("one of --kernel / --decoder")
    if a.kernel:
        run_kernel(a)
    if a.decoder:
        run_decoder(a)


if __name__ == "__main__":
    main()
