"""Development probe: where a workgroup of the fused dW + Adam launch spends its time, in the benchmark's own step.

The library must have been built with -DOVQA_PHASE_PROBE (OVQA_EXTRA_HIPCC_FLAGS); this script does not build.  It runs a
few replayed steps of bench.py's headline workload and reads the stamps gemm_bf16_grouped_wgrad_adam_kernel left for every
workgroup of the LAST launch: start, K loop done, state loads issued, last state store issued, end, and the CU it ran on.

Printed: the phases per fused workgroup (percentiles), the share of the workgroups' own time spent in tails, and -- per CU,
where two workgroups are resident -- how a tail's time splits by what its neighbour is doing meanwhile: K loop (the tail's
HBM traffic is hidden behind MFMA work), a tail of its own ("tails in rounds"), or nothing (the CU's other slot is empty).
"""
import collections
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OVQA_NO_BUILD", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from openvivqa_amd import _lib  # noqa: E402


def pct(a, qs=(0, 10, 50, 90, 100)):
    return " ".join(f"{np.percentile(a, q):8.2f}" for q in qs)


def overlap(lo, hi, a, b):
    return max(0.0, min(hi, b) - max(lo, a))


def main():
    sys.argv = [sys.argv[0], "--no-cpu-baseline", "--no-roofline", "--no-secondary", "--repeats", "1"]
    args = bench.parse()
    lib = _lib.load()
    if not hasattr(lib, "ovqa_debug_probe_wgrad_adam"):
        raise SystemExit("the library was not built with -DOVQA_PHASE_PROBE")
    lib.ovqa_debug_probe_wgrad_adam.argtypes = [C.c_void_p, C.c_int]
    torch.cuda.set_device(0)
    out, ts, cfg = bench.train_bench(args, "stack", torch.device("cuda", 0), 1, 0, None, torch.bfloat16, steps=5, warmup=3,
                                     repeats=1)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * (8 * 4096))()
    assert lib.ovqa_debug_probe_wgrad_adam(buf, 4096) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(4096, 8).copy()
    ran = a[:, 0] > 0
    last = a[ran, 0].max()
    ran &= a[:, 0] > last - np.uint64(100 * 5000)  # the last launch only (stamps are 100 MHz ticks; a launch is < 5 ms)
    fused = ran & (a[:, 4] > 0) & (a[:, 4] >= a[:, 0])
    print(f"ms_per_step (probe build, not a timing) {out['ms_per_step']}; workgroups that ran {int(ran.sum())}, fused {int(fused.sum())}")
    f = a[fused]
    t0 = int(f[:, 0].min())
    st, kd, ld, ls, en = [(f[:, i].astype(np.int64) - t0) / 100.0 for i in range(5)]
    hw = f[:, 5]
    cu = ((hw >> np.uint64(32)) & np.uint64(0xF)).astype(np.int64) * 1000 + ((hw >> np.uint64(13)) & np.uint64(7)).astype(np.int64) * 100 + \
        ((hw >> np.uint64(12)) & np.uint64(1)).astype(np.int64) * 50 + ((hw >> np.uint64(8)) & np.uint64(15)).astype(np.int64)
    print(f"launch span (first start -> last end of a fused workgroup) {en.max():.1f} us on {len(set(cu.tolist()))} CUs")
    print("phase (us)                          p0      p10      p50      p90     p100")
    print(f"K loop   (start -> K done)     {pct(kd - st)}")
    print(f"dump     (K done -> loads out) {pct(ld - kd)}")
    print(f"update   (loads out -> stores) {pct(ls - ld)}")
    print(f"gather   (stores out -> end)   {pct(en - ls)}")
    print(f"tail     (K done -> end)       {pct(en - kd)}")
    own, tail = (en - st).sum(), (en - kd).sum()
    print(f"share of the fused workgroups' own time spent in tails: {tail / own:.3f} ({tail / len(f):.2f} of {own / len(f):.2f} us per workgroup)")
    by_cu = collections.defaultdict(list)
    for i, c in enumerate(cu.tolist()):
        by_cu[c].append(i)
    in_k = in_tail = 0.0
    for idx in by_cu.values():
        for i in idx:
            for j in idx:
                if i != j:
                    in_k += overlap(kd[i], en[i], st[j], kd[j])
                    in_tail += overlap(kd[i], en[i], kd[j], en[j])
    print(f"of the tails' time, the CU's other workgroup is in its K loop {in_k / tail:.3f}, in a tail of its own "
          f"{in_tail / tail:.3f}, absent or unfused {max(0.0, 1 - (in_k + in_tail) / tail):.3f}")


if __name__ == "__main__":
    main()
