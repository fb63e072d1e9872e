"""CPU-side checks of the drop-in boundary and host logic (no kernel launches).

* the registry / factory surface behaves like the reference's;
* the reference's YAML configs load verbatim and build the same state_dict;
* libovqa_hip.so loads and exports every symbol include/ovqa_hip.h declares;
* the product path fails loudly without a GPU (no CPU fallback);
* the data-parallel exchange works over gloo with world_size 2.
"""
import json
import os
import re
import socket

import pytest
import torch

import openvivqa_amd as A
from openvivqa_amd import _lib
from openvivqa_amd.builders import Registry
from openvivqa_amd.config import ConfigNode, attention_config, get_config
from golden_cases import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_registry_semantics():
    reg = Registry("DEMO")

    @reg.register()
    class Foo:
        pass

    class Bar:
        pass
    reg.register(Bar)
    assert reg.get("Foo") is Foo and reg.get("Bar") is Bar and "Foo" in reg and len(reg) == 2
    with pytest.raises(KeyError, match="No object named 'Nope' found in 'DEMO' registry!"):
        reg.get("Nope")
    with pytest.raises(AssertionError, match="already registered"):
        reg.register(Foo)
    assert dict(iter(reg))["Bar"] is Bar and "DEMO" in repr(reg)


def test_registered_names_match_reference():
    assert {"ScaledDotProductAttention"} <= {k for k, _ in A.META_ATTENTION}
    assert {"Encoder", "GuidedAttentionEncoder", "CoAttentionEncoder", "CrossModalityEncoder"} == \
        {k for k, _ in A.META_ENCODER}
    assert {"Decoder"} == {k for k, _ in A.META_DECODER}
    assert A.META_ENCODER._name == "ENCODER_LAYER" and A.META_DECODER._name == "DECODER_LAYER"
    with pytest.raises(KeyError):
        A.build_encoder(ConfigNode(dict(ARCHITECTURE="NoSuchEncoder")))


def test_config_node_access():
    c = ConfigNode({"A": {"B": 1, "C": [{"D": 2}]}, "E": None})
    assert c.A.B == 1 and c.A.C[0].D == 2 and c.E is None and c["A"]["B"] == 1
    with pytest.raises(AttributeError):
        c.missing
    c2 = c.clone()
    c2.A.B = 5
    assert c.A.B == 1
    cfg = get_config(os.path.join(ROOT, "configs", "mcan_bench.yaml"))
    assert cfg.MODEL.SELF_ENCODER.LAYERS == 6 and cfg.MODEL.GUIDED_ENCODER.GUIDED_ATTENTION.DROPOUT == 0.1
    assert cfg.MODEL.SELF_ENCODER.SELF_ATTENTION.USE_AOA is False


def _reference_config(name):
    """MODEL node of one of the reference's BASELINE configs, exactly as its YAML file parses (G18: the parsed trees,
    stored as JSON -- itself YAML -- by tests/golden/make_golden.py:g18), read through ``get_config``."""
    return get_config(os.path.join(GOLDEN, "G18_reference_configs.json"))[name]


def test_reference_yamls_load_verbatim():
    """The five BASELINE configs are consumed as they are (yacs replaced by ConfigNode)."""
    with open(os.path.join(GOLDEN, "G10_state_dict_manifest.json")) as f:
        man = json.load(f)
    mcan = _reference_config("mcan").MODEL
    enc = A.build_encoder(mcan.SELF_ENCODER)
    genc = A.build_encoder(mcan.GUIDED_ENCODER)
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == man["Encoder"]
    assert {k: list(v.shape) for k, v in genc.state_dict().items()} == man["GuidedAttentionEncoder"]
    cmt = _reference_config("cross_modality_transformer").MODEL
    cm = A.build_encoder(cmt.ENCODER)
    assert {k: list(v.shape) for k, v in cm.state_dict().items()} == man["CrossModalityEncoder"]
    gen = _reference_config("vit_mbert_generation").MODEL

    class Vocab:
        max_answer_length, padding_idx = 20, 0

        def __len__(self):
            return 100
    dec = A.build_decoder(gen.DECODER, Vocab())
    assert dec.fc.weight.shape == (100, 512) and len(dec.layers) == gen.DECODER.LAYERS
    for name in ("mmf_m4c", "saaa"):
        assert "MODEL" in _reference_config(name)
    # the whole MCAN model resolves through build_model from the unmodified YAML (only DEVICE is overridden)
    mcan_model_cfg = _reference_config("mcan").MODEL
    mcan_model_cfg["DEVICE"] = "cpu"

    class ClsVocab:
        padding_idx, total_answers = 0, 353

        def __len__(self):
            return 4000
    model = A.build_model(mcan_model_cfg, ClsVocab())
    keys = set(model.state_dict())
    golden = set(load_case("G12_mcan_model").w)  # the reference model's own state_dict keys (L=2 there, 3 here)
    assert {k for k in keys if ".2." not in k} == golden
    assert model.classify.weight.shape == (353, 512) and model.vision_embedding.proj.weight.shape == (512, 1024)


def test_product_state_dicts_match_manifest():
    with open(os.path.join(GOLDEN, "G10_state_dict_manifest.json")) as f:
        man = json.load(f)
    import openvivqa_amd.modules as M
    sa = attention_config()
    cm = ConfigNode(dict(D_MODEL=512, LAYERS=3, VISION_LANGUAGE_ATTENTION=sa, LANGUAGE_VISION_ATTENTION=sa,
                         VISION_SELF_ATTENTION=sa, LANGUAGE_SELF_ATTENTION=sa))
    built = {
        "CoAttentionEncoder": M.CoAttentionEncoder(cm),
        "CrossModalityEncoder": M.CrossModalityEncoder(cm),
        "OcrPtrNet_768": M.OcrPtrNet(768),
        "MultiHeadAttention_aoa_stateful": M.MultiHeadAttention(attention_config(use_aoa=True, can_be_stateful=True)),
    }
    for name, mod in built.items():
        assert {k: list(v.shape) for k, v in mod.state_dict().items()} == man[name], name

    class Vocab:
        max_answer_length, padding_idx = 6, 0

        def __len__(self):
            return 11
    small = attention_config(d_model=32, head=4, d_key=8, d_value=8, d_ff=64)
    dcfg = ConfigNode(dict(ARCHITECTURE="Decoder", D_MODEL=32, LAYERS=3,
                           ATTENTION=dict(SELF_ATTENTION=attention_config(d_model=32, head=4, d_key=8, d_value=8, d_ff=64,
                                                                          can_be_stateful=True), ENC_ATTENTION=small),
                           TEXT_EMBEDDING=dict(ARCHITECTURE="UsualEmbedding", D_MODEL=32, D_EMBEDDING=16,
                                               WORD_EMBEDDING=None, WORD_EMBEDDING_CACHE=None, DROPOUT=0.1)))
    dec = A.build_decoder(dcfg, Vocab())
    assert {k: list(v.shape) for k, v in dec.state_dict().items()} == man["Decoder_D32_V11"]


def test_xavier_zero_bias_init():
    import openvivqa_amd.modules as M
    torch.manual_seed(0)
    m = M.ScaledDotProductAttention(attention_config())
    bound = (6.0 / (512 + 512)) ** 0.5
    for lin in (m.fc_q, m.fc_k, m.fc_v, m.fc_o):
        assert float(lin.bias.abs().max()) == 0.0
        assert float(lin.weight.abs().max()) <= bound + 1e-6 and float(lin.weight.std()) > 0.5 * bound / 3 ** 0.5


def test_library_exports_every_header_symbol():
    hdr = open(os.path.join(ROOT, "include", "ovqa_hip.h")).read()
    declared = set(re.findall(r"\b(ovqa_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"ovqa_dropout", "ovqa_status", "ovqa_dtype", "ovqa_epilogue"}
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    lib = _lib.load()  # raises if a symbol is missing; no kernel is launched
    assert lib.ovqa_abi_version() == _lib.ABI_VERSION
    assert lib.ovqa_workspace_bytes() >= (1 << 20)
    assert re.search(r"attentions\.py:\d+", hdr) and re.search(r"mmf_m4c\.py:\d+", hdr)  # citations present


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load(str(tmp_path / "nope.so"))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_forward_without_gpu_raises():
    import openvivqa_amd.modules as M
    m = M.PositionWiseFeedForward(attention_config(d_model=32, d_ff=64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 32))
    from openvivqa_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_fwd(torch.zeros(4, 8), torch.zeros(4, 8))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "openvivqa_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M), f"{f} imports the oracle"


def test_noam_schedule_matches_reference_formula():
    from openvivqa_amd.train import noam_lr_scale
    import oracle as O
    for s in (0, 1, 10, 9999, 10000, 50000):
        assert noam_lr_scale(s, 512, 10000) == O.noam_lambda(s, 512, 10000)
    assert abs(noam_lr_scale(0, 512, 10000) - 512 ** -0.5 * 10000 ** -1.5) < 1e-15


def test_sinusoid_table_matches_golden():
    from golden_cases import load_case
    from openvivqa_amd.modules.pos_embeddings import SinusoidPositionalEmbedding
    from openvivqa_amd.utils import (generate_padding_mask, generate_self_attention_masks, generate_sequential_mask,
                                     sinusoid_encoding_table)
    c = load_case("G6_pos_masks")
    pe = SinusoidPositionalEmbedding(8)(torch.zeros(2, 3, 8))
    assert pe.shape == (2, 3, 8) and torch.equal(pe[0], c.out["sinusoid_3_8"])
    big = SinusoidPositionalEmbedding(512)(torch.zeros(1, 100, 512))[0]
    assert torch.equal(big[::33, ::37], c.out["sinusoid_100_512"])
    assert torch.equal(sinusoid_encoding_table(6, 8, 0), c.out["table_6_8_pad0"])
    pm = generate_padding_mask(c.inputs["tokens"], 0)
    assert torch.equal(pm, c.out["padmask_tokens"])
    assert torch.equal(generate_padding_mask(c.inputs["feats"], 0), c.out["padmask_feats"])
    sm = generate_sequential_mask(5)
    assert torch.equal(sm, c.out["seqmask_5"])
    assert torch.equal(generate_self_attention_masks(pm, sm), c.out["selfmask"])


# ------------------------------------------------------------------ data-parallel exchange over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, rdv, comm_bf16, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + rdv, rank=rank, world_size=world)
    try:
        from openvivqa_amd.train import GradAllReducer
        n = 1000
        red = GradAllReducer(n, "cpu", torch.bfloat16 if comm_bf16 else torch.float32, bucket_mb=0.001)
        assert red.world == world and len(red.bounds(n)) > 1  # several buckets
        g = torch.arange(n, dtype=torch.float32) * (rank + 1) / 64.0
        g[100:200] = 0.0  # parameters without gradient (dead cross-attention): zeros on every rank
        out = red(g)
        q.put((rank, out.clone().numpy()))  # by value: a shared-memory tensor could outlive its sender
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("comm_bf16", [False, True])
def test_grad_allreduce_gloo_world2(comm_bf16):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    import tempfile
    rdv = os.path.join(tempfile.mkdtemp(prefix="ovqa_rdv_"), "store")
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, rdv, comm_bf16, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: torch.from_numpy(a) for r, a in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    base = torch.arange(1000, dtype=torch.float32) / 64.0
    expect = base * 3.0
    expect[100:200] = 0.0
    tol = 0.0 if not comm_bf16 else 2e-2
    for r in (0, 1):
        err = ((res[r] - expect).abs() / expect.abs().clamp_min(1.0)).max().item()
        assert err <= tol, err
    assert torch.equal(res[0], res[1])  # every rank ends with identical gradients


def _run_dp(world, overlap_mb, comm_bf16, kind, shard):
    import tempfile
    import torch.multiprocessing as mp
    import dp_helpers as H
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    rdv = os.path.join(tempfile.mkdtemp(prefix="ovqa_rdv_"), "store")
    procs = [ctx.Process(target=H.dp_worker, args=(r, world, rdv, overlap_mb, comm_bf16, q, kind, shard)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (torch.from_numpy(w), seg, torch.from_numpy(m), own) for r, w, seg, m, own in (q.get(timeout=300) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("overlap_mb,comm_bf16,kind,world", [
    (0.0, False, "mcan", 2), (0.02, False, "mcan", 2), (0.02, True, "mcan", 2), (0.02, False, "crossmodality", 2),
    (0.02, False, "mcan", 8)])
def test_sharded_optimizer_equals_replicated_bitwise(overlap_mb, comm_bf16, kind, world):
    """Round 6: with the optimiser SHARDED over the ranks -- gradients of the weight matrices
    reduce-scattered, Adam on the owned chunk of every exchanged bucket, the weights all-gathered -- every rank ends with
    the same weights and (after ``state_dict()``'s gather) the same moments as with the replicated optimiser, bit for bit
    (gloo has no reduce-scatter on CPU tensors: it is emulated by all-reduce + the rank's own slice, so the gradient sums
    are the same sums), and the ranks' owned ranges partition the matrix part of the arena."""
    rep = _run_dp(world, overlap_mb, comm_bf16, kind, False)
    sh = _run_dp(world, overlap_mb, comm_bf16, kind, True)
    assert rep[0][1] == sh[0][1]  # the same segment plan
    for r in range(world):
        assert torch.equal(sh[r][0], rep[0][0]), r
        assert torch.equal(sh[r][2], rep[0][2]), r
        assert rep[r][3] is None
    spans = sorted(tuple(x) for r in range(world) for x in sh[r][3])
    # chunks of the sharded part are disjoint; the replicated tail is listed by every rank
    numel = rep[0][0].numel()
    cover = torch.zeros(numel, dtype=torch.int32)
    for lo, hi in spans:
        cover[lo:hi] += 1
    first_tail = int((cover == world).nonzero()[0]) if (cover == world).any() else numel
    assert bool((cover[:first_tail] == 1).all()) and bool((cover[first_tail:] == world).all()), (first_tail, numel)
    assert first_tail > numel // 2  # (the weight matrices are the bulk of the arena)


@pytest.mark.parametrize("overlap_mb,comm_bf16,kind,world", [
    (0.0, False, "mcan", 2), (0.02, False, "mcan", 2), (0.02, True, "mcan", 2), (0.02, False, "crossmodality", 2),
    (0.02, False, "mcan", 8)])  # 8 ranks: the node size the driver scales to
def test_train_step_dp_gloo_world2_phased_backward(overlap_mb, comm_bf16, kind, world):
    """N ranks x TrainStep on a small MCAN stack (kernel wrappers mocked, gloo): with the gradient exchange
    released segment by segment during a phased backward (overlap_mb > 0) all ranks end with identical weights,
    equal to a single process that averages the ranks' gradients itself; the segment plan is identical on every
    rank (TrainStep._check_plan_identical runs inside)."""
    import dp_helpers as H
    res = _run_dp(world, overlap_mb, comm_bf16, kind, None)  # (the default: the sharded optimiser from two ranks on)
    for r in range(1, world):
        assert torch.equal(res[0][0], res[r][0])
        assert res[0][1] == res[r][1]
    segs = res[0][1]
    if overlap_mb > 0:
        assert len(segs) >= 3, segs  # several segments were released before the end of backward
    flat = sorted(tuple(r) for s in segs for r in s)
    assert flat[0][0] == 0 and all(a[1] == b[0] for a, b in zip(flat, flat[1:]))  # a partition of the buffer
    # single-process reference: same model/seed, gradients of the two batches averaged by hand
    import mock_ops, openvivqa_amd.train as tr, openvivqa_amd.functional as Fn, openvivqa_amd.runtime as rt
    saved = (tr.ops, Fn.ops, rt.ops, rt.build_arena, rt.step_tensor)
    try:
        H.patch_cpu_ops()
        model, ts = H.make_step(0.0, kind=kind)
        assert flat[-1][1] == ts.arena.numel
        ts.static_inputs = [t.clone() for t in H.batch(0)]
        ts._discover_foreign()
        for _ in range(2):
            g = torch.zeros_like(ts.arena.grad)
            for r in range(world):
                ts.static_inputs = [t.clone() for t in H.batch(r)]
                ts._fwd_bwd()
                g += ts.arena.grad
            ts.optim.step(g, grad_scale=1.0 / world)
        ref = ts.arena.master.clone()
        keep = torch.ones_like(ref, dtype=torch.bool)
        for n, prm in model.named_parameters():  # analytically zero gradient: Adam turns rounding noise into
            if n.endswith("fc_k.bias"):         # +-lr steps, not comparable
                o = ts.arena.offsets[id(prm)]
                keep[o:o + prm.numel()] = False
    finally:
        tr.ops, Fn.ops, rt.ops, rt.build_arena, rt.step_tensor = saved
        import openvivqa_amd as A
        A.set_compute_dtype(torch.bfloat16)
    tol = 1e-5 if not comm_bf16 else 2e-2
    err = ((res[0][0] - ref).abs() * keep).max().item()
    assert err <= tol, err


def test_segment_helpers():
    """Range bookkeeping of the overlapped gradient exchange (train._merge / _complement / _reaches)."""
    from openvivqa_amd.train import _complement, _merge, _reaches
    assert _merge([(10, 20), (0, 5), (5, 10), (30, 40)]) == [(0, 20), (30, 40)]
    assert _merge([(0, 4), (6, 8)], gap=2) == [(0, 8)]
    assert _complement([(10, 20), (30, 40)], 0, 50) == [(0, 10), (20, 30), (40, 50)]
    assert _complement([], 0, 7) == [(0, 7)] and _complement([(0, 7)], 0, 7) == []
    a = torch.randn(3, requires_grad=True)
    b = (a * 2).sin()
    c = b + 1
    d = torch.randn(3, requires_grad=True).cos()
    assert _reaches(c.grad_fn, b.grad_fn) and not _reaches(b.grad_fn, c.grad_fn) and not _reaches(c.grad_fn, d.grad_fn)


def test_reorder_states_cpu_path_equals_apply_to_states():
    """Module.reorder_states on CPU state buffers takes the reference's per-buffer torch.gather
    (beam_search.py:19-34) and must equal apply_to_states with that closure (the fused launch is GPU-only)."""
    import copy
    import torch
    from openvivqa_amd.modules.containers import Module

    class Leaf(Module):
        def __init__(self):
            super().__init__()
            self.register_state("running_keys", torch.zeros((0, 8)))
            self.register_state("running_seq", torch.zeros((1,)).long())

    class Net(Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = Leaf(), Leaf()
    b_s, cur, beam = 2, 3, 3
    net = Net()
    net.enable_statefulness(b_s * cur)
    g = torch.Generator().manual_seed(0)
    for leaf in (net.a, net.b):
        leaf.running_keys = torch.randn(b_s * cur, 5, 8, generator=g)
        leaf.running_seq = torch.randint(0, 9, (b_s * cur, 1), generator=g)
    sel = torch.randint(0, cur, (b_s, beam), generator=g)
    twin = copy.deepcopy(net)

    def fn(s):
        shape = [int(x) for x in s.shape]
        bm = sel
        for _ in shape[1:]:
            bm = bm.unsqueeze(-1)
        return torch.gather(s.view(*([b_s, cur] + shape[1:])), 1, bm.expand(*([b_s, beam] + shape[1:]))).view(*([-1] + shape[1:]))
    twin.apply_to_states(fn)
    net.reorder_states(sel, b_s, cur, beam)
    for x, y in zip(net.states(), twin.states()):
        assert torch.equal(x, y)


def _run_bench(*argv, env=None):
    import subprocess
    import sys
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=e, capture_output=True,
                          text=True, timeout=600)


def test_bench_gpus_flag_starts_that_many_ranks():
    """The driver's command shape is `python bench.py --gpus N ...` with no launcher around it: the script itself must
    become N ranks.  --dry-launch runs the launcher and the ranks' rendezvous on gloo, no GPU."""
    r = _run_bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-launch")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world_size"] == 2 and out["ranks_counted"] == 2
    assert out["config"]["parallelism"] == "dp2" and out["steps"] == 3 and out["warmup"] == 1


def test_bench_refuses_fewer_ranks_than_asked():
    """`--gpus 2` on a node with fewer than two devices fails loudly instead of printing a dp1 line, and a launcher
    that set a different WORLD_SIZE than --gpus is refused too."""
    if torch.cuda.device_count() < 2:
        r = _run_bench("--gpus", "2", "--steps", "1", "--warmup", "0")
        assert r.returncode != 0 and "refusing" in r.stderr and not r.stdout.strip()
    r = _run_bench("--gpus", "2", "--dry-launch", env={"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr and not r.stdout.strip()
    r = _run_bench("--dry-launch", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 1" in r.stderr


@pytest.mark.parametrize("beam", [1, 3])
def test_beam_search_driver_equals_reference_algorithm(beam):
    """openvivqa_amd.beam.BeamSearch (two-stage top-k selection, whole-buffer history gathers) against the oracle's
    restatement of the reference's list-based algorithm (models/modules/beam_search.py:36-118: full sort, per-element
    history gathers; pinned by G16) on a random step function that depends on the previous words; <eos> reachable."""
    from openvivqa_amd.beam import BeamSearch

    class NoStates:
        def reorder_states(self, *a):
            pass
    torch.manual_seed(beam)
    b_s, T, V, eos = 5, 9, 13, 2
    tables = [torch.randn(b_s * (1 if t == 0 else beam), 1, V) * 3 for t in range(T)]

    def step(t, prev):
        x = tables[t] if prev is None else tables[t] + 0.37 * torch.sin(prev.view(-1, 1, 1).float() + torch.arange(V))
        return torch.log_softmax(x, -1)
    out, lp = BeamSearch(NoStates(), step, b_s, T, eos, beam, "cpu").apply(1)

    import oracle as O  # (the restated reference search, pinned by G16: tests/test_oracle_golden.py)
    o2, l2 = O.oracle_beam_search(step, lambda fn: None, b_s, T, eos, beam, 1)
    assert torch.equal(out, o2) and torch.allclose(lp, l2)
    assert (out == eos).any()  # the finished-sequence branch was exercised
