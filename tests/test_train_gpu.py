"""GPU tests of the training harness (row T / SURVEY 8e): hipGraph-captured fwd+loss+bwd, fused Adam, and the
data-parallel code path rehearsed on ONE GPU through a single-rank RCCL group (phased backward captured as
several hipGraphs over one memory pool, gradient segments reduced on the communication stream)."""
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
# the default: the whole step is one graph; OVQA_WHOLE_STEP_GRAPH=0 (the A/B switch, scripts/gpu_r4_alt.sh) keeps the
# per-phase graphs, and the assertions about WHICH form was captured follow it
ONE_GRAPH = os.environ.get("OVQA_WHOLE_STEP_GRAPH", "1") != "0"


def _cfg(layers, dropout):
    from openvivqa_amd.config import ConfigNode
    att = dict(ARCHITECTURE="ScaledDotProductAttention", HEAD=8, D_MODEL=512, D_KEY=64, D_VALUE=64, D_FF=2048,
               USE_AOA=False, CAN_BE_STATEFUL=False, DROPOUT=dropout)
    return ConfigNode(dict(ARCHITECTURE="MCAN", D_MODEL=512,
                           SELF_ENCODER=dict(ARCHITECTURE="Encoder", D_MODEL=512, LAYERS=layers, SELF_ATTENTION=att),
                           GUIDED_ENCODER=dict(ARCHITECTURE="GuidedAttentionEncoder", D_MODEL=512, LAYERS=layers,
                                               SELF_ATTENTION=att, GUIDED_ATTENTION=att)))


def _make(layers, dropout=0.0, **kw):
    import openvivqa_amd as A
    from openvivqa_amd import ops
    from openvivqa_amd.mcan_stack import MCANEncoderStack, synthetic_batch
    from openvivqa_amd.train import TrainStep
    dev = torch.device("cuda", 0)
    A.set_compute_dtype(torch.bfloat16)
    A.manual_seed(11)
    torch.manual_seed(11)
    model = MCANEncoderStack(_cfg(layers, dropout)).to(dev).train()
    v, vm, t, tm = synthetic_batch(16, 100, 20, 512, 80, 8, 5, dev, torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    tv = torch.randn(v.shape, generator=g).to(dev, torch.bfloat16)
    tt = torch.randn(t.shape, generator=g).to(dev, torch.bfloat16)
    loss = torch.zeros(1, device=dev)

    def forward_loss(v_, vm_, t_, tm_):
        vo, lo = model(v_, vm_, t_, tm_)
        dvo = ops.sq_loss_fwd_bwd(vo.detach(), loss, accumulate=False, target=tv)
        dlo = ops.sq_loss_fwd_bwd(lo.detach(), loss, accumulate=True, target=tt)
        return (vo, lo), (dvo, dlo)
    ts = TrainStep(model, forward_loss, lr=1e-4, betas=(0.9, 0.98), compute_dtype=torch.bfloat16, **kw)
    ts.loss = loss
    return model, ts, (v, vm, t, tm)


@pytest.fixture
def single_rank_group():
    import torch.distributed as dist
    dist.init_process_group("nccl", init_method="file://" + os.path.join(tempfile.mkdtemp(prefix="ovqa_"), "rdv"),
                            rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("comm", [torch.float32, torch.bfloat16])
def test_phased_backward_with_comm_stream_matches_single_graph(single_rank_group, use_graph, comm):
    """The N>1 path (several backward phases, each its own hipGraph; segments cast / all-reduced / cast back on
    the communication stream while later phases run) yields the gradients and the weights of the plain
    single-graph step."""
    _, ref, batch = _make(3)
    for _ in range(3):
        ref.step(*batch)
    torch.cuda.synchronize()
    _, ts, batch = _make(3, force_comm=True, overlap_mb=16.0, comm_dtype=comm, use_graph=use_graph)
    for _ in range(3):
        ts.step(*batch)
    torch.cuda.synchronize()
    assert (ref.whole is not None) == ONE_GRAPH and ref.captured and len(ref.segments) == 1
    assert len(ts.segments) >= 4, ts.segments
    # one graph for the whole step, the exchange of every segment captured on a forked branch of it
    assert ((ts.whole is not None) == ONE_GRAPH and ts.captured) if use_graph else not ts.captured
    flat = sorted(r for s in ts.segments for r in s)
    assert flat[0][0] == 0 and flat[-1][1] == ts.arena.numel and all(a[1] == b[0] for a, b in zip(flat, flat[1:]))
    assert abs(float(ts.loss) - float(ref.loss)) <= 2e-3 * abs(float(ref.loss))
    # gradients of the last step: identical kernels; only the order in which the question-feature gradient is
    # summed differs (bf16 rounding), plus bf16 transport when comm is bf16
    assert _rel(ts.arena.grad, ref.arena.grad) <= (2e-2 if comm == torch.bfloat16 else 1e-2)
    # weights moved by 3 Adam steps of lr 1e-4
    moved = (ref.arena.master - ts.arena.master).abs().max().item()
    assert moved <= 6.5e-4


def test_graph_replay_equals_eager_steps():
    """Same kernels on the same weights.  Round 4: the step is DETERMINISTIC (bias gradients = fused column sums of the
    grouped dW, LayerNorm-parameter gradients and the loss through fixed-order reductions with plain stores; rounds 1-3
    used fp32 atomics there and two runs drifted apart by O(lr)): eager launches and graph replays give bit-identical
    gradients, weights and losses, step after step."""
    ma, a, batch = _make(2, use_graph=True)
    mb, b, _ = _make(2, use_graph=False)
    for _ in range(3):
        a.step(*batch)
        b.step(*batch)
        torch.cuda.synchronize()
        assert torch.equal(a.arena.grad, b.arena.grad)
        assert torch.equal(a.arena.master, b.arena.master)
        assert float(a.loss) == float(b.loss)


@pytest.mark.parametrize("use_graph", [True, False])
def test_adam_inside_the_weight_gradient_launch_equals_separate_adam(use_graph):
    """Round 5: at world size 1 the last grouped weight-gradient launch of a step applies Adam to the weight matrices itself
    (ovqa_grouped_linear_bwd_weight_adam: the fp32 gradient tile never reaches HBM).  Against the separate tiled Adam launch,
    over 4 steps of a schedule that changes every step: bit-identical losses, master weights, moments, bf16 shadows and
    transposed shadows -- the two kernels share one update function."""
    from openvivqa_amd.train import noam_lr_scale
    kw = dict(lr_lambda=lambda s: noam_lr_scale(s, 512, 3), use_graph=use_graph)
    _, a, batch = _make(2, fuse_adam=True, **kw)
    _, b, _ = _make(2, fuse_adam=False, **kw)
    assert a._fused is not None and b._fused is None
    for i in range(4):
        a.step(*batch)
        b.step(*batch)
        torch.cuda.synchronize()
        assert float(a.loss) == float(b.loss), i
        assert torch.equal(a.arena.master, b.arena.master), i
        assert torch.equal(a.arena.shadow, b.arena.shadow) and torch.equal(a.arena.shadow_t, b.arena.shadow_t), i
        assert torch.equal(a.optim.exp_avg, b.optim.exp_avg) and torch.equal(a.optim.exp_avg_sq, b.optim.exp_avg_sq), i
    # the launch took (nearly) every matrix of the stacks, and the 1-D parameters went through the separate launch
    fused = sum(hi - lo for lo, hi in a._fused.ranges)
    assert a._fused.began and fused >= 0.95 * a.arena.small_lo, (fused, a.arena.small_lo)
    assert int(a.optim.step_t.item()) == 4 == a.optim.host_step
    lo = a.arena.small_lo
    assert torch.equal(a.arena.grad[lo:], b.arena.grad[lo:])


@pytest.mark.parametrize("force", [False, True])
def test_whole_step_graph_equals_phase_graphs_with_eager_adam(single_rank_group, force, monkeypatch):
    """Round 4: the step is ONE graph -- forward, loss, backward, the gradient exchange of every segment (captured RCCL
    collectives on a forked branch) and Adam with the Noam schedule read from a device table (ovqa_begin_step).  Against
    the round-3 form (one graph per backward phase, exchange and Adam launched from the host with the schedule as a host
    float): bit-identical weights, moments and losses over 5 steps of a schedule that changes every step."""
    from openvivqa_amd.train import noam_lr_scale
    kw = dict(lr_lambda=lambda s: noam_lr_scale(s, 512, 3), force_comm=force, overlap_mb=16.0)
    # (dropout off: the dropout step counter is one device tensor per process, shared by every TrainStep in it, so two
    #  harnesses stepping in turns would draw each other's masks; the two-process test below covers dropout)
    _, a, batch = _make(2, **kw)
    a.prepare(*batch)  # (the capture happens here, under the default switch)
    monkeypatch.setenv("OVQA_WHOLE_STEP_GRAPH", "0")
    _, b, _ = _make(2, **kw)
    b.prepare(*batch)
    for i in range(5):
        a.step(*batch)
        b.step(*batch)
        torch.cuda.synchronize()
        assert float(a.loss) == float(b.loss), i
        assert torch.equal(a.arena.master, b.arena.master), i
    assert a.whole is not None and a.graphs is None and b.whole is None and b.graphs is not None
    assert len(a.segments) == len(b.segments) and (len(a.segments) >= 3 if force else len(a.segments) == 1)
    assert torch.equal(a.optim.exp_avg, b.optim.exp_avg) and torch.equal(a.optim.exp_avg_sq, b.optim.exp_avg_sq)
    assert int(a.optim.step_t.item()) == 5 == a.optim.host_step and abs(float(a.optim.lr_eff) - 1e-4 * noam_lr_scale(4, 512, 3)) < 1e-12


def test_failed_whole_step_capture_falls_back_cleanly(single_rank_group, monkeypatch):
    """a whole-step capture that dies MID-BODY -- behind the first segments' collectives -- must leave
    neither work handles of the aborted capture in the reducer (a later ``wait_segment(k)`` would join a dead handle, and
    Adam would run before segment k's all-reduce) nor queued products / deferred table uploads in the grouped-dW queue.
    The fallback (one graph per backward phase, exchange and Adam from the host) must then give the bits of a harness that
    took that route from the start."""
    from openvivqa_amd import functional as Fn
    from openvivqa_amd.train import TrainStep, noam_lr_scale
    kw = dict(lr_lambda=lambda s: noam_lr_scale(s, 512, 3), force_comm=True, overlap_mb=16.0)
    _, a, batch = _make(2, **kw)
    real, calls = TrainStep._release, {"n": 0}

    def failing(self, k):
        real(self, k)
        calls["n"] += 1
        if torch.cuda.is_current_stream_capturing() and self.whole is None and k == 1 and calls["n"] < 64:
            raise RuntimeError("injected: the capture dies behind the second segment's collective")
    monkeypatch.setattr(TrainStep, "_release", failing)
    a.prepare(*batch)
    monkeypatch.setattr(TrainStep, "_release", real)
    assert a.whole is None and a.graphs is not None and len(a.segments) >= 3
    assert a.reducer._done == [] and not a.reducer._pending
    q = Fn.wgrad_queue()
    assert not q.items and not q.reduces and not q._deferred and not q.defer_uploads
    monkeypatch.setenv("OVQA_WHOLE_STEP_GRAPH", "0")
    _, b, _ = _make(2, **kw)
    b.prepare(*batch)
    for i in range(4):
        a.step(*batch)
        b.step(*batch)
        torch.cuda.synchronize()
        assert float(a.loss) == float(b.loss), i
        assert torch.equal(a.arena.master, b.arena.master), i


def test_failed_whole_step_capture_with_adam_in_the_weight_gradient_launch(monkeypatch):
    """with the optimiser riding in the last weight-gradient launch (world size 1, bench.py's default) a
    whole-step capture that fails AFTER backward leaves ``_fused.began`` set, while the phase graphs of the fallback are
    captured unarmed (plain weight-gradient launches).  A stale flag made the optimiser tail skip the matrices the fused
    launch would have taken and never advance the step / schedule / dropout counters.  The fallback must give the bits of a
    harness with the separate Adam, and its counters must move."""
    from openvivqa_amd.train import TrainStep, noam_lr_scale
    kw = dict(lr_lambda=lambda s: noam_lr_scale(s, 512, 3))
    _, a, batch = _make(2, fuse_adam=True, **kw)
    real, fired = TrainStep._optimiser_tail, {"n": 0}

    def failing(self, host=True):
        if torch.cuda.is_current_stream_capturing() and self.whole is None and fired["n"] == 0:
            fired["n"] += 1
            assert self._fused is not None and self._fused.began  # (the state the fallback has to clean up)
            raise RuntimeError("injected: the capture dies behind backward")
        return real(self, host)
    monkeypatch.setattr(TrainStep, "_optimiser_tail", failing)
    a.prepare(*batch)
    monkeypatch.setattr(TrainStep, "_optimiser_tail", real)
    assert fired["n"] == 1 and a.whole is None and a.graphs is not None and a._fused is None
    _, b, _ = _make(2, fuse_adam=False, **kw)
    for i in range(4):
        a.step(*batch)
        b.step(*batch)
        torch.cuda.synchronize()
        assert float(a.loss) == float(b.loss), i
        assert torch.equal(a.arena.master, b.arena.master), i
        assert torch.equal(a.arena.shadow, b.arena.shadow) and torch.equal(a.arena.shadow_t, b.arena.shadow_t), i
    assert torch.equal(a.optim.exp_avg, b.optim.exp_avg) and torch.equal(a.optim.exp_avg_sq, b.optim.exp_avg_sq)
    assert int(a.optim.step_t.item()) == 4 == a.optim.host_step


def test_checkpoint_resume_inside_the_one_graph_step_is_bitwise():
    """Save after 3 steps (model state_dict + TrainStep.state_dict), rebuild everything, load, take 2 more: the weights,
    moments and loss of the uninterrupted 5-step run, bit for bit -- the step is deterministic, and the device-side
    schedule table is rebuilt from the restored step count and rate (``FlatAdam._resync_schedule``)."""
    import copy
    from openvivqa_amd.train import noam_lr_scale
    kw = dict(lr_lambda=lambda s: noam_lr_scale(s, 512, 3))
    ma, a, batch = _make(2, **kw)
    for _ in range(5):
        a.step(*batch)
    mb, b, _ = _make(2, **kw)
    for _ in range(3):
        b.step(*batch)
    torch.cuda.synchronize()
    ckpt = copy.deepcopy({"model": mb.state_dict(), "train": b.state_dict()})
    mc, c, _ = _make(2, **kw)
    c.prepare(*batch)  # (captured BEFORE the load: the graph must pick the restored state up)
    mc.load_state_dict(ckpt["model"])
    c.load_state_dict(ckpt["train"])
    for _ in range(2):
        c.step(*batch)
    torch.cuda.synchronize()
    assert (c.whole is not None) == ONE_GRAPH and int(c.optim.step_t.item()) == 5 == c.optim.host_step
    assert torch.equal(c.arena.master, a.arena.master) and float(c.loss) == float(a.loss)
    assert torch.equal(c.optim.exp_avg, a.optim.exp_avg) and torch.equal(c.optim.exp_avg_sq, a.optim.exp_avg_sq)


def test_device_schedule_table_wraps_and_refills():
    """FlatAdam's device-side LambdaLR table (4096 entries, half refilled every 2048 steps, a stream-ordered copy issued
    half a table ahead): the rate ovqa_begin_step hands Adam equals lr * lr_lambda(step) for 3 x 4096 steps."""
    from openvivqa_amd import ops
    from openvivqa_amd.train import FlatAdam, noam_lr_scale

    class Arena:
        device = torch.device("cuda", 0)
        master = torch.zeros(8, device="cuda")
    opt = FlatAdam(Arena(), lr=0.5, lr_lambda=lambda s: noam_lr_scale(s, 512, 100))
    opt.device_schedule()
    seen = torch.zeros(3 * opt.LR_TABLE, device="cuda")
    for s in range(3 * opt.LR_TABLE):
        ops.begin_step(opt.step_t, None, opt.lr_table, opt.lr_eff)
        seen[s:s + 1].copy_(opt.lr_eff)
        opt.advance_host()
    want = torch.tensor([0.5 * noam_lr_scale(s, 512, 100) for s in range(3 * opt.LR_TABLE)], dtype=torch.float32)
    assert torch.equal(seen.cpu(), want)


_DETERMINISM_SCRIPT = """
import hashlib, sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_train_gpu as T
model, ts, batch = T._make(2, use_graph={graph}, dropout=0.1)
losses = []
for _ in range(3):
    ts.step(*batch)
    losses.append(float(ts.loss))
torch.cuda.synchronize()
h = hashlib.sha256(ts.arena.master.cpu().numpy().tobytes()).hexdigest()
g = hashlib.sha256(ts.arena.grad.cpu().numpy().tobytes()).hexdigest()
print("RESULT", h, g, " ".join(repr(x) for x in losses))
"""


@pytest.mark.parametrize("graph", [True, False])
def test_two_fresh_processes_train_to_identical_bits(graph):
    """SURVEY section 5, "same seed => same bits" (VERDICT r3 item 8): two FRESH processes run three TrainStep steps of
    the MCAN stacks (L = 2, B = 16, dropout 0.1 on: the keep masks are a counter hash, not a device RNG) and end with
    bit-identical fp32 master weights, gradients and losses -- graph replays and eager launches alike, and the two modes
    agree with each other (previous test)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _DETERMINISM_SCRIPT.format(root=root, tests=os.path.join(root, "tests"), graph=graph)
    outs = []
    for _ in range(2):  # one after the other: never two extra processes on the card at once
        r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
        assert r.returncode == 0, r.stderr[-3000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
        assert len(line) == 1, r.stdout[-2000:]
        outs.append(line[0])
    assert outs[0] == outs[1], outs


@pytest.mark.parametrize("use_graph", [False, True])
def test_mcan_model_two_training_steps_match_oracle(use_graph):
    """Whole MCAN model (embeddings + both stacks + pooling head + classifier, weights and inputs of golden G12,
    which came from the reference's own models/mcan.py) trained for two steps by the product's TrainStep in fp32
    mode: losses and post-step weights follow the oracle's torch.optim.Adam trajectory (row T at model level).
    LSTM / embedding / head parameters get their gradients from torch, the stacks from the HIP kernels: both
    kinds live in the same flat arena."""
    import oracle as O
    import openvivqa_amd as A
    from types import SimpleNamespace
    from golden_cases import ModelVocab, load_case
    from openvivqa_amd.config import ConfigNode
    from openvivqa_amd.models import MCAN
    from openvivqa_amd.train import TrainStep
    case = load_case("G12_mcan_model")
    cfg = ConfigNode(case.meta["cfg"])
    vocab = ModelVocab(case.meta["vocab_len"], case.meta["total_answers"])
    y = torch.tensor([1, 4, 6])
    nll = torch.nn.NLLLoss()
    ref = O.OracleMCAN(cfg, vocab)
    ref.load_state_dict(case.w)
    ref.eval()  # dropout off on both sides; LSTM on CPU is fine in eval mode
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.9, 0.98))
    inp = SimpleNamespace(region_features=case.inputs["regions"], question_tokens=case.inputs["tokens"])
    ref_losses = [O.oracle_train_step(None, lambda: nll(ref(inp), y), opt) for _ in range(2)]

    A.set_compute_dtype(torch.float32)
    try:
        dev = torch.device("cuda", 0)
        m = MCAN(cfg, vocab)
        m.load_state_dict(case.w)
        m = m.to(dev).train()
        for mod in m.modules():  # train mode (MIOpen LSTM backward needs it), dropout off
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        yd = y.to(dev)

        def forward_loss(regions, tokens):
            return nll(m(SimpleNamespace(region_features=regions, question_tokens=tokens)), yd)
        ts = TrainStep(m, forward_loss, lr=1e-3, betas=(0.9, 0.98), use_graph=use_graph,
                       compute_dtype=torch.float32)
        batch = (case.inputs["regions"].to(dev), case.inputs["tokens"].to(dev))
        losses = [float(ts.step(*batch)) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        A.set_compute_dtype(torch.bfloat16)
    assert max(abs(a - b) for a, b in zip(losses, ref_losses)) < 2e-4, (losses, ref_losses)
    sd = m.state_dict()
    num = den = 0.0
    for k, v in ref.state_dict().items():
        if k.endswith("fc_k.bias") or k.endswith("attr_reduce.fc2.bias"):
            continue  # analytically zero gradients: Adam turns rounding noise into +-lr steps
        d = (sd[k].cpu().double() - v.double()).abs()
        # Adam normalises every element's step to ~lr, so an element whose gradient is itself rounding noise
        # (dead ReLU units of the pooling MLP) may differ by a fraction of the 2 x lr it can move at most
        assert d.max().item() < 1e-3, (k, d.max().item())
        upd = v.double() - case.w[k].double()
        num += ((sd[k].cpu().double() - case.w[k].double()) - upd).pow(2).sum().item()
        den += upd.pow(2).sum().item()
    assert (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5  # the two-step update as a whole


@pytest.mark.parametrize("use_graph", [False, True])
def test_decoder_two_training_steps_match_oracle(use_graph):
    """BASELINE configs[4], the training half (tasks/open_ended_task.py:150-169): the Decoder (L=3, d=512, 237 encoder
    positions, T=20) teacher-forced on <bos> a_1 .. a_n, NLLLoss(ignore_index = pad) against the right-shifted answer over
    every position, trained for two steps by the product's TrainStep in fp32 mode: losses and post-step weights follow the
    oracle's torch.optim.Adam trajectory (what bench.py times as `secondary.decoder_train`)."""
    import oracle as O
    import openvivqa_amd as A
    import openvivqa_amd.modules as M
    from openvivqa_amd.config import ConfigNode, attention_config
    from openvivqa_amd.losses import NLLLoss
    from openvivqa_amd.train import TrainStep
    V, T, NE, B = 1000, 20, 237, 4

    class Vocab:
        max_answer_length, padding_idx, bos_idx, eos_idx = T, 0, 1, 2

        def __len__(self):
            return V
    cfg = ConfigNode(dict(
        ARCHITECTURE="Decoder", D_MODEL=512, LAYERS=3,
        ATTENTION=dict(SELF_ATTENTION=attention_config(can_be_stateful=True), ENC_ATTENTION=attention_config()),
        TEXT_EMBEDDING=dict(ARCHITECTURE="UsualEmbedding", D_MODEL=512, D_EMBEDDING=300, WORD_EMBEDDING=None,
                            WORD_EMBEDDING_CACHE=None, DROPOUT=0.1)))
    torch.manual_seed(21)
    ref = O.OracleDecoder(cfg, Vocab())
    w0 = {k: v.clone() for k, v in ref.state_dict().items()}
    ref.eval()  # dropout off on both sides
    g = torch.Generator().manual_seed(9)
    ans = torch.randint(3, V, (B, T + 1), generator=g)
    ans[:, 0] = 1
    ans[1, 12:] = 0
    ans[3, 7:] = 0
    enc = torch.randn(B, NE, 512, generator=g)
    enc[2, 210:] = 0
    emask = O.padding_mask(enc, 0)
    tin, tgt = ans[:, :-1].contiguous(), ans[:, 1:].contiguous()
    nll = torch.nn.NLLLoss(ignore_index=0)
    opt = torch.optim.Adam([p for p in ref.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98))
    ref_losses = [O.oracle_train_step(None, lambda: nll(ref(tin, enc, emask).reshape(-1, V), tgt.reshape(-1)), opt)
                  for _ in range(2)]

    A.set_compute_dtype(torch.float32)
    try:
        dev = torch.device("cuda", 0)
        m = M.Decoder(cfg, Vocab())
        m.load_state_dict(w0, strict=False)
        m = m.to(dev).train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        loss_fn, tg = NLLLoss(ignore_index=0), tgt.to(dev)

        def forward_loss(tokens, enc_, emask_):
            return loss_fn(m(tokens, enc_, emask_), tg)
        ts = TrainStep(m, forward_loss, lr=1e-3, betas=(0.9, 0.98), use_graph=use_graph, compute_dtype=torch.float32)
        batch = (tin.to(dev), enc.to(dev), emask.to(dev))
        losses = [float(ts.step(*batch)) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        A.set_compute_dtype(torch.bfloat16)
    assert max(abs(a - b) for a, b in zip(losses, ref_losses)) < 2e-4, (losses, ref_losses)
    sd = m.state_dict()
    num = den = 0.0
    for k, v in ref.state_dict().items():
        if k.endswith("fc_k.bias") or k == "pos_emb.weight" or k not in sd or v.numel() == 0 or not v.is_floating_point():
            continue  # analytically zero gradients: Adam turns rounding noise into +-lr steps; frozen table; state buffers
        d = (sd[k].cpu().double() - v.double()).abs()
        assert d.max().item() < 1e-3, (k, d.max().item())
        upd = v.double() - w0[k].double()
        num += ((sd[k].cpu().double() - w0[k].double()) - upd).pow(2).sum().item()
        den += upd.pow(2).sum().item()
    assert den > 0 and (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5  # the two-step update as a whole


def test_training_reduces_loss_bf16():
    """30 hipGraph-replayed bf16 steps on one fixed batch (dropout on, lr 2e-4): the regression loss goes down
    monotonically on average and ends well below where it started -- the step is a working optimiser step, not
    only a timed one."""
    import openvivqa_amd as A
    from openvivqa_amd import ops
    from openvivqa_amd.mcan_stack import MCANEncoderStack, synthetic_batch
    from openvivqa_amd.train import TrainStep
    dev = torch.device("cuda", 0)
    A.set_compute_dtype(torch.bfloat16)
    A.manual_seed(5)
    torch.manual_seed(5)
    model = MCANEncoderStack(_cfg(2, 0.1)).to(dev).train()
    v, vm, t, tm = synthetic_batch(16, 100, 20, 512, 80, 8, 9, dev, torch.bfloat16)
    g = torch.Generator().manual_seed(4)
    tv = torch.randn(v.shape, generator=g).to(dev, torch.bfloat16)
    tt = torch.randn(t.shape, generator=g).to(dev, torch.bfloat16)
    loss = torch.zeros(1, device=dev)

    def forward_loss(v_, vm_, t_, tm_):
        vo, lo = model(v_, vm_, t_, tm_)
        return (vo, lo), (ops.sq_loss_fwd_bwd(vo.detach(), loss, accumulate=False, target=tv),
                          ops.sq_loss_fwd_bwd(lo.detach(), loss, accumulate=True, target=tt))
    ts = TrainStep(model, forward_loss, lr=2e-4, betas=(0.9, 0.98), compute_dtype=torch.bfloat16)
    ts.loss = loss
    hist = [float(ts.step(v, vm, t, tm)) for _ in range(30)]
    assert all(h == h for h in hist)  # no NaN
    assert sum(hist[-5:]) / 5 < 0.93 * sum(hist[:5]) / 5, hist


def test_crossmodality_train_step_with_comm(single_rank_group):
    """BASELINE configs[2] path: CrossModalityEncoder under TrainStep.  Its dead cross-attention parameters never
    get a gradient: their ranges of the flat buffer must stay zero -- on every rank alike -- through
    the data-parallel exchange, and their weights must not move."""
    import openvivqa_amd as A
    import openvivqa_amd.modules as M
    from openvivqa_amd import ops
    from openvivqa_amd.config import ConfigNode, attention_config
    from openvivqa_amd.mcan_stack import synthetic_batch
    from openvivqa_amd.train import TrainStep
    dev = torch.device("cuda", 0)
    A.set_compute_dtype(torch.bfloat16)
    sa = attention_config(dropout=0.0)
    cfg = ConfigNode(dict(D_MODEL=512, LAYERS=2, VISION_LANGUAGE_ATTENTION=sa, LANGUAGE_VISION_ATTENTION=sa,
                          VISION_SELF_ATTENTION=sa, LANGUAGE_SELF_ATTENTION=sa))
    results, masters = [], []
    for force, fuse in ((False, False), (True, False), (False, True)):
        A.manual_seed(3)
        torch.manual_seed(3)
        model = M.CrossModalityEncoder(cfg).to(dev).train()
        w0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        v, vm, t, tm = synthetic_batch(8, 100, 20, 512, 80, 8, 5, dev, torch.bfloat16)
        g = torch.Generator().manual_seed(3)
        tv = torch.randn(v.shape, generator=g).to(dev, torch.bfloat16)
        tt = torch.randn(t.shape, generator=g).to(dev, torch.bfloat16)
        loss = torch.zeros(1, device=dev)

        def forward_loss(v_, vm_, t_, tm_):
            vo, lo = model(v_, vm_, t_, tm_)
            return (vo, lo), (ops.sq_loss_fwd_bwd(vo.detach(), loss, accumulate=False, target=tv),
                              ops.sq_loss_fwd_bwd(lo.detach(), loss, accumulate=True, target=tt))
        ts = TrainStep(model, forward_loss, lr=1e-4, betas=(0.9, 0.98), compute_dtype=torch.bfloat16,
                       force_comm=force, comm_dtype=torch.float32, overlap_mb=8.0, fuse_adam=fuse)
        ts.loss = loss
        for _ in range(2):
            ts.step(v, vm, t, tm)
        torch.cuda.synchronize()
        assert (ts.whole is not None) == ONE_GRAPH and (len(ts.segments) >= 2 if force else len(ts.segments) == 1)
        # (round 5) the dead parameters are found by the discovery pass: zeroed once, left out of the fused optimiser path
        assert ts._dead and sum(e - s_ for s_, e in ts._dead) >= 2 * 2 * 4 * 512 * 512
        assert all(int(torch.count_nonzero(ts.arena.grad[s_:e]).item()) == 0 for s_, e in ts._dead)
        masters.append(ts.arena.master.clone())
        dead = [k for k in w0 if "language_vision_mhattn" in k or "vision_language_mhattn" in k]
        assert dead
        for k in dead:
            assert torch.equal(model.state_dict()[k], w0[k]), k  # zero gradient -> Adam leaves them alone
        moved = [k for k in w0 if k not in dead and not torch.equal(model.state_dict()[k], w0[k])]
        assert len(moved) > 20
        results.append((ts.arena.grad.clone(), float(ts.loss)))
    assert _rel(results[1][0], results[0][0]) <= 1e-5 and abs(results[1][1] - results[0][1]) <= 1e-5 * abs(results[0][1])
    # Adam inside the last weight-gradient launch (and no Adam at all for the dead parameters): the same weights, bit for bit
    assert torch.equal(masters[2], masters[0]) and results[2][1] == results[0][1]


def test_tiled_adam_equals_flat_adam_plus_transpose(monkeypatch):
    """ovqa_adam_step_tiled (update + bf16 shadow + its transpose in one pass over 64 x 64 tiles) against the flat
    ovqa_adam_step followed by ovqa_grouped_transpose on the SAME state and gradients: the same arithmetic per element,
    so masters and moments agree to 2 ulp and the bf16 copies up to rare rounding flips (two kernels: the compiler
    contracts multiply-adds differently); fp32 and bf16 gradient buffers (the latter is
    what a bf16 all-reduce leaves), two consecutive updates each."""
    model, ts, batch = _make(1, use_graph=False)
    ts.step(*batch)  # a real step: non-trivial moments and gradients
    a, opt = ts.arena, ts.optim
    assert a.adam_tiles() is not None
    state = [t.clone() for t in (a.master, opt.exp_avg, opt.exp_avg_sq, a.shadow, a.shadow_t, opt.step_t)]
    grads = {"fp32": a.grad.clone(), "bf16": a.grad.to(torch.bfloat16)}
    for kind, g in grads.items():
        results = {}
        tiles_in = a.adam_tiles_in
        for tiled in ("1", "0"):
            # "0": no tile table for any range -> FlatAdam.apply takes the flat kernel + the separate grouped transpose
            monkeypatch.setattr(a, "adam_tiles_in", tiles_in if tiled == "1" else (lambda lo, hi: None))
            for dst, src in zip((a.master, opt.exp_avg, opt.exp_avg_sq, a.shadow, a.shadow_t, opt.step_t), state):
                dst.copy_(src)
            opt.step(g, grad_scale=0.5)
            opt.step(g, grad_scale=0.25)
            torch.cuda.synchronize()
            results[tiled] = [t.clone() for t in (a.master, opt.exp_avg, opt.exp_avg_sq, a.shadow, a.shadow_t)]
        for name, x, y in zip(("master", "exp_avg", "exp_avg_sq", "shadow", "shadow_t"), results["1"], results["0"]):
            # the same formulas, but two kernels: the compiler may contract a*b+c differently -> allow 2 ulp of fp32
            # on the fp32 state and, for the bf16 copies, a rounding flip on a vanishing fraction of the elements
            xd, yd = x.double(), y.double()
            if x.dtype == torch.float32:
                # (a weight is p - update: its error is an ulp of the larger of the two, not of the result)
                err = ((xd - yd).abs() / yd.abs().clamp_min(1e-3 if name == "master" else 1e-12)).max().item()
                assert err < 3e-5 if name == "master" else err < 3e-7, (kind, name, err, (xd - yd).abs().max().item())
            else:
                flips = (x != y).float().mean().item()
                assert flips < 1e-3, (kind, name, flips)
                if name == "shadow":  # one bf16 step at the larger of the two, on top of what separates the masters
                    ulp = torch.maximum(xd.abs(), yd.abs()) * 2 ** -7
                    dm = (results["1"][0].double() - results["0"][0].double()).abs()
                    assert ((xd - yd).abs() <= ulp + dm + 1e-30).all(), (kind, name)
        assert not torch.equal(results["1"][0], state[0])
        # and the transposed copy IS the transpose of the shadow
        for off, rows, cols in a._groups2d:
            assert torch.equal(results["1"][4][off:off + rows * cols].view(cols, rows),
                               results["1"][3][off:off + rows * cols].view(rows, cols).t())


def test_data_parallel_exchange_bf16_vs_fp32_vs_single_process():
    """FOUR real ranks (real kernels, all on this one GPU, gradients over gloo) take two optimiser
    steps with the gradient exchange in bf16 (opt-in: half the bytes per xGMI link) and in fp32 (the default); a single process
    takes the same two steps on the four shards concatenated (mean loss over 4 B samples, B = 8 = the average of the ranks'
    means).  Measured, post-step fp32 master weights:
      * fp32 exchange vs the single process: accumulation order only;
      * bf16 exchange vs fp32 exchange: no weight moves by more than one bf16 step of its own value plus 2 % of an
        optimiser step (lr) -- the exchange's rounding is below what the bf16 shadow of the weights resolves."""
    import numpy as np
    import torch.multiprocessing as mp
    import dp_helpers as H
    world, steps, lr = 4, 2, 1e-4
    ctx = mp.get_context("spawn")
    results = {}
    for comm_bf16 in (True, False):
        rdv = os.path.join(tempfile.mkdtemp(prefix="ovqa_dp_"), "rdv")
        q = ctx.Queue()
        procs = [ctx.Process(target=H.dp_gpu_worker, args=(r, world, rdv, comm_bf16, steps, q)) for r in range(world)]
        for p in procs:
            p.start()
        results[comm_bf16] = torch.from_numpy(q.get(timeout=300))
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    # the single process: all shards at once
    model, ts, tgt = H.gpu_stack_step(H.DP_GPU_BATCH * world, torch.float32)
    shards = [H.gpu_rank_batch(r, H.DP_GPU_BATCH) for r in range(world)]
    batch = tuple(torch.cat([s[0][i] for s in shards], 0) for i in range(4))
    tgt["v"], tgt["t"] = torch.cat([s[1][0] for s in shards], 0), torch.cat([s[1][1] for s in shards], 0)
    w0 = ts.arena.master.detach().clone().cpu()
    for _ in range(steps):
        ts.step(*batch)
    torch.cuda.synchronize()
    single = ts.arena.master.detach().cpu()
    moved = (single - w0).abs()
    assert moved.max() > 0.5 * lr  # the steps did move the weights
    from conftest import parity_record as rec
    w32, w16 = results[False], results[True]
    # masters after two steps: compare the UPDATES (w - w0), the weights themselves are ~1e-2
    upd = lambda w: (w - w0).double()
    e32 = ((upd(w32) - upd(single)).norm() / upd(single).norm()).item()
    e16 = ((upd(w16) - upd(w32)).norm() / upd(w32).norm()).item()
    rec("dp[4 ranks, gloo, 1 GPU]", "update, fp32 exchange vs single process (rel L2)", e32, 1e-2)
    rec("dp[4 ranks, gloo, 1 GPU]", "update, bf16 exchange vs fp32 exchange (rel L2)", e16, 5e-2)
    # (Adam normalises every element, so a gradient's relative error IS the update's: where the four ranks' gradients of
    # an element cancel -- B = 8 per rank is a noisy extreme -- the bf16 sum's 2^-9 is relative to their magnitudes,
    # not to the sum: ~2 % of the update in L2, measured; far below what the weights' bf16 shadow resolves, next check)
    assert e32 < 1e-2 and e16 < 5e-2, (e32, e16)
    # weight level.  fc_k.bias is left out as everywhere (its gradient is analytically zero: pure rounding noise that
    # Adam turns into +-lr steps of random sign in ANY two runs).  The same mechanism acts on single elements of other
    # parameters: where the ranks' gradients of an element cancel to (nearly) nothing, the sign of the sum -- and with it
    # a full +-lr step -- depends on the last bits of the exchange.  Measured here: how many elements move by more than
    # one bf16 step of their own value plus 5 % of what Adam could have moved them, and by how much at worst.
    names = {id(p): n for n, p in model.named_parameters()}
    tag, worst, over, total = "dp[4 ranks, gloo, 1 GPU]", ("", 0.0), 0, 0
    for name, shape, off in ts.arena.layout(names):
        if name.endswith("fc_k.bias"):
            continue
        n = int(torch.tensor(shape).prod())
        a, b = w16[off:off + n], w32[off:off + n]
        bound = b.abs() * 2.0 ** -8 + 0.05 * lr * steps
        r = (a - b).abs() / bound
        over, total = over + int((r > 1).sum()), total + n
        if r.max().item() > worst[1]:
            worst = (name, r.max().item())
    frac = over / total
    rec(tag, f"worst |w_bf16x - w_fp32x| / (bf16 step of w + 5% of lr*steps)  [{worst[0]}]", worst[1], 0.0)
    rec(tag, "fraction of weights beyond that bound after two steps", frac, 2e-3)
    max_step = (w16 - w32).abs().max().item() / (lr * steps)
    rec(tag, "largest |w_bf16x - w_fp32x| in units of lr*steps (2 = opposite full steps)", max_step, 2.001)
    assert frac < 2e-3 and max_step <= 2.001, (frac, worst, max_step)


def test_bench_launcher_two_ranks_on_this_gpu():
    """The contract form `python bench.py --gpus N` end to end with the real kernels: the parent starts two ranks through
    torch.distributed.run (both on this GPU, gradients over gloo: OVQA_REHEARSE_BACKEND), they agree on the segment plan,
    exchange every step, and rank 0 prints ONE JSON line with n_gpus = world_size = 2 and a global batch of 128."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OVQA_REHEARSE_BACKEND="gloo", OVQA_NO_BUILD="1", PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--repeats", "1", "--no-cpu-baseline", "--no-roofline", "--full"], env=env, capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 128 and d["config"]["comm_dtype"] == "fp32" and d["config"]["grad_segments"] >= 2
    assert d["value"] > 0 and d["gradient_exchange"]["world"] == 2
