"""Autoregressive decoding over more keys than one window of the single-query attention kernel (512).

* A stateful Decoder over 617 encoder positions (577 ViT patches at 384 pixels + 40 question tokens), beams 3 and 5: every
  step's attentions are attn_decode_kernel launches (the windowed form for the encoder attention, shared by the beams of a
  sample), the encoder K / V are projected once per encoder tensor, and the steps equal the teacher-forced full forward.
* Beam search over 617 positions against the oracle's search, as test_blocks_gpu.test_beam_search_decode_matches_oracle.
* The whole decode replayed from one hipGraph equals the eager decode, beams 1, 3 and 5.
* A self-attention cache whose prefix crosses 512 positions against the full causal forward.
"""
import pytest
import torch

from test_blocks_gpu import BF16, DEV, F32, _cfg, _replay_search_choices, rel_l2

pytestmark = pytest.mark.gpu

NE = 617


@pytest.fixture(params=[F32, BF16], ids=["fp32", "bf16"])
def mode(request):
    import openvivqa_amd as A
    A.set_compute_dtype(request.param)
    yield request.param
    A.set_compute_dtype(BF16)


def _vocab(max_len, size):
    class Vocab:
        max_answer_length, padding_idx, bos_idx, eos_idx = max_len, 0, 1, 2

        def __len__(self):
            return size
    return Vocab()


def _decoder_cfg(layers):
    from openvivqa_amd.config import ConfigNode
    return ConfigNode(dict(
        ARCHITECTURE="Decoder", D_MODEL=512, LAYERS=layers,
        ATTENTION=dict(SELF_ATTENTION=_cfg(can_be_stateful=True), ENC_ATTENTION=_cfg()),
        TEXT_EMBEDDING=dict(ARCHITECTURE="UsualEmbedding", D_MODEL=512, D_EMBEDDING=300, WORD_EMBEDDING=None,
                            WORD_EMBEDDING_CACHE=None, DROPOUT=0.1)))


def _encoder_features(b_s, seed):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(b_s, NE, 512, generator=g)
    enc[1, 530:] = 0  # a padded sample: its last window of keys is masked in part
    return enc


@pytest.mark.parametrize("beam", [3, 5])
def test_stateful_decoder_over_617_encoder_positions(beam, mode):
    """The steps against the ORACLE decoder's teacher-forced forward (fp32, CPU) on the same weights, under the bars of
    test_decoder_config5_shapes' stateful decoding (rel-L2 1e-4 fp32, 1e-2 bf16); in bf16 also against this package's own
    full forward (the fp32 parity mode's general attention kernel does not hold 617 keys)."""
    import oracle as O
    import openvivqa_amd.modules as M
    from openvivqa_amd import _lib
    from openvivqa_amd.utils import generate_padding_mask
    torch.manual_seed(5)
    T, b_s, L = 6, 3, 2
    orc, dec = O.OracleDecoder(_decoder_cfg(L), _vocab(T, 60)), M.Decoder(_decoder_cfg(L), _vocab(T, 60))
    dec.load_state_dict(orc.state_dict(), strict=False)
    orc.eval()
    dec = dec.to(DEV).eval()
    enc_cpu = _encoder_features(b_s, 3)
    enc = enc_cpu.to(DEV)
    emask = generate_padding_mask(enc, 0)
    R = b_s * beam
    toks = torch.randint(3, 60, (R, T), generator=torch.Generator().manual_seed(6)).to(DEV)
    tname = "float" if mode == F32 else "__bf16"
    # (three samples leave most CUs idle: five beams then run as workgroups of their own, csrc/attention_decode.hip)
    shared = beam if beam <= 4 else 1
    steps, projected = [], []
    with torch.no_grad():
        with dec.statefulness(R):
            for t in range(T):
                _lib.launch_log_clear()
                steps.append(dec(toks[:, t:t + 1], enc, emask, encoder_group=beam))
                log = _lib.launch_log()
                # per layer: the self-attention over the cache (a few keys, a row each) and the encoder attention
                # (617 keys: the windowed form, three beams of a sample sharing one read)
                assert [e for e in log if "attn_" in e] == [f"attn_decode_kernel<{tname},64,1,false,false>",
                                                            f"attn_decode_kernel<{tname},64,{shared},true,true>"] * L, (t, log)
                projected.append([layer.enc_attn._enc[1] for layer in dec.layers])
                # no re-projection: the very tensors of step 0
                assert all(a is b for a, b in zip(projected[t], projected[0]))
            assert tuple(projected[0][0].shape) == (b_s, NE, 1024)  # one row per SAMPLE, K | V packed
        ref = orc(toks.cpu(), enc_cpu.repeat_interleave(beam, 0), O.padding_mask(enc_cpu, 0).repeat_interleave(beam, 0))
        assert rel_l2(torch.cat(steps, 1), ref) < (1e-4 if mode == F32 else 1e-2)
        if mode == BF16:
            full = dec(toks, enc.repeat_interleave(beam, 0), emask.repeat_interleave(beam, 0))
            assert rel_l2(torch.cat(steps, 1), full) < 1e-2


@pytest.mark.parametrize("beam", [3, 5])
def test_beam_search_over_617_positions_matches_oracle(beam, mode):
    """fp32: the tokens of the oracle's search and its log-probabilities (1e-3).  bf16: near-ties may flip a beam in a
    free-running search, so the decoder is driven through the oracle's choices and every step's log-probabilities are
    compared (1e-2), as test_beam_search_decode_matches_oracle does."""
    import oracle as O
    import openvivqa_amd.modules as M
    from openvivqa_amd.beam import GraphedBeamSearch
    vocab = _vocab(8, 60)
    cfg = _decoder_cfg(2)
    torch.manual_seed(12)
    o, h = O.OracleDecoder(cfg, vocab), M.Decoder(cfg, vocab)
    with torch.no_grad():
        o.fc.weight.mul_(6.0)  # spread the vocabulary distribution: fewer near-ties between candidates
    h.load_state_dict(o.state_dict(), strict=False)
    o.eval()
    h = h.to(DEV).eval()
    b_s, T = 4, 8
    enc = _encoder_features(b_s, 4)
    emask = O.padding_mask(enc, 0)
    search = GraphedBeamSearch(h, b_s, T, 1, 2, beam)
    out_h, lp_h = search(enc.to(DEV), emask.to(DEV), use_graph=False)
    trace = []
    out_o, lp_o = O.oracle_generate(o, enc, emask, 1, 2, beam, max_len=T, trace=trace)
    if mode == F32:
        assert torch.equal(out_h.cpu(), out_o), (out_h, out_o)
        assert rel_l2(lp_h, lp_o) < 1e-3
    _replay_search_choices(h, enc, emask, trace, beam, 1, 1e-3 if mode == F32 else 1e-2, f"beam-replay-617[{beam}]")


@pytest.mark.parametrize("beam", [1, 3, 5])
def test_graphed_decode_equals_eager_over_617_positions(beam):
    """Tokens equal and log-probabilities bit-equal, as test_graphed_beam_search_equals_eager asserts at 50 positions."""
    import openvivqa_amd as A
    import openvivqa_amd.modules as M
    from openvivqa_amd.beam import GraphedBeamSearch
    from openvivqa_amd.utils import generate_padding_mask
    A.set_compute_dtype(BF16)
    torch.manual_seed(21)
    dec = M.Decoder(_decoder_cfg(3), _vocab(10, 200)).to(DEV).eval()
    with torch.no_grad():
        dec.fc.weight.mul_(6.0)
    b_s = 6
    search = GraphedBeamSearch(dec, b_s, 10, 1, 2, beam)
    g = torch.Generator().manual_seed(2)
    for trial in range(3):
        enc = torch.randn(b_s, NE, 512, generator=g)
        enc[trial % b_s, 540:] = 0
        enc = enc.to(DEV)
        mask = generate_padding_mask(enc, 0)
        out_e, lp_e = search(enc, mask, use_graph=False)
        out_g, lp_g = search(enc, mask)
        assert search.graph is not None
        assert torch.equal(out_g, out_e) and torch.equal(lp_g, lp_e), trial
    assert out_g.shape == (b_s, 10)


def _mha_fp64(m, x, mask):
    """The module's computation in fp64 torch math on its own (fp32 master) weights: LN(x + fc_o(attention))."""
    a, ln = m.attention, m.layer_norm
    xd = x.double()
    lin = lambda l, t: t @ l.weight.double().t() + l.bias.double()
    B, N, _ = x.shape
    q, k, v = (lin(l, xd).view(B, N, a.h, a.d_k).transpose(1, 2) for l in (a.fc_q, a.fc_k, a.fc_v))
    p = torch.softmax(q @ k.transpose(-1, -2) / a.d_k ** 0.5 + mask.double(), -1)
    o = lin(a.fc_o, (p @ v).transpose(1, 2).reshape(B, N, a.h * a.d_k))
    return torch.nn.functional.layer_norm(xd + o, (x.shape[-1],), ln.weight.double(), ln.bias.double(), ln.eps)


def test_self_attention_prefix_crosses_512(mode):
    """A stateful MultiHeadAttention is teacher-forced over a prefix in chunks (the general kernel on a grown cache; the fp32
    parity mode's general kernel holds 303 keys, so its prefix ends at 300), then fed single positions up to 540: the
    in-place cache is re-seated and doubled when full (DECODE_CAPACITY) and the single-query kernel runs over the cached
    keys, windowed past 512.  Against the full causal computation in fp64 (bf16 also against the module's full forward)."""
    import openvivqa_amd.modules as M
    from openvivqa_amd import _lib
    from openvivqa_amd.utils import generate_sequential_mask
    torch.manual_seed(9)
    m = M.MultiHeadAttention(_cfg(can_be_stateful=True)).to(DEV).eval()
    B, N, CH = 3, 540, ((0, 150, 300) if mode == F32 else (0, 200, 500))
    x = torch.randn(B, N, 512, generator=torch.Generator().manual_seed(8)).to(DEV)
    causal = generate_sequential_mask(N, device=DEV)
    tname = "float" if mode == F32 else "__bf16"
    bar = 1e-4 if mode == F32 else 1e-2
    outs = []
    with torch.no_grad():
        ref = _mha_fp64(m, x, causal)
        with m.statefulness(B):
            for a, b in zip(CH[:-1], CH[1:]):
                outs.append(m(x[:, a:b], x[:, a:b], x[:, a:b], causal[:, :, a:b, :b]))
            for t in range(CH[-1], N):
                _lib.launch_log_clear()
                outs.append(m(x[:, t:t + 1], x[:, t:t + 1], x[:, t:t + 1], torch.zeros(1, 1, 1, t + 1, device=DEV)))
                att = [e for e in _lib.launch_log() if "attn_" in e]
                assert att == [f"attn_decode_kernel<{tname},64,1,true,{'true' if t + 1 > 512 else 'false'}>"], (t, att)
            assert tuple(m.running_keys.shape) == (B, N, 512)
            assert m._kv[0].shape[1] >= N and m.running_keys.data_ptr() == m._kv[0].data_ptr()  # still the in-place cache
        got = torch.cat(outs, 1)
        assert got.shape == ref.shape
        assert rel_l2(got, ref) < bar and rel_l2(got[:, 512:], ref[:, 512:]) < bar
        if mode == BF16:
            full = m(x, x, x, causal)
            assert rel_l2(got, full) < bar and rel_l2(got[:, 512:], full[:, 512:]) < bar
