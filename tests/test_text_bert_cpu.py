"""TextBert and the whole-model ``MMF_M4C`` without a GPU: the plain-torch reference of the GPU tests against the golden of
the installed transformers (tests/golden/G18_text_bert.npz), the registry entry and its state dict, the local
LOAD_PRETRAINED loader, and the two C entry points' signatures."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from golden_cases import GOLDEN_DIR, FakeVocab, load_case
from test_m4c_train_cpu import reference_keys
from test_oracle_golden import FWD_TOL, GRAD_TOL, _close
from text_bert_ref import RefTextBert

from openvivqa_amd import _lib
from openvivqa_amd.config import get_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_cfg(meta):
    c = meta["cfg"]
    return SimpleNamespace(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, **c)


def test_text_bert_ref_matches_transformers_golden():
    """Output <= 1e-6, every parameter gradient <= 1e-5 (the bars of tests/test_oracle_golden.py); the generator itself
    checked that the installed BertEmbeddings is LN(word[tok] + pos[:T] + type[0]) to 4.8e-7."""
    case = load_case("G18_text_bert")
    assert case.meta["embeddings_restatement_error"] <= 4.8e-7
    assert case.meta["cfg"]["vocab_size"] == 37 and tuple(case.inputs["tokens"].shape) == (3, 9)
    tok = case.inputs["tokens"]
    assert (tok == 0).any() and (tok == 36).any() and bool((case.inputs["mask"][1, 0, 0, 6:] == -10e4).all())
    ref = RefTextBert(golden_cfg(case.meta)).eval()
    missing, unexpected = ref.load_state_dict(case.w, strict=False)
    assert missing == [] and unexpected == []
    assert sorted(case.meta["state_dict_keys"]) == sorted(ref.state_dict())
    _close(ref.embeddings(tok), case.out["embeddings"], FWD_TOL, "embeddings")
    out = ref(tok, case.inputs["mask"])
    _close(out, case.out["out"], FWD_TOL, "out")
    (out * case.lw["out"]).sum().backward()
    grads = dict(ref.named_parameters())
    assert set(case.gw) | set(case.meta["grad_none"]) == set(grads)
    for k, g in case.gw.items():
        _close(grads[k].grad, g, GRAD_TOL, f"gw/{k}")
    assert float(grads["embeddings.word_embeddings.weight"].grad[0].abs().max()) == 0.0  # the table's padding row


def _m4c_config(**text_bert):
    cfg = get_config(os.path.join(GOLDEN_DIR, "G18_reference_configs.json"))["mmf_m4c"].MODEL.clone()
    cfg.DEVICE = "cpu"
    cfg.TEXT_BERT.LOAD_PRETRAINED = False
    for k, v in text_bert.items():
        cfg.TEXT_BERT[k] = v
    return cfg


def text_bert_keys(layers, hidden, vocab, positions=512):
    """'text_bert.' + G18's key list at other sizes: the golden's own sizes (48 / 96 / 37 / 16) replaced."""
    dims = {48: hidden, 96: 4 * hidden, 37: vocab, 16: positions}
    out = {}
    for k, shape in load_case("G18_text_bert").meta["state_dict_keys"].items():
        m = re.match(r"encoder\.layer\.(\d+)\.(.*)", k)
        names = [k] if m is None else ([f"encoder.layer.{i}.{m.group(2)}" for i in range(layers)] if m.group(1) == "0" else [])
        for n in names:
            out["text_bert." + n] = tuple(dims.get(s, s) for s in shape)
    return out


def test_mmf_m4c_is_registered_and_has_the_reference_state_dict():
    from openvivqa_amd.builders.model_builder import META_ARCHITECTURE, build_model
    from openvivqa_amd.models import MMF_M4C
    assert META_ARCHITECTURE.get("MMF_M4C") is MMF_M4C
    cfg = _m4c_config(NUM_HIDDEN_LAYERS=3)  # (12 in the YAML: 3 here keep the CPU test quick; the keys repeat per layer)
    assert cfg.ARCHITECTURE == "MMF_M4C" and cfg.TEXT_BERT.NUM_ATTENTION_HEADS == 12 and cfg.TEXT_BERT.FREEZE_WEIGHTS
    vocab = FakeVocab()
    m = build_model(cfg, vocab)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = dict(reference_keys(len(vocab)))
    want.update(text_bert_keys(3, 768, 30522))
    assert got == want
    assert isinstance(m.text_bert_out_linear, torch.nn.Identity)
    assert m.text_bert.encoder.layer[0].heads == cfg.MMT.NUM_ATTENTION_HEADS == 8  # mmf_m4c.py:51, not TEXT_BERT's 12
    assert all(p.requires_grad for p in m.parameters())  # FREEZE_WEIGHTS is ignored, as the reference ignores it
    e = m.text_bert.embeddings
    assert e.word_embeddings.padding_idx == 0 and float(e.word_embeddings.weight[0].detach().abs().max()) == 0.0
    assert abs(float(e.word_embeddings.weight[1:].detach().std()) - 0.02) < 1e-3 and e.LayerNorm.eps == 1e-12
    assert float(m.text_bert.encoder.layer[0].intermediate.dense.bias.detach().abs().max()) == 0.0
    # a checkpoint of an older transformers carries the position-id buffer: nothing missing, nothing unexpected
    ckpt = dict(m.state_dict())
    ckpt["text_bert.embeddings.position_ids"] = torch.arange(512)[None]
    ckpt["text_bert.embeddings.token_type_ids"] = torch.zeros(1, 512, dtype=torch.long)
    missing, unexpected = m.load_state_dict(ckpt, strict=False)
    assert missing == [] and unexpected == []
    m.load_state_dict(ckpt, strict=True)


def test_mmf_m4c_projects_text_bert_when_the_mmt_is_not_768_wide():
    from openvivqa_amd.builders.model_builder import build_model
    cfg = _m4c_config(NUM_HIDDEN_LAYERS=1, VOCAB_SIZE=50)
    cfg.MMT.HIDDEN_SIZE = 512
    vocab = FakeVocab()
    m = build_model(cfg, vocab)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = dict(reference_keys(len(vocab), d=512, ff=2048, ptr=768))
    want.update(text_bert_keys(1, 768, 50))
    want["text_bert_out_linear.weight"], want["text_bert_out_linear.bias"] = (512, 768), (512,)
    assert got == want


def test_load_pretrained_reads_local_state_dicts_only(tmp_path, monkeypatch):
    """Prefix handling, layer truncation, the directory form, and the error for a name that is not a local path -- with
    every ``from_pretrained`` of transformers (if installed) made to raise if touched."""
    from openvivqa_amd.builders.model_builder import build_model
    from openvivqa_amd.models.mmf_m4c import text_bert_config
    from openvivqa_amd.modules.mmt import TextBert, load_text_bert_weights
    try:
        import transformers

        def boom(*a, **k):
            raise AssertionError("from_pretrained was called")
        monkeypatch.setattr(transformers.PreTrainedModel, "from_pretrained", classmethod(boom))
    except ImportError:
        pass
    torch.manual_seed(3)
    src = TextBert(text_bert_config(48, 4, 4, vocab_size=37))
    with torch.no_grad():
        for p in src.parameters():
            p.normal_()
    sd = {"bert." + k: v for k, v in src.state_dict().items()}
    sd["bert.pooler.dense.weight"], sd["cls.predictions.bias"] = torch.zeros(48, 48), torch.zeros(37)
    sd["bert.embeddings.position_ids"] = torch.arange(512)[None]
    torch.save(sd, tmp_path / "with_prefix.bin")
    torch.save({k: v for k, v in src.state_dict().items()}, tmp_path / "pytorch_model.bin")
    for path in (tmp_path / "with_prefix.bin", tmp_path):  # a file with the bert. prefix; a directory without
        dst = TextBert(text_bert_config(48, 2, 4, vocab_size=37))  # 2 of the 4 layers
        load_text_bert_weights(dst, str(path))
        want = {k: v for k, v in src.state_dict().items() if not re.match(r"encoder\.layer\.[23]\.", k)}
        got = dst.state_dict()
        assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    with pytest.raises(RuntimeError, match="bert-base-uncased.*supplied locally"):
        load_text_bert_weights(TextBert(text_bert_config(48, 1, 4, vocab_size=37)), "bert-base-uncased")
    cfg = _m4c_config(NUM_HIDDEN_LAYERS=1, VOCAB_SIZE=50)
    cfg.TEXT_BERT.LOAD_PRETRAINED = True  # the YAML's own values: PRETRAINED_NAME = "bert-base-uncased"
    with pytest.raises(RuntimeError, match="bert-base-uncased.*supplied locally"):
        build_model(cfg, FakeVocab())


def test_bert_embeddings_signatures_and_abi_version():
    assert _lib.ABI_VERSION == 12
    hdr = open(os.path.join(ROOT, "include", "ovqa_hip.h")).read()
    assert re.search(r"#define OVQA_ABI_VERSION 12\b", hdr)
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for name in ("ovqa_bert_embeddings_fwd", "ovqa_bert_embeddings_bwd"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            if "*" in arg:
                want.append(_lib._DP if "ovqa_dropout" in arg else C.c_void_p)
            else:
                want.append(kinds[arg.replace("const ", "").rsplit(" ", 1)[0]])
        assert _lib.SIGNATURES[name] == want, name
        fn = getattr(_lib.load(), name)  # raises if the library does not export it
        assert fn.argtypes == want and fn.restype == C.c_int
    assert re.search(r"BertEmbeddings\.forward as TextBert\.forward calls it,[^;]*mmf_m4c\.py:266-267", hdr, re.S)
