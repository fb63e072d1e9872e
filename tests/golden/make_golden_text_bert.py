"""Golden of the reference's TextBert (models/mmf_m4c.py:258-279): tests/golden/G18_text_bert.npz.

Follows make_golden.py's recipe (and imports its helpers): the installed transformers' ``BertEmbeddings`` + ``BertEncoder`` on
a stand-in ``self``, run through the reference's unbound ``TextBert.forward`` as G13 does for ``MMT`` -- ``TextBert.__init__``
itself does not run under transformers 5 (init_weights API drift).  Evaluation mode, so no dropout.  Stored: the inputs, the
weights, the output, every parameter gradient and the ``state_dict`` key list.  Needs the reference tree and transformers;
the tests read only the .npz.

    python tests/golden/make_golden_text_bert.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402

CFG = dict(vocab_size=37, hidden_size=48, num_hidden_layers=2, num_attention_heads=4, intermediate_size=96,
           max_position_embeddings=16)
EMBEDDINGS_BAR = 4.8e-7  # 4 ulp of fp32 at |y| <= 1: the restated sum differs from the library's in association only


def main():
    import transformers
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings, BertEncoder
    cfg = BertConfig(**CFG)
    torch.manual_seed(1801)
    holder = torch.nn.Module()
    holder.embeddings, holder.encoder = BertEmbeddings(cfg), BertEncoder(cfg)
    holder.config = cfg
    with torch.no_grad():
        for n_, p_ in holder.named_parameters():
            if n_.endswith("bias"):
                p_.normal_(0, 0.1)
            elif "LayerNorm.weight" in n_:
                p_.uniform_(0.5, 1.5)
    # repeated ids within and across samples, id 0 (the table's padding row) and id 36 (the last row); sample 1 is padding
    # (id 0) and masked from position 6
    tokens = torch.tensor([[5, 7, 5, 36, 1, 0, 12, 7, 30],
                           [7, 36, 2, 9, 5, 11, 0, 0, 0],
                           [20, 20, 20, 3, 36, 8, 1, 7, 4]])
    mask = torch.zeros(3, 1, 1, 9)
    mask[1, ..., 6:] = -10e4
    c = G.Case("G18_text_bert")
    c.meta.update(cfg=dict(CFG, layer_norm_eps=cfg.layer_norm_eps, type_vocab_size=cfg.type_vocab_size,
                           pad_token_id=cfg.pad_token_id), transformers=transformers.__version__)
    G.run_with_grads(c, holder, {"tokens": tokens, "mask": mask},
                     lambda mod, ins: {"out": G.R_m4c.TextBert.forward(mod, ins["tokens"], ins["mask"])}, [])
    c.meta["state_dict_keys"] = {k: list(v.shape) for k, v in holder.state_dict().items()}
    # the installed BertEmbeddings IS LN(word[tok] + pos[:T] + type[0]) (no token types, no position ids passed)
    e = holder.embeddings
    with torch.no_grad():
        x = e.word_embeddings.weight[tokens] + e.position_embeddings.weight[:9] + e.token_type_embeddings.weight[0]
        mine = torch.nn.functional.layer_norm(x, (48,), e.LayerNorm.weight, e.LayerNorm.bias, cfg.layer_norm_eps)
        err = (mine - e(tokens)).abs().max().item()
    assert err <= EMBEDDINGS_BAR, err
    c.meta["embeddings_restatement_error"] = err
    c.add("out", "embeddings", e(tokens))
    p = c.save()
    print(f"{c.name}: {os.path.getsize(p)} B, {len(c.arrays)} arrays; embeddings restatement error {err:.2e}")


if __name__ == "__main__":
    main()
