"""Plain-torch TextBert (models/mmf_m4c.py:258-279): the reference of the TextBert / MMF_M4C tests.

The embeddings arithmetic is written out here -- LN(word[tok] + token_type[0] + position[:T]), dropout -- and the layers are
the oracle's ``OracleBertEncoder``; parameter names are transformers'.  Pinned against the installed transformers through
tests/golden/G18_text_bert.npz (tests/test_text_bert_cpu.py)."""
import torch
from torch import nn


class RefBertEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d = cfg.hidden_size
        self.word_embeddings = nn.Embedding(cfg.vocab_size, d, padding_idx=getattr(cfg, "pad_token_id", 0))
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, d)
        self.token_type_embeddings = nn.Embedding(getattr(cfg, "type_vocab_size", 2), d)
        self.LayerNorm = nn.LayerNorm(d, eps=cfg.layer_norm_eps)
        self.dropout = nn.Dropout(cfg.hidden_dropout_prob)

    def forward(self, ids):
        T = ids.shape[1]
        x = self.word_embeddings(ids) + self.token_type_embeddings.weight[0] + self.position_embeddings.weight[:T]
        return self.dropout(self.LayerNorm(x))


class RefTextBert(nn.Module):
    def __init__(self, cfg):
        import oracle as O
        super().__init__()
        self.embeddings = RefBertEmbeddings(cfg)
        self.encoder = O.OracleBertEncoder(cfg)

    def forward(self, txt_inds, txt_mask):
        return self.encoder(self.embeddings(txt_inds), txt_mask, head_mask=[None] * len(self.encoder.layer))[0]
