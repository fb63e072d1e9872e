"""M4CTrainModel's parameters are the reference MMF_M4C's (models/mmf_m4c.py:74-114, 367-380, 399-416 and MMT / HF
BertEncoder), minus the frozen text encoder's ``text_bert.*``: a reference checkpoint loads into it."""
import torch


def reference_keys(V, d=768, layers=4, ff=3072, obj_feat=1024, ocr_feat=812, ptr=768):
    """{name: shape} of MMF_M4C's state_dict without text_bert.* (text_bert_out_linear is nn.Identity at d = 768)."""
    ref = {}

    def linear(name, i, o):
        ref[name + ".weight"], ref[name + ".bias"] = (o, i), (o,)

    def ln(name):
        ref[name + ".weight"], ref[name + ".bias"] = (d,), (d,)
    linear("linear_obj_feat_to_mmt_in", obj_feat, d)
    linear("linear_obj_bbox_to_mmt_in", 4, d)
    ln("obj_feat_layer_norm")
    ln("obj_bbox_layer_norm")
    linear("linear_ocr_feat_to_mmt_in", ocr_feat, d)
    linear("linear_ocr_bbox_to_mmt_in", 4, d)
    ln("ocr_feat_layer_norm")
    ln("ocr_bbox_layer_norm")
    ln("ocr_text_layer_norm")
    p = "mmt.prev_pred_embeddings."
    ref[p + "position_embeddings.weight"] = (100, d)
    ref[p + "token_type_embeddings.weight"] = (5, d)
    for n in ("ans_layer_norm", "ocr_layer_norm", "emb_layer_norm"):
        ln(p + n)
    for i in range(layers):
        p = f"mmt.encoder.layer.{i}."
        for n in ("query", "key", "value"):
            linear(p + "attention.self." + n, d, d)
        linear(p + "attention.output.dense", d, d)
        ln(p + "attention.output.LayerNorm")
        linear(p + "intermediate.dense", d, ff)
        linear(p + "output.dense", ff, d)
        ln(p + "output.LayerNorm")
    linear("ocr_ptr_net.query", d, ptr)
    linear("ocr_ptr_net.key", d, ptr)
    linear("classifier", d, V)
    return ref


def test_m4c_train_model_state_dict_matches_reference_keys():
    from openvivqa_amd.models.mmf_m4c import M4CTrainModel
    m = M4CTrainModel(5000)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == reference_keys(5000)


def test_m4c_train_model_loads_a_reference_checkpoint_without_text_bert():
    from openvivqa_amd.models.mmf_m4c import M4CTrainModel
    g = torch.Generator().manual_seed(3)
    ckpt = {k: torch.randn(s, generator=g) for k, s in reference_keys(300).items()}
    ckpt["text_bert.embeddings.word_embeddings.weight"] = torch.zeros(10, 768)
    m = M4CTrainModel(300)
    missing, unexpected = m.load_state_dict(ckpt, strict=False)
    assert missing == [] and unexpected == ["text_bert.embeddings.word_embeddings.weight"]
    assert torch.equal(m.classifier.weight, ckpt["classifier.weight"])
