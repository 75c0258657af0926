"""CPU-only: the host half of Moxin-VLM (ominix_mlx_amd/moxin_vlm.py): the checkpoint's name mapping, config defaults, the prompt's
layout and the refusals that need no device."""
import json

import numpy as np
import pytest


def _names(dino_p, sig_p, llm_p, proj_names, gamma, reg):
    t = {}
    for p, d, ls in ((dino_p, 8, True), (sig_p, 12, False)):
        t[f"{p}.patch_embed.proj.weight"] = np.zeros((d, 3, 2, 2), np.float32)
        t[f"{p}.pos_embed"] = np.zeros((1, 4, d), np.float32)
        t[f"{p}.blocks.0.attn.qkv.weight"] = np.full((3 * d, d), 0.5, np.float32)
        if ls:
            t[f"{p}.blocks.0.ls1.{gamma}"] = np.ones(d, np.float32)
            t[f"{p}.{reg}"] = np.zeros((1, 4, d), np.float32)
    for i, n in enumerate(proj_names):
        t[f"projector.{n}.weight"] = np.full((4, 4), float(i), np.float32)
        t[f"projector.{n}.bias"] = np.zeros(4, np.float32)
    t[f"{llm_p}.model.embed_tokens.weight"] = np.zeros((16, 4), np.float32)
    t[f"{llm_p}.model.layers.0.self_attn.q_proj.weight"] = np.zeros((4, 4), np.float32)
    t[f"{llm_p}.lm_head.weight"] = np.zeros((16, 4), np.float32)
    return t


@pytest.mark.parametrize("dino_p,sig_p,llm_p,proj_names,gamma,reg", [
    ("vision_backbone.featurizer", "vision_backbone.fused_featurizer", "language_model", ("fc1", "fc2", "fc3"), "gamma", "reg_token"),
    ("vision_backbone.featurizer.0", "vision_backbone.featurizer.1", "llm_backbone.llm", ("0", "2", "4"), "scale_factor", "register_tokens")])
def test_the_name_mapping_of_a_tiny_checkpoint(omx, tmp_path, dino_p, sig_p, llm_p, proj_names, gamma, reg):
    """both prefix conventions (lib.rs:626-643), both projector spellings (projector.rs:60-101); LayerScale and register keys keep
    their spelling (the tower takes either)"""
    from ominix_mlx_amd import loader, moxin_vlm
    loader.write_safetensors(str(tmp_path / "model.safetensors"), _names(dino_p, sig_p, llm_p, proj_names, gamma, reg))
    (tmp_path / "config.json").write_text(json.dumps({"text_config": {"hidden_size": 4, "num_hidden_layers": 1, "vocab_size": 16},
                                                      "image_token_index": 15}))
    config, dino, siglip, proj, text, prefixes = moxin_vlm.read_checkpoint(str(tmp_path))
    assert prefixes == dict(dino=dino_p, siglip=sig_p, llm=llm_p)
    assert sorted(dino) == sorted(["patch_embed.proj.weight", "pos_embed", "blocks.0.attn.qkv.weight", f"blocks.0.ls1.{gamma}", reg])
    assert sorted(siglip) == sorted(["patch_embed.proj.weight", "pos_embed", "blocks.0.attn.qkv.weight"])
    assert dino["pos_embed"].shape == (1, 4, 8) and siglip["pos_embed"].shape == (1, 4, 12)
    assert sorted(proj) == ["fc1.bias", "fc1.weight", "fc2.bias", "fc2.weight", "fc3.bias", "fc3.weight"]
    assert [float(proj[f"fc{i + 1}.weight"][0, 0]) for i in range(3)] == [0.0, 1.0, 2.0]
    assert sorted(text) == ["lm_head.weight", "model.embed_tokens.weight", "model.layers.0.self_attn.q_proj.weight"]
    args = moxin_vlm.text_model_args(config)
    assert (args["hidden_size"], args["num_hidden_layers"], args["vocab_size"]) == (4, 1, 16)
    assert args["num_key_value_heads"] == 8 and args["rms_norm_eps"] == 1e-5 and args["rope_theta"] == 10000.0       # MistralConfig's defaults
    assert args["qk_norm"] is False and args["attention_bias"] is False and args["tie_word_embeddings"] is False


def test_config_defaults_are_mistral_7b(omx):
    from ominix_mlx_amd import moxin_vlm
    a = moxin_vlm.text_model_args({})
    assert (a["hidden_size"], a["num_hidden_layers"], a["num_attention_heads"], a["num_key_value_heads"], a["intermediate_size"],
            a["vocab_size"], a["head_dim"]) == (4096, 36, 32, 8, 14336, 32064, 128)


def test_a_missing_projector_matrix_is_named(omx):
    from ominix_mlx_amd import moxin_vlm
    t = _names("vision_backbone.featurizer", "vision_backbone.fused_featurizer", "language_model", ("fc1", "fc2", "fc3"), "gamma", "reg_token")
    del t["projector.fc2.weight"]
    with pytest.raises(omx.OmxError, match="WeightNotFound: projector.fc2.weight or projector.2.weight"):
        moxin_vlm.split_weights(t)


class Tok:
    def __init__(self, bos=True):
        self.bos = bos

    def encode(self, text, add_special_tokens=True):
        return ([1] if self.bos and add_special_tokens else []) + [10 + ord(c) % 100 for c in text]


def test_prompt_ids_layout(omx):
    """BOS, then the placeholder ids, then "In: {prompt}\\nOut:" """
    from ominix_mlx_amd import moxin_vlm
    ids = moxin_vlm.build_prompt_ids(Tok(), "hi", 256, 32000)
    body = [10 + ord(c) % 100 for c in "In: hi\nOut:"]
    assert ids.dtype == np.uint32 and ids.size == 1 + 256 + len(body)
    assert ids[0] == 1 and (ids[1:257] == 32000).all() and list(ids[257:]) == body
    assert moxin_vlm.placeholder_span(ids, 32000, 256) == 1


def test_placeholder_refusals(omx):
    from ominix_mlx_amd import moxin_vlm
    ids = moxin_vlm.build_prompt_ids(Tok(), "hi", 16, 99)
    with pytest.raises(omx.OmxError, match="holds 16 placeholder ids but the towers made 17 rows"):
        moxin_vlm.placeholder_span(ids, 99, 17)
    moved = np.concatenate([ids[:1], ids[17:18], ids[1:17], ids[18:]])
    with pytest.raises(omx.OmxError, match="not one span directly behind the BOS id"):
        moxin_vlm.placeholder_span(moved, 99, 16)
    split = ids.copy()
    split[5], split[20] = split[20], split[5]
    with pytest.raises(omx.OmxError, match="not one span"):
        moxin_vlm.placeholder_span(split, 99, 16)


def test_image_refusals_need_no_device(omx):
    from ominix_mlx_amd import vision
    with pytest.raises(omx.OmxError, match="ShapeMismatch: image has shape"):
        vision.image_array(np.zeros((224, 224), np.float32), 224)
    with pytest.raises(omx.OmxError, match="image dtype int32"):
        vision.image_array(np.zeros((4, 4, 3), np.int32), 4)
    a = vision.image_array(np.full((4, 4, 3), 255, np.uint8), 4)
    assert a.dtype == np.float32 and (a == 1.0).all()
