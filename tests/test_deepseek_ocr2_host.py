"""CPU: the host side of the DeepSeek-OCR-2 decoder -- config defaults, loader stacking, the shared MLP's pseudo-expert split, the
prompt layout of tokenize_prompt (deepseek-ocr2-mlx/src/lib.rs:791-870) with a stub tokenizer, is_repeating (:675-698) and the
repetition penalty's window (:631-660)."""
import numpy as np
import pytest

import deepseek_moe_rule as dr


@pytest.fixture(scope="module")
def mods(omx):
    from ominix_mlx_amd import deepseek_ocr2, engine, loader, moe
    return deepseek_ocr2, engine, loader, moe


def test_config_defaults(mods):
    _, _, loader, _ = mods
    a = loader.deepseek_ocr2_args({})
    assert (a["hidden_size"], a["num_hidden_layers"], a["num_attention_heads"], a["num_key_value_heads"], a["head_dim"]) == (1280, 12, 10, 10, 128)
    assert (a["intermediate_size"], a["vocab_size"], a["moe_intermediate_size"], a["num_experts"], a["num_experts_per_tok"]) == (6848, 129280, 896, 64, 6)
    assert (a["n_shared_experts"], a["first_k_dense_replace"], a["routed_scaling_factor"], a["norm_topk_prob"]) == (2, 1, 1.0, False)
    assert a["moe_mode"] == "deepseek" and a["qk_norm"] is False and a["rope_theta"] == 10000.0 and a["rms_norm_eps"] == 1e-6
    b = loader.deepseek_ocr2_args({"hidden_size": 256, "num_attention_heads": 2, "routed_scaling_factor": 2.5, "norm_topk_prob": True})
    assert (b["head_dim"], b["routed_scaling_factor"], b["norm_topk_prob"]) == (128, 2.5, True)
    c = loader.deepseek_ocr2_config({})
    assert (c["bos_token_id"], c["eos_token_id"], c["max_position_embeddings"], c["topk_method"]) == (0, 1, 8192, "greedy")
    with pytest.raises(ValueError, match="MLA"):
        loader.deepseek_ocr2_args({"use_mla": True})


def test_expected_shapes_follow_the_layer_plan(mods):
    _, engine, loader, _ = mods
    a = loader.deepseek_ocr2_args({})
    c = engine.Qwen3Config(a["hidden_size"], a["num_hidden_layers"], a["intermediate_size"], 10, 10, 128, a["vocab_size"])
    c.num_experts, c.num_experts_per_tok, c.moe_intermediate_size, c.moe_mode = 64, 6, 896, engine.MOE_MODES["deepseek"]
    c.tp_size, c.ep_size = 1, 1
    shape = lambda n: engine.expected_shape(c, n, None, engine.DeepseekPlan(1, 2, 1.0))
    assert engine.expected_shape(c, "model.layers.0.mlp.gate.weight") == (64, 1280)          # without a plan every layer routes
    assert shape("model.layers.0.mlp.gate_proj.weight") == (6848, 1280) and shape("model.layers.0.mlp.gate.weight") is None
    assert shape("model.layers.1.mlp.gate_proj.weight") is None and shape("model.layers.1.mlp.gate.weight") == (64, 1280)
    assert shape("model.layers.11.mlp.switch_mlp.down_proj.weight") == (64, 1280, 896)
    assert shape("model.layers.3.mlp.shared_experts.up_proj.weight") == (1792, 1280)
    assert shape("model.layers.3.mlp.shared_experts.down_proj.weight") == (1280, 1792)
    assert shape("model.layers.0.mlp.shared_experts.down_proj.weight") is None


def test_loader_stacks_the_per_expert_keys(mods):
    _, _, loader, _ = mods
    g = np.random.default_rng(3)
    w = {"model.layers.0.mlp.gate_proj.weight": g.standard_normal((8, 4)).astype(np.float32),
         "model.layers.1.mlp.gate.weight": g.standard_normal((3, 4)).astype(np.float32),
         "model.layers.1.mlp.shared_experts.up_proj.weight": g.standard_normal((4, 4)).astype(np.float32),
         "model.sam_model.pos_embed": np.zeros(2, np.float32)}
    for e in range(3):
        for proj, shp in (("gate_proj", (2, 4)), ("up_proj", (2, 4)), ("down_proj", (4, 2))):
            w[f"model.layers.1.mlp.experts.{e}.{proj}.weight"] = g.standard_normal(shp).astype(np.float32)
    out = loader.stack_deepseek_experts(w, 2, 3)
    assert out["model.layers.1.mlp.switch_mlp.gate_proj.weight"].shape == (3, 2, 4)
    assert out["model.layers.1.mlp.switch_mlp.down_proj.weight"].shape == (3, 4, 2)
    np.testing.assert_array_equal(out["model.layers.1.mlp.switch_mlp.up_proj.weight"][2], w["model.layers.1.mlp.experts.2.up_proj.weight"])
    assert not any(".experts." in k for k in out)
    for k in ("model.layers.0.mlp.gate_proj.weight", "model.layers.1.mlp.gate.weight", "model.layers.1.mlp.shared_experts.up_proj.weight",
              "model.sam_model.pos_embed"):
        assert out[k] is w[k]
    assert loader.stack_deepseek_experts(out, 2, 3).keys() == out.keys()          # already stacked: passes through
    del w["model.layers.1.mlp.experts.1.up_proj.weight"]
    with pytest.raises(KeyError, match="WeightNotFound"):
        loader.stack_deepseek_experts(w, 2, 3)


def test_pseudo_expert_split_of_the_shared_mlp(mods):
    _, _, _, moe = mods
    _, _, _, _, sh = dr.weights_for(4, 64, 64, 2, 51)
    pg, pu, pd = moe.split_shared_mlp(*sh, 2)
    assert pg.shape == (2, 64, 64) and pd.shape == (2, 64, 64)
    x = dr.rows_for(5, 64, 52)
    whole = dr.mlp(x, *sh)
    parts = sum(dr.mlp(x, pg[i], pu[i], pd[i]) for i in range(2))
    assert np.abs(whole - parts).max() <= 1e-13 * np.abs(whole).max()


class StubTokenizer:
    """one id per character, offset so that no id collides with BOS / the image id"""
    def encode(self, text, add_special_tokens=False):
        assert add_special_tokens is False
        return [1000 + ord(ch) for ch in text]


def test_tokenize_prompt_layout(mods):
    d, _, _, _ = mods
    tok, enc = StubTokenizer(), lambda s: [1000 + ord(ch) for ch in s]
    # with <image>, no crops: 1024 px global view -> 16 x 16 placeholders + the separator
    ids, mask = d.tokenize_prompt(tok, "<image>\nFree OCR.", True, 1024, 640, (1, 1))
    pre, post = enc("<|User|>: "), enc("\nFree OCR.\n\n<|Assistant|>:")
    assert ids == [0] + pre + [d.IMAGE_TOKEN_ID] * 257 + post
    assert mask == [False] * (1 + len(pre)) + [True] * 257 + [False] * len(post)
    assert d.image_span(mask) == (1 + len(pre), 257)
    # with crops: (2, 3) tiles of 640 px -> 100 placeholders each, behind the global block and the separator
    ids2, mask2 = d.tokenize_prompt(tok, "a<image>b<image>c", True, 1024, 640, (2, 3))
    assert sum(mask2) == 256 + 1 + 6 * 100 == d.image_token_count(1024, 640, (2, 3))
    assert ids2[-len(enc("b<image>c\n\n<|Assistant|>:")):] == enc("b<image>c\n\n<|Assistant|>:")     # a second <image> stays text
    assert ids2[0] == 0 and not mask2[0]
    # without an image, or without a placeholder: the frame as text
    for has_image, prompt in ((False, "<image>hello"), (True, "hello")):
        ids3, mask3 = d.tokenize_prompt(tok, prompt, has_image, 1024, 640, (1, 1))
        assert ids3 == [0] + enc(f"<|User|>: {prompt}\n\n<|Assistant|>:") and not any(mask3)
        assert d.image_span(mask3) == (0, 0)
    with pytest.raises(Exception, match="contiguous"):
        d.image_span([False, True, False, True])
    # the id sequence counts global + separator + crops; encode_image's rows come crops first (row_plan): same total
    plan = d.row_plan(1024, 640, 6)
    assert plan[0][0] == "crop0" and plan[-1] == ("separator", 856, 1) and plan[-1][1] + 1 == sum(mask2)


def test_is_repeating(mods):
    d, _, _, _ = mods
    four = [5, 6, 7, 8]
    assert d.is_repeating(four * 3)                         # 12 tokens: n = 4 three times
    assert not d.is_repeating((four * 3)[1:])               # 11 tokens: too short to look
    assert not d.is_repeating([9] + four * 2 + [5, 6, 7, 9])
    assert d.is_repeating([1, 2, 3] + four * 3)
    gram = list(range(100, 132))                            # n = 32, the largest
    assert d.is_repeating(gram * 3) and not d.is_repeating(gram * 2 + gram[:-1] + [7])
    big = list(range(200, 233))                             # n = 33 is not looked for
    assert not d.is_repeating(big * 3)
    assert d.is_repeating([3] * 12)                         # a single token repeating is a 4-gram repeating


def test_penalty_window_and_penalty(mods):
    d, _, _, _ = mods
    gen = [4, 9, 4, 7, 9, 2]
    assert d.penalty_window(gen, 0) == [4, 9, 7, 2]
    assert d.penalty_window(gen, 6) == [4, 9, 7, 2] and d.penalty_window(gen, 20) == [4, 9, 7, 2]
    assert d.penalty_window(gen, 3) == [7, 9, 2]            # the last three only: token 4 is forgotten
    assert d.penalty_window([], 3) == []
    logits = np.array([1.0, -1.0, 2.0, 0.0, -4.0], np.float32)
    out = d.penalize(logits, [0, 1, 3, 99], 2.0)
    np.testing.assert_array_equal(out, np.array([0.5, -2.0, 2.0, 0.0, -4.0], np.float32))
    np.testing.assert_array_equal(logits, np.array([1.0, -1.0, 2.0, 0.0, -4.0], np.float32))
