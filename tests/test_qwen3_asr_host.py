"""CPU: the host logic of ominix_mlx_amd/qwen3_asr.py -- config parsing, key splitting, the prompt template and the pad-count check,
the stop rule on a scripted fake model, EOS ids, and a safetensors round trip of a tiny checkpoint as far as it goes without a device."""
import json

import numpy as np
import pytest


@pytest.fixture
def qa(omx):
    from ominix_mlx_amd import qwen3_asr
    return qwen3_asr


def test_config_parsing_mirrors_the_reference(qa):
    nested = {"thinker_config": {"audio_config": {"d_model": 896, "encoder_layers": 18}, "text_config": {"hidden_size": 1024},
                                 "audio_token_id": 7, "audio_start_token_id": 8, "audio_end_token_id": 9},
              "support_languages": ["English", 3, "Chinese"], "quantization": {"group_size": 64, "bits": 8},
              "audio_token_id": 99}
    c = qa.Qwen3ASRConfig.from_config_json(nested)
    assert c.audio_config == {"d_model": 896, "encoder_layers": 18} and c.text_config == {"hidden_size": 1024}
    assert (c.audio_token_id, c.audio_start_token_id, c.audio_end_token_id) == (7, 8, 9)      # from thinker_config, not the top level
    assert c.support_languages == ["English", "Chinese"] and c.quantization == {"group_size": 64, "bits": 8}
    flat = qa.Qwen3ASRConfig.from_config_json({"audio_config": {"n_window": 50}, "audio_token_id": "x"})
    assert flat.audio_config == {"n_window": 50} and flat.text_config == {} and flat.quantization is None
    assert (flat.audio_token_id, flat.audio_start_token_id, flat.audio_end_token_id) == (151676, 151669, 151670)
    with pytest.raises(Exception, match="text_config lacks hidden_size"):
        flat.text_model_args()
    args = qa.Qwen3ASRConfig.from_config_json({"text_config": {"hidden_size": 128, "num_hidden_layers": 2, "intermediate_size": 256,
                                                               "num_attention_heads": 2, "vocab_size": 512},
                                               "quantization": {"bits": 4, "group_size": 64}}).text_model_args()
    assert args["head_dim"] == 64 and args["num_key_value_heads"] == 2 and args["tie_word_embeddings"] is True
    assert args["quantization"] == {"bits": 4, "group_size": 64}


def test_key_splitting(qa):
    w = {"audio_tower.conv2d1.weight": 1, "audio_tower.layers.0.fc1.bias": 2, "model.embed_tokens.weight": 3, "model.layers.0.mlp.up_proj.scales": 4,
         "lm_head.weight": 5, "something.else": 6}
    tower, text = qa.split_weights(w)
    assert tower == {"conv2d1.weight": 1, "layers.0.fc1.bias": 2}
    assert text == {"model.embed_tokens.weight": 3, "model.layers.0.mlp.up_proj.scales": 4, "lm_head.weight": 5}


def test_prompt_template_and_pad_count(qa, omx):
    assert qa.prompt_text(2, "English") == ("<|im_start|>system\n<|im_end|>\n<|im_start|>user\n<|audio_start|><|audio_pad|><|audio_pad|>"
                                            "<|audio_end|><|im_end|>\n<|im_start|>assistant\nlanguage English<asr_text>")
    assert qa.prompt_text(0, "Chinese").count("<|audio_pad|>") == 0 and qa.prompt_text(390, "x").count("<|audio_pad|>") == 390
    pad = 151676
    ids = [1, 2, 3, pad, pad, pad, 4, 5]
    assert qa.audio_span(ids, pad, 3) == 3
    with pytest.raises(omx.OmxError, match="holds 3 <.audio_pad.> ids but the tower made 4 rows"):
        qa.audio_span(ids, pad, 4)
    with pytest.raises(omx.OmxError, match="not one contiguous span"):
        qa.audio_span([1, pad, 2, pad, pad], pad, 3)

    class Tok:
        def encode(self, text, add_special_tokens=True):
            assert add_special_tokens is False
            return type("E", (), {"ids": [len(text), 5]})()
    np.testing.assert_array_equal(qa.encode(Tok(), "abc"), np.array([3, 5], np.uint32))


class Scripted:
    """a model that has been prefilled: decode(n) hands out the next n tokens of a script"""

    def __init__(self, script):
        self.script, self.at, self.calls = list(script), 0, []

    def decode(self, n):
        self.calls.append(n)
        out = (self.script + [0] * n)[self.at:self.at + n]
        self.at += n
        return np.array(out, np.uint32)


def reference_loop(tokens, max_tokens, eos):
    """model.rs:794-830, one token per turn"""
    out, recent, it = [], [], iter(tokens)
    tok = next(it)
    for _ in range(max_tokens):
        if tok in eos:
            break
        recent.append(tok)
        if len(recent) > 10:
            recent.pop(0)
        if len(recent) >= 10 and all(t == tok for t in recent):
            break
        out.append(tok)
        tok = next(it)
    return out


@pytest.mark.parametrize("chunk", [1, 4, 16])
def test_stop_rule(qa, chunk):
    eos = (900, 901)
    # EOS in the middle: not emitted, nothing after it
    assert qa.generate_ids(Scripted([11, 12, 900, 13]), 10, 50, eos, chunk) == [10, 11, 12]
    # the prompt's own first token is an EOS: nothing, and no decode step is asked for
    m = Scripted([1, 2, 3])
    assert qa.generate_ids(m, 901, 50, eos, chunk) == [] and m.calls == []
    # ten equal tokens in a row: nine are emitted, the tenth stops the loop
    assert qa.generate_ids(Scripted([7] * 30), 5, 50, eos, chunk) == [5] + [7] * 9
    assert qa.generate_ids(Scripted([7] * 30), 7, 50, eos, chunk) == [7] * 9
    # nine equal ones, another, nine again: no stop
    script = [7] * 8 + [8] + [7] * 9 + [900]
    assert qa.generate_ids(Scripted(script), 7, 50, eos, chunk) == [7] * 9 + [8] + [7] * 9
    # max_tokens
    assert qa.generate_ids(Scripted(list(range(100, 200))), 99, 5, eos, chunk) == [99, 100, 101, 102, 103]
    assert qa.generate_ids(Scripted([1]), 99, 0, eos, chunk) == []
    # and the loop is the reference's, turn for turn, on seeded scripts
    g = np.random.default_rng(chunk)
    for _ in range(50):
        script = [int(t) for t in g.choice([3, 3, 3, 3, 4, 900], size=60)]
        assert qa.generate_ids(Scripted(script[1:]), script[0], 40, eos, chunk) == reference_loop(script + [0] * 50, 40, eos)


def test_eos_ids(qa, tmp_path):
    assert qa.parse_eos_tokens(str(tmp_path)) == [151645, 151643]            # no tokenizer_config.json: the Qwen3 defaults
    cfg = {"eos_token": "<|im_end|>", "added_tokens_decoder": {"5": {"content": "<|im_end|>"}, "6": {"content": "<|endoftext|>"}}}
    (tmp_path / "tokenizer_config.json").write_text(json.dumps(cfg))
    assert qa.parse_eos_tokens(str(tmp_path)) == [5]
    cfg["eos_token"] = {"content": "<|endoftext|>"}
    (tmp_path / "tokenizer_config.json").write_text(json.dumps(cfg))
    assert qa.parse_eos_tokens(str(tmp_path)) == [6]
    cfg["eos_token"] = "<none>"
    (tmp_path / "tokenizer_config.json").write_text(json.dumps(cfg))
    assert qa.parse_eos_tokens(str(tmp_path)) == [151645, 151643]


def test_checkpoint_round_trip_without_a_device(qa, omx, tmp_path):
    """A tiny checkpoint written as safetensors + config.json comes back split and intact through read_checkpoint, the device-free
    half of Qwen3ASR.load; load itself needs a device and says so."""
    from ominix_mlx_amd import loader
    g = np.random.default_rng(0)
    tensors = {"audio_tower.conv2d1.weight": g.standard_normal((32, 3, 3, 1)).astype(np.float32),
               "audio_tower.conv2d1.bias": g.standard_normal(32).astype(np.float32),
               "audio_tower.layers.0.fc1.weight": g.standard_normal((8, 4)).astype(np.float32),
               "model.embed_tokens.weight": g.standard_normal((16, 8)).astype(np.float32),
               "model.norm.weight": np.ones(8, np.float32)}
    loader.write_safetensors(str(tmp_path / "model.safetensors"), tensors)
    config = {"thinker_config": {"audio_config": {"num_mel_bins": 16, "d_model": 128, "encoder_attention_heads": 2},
                                 "text_config": {"hidden_size": 8, "num_hidden_layers": 1, "intermediate_size": 16, "num_attention_heads": 1,
                                                 "vocab_size": 16}, "audio_token_id": 3}}
    (tmp_path / "config.json").write_text(json.dumps(config))
    cfg, tower, text, eos = qa.read_checkpoint(str(tmp_path))
    assert cfg.audio_token_id == 3 and cfg.audio_config["d_model"] == 128 and eos == [151645, 151643]
    assert sorted(tower) == ["conv2d1.bias", "conv2d1.weight", "layers.0.fc1.weight"] and sorted(text) == ["model.embed_tokens.weight", "model.norm.weight"]
    for k, v in tower.items():
        np.testing.assert_array_equal(np.asarray(v), tensors["audio_tower." + k])
    np.testing.assert_array_equal(np.asarray(text["model.embed_tokens.weight"]), tensors["model.embed_tokens.weight"])
    (tmp_path / "sub").mkdir()
    loader.write_safetensors(str(tmp_path / "sub" / "model.safetensors"), {"model.norm.weight": np.ones(8, np.float32)})
    (tmp_path / "sub" / "config.json").write_text(json.dumps(config))
    with pytest.raises(omx.OmxError, match="no audio_tower"):
        qa.read_checkpoint(str(tmp_path / "sub"))
    if omx.device_count() == 0:
        with pytest.raises(omx.OmxError):
            qa.Qwen3ASR.load(str(tmp_path))
