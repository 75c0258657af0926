"""Host logic of ominix-mlx_amd/funasr_nano.py, no device: the reference's key map and the decoder's renaming, config.yaml, the prompt
layout, the stop rules, grouping -- and the new exports in the built library."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fn(omx):
    from ominix_mlx_amd import funasr_nano
    return funasr_nano


def test_key_map_and_llm_renaming(fn):
    keys = ["encoder.encoders0.0.attn.qkv.weight", "encoder.encoders.3.attn.out.bias", "encoder.tp_encoders.19.attn.fsmn.weight",
            "encoder.encoders.0.ffn.w1.weight", "encoder.encoders.0.ffn.w2.bias", "encoder.encoders.0.norm1.weight", "encoder.after_norm.bias",
            "adaptor.linear1.weight", "adaptor.blocks.1.attn.q.weight", "adaptor.blocks.1.attn.k.bias", "adaptor.blocks.0.attn.v.weight",
            "adaptor.blocks.0.attn.out.weight", "adaptor.blocks.0.ffn.w1.weight",
            "llm.layers.5.attn.q_proj.weight", "llm.layers.5.attn.k_norm.weight", "llm.layers.5.attn.o_proj.weight",
            "llm.layers.5.mlp.gate_proj.weight", "llm.layers.5.input_layernorm.weight", "llm.embed_tokens.weight", "llm.norm.weight",
            "llm.lm_head.weight", "ctc.something.weight"]
    assert fn.map_key(keys[0]) == "encoder.encoders0.0.self_attn.linear_q_k_v.weight"
    assert fn.map_key(keys[1]) == "encoder.encoders.3.self_attn.linear_out.bias"
    assert fn.map_key(keys[2]) == "encoder.tp_encoders.19.self_attn.fsmn.weight"
    assert fn.map_key(keys[3]) == "encoder.encoders.0.feed_forward.w_1.weight"
    assert fn.map_key(keys[8]) == "adaptor.blocks.1.self_attn.linear_q.weight"
    assert fn.map_key(keys[11]) == "adaptor.blocks.0.self_attn.linear_out.weight"
    assert fn.map_key("llm.layers.5.attn.q_proj.weight") == "llm.layers.5.self_attn.q_proj.weight"     # not taken by the ".attn.q." rule
    tower, text, other = fn.split_weights({k: i for i, k in enumerate(keys)})
    assert other == ["ctc.something.weight"]
    assert set(tower) == {fn.map_key(k) for k in keys[:13]}
    assert set(text) == {"model.layers.5.self_attn.q_proj.weight", "model.layers.5.self_attn.k_norm.weight", "model.layers.5.self_attn.o_proj.weight",
                         "model.layers.5.mlp.gate_proj.weight", "model.layers.5.input_layernorm.weight", "model.embed_tokens.weight",
                         "model.norm.weight", "lm_head.weight"}
    assert text["lm_head.weight"] == keys.index("llm.lm_head.weight")
    # every mapped tower key is one the float64 rule's tower names
    import funasr_nano_rule as rule
    names = set(rule.weight_shapes(rule.DEFAULT_CFG))
    assert all(k in names for k in tower)


def test_config_yaml(fn):
    full = """
audio_encoder_conf:
  output_size: 256
  attention_heads: 2
  linear_units: 1024
  num_blocks: 3
  tp_blocks: 2
  kernel_size: 9
  dropout_rate: 0.1
audio_adaptor_conf:
  encoder_dim: 256
  ffn_dim: 512
  llm_dim: 1024
  n_layer: 1
  downsample_rate: 1
"""
    c = fn.parse_config(full)
    assert c == dict(lfr_dim=560, output_size=256, attention_heads=2, linear_units=1024, num_blocks=3, tp_blocks=2, kernel_size=9,
                     encoder_dim=256, ffn_dim=512, llm_dim=1024, n_layer=1)
    default = dict(lfr_dim=560, output_size=512, attention_heads=4, linear_units=2048, num_blocks=50, tp_blocks=20, kernel_size=11,
                   encoder_dim=512, ffn_dim=2048, llm_dim=1024, n_layer=2)
    assert fn.parse_config(None) == default and fn.parse_config("") == default and fn.parse_config("model: FunASRNano\n") == default
    part = fn.parse_config("audio_encoder_conf:\n  num_blocks: 4\n  kernel_size: eleven\n")      # a field that is no integer: the default
    assert part == dict(default, num_blocks=4)
    assert fn.parse_config("audio_adaptor_conf:\n  llm_dim: 2560\n")["llm_dim"] == 2560


class StubTokenizer:
    """one id per character, specials by name"""
    SPECIALS = {"<|endoftext|>": 900, "<|im_start|>": 901, "<|im_end|>": 902, "<|startofspeech|>": 903, "<|endofspeech|>": 904}

    def token_to_id(self, text):
        return self.SPECIALS.get(text)

    def encode(self, text, add_special_tokens=False):
        assert add_special_tokens is False
        return [ord(c) % 800 + 1 for c in text]


def test_prompt_layout_and_embeds_at(fn):
    tok = StubTokenizer()
    m = fn.Markers.from_tokenizer(tok)
    assert (m.eos, m.im_start, m.im_end, m.speech_start, m.speech_end) == (900, 901, 902, 903, 904)
    p = fn.build_prompt(tok, m)
    e = lambda s: tok.encode(s)
    want_prefix = [901] + e("system\n") + e("You are a helpful assistant.") + [902] + e("\n") + [901] + e("user\n") + e("语音转写成中文：")
    want_suffix = [902] + e("\n") + [901] + e("assistant\n")
    assert p.prefix == want_prefix and p.suffix == want_suffix
    for n in (1, 84, 501):
        ids, at = p.ids(n)
        assert ids.dtype == np.uint32 and ids.size == len(want_prefix) + 1 + n + 1 + len(want_suffix)
        assert at == len(want_prefix) + 1 and ids[at - 1] == 903 and ids[at + n] == 904
        assert (ids[at:at + n] == 0).all() and list(ids[at + n + 1:]) == want_suffix
    q = fn.build_prompt(tok, m, "Be brief.", "Transcribe:")
    assert q.prefix == [901] + e("system\n") + e("Be brief.\n") + [902] + e("\n") + [901] + e("user\n") + e("Transcribe:")
    assert q.suffix == want_suffix

    class NoSpeech(StubTokenizer):
        SPECIALS = {k: v for k, v in StubTokenizer.SPECIALS.items() if k != "<|startofspeech|>"}

    with pytest.raises(Exception, match="startofspeech"):
        fn.Markers.from_tokenizer(NoSpeech())


class Script:
    """a scripted token source: decode(n) hands out the next n tokens (zeros past the script) and records the call"""

    def __init__(self, tokens):
        self.tokens, self.at, self.calls = list(tokens), 0, []

    def decode(self, n):
        self.calls.append(n)
        out = (self.tokens[self.at:self.at + n] + [0] * n)[:n]
        self.at += n
        return np.asarray(out, dtype=np.uint32)


def test_the_four_stop_rules(fn):
    m = fn.Markers(im_start=901, im_end=902, eos=900, speech_start=903, speech_end=904)
    run = lambda first, rest, max_tokens=256: fn.generate_ids(Script(rest), first, fn.StopRule(m, max_tokens), chunk=4)
    assert run(5, [6, 7, 900, 8, 9]) == [5, 6, 7]                          # <|endoftext|>
    assert run(5, [6, 902, 8]) == [5, 6]                                   # <|im_end|>
    assert run(900, [1, 2]) == [] and run(902, [1, 2]) == []               # the prompt's own token stops
    assert run(3, [4] + [7] * 12 + [8]) == [3, 4] + [7] * 9                # the tenth equal token in a row is not emitted
    assert run(7, [7] * 8 + [5, 900]) == [7] * 9 + [5]                     # nine in a row go on
    assert run(1, list(range(2, 50)), max_tokens=5) == [1, 2, 3, 4, 5]     # max_tokens
    assert len(run(1, [2 + i % 3 for i in range(600)])) == 256             # its default
    assert run(1, [2, 3], max_tokens=0) == []
    s = Script(list(range(2, 50)))
    fn.generate_ids(s, 1, fn.StopRule(m, 5), chunk=4)
    assert s.calls == [4]                                                  # nothing is decoded past the stop


class ScriptBatch:
    def __init__(self, per_slot):
        self.src = [Script(t) for t in per_slot]
        self.calls = []

    def decode(self, n, slots):
        self.calls.append(list(slots))
        return np.stack([self.src[s].decode(n) for s in slots], axis=1)


def test_batched_generation_drops_stopped_slots(fn):
    m = fn.Markers(im_start=901, im_end=902, eos=900, speech_start=903, speech_end=904)
    b = ScriptBatch([[11, 900, 5, 5], [21, 22, 23, 24, 25, 902], [31] * 30, [41, 42]])
    out = fn.generate_ids_batch(b, [10, 20, 30, 900], [fn.StopRule(m, 8) for _ in range(4)], chunk=2)
    assert out == [[10, 11], [20, 21, 22, 23, 24, 25], [30] + [31] * 7, []]
    assert b.calls[0] == [0, 1, 2]                                         # slot 3 stopped on its first token
    assert b.calls[1] == [1, 2] and all(0 not in c for c in b.calls[1:])
    assert b.calls[-1] == [2] or b.calls[-1] == [1, 2]


def test_grouping(fn):
    assert [list(g) for g in fn.groups(11)] == [list(range(8)), [8, 9, 10]]
    assert [len(g) for g in fn.groups(16)] == [8, 8] and [len(g) for g in fn.groups(1)] == [1] and fn.groups(0) == []


def test_new_exports_are_in_the_built_library(omx):
    lib = ctypes.CDLL(omx.LIB_PATH)
    for name in ("omx_funasr_nano_encoder_create", "omx_funasr_nano_encoder_load", "omx_funasr_nano_encoder_forward",
                 "omx_funasr_nano_encoder_debug_read", "omx_funasr_nano_encoder_destroy", "omx_segment_attention_f32",
                 "omx_sanm_segment_layer_f32", "omx_qwen3_batch_prefill_embeds"):
        assert hasattr(lib, name), name
    from ominix_mlx_amd import audio, engine, paraformer
    assert "omx_funasr_nano_encoder_forward" in audio.AUDIO_SIGNATURES and "omx_qwen3_batch_prefill_embeds" in engine.ENGINE_SIGNATURES
    assert "omx_sanm_segment_layer_f32" in paraformer.PARAFORMER_SIGNATURES


def test_tower_weight_shapes_are_the_rules(fn):
    import funasr_nano_rule as rule
    for cfg in (rule.DEFAULT_CFG, rule.TINY_CFG):
        assert fn.tower_weight_shapes(cfg) == rule.weight_shapes(cfg)
