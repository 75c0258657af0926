"""tests/funasr_nano_rule.py held to the float32 oracle of the Paraformer layer it shares its structure with, and to its own definition:
an utterance in a joint pass is that utterance alone."""
import numpy as np

import funasr_nano_rule as rule
from oracle import ref_paraformer as rp


def _layer(in_dim, dim, ffn, k, seed):
    g = np.random.default_rng(seed)
    r = lambda *s, sc=1.0: (g.standard_normal(s) * sc).astype(np.float32)
    return {"norm1_w": r(in_dim, sc=0.1) + 1, "norm1_b": r(in_dim, sc=0.1), "qkv_w": r(3 * dim, in_dim, sc=in_dim ** -0.5), "qkv_b": r(3 * dim, sc=0.1),
            "out_w": r(dim, dim, sc=dim ** -0.5), "out_b": r(dim, sc=0.1), "fsmn_w": r(dim, k, sc=0.3), "norm2_w": r(dim, sc=0.1) + 1,
            "norm2_b": r(dim, sc=0.1), "ffn_up_w": r(ffn, dim, sc=dim ** -0.5), "ffn_up_b": r(ffn, sc=0.1), "ffn_down_w": r(dim, ffn, sc=ffn ** -0.5),
            "ffn_down_b": r(dim, sc=0.1)}


def test_layer_matches_the_paraformer_oracle_in_both_forms():
    """SenseVoiceEncoderLayer (sensevoice_encoder.rs:368-384) is SanmEncoderLayer (paraformer.rs:618-634) term for term; the oracle's
    weights and inputs are float32 values: agreement to 1e-5 of the largest value"""
    for in_dim in (256, 280):                                        # keeps the width / changes it (no attention residual)
        w = _layer(in_dim, 256, 512, 11, 1)
        x = np.random.default_rng(2).standard_normal((23, in_dim)).astype(np.float32)
        ref = rp.sanm_encoder_layer(x, w, 2)
        got = rule.encoder_layer(x, w, 2)
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


def test_position_add_is_the_oracle_embed_without_its_scale():
    x = np.random.default_rng(3).standard_normal((501, 560)).astype(np.float32)
    ref = rp.encoder_embed(x) - x.astype(np.float64) * np.sqrt(np.float32(512.0)).astype(np.float64)    # the sqrt(512) factor undone
    got = rule.position_add(x) - x
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.abs(rule.position_encoding(501, 560) - rp.position_encoding(501, 560)).max() <= 1e-5
    # positions start at 1: the first row is sin(ts_i) | cos(ts_i), not 0 | 1
    assert abs(rule.position_encoding(1, 8)[0, 0] - np.sin(1.0)) < 1e-6


def test_fsmn_matches_the_oracle_and_stops_at_boundaries():
    g = np.random.default_rng(4)
    v, w = g.standard_normal((30, 16)), g.standard_normal((16, 11))
    assert np.abs(rule.fsmn(v, w) - rp.fsmn(v, w)).max() <= 1e-12
    lengths = (3, 1, 20, 6)
    cut = rule.fsmn(v, w.reshape(16, 1, 11), lengths)
    for lo, hi in rule.segments(lengths):
        np.testing.assert_array_equal(cut[lo:hi], rule.fsmn(v[lo:hi], w))
    assert np.abs(cut - rule.fsmn(v, w)).max() > 0.5                 # taps ~ N(0, 1): a leak is an O(1) error


def test_segment_attention_is_full_attention_under_a_block_mask():
    g = np.random.default_rng(5)
    lengths = (5, 16, 1, 33)
    T, heads, dim = sum(lengths), 2, 256
    q, k, v = (g.standard_normal((T, dim)) for _ in range(3))
    seg = rule.attention(q, k, v, heads, lengths)
    full = rule.attention(q, k, v, heads, mask=rule.block_mask(lengths))
    assert np.abs(seg - full).max() <= 1e-12 * np.abs(seg).max()
    for lo, hi in rule.segments(lengths):
        np.testing.assert_array_equal(seg[lo:hi], rule.attention(q[lo:hi], k[lo:hi], v[lo:hi], heads))
    assert np.abs(seg - rule.attention(q, k, v, heads)).max() > 1e-2


def test_segmented_tower_equals_each_utterance_alone():
    cfg = dict(rule.TINY_CFG, output_size=128, attention_heads=1, linear_units=64, encoder_dim=128, ffn_dim=64, lfr_dim=24)
    w = rule.synth_weights(cfg, 9)
    lengths = (7, 1, 19, 3)
    x = np.random.default_rng(6).standard_normal((sum(lengths), cfg["lfr_dim"])).astype(np.float32)
    joint = rule.tower_segments(x, lengths, w, cfg)
    for lo, hi in rule.segments(lengths):
        alone = rule.tower(x[lo:hi], w, cfg)
        for name in ("pos", "after_norm", "tp_norm", "linear2", "out"):
            np.testing.assert_array_equal(joint[name][lo:hi], alone[name], err_msg=name)
    assert joint["out"].shape == (sum(lengths), cfg["llm_dim"])


def test_synth_weights_cover_the_config():
    cfg = rule.TINY_CFG
    w = rule.synth_weights(cfg, 1)
    assert set(w) == set(rule.weight_shapes(cfg)) and all(a.dtype == np.float32 for a in w.values())
    taps = w["encoder.encoders.0.self_attn.fsmn.weight"]
    assert taps.shape == (cfg["output_size"], 1, cfg["kernel_size"]) and 0.25 < taps.std() < 0.35
    assert len([k for k in w if k.startswith("encoder.encoders.")]) == 13 * (cfg["num_blocks"] - 1)
