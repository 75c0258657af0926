"""CPU-only: the parsing and bookkeeping of mixed-precision MLX checkpoints -- config.json's nested "quantization" entries
(engine.quant_formats), the shapes a matrix with its own format has (engine.expected_shape) and the recipe tables the decode tool builds."""
import pytest


def _engine(omx):
    from ominix_mlx_amd import engine
    return engine


def test_parser_accepts_nested_entries(omx):
    e = _engine(omx)
    base, table = e.quant_formats({"group_size": 64, "bits": 4,
                                   "model.layers.3.mlp.down_proj": {"group_size": 64, "bits": 6},
                                   "model.layers.3.self_attn.v_proj": {"bits": 8, "group_size": 32},
                                   "lm_head": {"bits": 6}})
    assert base == (4, 64)
    assert table == {"model.layers.3.mlp.down_proj": (6, 64), "model.layers.3.self_attn.v_proj": (8, 32), "lm_head": (6, 64)}
    assert e.quant_formats(None) == (None, {})
    assert e.quant_formats({"bits": 4, "group_size": 128}) == ((4, 128), {})


def test_parser_fills_a_missing_group_size_from_the_base(omx):
    e = _engine(omx)
    _, table = e.quant_formats({"bits": 3, "group_size": 128, "model.embed_tokens": {"bits": 8}})
    assert table == {"model.embed_tokens": (8, 128)}


def test_parser_accepts_the_affine_mode_only(omx):
    e = _engine(omx)
    base, table = e.quant_formats({"bits": 4, "group_size": 64, "mode": "affine",
                                   "model.layers.0.self_attn.v_proj": {"bits": 6, "group_size": 64, "mode": "affine"}})
    assert base == (4, 64) and table == {"model.layers.0.self_attn.v_proj": (6, 64)}
    with pytest.raises(omx.OmxError, match=r"InvalidConfig:.*model\.layers\.0\.self_attn\.v_proj.*mxfp4"):
        e.quant_formats({"bits": 4, "group_size": 64, "model.layers.0.self_attn.v_proj": {"bits": 4, "group_size": 32, "mode": "mxfp4"}})
    with pytest.raises(omx.OmxError, match="InvalidConfig:.*mxfp4"):
        e.quant_formats({"bits": 4, "group_size": 32, "mode": "mxfp4"})


@pytest.mark.parametrize("entry,what", [(False, "False"), (True, "True")])
def test_parser_refuses_a_boolean_entry(omx, entry, what):
    e = _engine(omx)
    with pytest.raises(omx.OmxError, match=rf"InvalidConfig:.*model\.layers\.1\.mlp\.gate_proj.*{what}"):
        e.quant_formats({"bits": 4, "group_size": 64, "model.layers.1.mlp.gate_proj": entry})


def test_parser_refuses_bits_7_and_group_48(omx):
    e = _engine(omx)
    with pytest.raises(omx.OmxError, match=r"InvalidConfig:.*lm_head.*bits 7"):
        e.quant_formats({"bits": 4, "group_size": 64, "lm_head": {"bits": 7, "group_size": 64}})
    with pytest.raises(omx.OmxError, match=r"InvalidConfig:.*model\.embed_tokens.*group_size 48"):
        e.quant_formats({"bits": 4, "group_size": 64, "model.embed_tokens": {"bits": 4, "group_size": 48}})


def test_expected_shape_uses_the_matrix_own_format(omx):
    e = _engine(omx)
    # hidden 1024, 3 layers, intermediate 3072, 8 heads / 2 kv heads of 128, vocab 4096; base (4, 64)
    c = e.Qwen3Config(1024, 3, 3072, 8, 2, 128, 4096, 1e-6, 1e6, 1.0, 1, 256, 0, 1, 4, 64, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    formats = {"model.layers.0.self_attn.v_proj": (6, 64), "model.layers.2.mlp.down_proj": (8, 32)}
    v, d = "model.layers.0.self_attn.v_proj", "model.layers.2.mlp.down_proj"
    assert e.expected_shape(c, v + ".weight", formats) == (256, 1024 * 6 // 32)
    assert e.expected_shape(c, v + ".scales", formats) == (256, 1024 // 64)
    assert e.expected_shape(c, d + ".weight", formats) == (1024, 3072 * 8 // 32)
    assert e.expected_shape(c, d + ".scales", formats) == (1024, 3072 // 32)
    assert e.expected_shape(c, d + ".biases", formats) == (1024, 3072 // 32)
    # a matrix without an entry, and every matrix without a table, keeps the base format
    assert e.expected_shape(c, "model.layers.1.self_attn.v_proj.weight", formats) == (256, 1024 * 4 // 32)
    assert e.expected_shape(c, v + ".weight") == (256, 1024 * 4 // 32)
    assert e.expected_shape(c, d + ".scales") == (1024, 3072 // 64)


def test_recipe_layer_sets(omx):
    e = _engine(omx)
    # the rule as the tool states it: i < L // 8 or i >= 7 * L // 8 or (i - L // 8) % 3 == 2
    assert e.mixed_recipe("mixed_4_6", 8) == (4, 6, [0, 3, 6, 7])
    low, high, wide = e.mixed_recipe("mixed_3_6", 36)
    assert (low, high) == (3, 6)
    assert wide == [0, 1, 2, 3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 31, 32, 33, 34, 35]
    assert e.mixed_recipe("mixed_2_6", 8)[:2] == (2, 6) and e.mixed_recipe("mixed_3_4", 8)[:2] == (3, 4)
    q = e.mixed_recipe_quantization("mixed_4_6", 8)
    base, table = e.quant_formats(q)
    assert base == (4, 64)
    assert table == dict([(f"model.layers.{i}.{s}", (6, 64)) for i in (0, 3, 6, 7) for s in ("self_attn.v_proj", "mlp.down_proj")] + [("lm_head", (6, 64))])
    assert "lm_head" not in e.mixed_recipe_quantization("mixed_4_6", 8, tie_word_embeddings=True)
    with pytest.raises(omx.OmxError, match="mixed_5_5"):
        e.mixed_recipe("mixed_5_5", 8)
