"""CPU: the host side of dense float16 checkpoints -- the loader's dtype decision and the omx_qwen3_config field the engine reads."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import omx_import
    omx_import.load_package()
    from ominix_mlx_amd import engine, loader
    return engine, loader


def _dense(dt):
    mk = (lambda s: np.zeros(s, np.float16)) if dt == "f16" else (lambda s: np.zeros(s, np.uint16).view(_bits()))
    return {"model.embed_tokens.weight": mk((64, 16)), "model.layers.0.self_attn.q_proj.weight": mk((16, 16)),
            "model.layers.0.input_layernorm.weight": mk((16,)), "model.norm.weight": mk((16,))}


def _bits():
    import omx_import
    omx_import.load_package()
    from ominix_mlx_amd.loader import Bf16Bits
    return Bf16Bits


ARGS = dict(head_dim=128, quantization=None)


def test_f16_checkpoint_is_float16(pkg):
    _, loader = pkg
    assert loader.dense_dtype(_dense("f16"), ARGS) == "float16"


def test_bf16_checkpoint_stays_bfloat16(pkg):
    _, loader = pkg
    assert loader.dense_dtype(_dense("bf16"), ARGS) == "bfloat16"


def test_mixed_or_quantized_checkpoints_stay_bfloat16(pkg):
    _, loader = pkg
    w = _dense("f16")
    w["model.layers.0.self_attn.q_proj.weight"] = np.zeros((16, 16), np.float32)
    assert loader.dense_dtype(w, ARGS) == "bfloat16"
    # a packed checkpoint decides by its scales (quant_scales_f16), not here
    assert loader.dense_dtype(_dense("f16"), dict(ARGS, quantization={"bits": 4, "group_size": 64})) == "bfloat16"
    # only the 1-D norm weights float16: not a float16 checkpoint
    w = _dense("bf16")
    w["model.norm.weight"] = np.zeros((16,), np.float16)
    assert loader.dense_dtype(w, ARGS) == "bfloat16"


@pytest.mark.parametrize("extra", [dict(num_experts=8), dict(attention_bias=True), dict(head_dim=64), dict(tp_size=2)])
def test_shapes_the_float16_engine_refuses_keep_the_bf16_conversion(pkg, extra):
    _, loader = pkg
    assert loader.dense_dtype(_dense("f16"), dict(ARGS, **extra)) == "bfloat16"


def test_model_dtype_names(pkg):
    engine, _ = pkg
    assert engine.dense_dtype_is_f16("float16") and engine.dense_dtype_is_f16("f16")
    assert not engine.dense_dtype_is_f16("bfloat16") and not engine.dense_dtype_is_f16("bf16")
    with pytest.raises(Exception, match="dtype 'float32'"):
        engine.dense_dtype_is_f16("float32")


def test_config_layout_matches_the_header(pkg):
    """Qwen3Config mirrors omx_qwen3_config field for field (all 4-byte members): float16_weights is the trailing field."""
    engine, _ = pkg
    src = open(os.path.join(ROOT, "include", "omx.h")).read()
    body = re.search(r"typedef struct omx_qwen3_config_ \{(.*?)\} omx_qwen3_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip() for n in re.sub(r"^(int|float)\s+", "", decl).split(",")]
    fields = [f[0] for f in engine.Qwen3Config._fields_]
    assert fields == names
    assert fields[-1] == "float16_weights"
    assert engine.Qwen3Config.float16_weights.offset == 4 * (len(fields) - 1)
    assert ctypes.sizeof(engine.Qwen3Config) == 4 * len(fields)
    # a caller that does not know the field leaves it 0: a bfloat16 model
    assert engine.Qwen3Config(1024, 3).float16_weights == 0
