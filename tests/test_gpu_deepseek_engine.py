"""GPU: the decode engine on the DeepSeek-V2 family layer plan (moe_mode="deepseek": a dense prefix, a float32 scaled router, shared experts)
against the decoder rule of tests/deepseek_moe_rule.py -- Qwen3Oracle's attention, norms and head around the rule's feed-forward.
Model: 3 layers, first_k_dense_replace 1, hidden 256, 2 / 2 heads of 128, dense width 448, 16 experts of 192, top-6, 2 shared, vocabulary
1024.  Bound and token rule of tests/test_gpu_moe_engine.py: |logits - ref| <= 2^-7 * max|ref| * sqrt(layers) * 2, a token may differ only
where the rule's top-1 margin is within twice that.  The weight seeds come from tests/test_deepseek_moe_rule.py."""
import numpy as np
import pytest

import deepseek_moe_rule as dr
from oracle import ref_core as rc
from oracle import synth

pytestmark = pytest.mark.gpu
BASE = dict(hidden_size=256, num_hidden_layers=3, intermediate_size=448, num_attention_heads=2, num_key_value_heads=2, head_dim=128,
            vocab_size=1024, rms_norm_eps=1e-6, rope_theta=10000.0, max_context=256, qk_norm=False)
DS = dict(num_experts=16, num_experts_per_tok=6, moe_intermediate_size=192, moe_mode="deepseek", norm_topk_prob=True,
          first_k_dense_replace=1, n_shared_experts=2, routed_scaling_factor=1.0)


def _engine(omx, weights=None, seed=0x0C0FFEE5, **over):
    from ominix_mlx_amd import engine
    m = engine.Model(**{**BASE, **DS, **over})
    m.synth_weights(seed) if weights is None else m.load_weights(weights)
    return m


def _bound(ref_logits):
    return 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(BASE["num_hidden_layers"]) * 2


@pytest.mark.parametrize("scale,seed", dr.ENGINE_RUNS)
@pytest.mark.parametrize("slots_env", ["1", "0"])
def test_decode_matches_the_rule(omx, monkeypatch, scale, seed, slots_env):
    monkeypatch.setenv("OMX_MOE_SHARED_SLOTS", slots_env)
    _, ref_tokens, ref_logits = dr.engine_selections(scale, seed, "bf16")
    prompt = synth.prompt_ids(dr.ENGINE_PROMPT, BASE["vocab_size"])
    m = _engine(omx, seed=seed, routed_scaling_factor=scale)
    first = m.prefill(prompt)
    logits0 = m.last_logits()
    got = np.concatenate([[first], m.decode(dr.ENGINE_NEW - 1)]).astype(np.uint32)
    assert m.decode_path() == "graph" and m.offset() == dr.ENGINE_PROMPT + dr.ENGINE_NEW - 1
    bound = _bound(ref_logits)
    print(f"scale {scale} slots {slots_env}: prompt logits off by {np.abs(logits0 - ref_logits[0]).max():.4e}, bound {bound:.4e}")
    assert np.abs(logits0 - ref_logits[0]).max() <= bound
    margins = rc.argmax_margin(ref_logits)
    for i in range(dr.ENGINE_NEW):
        if got[i] != ref_tokens[i]:
            assert margins[i] <= 2 * bound, f"token {i}: got {got[i]} want {ref_tokens[i]} with margin {margins[i]:.4f}"
            break
    else:
        np.testing.assert_array_equal(got, ref_tokens)
    # uploaded tensors == the device generator's, bit for bit
    cfg = dr.tiny_decoder_config()
    m2 = _engine(omx, dr.decoder_weights(cfg, 1, 2, seed), routed_scaling_factor=scale)
    got2 = np.concatenate([[m2.prefill(prompt)], m2.decode(dr.ENGINE_NEW - 1)]).astype(np.uint32)
    np.testing.assert_array_equal(got2, got)
    np.testing.assert_array_equal(m2.last_logits(), m.last_logits())


def test_serial_and_batched_prompt_agree(omx, monkeypatch):
    prompt = synth.prompt_ids(dr.ENGINE_PROMPT, BASE["vocab_size"])
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("OMX_PREFILL_SERIAL", mode)
        m = _engine(omx)
        outs[mode] = (m.prefill(prompt), m.last_logits())
    assert np.abs(outs["0"][1] - outs["1"][1]).max() <= _bound(outs["1"][1])
    monkeypatch.setenv("OMX_PREFILL_SERIAL", "0")
    monkeypatch.setenv("OMX_PREFILL_TAIL_STEP", "1")          # the prompt's last token through the decode step
    m = _engine(omx)
    m.prefill(prompt)
    assert np.abs(m.last_logits() - outs["1"][1]).max() <= _bound(outs["1"][1])


def test_all_layers_dense_gives_the_dense_models_bits(omx):
    """first_k_dense_replace == num_hidden_layers: no layer routes, and the step is the dense model's on the same tensors"""
    from ominix_mlx_amd import engine
    cfg = dr.tiny_decoder_config()
    w = dr.decoder_weights(cfg, 3, 0, 0x0C0FFEE5)
    prompt = synth.prompt_ids(24, BASE["vocab_size"])
    dense = engine.Model(**BASE)
    dense.load_weights(w)
    ds = _engine(omx, w, first_k_dense_replace=3)
    a = np.concatenate([[dense.prefill(prompt)], dense.decode(4)])
    b = np.concatenate([[ds.prefill(prompt)], ds.decode(4)])
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(dense.last_logits(), ds.last_logits())


def test_no_dense_layer_and_no_shared_experts(omx):
    """first_k_dense_replace 0, n_shared_experts 0: every layer routes, nothing is added -- against the rule"""
    cfg = dr.tiny_decoder_config()
    w = dr.decoder_weights(cfg, 0, 0, 0x0C0FFEE5)
    prompt = synth.prompt_ids(12, BASE["vocab_size"])
    o = dr.make_oracle(cfg, w, 0, 0, 1.0)
    _, ref_logits = o.generate(prompt, 1, return_logits=True)
    m = _engine(omx, w, first_k_dense_replace=0, n_shared_experts=0)
    m.prefill(prompt)
    assert np.abs(m.last_logits() - ref_logits[0]).max() <= _bound(ref_logits)


def test_prompt_of_embedding_rows_gives_the_bits_of_the_prompt_of_ids(omx):
    prompt = synth.prompt_ids(dr.ENGINE_PROMPT, BASE["vocab_size"])
    a = _engine(omx)
    ta = a.prefill(prompt)
    b = _engine(omx)
    tb = b.prefill(prompt, embeds=b.embed_tokens(prompt[5:30]), embeds_at=5)
    assert ta == tb
    np.testing.assert_array_equal(a.last_logits(), b.last_logits())
    np.testing.assert_array_equal(a.decode(3), b.decode(3))


def test_modes_0_and_1_still_refuse_prompt_rows(omx):
    from ominix_mlx_amd import engine
    m = engine.Model(**{**BASE, "hidden_size": 256}, num_experts=4, num_experts_per_tok=2, moe_intermediate_size=192, moe_mode="qwen3_moe")
    m.synth_weights()
    with pytest.raises(omx.OmxError, match="sparse-MoE .* not supported"):
        m.prefill([1, 2, 3, 4], embeds=np.zeros((2, 256), np.float32), embeds_at=1)


def test_refusals_by_name(omx):
    from ominix_mlx_amd import engine
    mk = lambda **over: engine.Model(**{**BASE, **DS, **over})
    with pytest.raises(omx.OmxError, match="quant_bits"):
        mk(hidden_size=512, num_attention_heads=4, num_key_value_heads=4, moe_intermediate_size=512, intermediate_size=512,
           quantization={"bits": 4, "group_size": 64})
    with pytest.raises(omx.OmxError, match="float16_weights"):
        mk(dtype="float16")
    with pytest.raises(omx.OmxError, match="attention_bias"):
        mk(attention_bias=True)
    with pytest.raises(omx.OmxError, match="tp_size"):
        mk(tp_size=2)
    with pytest.raises(omx.OmxError, match="ep_size"):
        mk(ep_size=2)
    with pytest.raises(omx.OmxError, match="first_k_dense_replace"):
        mk(first_k_dense_replace=4)
    for mode in ("qwen3_moe", "mixtral"):      # the new fields belong to mode 2
        with pytest.raises(omx.OmxError, match="InvalidConfig.*moe_mode 2"):
            engine.Model(**{**BASE, **DS, "moe_mode": mode, "first_k_dense_replace": 1, "n_shared_experts": 0})
        with pytest.raises(omx.OmxError, match="InvalidConfig.*moe_mode 2"):
            engine.Model(**{**BASE, **DS, "moe_mode": mode, "first_k_dense_replace": 0, "n_shared_experts": 2})
    m = _engine(omx)
    with pytest.raises(omx.OmxError, match="omx_qwen3_verify: moe_mode 2"):
        m.verify([1, 2, 3])
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: moe_mode 2"):
        m.score([1, 2, 3, 4])
    with pytest.raises(omx.OmxError, match="omx_qwen3_set_logprobs: moe_mode 2"):
        m.set_logprobs(2)
    missing = mk()
    with pytest.raises(omx.OmxError, match="WeightNotFound"):
        missing.prefill([1, 2, 3])
    cfg = dr.tiny_decoder_config()
    w = dr.decoder_weights(cfg, 1, 2, 0x0C0FFEE5)
    w["model.layers.1.mlp.shared_experts.down_proj.weight"] = np.zeros((256, 192), np.float32)      # one shared expert's width, not two
    with pytest.raises(omx.OmxError, match="ShapeMismatch"):
        mk().load_weights(w)
