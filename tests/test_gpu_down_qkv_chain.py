"""down + residual of a layer and [RMSNorm + q/k/v] of the next layer as ONE launch (csrc/gemv_chain.hip): the launch reproduces the
arithmetic of the two GEMV launches it replaces, so everything the engine emits is compared BIT FOR BIT with the two-launch step
(OMX_DOWN_QKV=0) -- no tolerance.  The two-launch step is the one the other GPU tests hold against the oracle."""
import numpy as np
import pytest

from oracle import ref_qwen3 as rq
from oracle import synth

pytestmark = pytest.mark.gpu

# Qwen3-8B widths (hidden 4096, intermediate 12288, 32 / 8 heads of 128: the shape the kernel has a register layout for), 3 layers so
# that the step has a first layer (own q/k/v launch), a middle one (both folds) and a last one (plain down in front of the lm_head)
WIDE = rq.Qwen3Config(4096, 3, 12288, 32, 8, 128, 2048, 1e-6, 1e6, False)
# the same widths the way Qwen2 wires them: no q/k norm, projection biases (carried by the fused launch like by the q/k/v GEMV)
WIDE_BIAS = rq.Qwen3Config(4096, 2, 12288, 32, 8, 128, 1024, 1e-6, 1e6, False, qk_norm=False, attention_bias=True)
# no register layout: hidden 1024
NARROW = rq.Qwen3Config(1024, 3, 3072, 8, 2, 128, 4096, 1e-6, 1e6, True)


def _engine(cfg, max_context):
    from ominix_mlx_amd import engine
    m = engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                     intermediate_size=cfg.intermediate_size, num_attention_heads=cfg.num_attention_heads,
                     num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, vocab_size=cfg.vocab_size,
                     rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                     tie_word_embeddings=cfg.tie_word_embeddings, rope_scaling=cfg.rope_scaling,
                     max_context=max_context, qk_norm=cfg.qk_norm, attention_bias=cfg.attention_bias)
    m.synth_weights()
    return m


def _run(monkeypatch, cfg, mode, n_prompt=1000, n_new=40):
    """mode "0": two launches; "1": the default; "eager": the default without graphs.  -> (tokens, last logits, forms of the step)"""
    if mode == "0":
        monkeypatch.setenv("OMX_DOWN_QKV", "0")
    else:
        monkeypatch.delenv("OMX_DOWN_QKV", raising=False)
    monkeypatch.setenv("OMX_NO_GRAPH", "1" if mode == "eager" else "0")
    m = _engine(cfg, max_context=n_prompt + 280)
    prompt = synth.prompt_ids(n_prompt, cfg.vocab_size)
    toks = np.concatenate([[m.prefill(prompt)], m.decode(n_new)])       # positions 1000 .. 1039: crosses the bucket boundary at 1024
    forms = m.step_forms()
    out = (toks, m.last_logits(), forms)
    m.close()
    return out


def _resident(omx):
    """the fused grid (hidden / 8 workgroups, two per CU) is resident as a whole on this device"""
    import torch
    return 4096 // 8 <= 2 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("oproj", ["1", "0"])
def test_down_qkv_in_one_launch_is_bit_identical(omx, monkeypatch, oproj):
    """Tokens and last-step logits of 40 decode steps across a context-bucket boundary: OMX_DOWN_QKV=0 == default == default under
    OMX_NO_GRAPH=1, with the O projection inside the attention launch and (OMX_ATTN_OPROJ=0) without."""
    monkeypatch.setenv("OMX_ATTN_OPROJ", oproj)
    outs = {mode: _run(monkeypatch, WIDE, mode) for mode in ("0", "1", "eager")}
    assert not outs["0"][2]["down_qkv"]
    if _resident(omx):
        assert outs["1"][2]["down_qkv"] and outs["eager"][2]["down_qkv"], outs["1"][2]
        assert not outs["1"][2]["down_qkv_gave_up"]
    assert outs["1"][2]["attn_oproj"] == (oproj == "1" and _resident(omx))
    for mode in ("1", "eager"):
        np.testing.assert_array_equal(outs["0"][0], outs[mode][0])
        np.testing.assert_array_equal(outs["0"][1], outs[mode][1])


def test_projection_biases_ride_in_the_fused_launch(omx, monkeypatch):
    """attention_bias (Qwen2 wiring): the fused launch adds the next layer's q/k/v bias before the one rounding, like EPI_STORE."""
    outs = {mode: _run(monkeypatch, WIDE_BIAS, mode, n_prompt=200, n_new=12) for mode in ("0", "1")}
    if _resident(omx):
        assert outs["1"][2]["down_qkv"]
    np.testing.assert_array_equal(outs["0"][0], outs["1"][0])
    np.testing.assert_array_equal(outs["0"][1], outs["1"][1])


def test_shape_without_layout_keeps_two_launches(omx, monkeypatch):
    """hidden 1024 has no register layout: the step is the two-launch step whatever the switch says."""
    outs = {mode: _run(monkeypatch, NARROW, mode, n_prompt=100, n_new=12) for mode in ("0", "1")}
    assert not outs["0"][2]["down_qkv"] and not outs["1"][2]["down_qkv"]
    np.testing.assert_array_equal(outs["0"][0], outs["1"][0])
    np.testing.assert_array_equal(outs["0"][1], outs["1"][1])


def test_overrides_and_other_forms_keep_two_launches(omx, monkeypatch):
    """A rows-per-wave override of either GEMV the launch stands for, or the switch, turns the fold off."""
    monkeypatch.delenv("OMX_DOWN_QKV", raising=False)
    m = _engine(WIDE, max_context=256)
    m.prefill(synth.prompt_ids(16, WIDE.vocab_size))
    base = m.step_forms()["down_qkv"]
    assert base == _resident(omx)
    for name in ("OMX_GEMV_RPW_QKV", "OMX_GEMV_RPW_DOWN"):
        monkeypatch.setenv(name, "4")
        assert not m.step_forms()["down_qkv"]
        monkeypatch.delenv(name)
    monkeypatch.setenv("OMX_DOWN_QKV", "0")
    assert not m.step_forms()["down_qkv"]
    m.close()


def test_give_up_falls_back_to_two_launches(omx, monkeypatch):
    """The fallback rung: the give-up word is raised from the host (never by starving a launch); the decode call finds its steps void,
    switches the fold off for this engine, replays them on two launches and returns the same tokens."""
    monkeypatch.delenv("OMX_DOWN_QKV", raising=False)
    if not _resident(omx):
        pytest.skip("the fused grid is not resident on this device: the fold is never taken")
    prompt = synth.prompt_ids(64, WIDE.vocab_size)
    a = _engine(WIDE, max_context=256)
    want = np.concatenate([[a.prefill(prompt)], a.decode(14)])
    want_logits = a.last_logits()
    a.close()
    b = _engine(WIDE, max_context=256)
    got = [b.prefill(prompt)] + list(b.decode(4))
    assert b.step_forms()["down_qkv"]
    b.raise_give_up()
    got += list(b.decode(6))
    forms = b.step_forms()
    assert not forms["down_qkv"] and forms["down_qkv_gave_up"] and forms["attn_oproj"], forms   # one rung only
    got += list(b.decode(4))
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    np.testing.assert_array_equal(b.last_logits(), want_logits)
    b.close()


def test_timing_hook_splits_the_fused_launch(omx, monkeypatch):
    """omx_qwen3_time_step_kernels with the fold on: no event pair is read that was never armed, qkv and down stay positive, the
    timed steps are ordinary steps."""
    monkeypatch.delenv("OMX_DOWN_QKV", raising=False)
    prompt = synth.prompt_ids(48, WIDE.vocab_size)
    a = _engine(WIDE, max_context=256)
    want = np.concatenate([[a.prefill(prompt)], a.decode(12)])
    a.close()
    want = np.concatenate([want[:5], want[7:]])
    b = _engine(WIDE, max_context=256)
    got = [b.prefill(prompt)] + list(b.decode(4))
    us = b.time_step_kernels(2)
    got += list(b.decode(6))
    print("time_step_kernels:", us)
    assert all(0 < us[k] < 1000 for k in ("qkv", "attention", "gate_up", "down", "lm_head")), us
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    b.close()


def test_fused_launch_is_a_recording_site(omx, monkeypatch):
    """The step as AQL packets (csrc/aql_step.hip, the EXPERIMENTS=1 build) records the fused launch like every other launch of the step:
    the program is built (a launch that is no recording site would refuse it) and replays to the tokens and logits of the hipGraph step."""
    from conftest import needs_experiments
    needs_experiments(omx)
    monkeypatch.delenv("OMX_DOWN_QKV", raising=False)
    prompt = synth.prompt_ids(1000, WIDE.vocab_size)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("OMX_STEP_AQL", mode)
        m = _engine(WIDE, max_context=1280)
        toks = np.concatenate([[m.prefill(prompt)], m.decode(10), m.decode(30), m.decode(5)])   # 1010 .. 1040 crosses 1024 inside a call
        outs[mode] = (toks, m.last_logits(), m.decode_path(), m.step_forms()["down_qkv"])
        m.close()
    assert outs["1"][2] == "aql", "the AQL program was not built (OMX_STEP_AQL_VERBOSE=1 prints why)"
    assert outs["1"][3] == _resident(omx)
    np.testing.assert_array_equal(outs["0"][0], outs["1"][0])
    np.testing.assert_array_equal(outs["0"][1], outs["1"][1])
