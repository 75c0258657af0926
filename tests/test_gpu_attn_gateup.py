"""[RMSNorm + gate/up + SwiGLU] of a layer inside its attention + O launch (csrc/attn_step.hip, gateup_phase): the phase reproduces the
arithmetic of the gate/up GEMV launch it replaces, so everything the engine emits is compared BIT FOR BIT with the launch-per-op step
(OMX_ATTN_GATEUP=0) -- no tolerance; one step's hidden row and activation vector are also held to float64 at the bounds of the
GEMV-form tests (tests/test_gpu_gemv_forms.py: oracle/ref_decode.py check_residual, check_swiglu behind norm_slack) and the row to the
forward of oracle/ref_qwen3.py.  The step sequence number cannot be set through
any debug entry point, so the tag arithmetic near its 32-bit wrap is not exercised here."""
import ctypes

import numpy as np
import pytest

from oracle import ref_decode as rd
from oracle import ref_qwen3 as rq
from oracle import synth

pytestmark = pytest.mark.gpu

# the form is gated on these widths (hidden 4096, intermediate 12288, 32 / 8 heads of 128): they cannot shrink
WIDE = rq.Qwen3Config(4096, 2, 12288, 32, 8, 128, 1024, 1e-6, 1e6, False)
# outside the gate: Llama's intermediate size
OTHER_FFN = rq.Qwen3Config(4096, 2, 11008, 32, 8, 128, 1024, 1e-6, 1e6, False)
STEPS = 24
CAP = 2304          # context buckets of 1024 and 2048 tokens: both split plans have 256 blocks


def _engine(cfg, max_context=CAP):
    from ominix_mlx_amd import engine
    m = engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                     intermediate_size=cfg.intermediate_size, num_attention_heads=cfg.num_attention_heads,
                     num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, vocab_size=cfg.vocab_size,
                     rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                     tie_word_embeddings=cfg.tie_word_embeddings, rope_scaling=cfg.rope_scaling,
                     max_context=max_context, qk_norm=cfg.qk_norm, attention_bias=cfg.attention_bias)
    m.synth_weights()
    return m


def _resident(omx):
    """the 256-block attention grid is resident as a whole on this device"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count >= 256


def _plan(omx, tk_max):
    """(chunk, nsplit) of attn_step_plan for a context bucket, read back from one step attention launch on scratch slabs"""
    from ominix_mlx_amd.engine import AttnStepDbg
    from ominix_mlx_amd.ops import Tensor as T
    H, Hkv, D, cap = WIDE.num_attention_heads, WIDE.num_key_value_heads, WIDE.head_dim, 64
    rng = np.random.default_rng(1)
    qkv = T.from_numpy(rd.rand16(rng, ((H + 2 * Hkv) * D,), "bf16", -2, 0), "bf16")
    k, v = T.from_numpy(np.zeros((Hkv, cap, D), np.float32), "bf16"), T.from_numpy(np.zeros((Hkv, cap, D), np.float32), "bf16")
    nw = T.from_numpy(np.ones(D, np.float32), "bf16")
    rope = T.from_numpy(rd.rope_cur(0, D), "f32")
    n_gran = H * 48 * (D + 2)
    gran = T.from_numpy(np.zeros(n_gran * 2, np.uint32), "u32")
    out = T((H * D,), "bf16")
    a = AttnStepDbg(qkv=qkv.ptr, k=k.ptr, v=v.ptr, H=H, Hkv=Hkv, D=D, cap=cap, scale=float(np.float32(D ** -0.5)), eps=1e-6,
                    q_norm_w=nw.ptr, k_norm_w=nw.ptr, rope_cur=rope.ptr, granules=gran.ptr, granules_n=n_gran, pos=0, seq=1, tag_mul=1,
                    tag_add=1, f16=0, chunk=0, nsplit=0, tk_max=tk_max, out=out.ptr)
    omx.check(omx.lib.omx_debug_attn_step(ctypes.byref(a), None))
    assert a.abort_flag == 0
    return a.chunk, a.nsplit


@pytest.fixture(scope="module")
def starts(omx):
    """start positions of the 24-step runs, from the 1024 bucket's plan: one live split; n_active 16 -> 17 (the second gather batch);
    the last position of a split's chunk and the first of the next; the last position of the bucket (graphs rebuilt mid-run)"""
    chunk, nsplit = _plan(omx, 1024)
    assert WIDE.num_key_value_heads * nsplit == 256 and chunk * nsplit >= 1024, (chunk, nsplit)
    assert WIDE.num_key_value_heads * _plan(omx, 2048)[1] == 256
    half = STEPS // 2
    return {"one_split": 3, "second_batch": 16 * chunk - half, "chunk_edge": 5 * chunk - 1 - half, "bucket_edge": 1024 - 1 - half}


@pytest.fixture(scope="module")
def runs(omx, starts):
    """{mode: {case: (tokens, last logits, forms before, forms after)}}: one engine per mode, re-prefilled for every start position"""
    import os
    prompt = synth.prompt_ids(1100, WIDE.vocab_size)
    out = {}
    saved = os.environ.get("OMX_ATTN_GATEUP")
    try:
        for mode in ("0", "1"):
            os.environ["OMX_ATTN_GATEUP"] = mode
            m = _engine(WIDE)
            out[mode] = {}
            for case, start in starts.items():
                m.reset()
                first = m.prefill(prompt[:start])
                before = m.step_forms()
                toks = np.concatenate([[first], m.decode(STEPS)])
                out[mode][case] = (toks, m.last_logits(), before, m.step_forms())
            m.close()
    finally:
        if saved is None:
            os.environ.pop("OMX_ATTN_GATEUP", None)
        else:
            os.environ["OMX_ATTN_GATEUP"] = saved
    return out


@pytest.mark.parametrize("case", ["one_split", "second_batch", "chunk_edge", "bucket_edge"])
def test_gateup_in_the_attention_launch_is_bit_identical(omx, runs, case):
    """Tokens and last-step logits of 24 greedy steps: OMX_ATTN_GATEUP=1 == OMX_ATTN_GATEUP=0."""
    off, on = runs["0"][case], runs["1"][case]
    assert not off[2]["attn_gateup"] and not off[3]["attn_gateup"]
    assert on[3]["attn_gateup"] == _resident(omx), on[3]
    assert not on[3]["attn_gateup_gave_up"]
    np.testing.assert_array_equal(off[0], on[0])
    np.testing.assert_array_equal(off[1], on[1])


def test_give_up_takes_the_first_rung(omx, monkeypatch):
    """The give-up word is raised from the host (never by starving a launch): the decode call finds its steps void, takes the first
    rung -- this form off, together with down + q/k/v in one launch (the flag does not say which launch gave up); the O projection
    stays in the attention launch --, replays on the launch-per-op GEMVs and returns the same tokens."""
    monkeypatch.delenv("OMX_ATTN_GATEUP", raising=False)
    if not _resident(omx):
        pytest.skip("the 256-block grid is not resident on this device: the form is never taken")
    prompt = synth.prompt_ids(64, WIDE.vocab_size)
    a = _engine(WIDE)
    want = np.concatenate([[a.prefill(prompt)], a.decode(14)])
    want_logits = a.last_logits()
    a.close()
    b = _engine(WIDE)
    got = [b.prefill(prompt)] + list(b.decode(4))
    assert b.step_forms()["attn_gateup"] and "disabled" not in b.decode_path()
    b.raise_give_up()
    got += list(b.decode(6))
    forms = b.step_forms()
    assert not forms["attn_gateup"] and forms["attn_gateup_gave_up"], forms
    assert not forms["down_qkv"] and forms["down_qkv_gave_up"] and forms["attn_oproj"], forms   # one rung only
    assert b.decode_path().endswith(" gateup_disabled chain_disabled"), b.decode_path()
    got += list(b.decode(4))
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    np.testing.assert_array_equal(b.last_logits(), want_logits)
    b.close()


def test_shape_outside_the_gate_keeps_the_launches(omx, monkeypatch):
    """intermediate 11008 does not share out over the grid: the step is the launch-per-op step whatever the switch says."""
    outs = {}
    prompt = synth.prompt_ids(40, OTHER_FFN.vocab_size)
    for mode in ("0", "1"):
        monkeypatch.setenv("OMX_ATTN_GATEUP", mode)
        m = _engine(OTHER_FFN, max_context=1280)
        toks = np.concatenate([[m.prefill(prompt)], m.decode(8)])
        outs[mode] = (toks, m.last_logits(), m.step_forms())
        m.close()
    assert not outs["0"][2]["attn_gateup"] and not outs["1"][2]["attn_gateup"]
    np.testing.assert_array_equal(outs["0"][0], outs["1"][0])
    np.testing.assert_array_equal(outs["0"][1], outs["1"][1])


def test_switches_and_overrides_keep_the_launches(omx, monkeypatch):
    """A rows-per-wave override of either GEMV the phase stands for, the O projection out of the launch or the switch turn the form
    off (every split plan of these heads has 256 blocks from a 256-token cache on: no plan is outside the gate)."""
    monkeypatch.delenv("OMX_ATTN_GATEUP", raising=False)
    m = _engine(WIDE)
    m.prefill(synth.prompt_ids(16, WIDE.vocab_size))
    m.decode(1)
    assert m.step_forms()["attn_gateup"] == _resident(omx)
    for name, value in (("OMX_GEMV_RPW_O", "4"), ("OMX_GEMV_RPW_GU", "4"), ("OMX_ATTN_OPROJ", "0"), ("OMX_ATTN_GATEUP", "0")):
        monkeypatch.setenv(name, value)
        assert not m.step_forms()["attn_gateup"], name
        monkeypatch.delenv(name)
    m.close()


def test_timing_hook_splits_the_fused_launch(omx, monkeypatch):
    """omx_qwen3_time_step_kernels with the form on: the gate/up pair is never armed and never read, attention and gate_up stay
    positive and the timed steps are ordinary steps."""
    monkeypatch.delenv("OMX_ATTN_GATEUP", raising=False)
    prompt = synth.prompt_ids(48, WIDE.vocab_size)
    a = _engine(WIDE)
    want = np.concatenate([[a.prefill(prompt)], a.decode(12)])
    a.close()
    want = np.concatenate([want[:5], want[7:]])
    b = _engine(WIDE)
    got = [b.prefill(prompt)] + list(b.decode(4))
    us = b.time_step_kernels(2)
    got += list(b.decode(6))
    print("time_step_kernels:", us)
    assert all(0 < us[k] < 1000 for k in ("qkv", "attention", "gate_up", "down", "lm_head")), us
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    b.close()


def test_hidden_row_and_activation_against_float64(omx, monkeypatch):
    """One decode step behind a 37-token prompt, the last layer's two vectors the fused launch leaves: the hidden row behind the O
    projection (buffer h2: every layer enters on h and the O projection writes the ping-pong partner) and `act`.

    * At the bounds of the residual and the gate/up form in tests/test_gpu_gemv_forms.py (check_form: rows_dot + check_residual;
      norm_slack + rows_dot + check_swiglu, depth gemv_acc_depth), each against float64 on the launch's OWN inputs -- those bounds are
      per launch: they allow the rounding of one accumulation, not the flips every earlier launch of the prompt and the step has left
      in its inputs.  The inputs are device values that do not come from the launch under test: the attention vector (buffer
      attn_out, the split merge's plain store), the residual entering the last layer -- overwritten by the layer's own down launch,
      so taken from a ONE-layer twin engine fed the same tokens as decode steps (OMX_PREFILL_SERIAL=1 on both: layer 0 sees the same
      embedding rows and cache, its row leaves in the twin's buffer h) -- and, for `act`, the hidden row just checked.
    * The hidden row against the float64 forward of oracle/ref_qwen3.py for the same prompt and step, at the bound the engine tests
      hold a whole model's output to (tests/test_gpu_qwen3.py: 2^-7 max|ref| sqrt(layers))."""
    from oracle import ref_core as rc
    monkeypatch.delenv("OMX_ATTN_GATEUP", raising=False)
    monkeypatch.setenv("OMX_PREFILL_SERIAL", "1")
    cfg, BF = WIDE, "bf16"
    hd, I, last = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers - 1
    prompt = synth.prompt_ids(37, cfg.vocab_size)

    def read(m, name, n):
        raw = np.empty(n, np.uint16)
        omx.check(omx.lib.omx_qwen3_debug_read(m._h, name.encode(), raw.ctypes.data, n))
        return (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)

    m = _engine(cfg)
    first = m.prefill(prompt)
    m.decode(1)
    assert m.step_forms()["attn_gateup"] == _resident(omx)
    act, row, attn_vec = read(m, "act", I), read(m, "h2", hd), read(m, "attn_out", cfg.num_attention_heads * cfg.head_dim)
    # the engine's own weights (the twin of rq.synth_weights, which takes 20 s at these widths on the host): bf16 bits, widened exactly
    w = {}
    for name, shape in rq.weight_shapes(cfg).items():
        ptr, nb = ctypes.c_void_p(), ctypes.c_size_t()
        omx.check(omx.lib.omx_qwen3_get_weight(m._h, name.encode(), ctypes.byref(ptr), ctypes.byref(nb)))
        raw = np.empty(int(np.prod(shape)), np.uint16)
        assert nb.value == raw.nbytes, name
        omx.check(omx.lib.omx_memcpy_d2h(raw.ctypes.data, ptr, raw.nbytes, None))
        w[name] = (raw.astype(np.uint32) << np.uint32(16)).view(np.float32).reshape(shape)
    m.close()
    assert last == 1, "the twin below stands for the layers in front of the last one"
    one = rq.Qwen3Config(hd, 1, I, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.vocab_size, cfg.rms_norm_eps,
                         cfg.rope_theta, cfg.tie_word_embeddings)
    t = _engine(one)
    t.prefill(np.concatenate([prompt, [first]]).astype(np.uint32))
    resid = read(t, "h", hd)
    t.close()

    p = f"model.layers.{last}."
    n = rd.gemv_acc_depth(hd)
    exact, mag = rd.rows_dot(w[p + "self_attn.o_proj.weight"], attn_vec)
    rd.check_residual(row.astype(np.float64), resid, exact, mag, n, BF, np.zeros(hd))

    gate, up, nw = w[p + "mlp.gate_proj.weight"], w[p + "mlp.up_proj.weight"], w[p + "post_attention_layernorm.weight"]
    xin, slack = rd.norm_slack(np.concatenate([gate, up]), row, nw, cfg.rms_norm_eps, BF)
    eg, mg = rd.rows_dot(gate, xin)
    eu, mu = rd.rows_dot(up, xin)
    rd.check_swiglu(act.astype(np.float64), eg, mg, eu, mu, n, BF, 0, slack[:I], slack[I:])

    orc = rq.Qwen3Oracle(cfg, w)
    caches = []
    logits = orc.forward(prompt[None, :].astype(np.int64), caches)
    assert int(rc.sample_greedy(logits[:, -1, :])[0]) == int(first), "the step's input token differs from the oracle's"
    h = w["model.embed_tokens.weight"][np.array([[int(first)]])]
    for i in range(cfg.num_hidden_layers):
        xn = rc.rms_norm(h, w[f"model.layers.{i}.input_layernorm.weight"], cfg.rms_norm_eps, BF)
        h1 = rc.add(h, orc.attention(i, xn, None, caches[i]), BF)
        h = rc.add(h1, orc.mlp(i, rc.rms_norm(h1, w[f"model.layers.{i}.post_attention_layernorm.weight"], cfg.rms_norm_eps, BF)), BF)
    h1 = h1.reshape(hd)                                                # the row behind the last layer's O projection
    bound = 2.0 ** -7 * np.abs(h1).max() * np.sqrt(cfg.num_hidden_layers)
    print("hidden row against the oracle: max |diff|", np.abs(row - h1).max(), "bound", bound, "rows differing", int((row != h1).sum()))
    assert np.abs(row - h1).max() <= bound
