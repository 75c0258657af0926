"""One launch per layer: [down + residual] of a layer and [RMSNorm + q/k/v] of the next one behind gate/up inside the attention + O launch
(csrc/attn_step.hip down_qkv_phase, engine switch OMX_ATTN_DOWN).  The phase reproduces the arithmetic of the down + q/k/v launch it
replaces (csrc/gemv_chain.hip), so everything the engine emits is compared BIT FOR BIT with the two-launch layer (OMX_ATTN_DOWN=0) -- no
tolerance.  The launches it is compared with are held to float64 per launch by tests/test_gpu_gemv_forms.py and
tests/test_gpu_down_qkv_chain.py; here the 3-layer model's hidden row is held to the float64 forward of oracle/ref_qwen3.py once more.
The form is gated on the widths (hidden 4096, intermediate 12288, 32 / 8 heads of 128, 256 resident blocks): they cannot shrink, so the
models have 3 layers (two take the form, the last does not), a vocabulary of 1024 and a 2304-token cache.
The step sequence number cannot be set through any debug entry point, so the tag arithmetic near its 32-bit wrap is not exercised here."""
import ctypes

import numpy as np
import pytest

from oracle import ref_core as rc
from oracle import ref_qwen3 as rq
from oracle import synth
from test_gpu_attn_gateup import CAP, STEPS, _engine, _resident, starts   # noqa: F401  (starts: the module-scoped fixture)
from test_gpu_hop_issue import _env

pytestmark = pytest.mark.gpu

WIDE3 = rq.Qwen3Config(4096, 3, 12288, 32, 8, 128, 1024, 1e-6, 1e6, False)
# the same widths the way Qwen2 wires them: no q/k norm, q/k/v biases (carried by the phase like by the q/k/v GEMV)
WIDE3_BIAS = rq.Qwen3Config(4096, 3, 12288, 32, 8, 128, 1024, 1e-6, 1e6, False, qk_norm=False, attention_bias=True)
# outside the gate: Llama's intermediate size
OTHER_FFN3 = rq.Qwen3Config(4096, 3, 11008, 32, 8, 128, 1024, 1e-6, 1e6, False)
CASES = ["one_split", "second_batch", "chunk_edge", "bucket_edge"]
REPEATS = 20
TRACE_WORDS = 16          # words per block of omx_qwen3_debug_trace_step; word 15: down units reduced | q/k/v rows stored << 32
BLOCK_UNITS, BLOCK_QKV_ROWS = 32, 24
NAN16 = 0x7FC1            # a bf16 NaN pattern


def _continuation(m, prompt, start, steps=STEPS):
    m.reset()
    first = m.prefill(prompt[:start])
    return np.concatenate([[first], m.decode(steps)]), m.last_logits()


def _bits(m, omx, name, n):
    raw = np.empty(n, np.uint16)
    omx.check(omx.lib.omx_qwen3_debug_read(m._h, name.encode(), raw.ctypes.data, n))
    return raw


def _f32(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _run_cases(cfg, cases, starts, down, no_graph):
    """{case: (tokens, last logits, forms before, forms after)} of one engine, re-prefilled for every start position"""
    prompt = synth.prompt_ids(1100, cfg.vocab_size)
    out = {}
    with _env("OMX_ATTN_DOWN", down), _env("OMX_NO_GRAPH", "1" if no_graph else None):
        m = _engine(cfg)
        for case in cases:
            m.reset()
            first = m.prefill(prompt[:starts[case]])
            before = m.step_forms()
            toks = np.concatenate([[first], m.decode(STEPS)])
            out[case] = (toks, m.last_logits(), before, m.step_forms(), m.decode_path())
        m.close()
    return out


@pytest.fixture(scope="module")
def runs(omx, starts):
    """{(no_graph, down): {case: ...}}: the two-launch layer (OMX_ATTN_DOWN=0) and the default, under the graph and eagerly"""
    return {(ng, down): _run_cases(WIDE3, CASES, starts, down, ng) for ng in (False, True) for down in ("0", None)}


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "no_graph"])
@pytest.mark.parametrize("case", CASES)
def test_one_launch_per_layer_is_bit_identical(omx, runs, case, no_graph):
    """Tokens and last-step logits of 24 greedy steps: the default == OMX_ATTN_DOWN=0, under the graph and under OMX_NO_GRAPH=1, from the
    four start positions of tests/test_gpu_attn_gateup.py (one live split, the 16 -> 17 split edge, a chunk edge, a bucket edge with a
    graph rebuild mid-run)."""
    off, on = runs[(no_graph, "0")][case], runs[(no_graph, None)][case]
    assert off[4].startswith("eager" if no_graph else "graph") and on[4].startswith("eager" if no_graph else "graph"), (off[4], on[4])
    assert not off[2]["attn_down"] and not off[3]["attn_down"]
    assert off[3]["attn_gateup"] == _resident(omx) and off[3]["down_qkv"]
    assert on[2]["attn_down"] == _resident(omx) and on[3]["attn_down"] == _resident(omx), on[3]
    assert not on[3]["attn_gateup_gave_up"] and not on[3]["down_qkv_gave_up"]
    np.testing.assert_array_equal(off[0], on[0])
    np.testing.assert_array_equal(off[1], on[1])


def test_qwen2_wiring_is_bit_identical(omx, starts):
    """The same on the Qwen2-wired model (q/k/v bias, no q/k norm): the phase adds the bias the q/k/v GEMV adds."""
    off = _run_cases(WIDE3_BIAS, ["second_batch"], starts, "0", False)["second_batch"]
    on = _run_cases(WIDE3_BIAS, ["second_batch"], starts, None, False)["second_batch"]
    assert not off[3]["attn_down"] and on[3]["attn_down"] == _resident(omx)
    np.testing.assert_array_equal(off[0], on[0])
    np.testing.assert_array_equal(off[1], on[1])


def test_every_value_the_phases_consume_arrives_in_the_launch(omx, monkeypatch):
    """`act`, `qkv` and both hidden buffers filled with a NaN pattern before a step: its token and logits are those of the unpoisoned
    run and the buffers come back finite -- nothing the new phases consume is a plain load of what an earlier launch left."""
    monkeypatch.delenv("OMX_ATTN_DOWN", raising=False)
    cfg = WIDE3
    sizes = {"act": cfg.intermediate_size, "qkv": (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim,
             "h": cfg.hidden_size, "h2": cfg.hidden_size}
    prompt = synth.prompt_ids(37, cfg.vocab_size)
    m = _engine(cfg)
    want, want_logits = _continuation(m, prompt, 37, 3)
    m.reset()
    got = [m.prefill(prompt)] + list(m.decode(2))
    assert m.step_forms()["attn_down"] == _resident(omx)
    for name, n in sizes.items():
        poison = np.full(n, NAN16, np.uint16)
        omx.check(omx.lib.omx_qwen3_debug_write(m._h, name.encode(), poison.ctypes.data, n))
        np.testing.assert_array_equal(_bits(m, omx, name, n), poison)
    got += list(m.decode(1))
    logits = m.last_logits()
    after = {name: _f32(_bits(m, omx, name, n)) for name, n in sizes.items()}
    m.close()
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    np.testing.assert_array_equal(logits, want_logits)
    for name, v in after.items():
        assert np.isfinite(v).all(), f"{int((~np.isfinite(v)).sum())} of {v.size} values of {name} were not rewritten"


def test_repeats_on_one_engine(omx, runs, starts):
    """The hand-over race check of tests/test_gpu_hop_issue.py: the same 24-step continuation 20 times on one engine (reset between
    runs) -- the waves draw their units in whatever order the hardware schedules them -- equals the first and the two-launch layer."""
    if not _resident(omx):
        pytest.skip("the 256-block grid is not resident on this device: the form is never taken")
    prompt = synth.prompt_ids(1100, WIDE3.vocab_size)
    want = runs[(False, "0")]["second_batch"]
    with _env("OMX_ATTN_DOWN", None):
        m = _engine(WIDE3)
        got = [_continuation(m, prompt, starts["second_batch"]) for _ in range(REPEATS)]
        forms = m.step_forms()
        m.close()
    assert forms["attn_down"] and not forms["attn_gateup_gave_up"] and not forms["down_qkv_gave_up"], forms
    for toks, logits in got:
        np.testing.assert_array_equal(toks, got[0][0])
        np.testing.assert_array_equal(logits, got[0][1])
        np.testing.assert_array_equal(toks, want[0])
        np.testing.assert_array_equal(logits, want[1])


def test_trace_counts_units_and_rows(omx, monkeypatch):
    """The traced instantiation: every block of the two fused layers reports 32 down units reduced and 24 q/k/v rows stored (a unit
    nobody drew or one drawn twice changes the count); the last layer's launch does not take the form and leaves the word 0."""
    monkeypatch.delenv("OMX_ATTN_DOWN", raising=False)
    if not _resident(omx):
        pytest.skip("the 256-block grid is not resident on this device: the form is never taken")
    m = _engine(WIDE3)
    m.prefill(synth.prompt_ids(37, WIDE3.vocab_size))
    m.decode(2)
    L = WIDE3.num_hidden_layers
    buf = np.zeros(L * 256 * TRACE_WORDS, np.uint64)
    nb = ctypes.c_int()
    omx.check(omx.lib.omx_qwen3_debug_trace_step(m._h, buf.ctypes.data, buf.size, ctypes.byref(nb)))
    m.close()
    assert nb.value == 256
    word = buf.reshape(L, 256, TRACE_WORDS)[:, :, 15]
    units, rows = word & np.uint64(0xFFFFFFFF), word >> np.uint64(32)
    print("down units per block: min", units[:L - 1].min(), "max", units[:L - 1].max(), " q/k/v rows per block: min", rows[:L - 1].min(),
          "max", rows[:L - 1].max())
    np.testing.assert_array_equal(units[:L - 1], np.full_like(units[:L - 1], BLOCK_UNITS))
    np.testing.assert_array_equal(rows[:L - 1], np.full_like(rows[:L - 1], BLOCK_QKV_ROWS))
    np.testing.assert_array_equal(word[L - 1], np.zeros_like(word[L - 1]))
    stamps = buf.reshape(L, 256, TRACE_WORDS)[:L - 1, :, 11:15]
    assert (stamps > 0).all(), "a stamp of the down / q/k/v phases is missing"


def test_give_up_takes_the_first_rung(omx, monkeypatch):
    """The give-up word raised from the host (never by starving a launch): the decode call replays and returns the tokens and logits of
    an undisturbed engine; the form is off with the two folds it joins, the O projection stays in the attention launch, and
    decode_path() names the first rung only."""
    for name in ("OMX_ATTN_DOWN", "OMX_ATTN_GATEUP", "OMX_DOWN_QKV"):
        monkeypatch.delenv(name, raising=False)
    if not _resident(omx):
        pytest.skip("the 256-block grid is not resident on this device: the form is never taken")
    prompt = synth.prompt_ids(64, WIDE3.vocab_size)
    a = _engine(WIDE3)
    want = np.concatenate([[a.prefill(prompt)], a.decode(14)])
    want_logits = a.last_logits()
    assert "disabled" not in a.decode_path()
    a.close()
    b = _engine(WIDE3)
    got = [b.prefill(prompt)] + list(b.decode(4))
    assert b.step_forms()["attn_down"] and "disabled" not in b.decode_path()
    b.raise_give_up()
    got += list(b.decode(6))
    forms = b.step_forms()
    assert not forms["attn_down"] and not forms["attn_gateup"] and not forms["down_qkv"] and forms["attn_oproj"], forms
    assert b.decode_path().endswith(" gateup_disabled chain_disabled"), b.decode_path()
    got += list(b.decode(4))
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    np.testing.assert_array_equal(b.last_logits(), want_logits)
    b.close()


def test_switches_and_overrides_keep_the_launches(omx, monkeypatch):
    """Its own switch, the switch of either fold it joins, the O projection out of the launch or a rows-per-wave override of any GEMV
    the launch stands for turns the form off; intermediate 11008 never takes it."""
    names = ("OMX_ATTN_DOWN", "OMX_ATTN_GATEUP", "OMX_DOWN_QKV", "OMX_ATTN_OPROJ", "OMX_GEMV_RPW_O", "OMX_GEMV_RPW_GU", "OMX_GEMV_RPW_QKV",
             "OMX_GEMV_RPW_DOWN")
    for name in names:
        monkeypatch.delenv(name, raising=False)
    m = _engine(WIDE3)
    m.prefill(synth.prompt_ids(16, WIDE3.vocab_size))
    m.decode(1)
    assert m.step_forms()["attn_down"] == _resident(omx)
    for name in names:
        monkeypatch.setenv(name, "4" if "RPW" in name else "0")
        assert not m.step_forms()["attn_down"], name
        monkeypatch.delenv(name)
    assert m.step_forms()["attn_down"] == _resident(omx)
    m.close()
    m = _engine(OTHER_FFN3, max_context=1280)
    m.prefill(synth.prompt_ids(16, OTHER_FFN3.vocab_size))
    m.decode(1)
    assert not m.step_forms()["attn_down"]
    m.close()


def test_timing_hook_splits_the_layer_launch(omx, monkeypatch):
    """omx_qwen3_time_step_kernels with the form on: the gate/up and down pairs of a fused layer are never armed and never read, every
    class stays positive and the timed steps are ordinary steps."""
    monkeypatch.delenv("OMX_ATTN_DOWN", raising=False)
    prompt = synth.prompt_ids(48, WIDE3.vocab_size)
    a = _engine(WIDE3)
    want = np.concatenate([[a.prefill(prompt)], a.decode(12)])
    a.close()
    want = np.concatenate([want[:5], want[7:]])
    b = _engine(WIDE3)
    got = [b.prefill(prompt)] + list(b.decode(4))
    assert b.step_forms()["attn_down"] == _resident(omx)
    us = b.time_step_kernels(2)
    got += list(b.decode(6))
    print("time_step_kernels:", us)
    assert all(0 < us[k] < 1000 for k in ("qkv", "attention", "gate_up", "down", "lm_head")), us
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    b.close()


def test_hidden_row_against_float64(omx, monkeypatch):
    """One decode step behind a 37-token prompt: the hidden row behind the LAST layer's O projection (buffer h2: every layer enters on h
    and the O projection writes the ping-pong partner) -- two fused layers in front of it -- against the float64 forward of
    oracle/ref_qwen3.py for the same prompt and step, at the bound the engine tests hold a whole model's output to
    (tests/test_gpu_qwen3.py: 2^-7 max|ref| sqrt(layers))."""
    monkeypatch.delenv("OMX_ATTN_DOWN", raising=False)
    cfg, BF = WIDE3, "bf16"
    hd = cfg.hidden_size
    prompt = synth.prompt_ids(37, cfg.vocab_size)
    m = _engine(cfg)
    first = m.prefill(prompt)
    m.decode(1)
    assert m.step_forms()["attn_down"] == _resident(omx)
    row = _f32(_bits(m, omx, "h2", hd))
    w = {}
    for name, shape in rq.weight_shapes(cfg).items():   # the engine's own weights: bf16 bits, widened exactly
        ptr, nb = ctypes.c_void_p(), ctypes.c_size_t()
        omx.check(omx.lib.omx_qwen3_get_weight(m._h, name.encode(), ctypes.byref(ptr), ctypes.byref(nb)))
        raw = np.empty(int(np.prod(shape)), np.uint16)
        assert nb.value == raw.nbytes, name
        omx.check(omx.lib.omx_memcpy_d2h(raw.ctypes.data, ptr, raw.nbytes, None))
        w[name] = _f32(raw).reshape(shape)
    m.close()
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
