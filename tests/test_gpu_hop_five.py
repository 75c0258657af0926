"""Hop five of the layer launch (csrc/attn_step.hip down_qkv_phase): the next layer's q/k/v rows are asked for around the residual row's
crossing instead of around the activation vector's.  Only the point at which loads are issued moves, so everything is compared BIT FOR BIT
with the two-launch layer (OMX_ATTN_DOWN=0), and the traced instantiation's stamps must stay in the order of the phases.
The form is gated on the widths, so the models are the 3-layer wide ones of tests/test_gpu_layer_launch.py (two layers take the form)."""
import ctypes

import numpy as np
import pytest

from oracle import synth
from test_gpu_attn_gateup import _engine, _resident, starts   # noqa: F401  (starts: the module-scoped fixture)
from test_gpu_hop_issue import _env
from test_gpu_layer_launch import NAN16, TRACE_WORDS, WIDE3, WIDE3_BIAS, _bits, _continuation, _f32

pytestmark = pytest.mark.gpu

REPEATS = 20
STARTS = ["second_batch", "chunk_edge"]
BLOCK_PAIRS, BLOCK_UNITS, BLOCK_QKV_ROWS = 48, 32, 24
WIRINGS = {"qwen3": WIDE3, "qwen2": WIDE3_BIAS}


def _needs_resident(omx):
    if not _resident(omx):
        pytest.skip("the 256-block grid is not resident on this device: the form is never taken")


def _qkv_size(cfg):
    return (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim


def _buffers_after_one_step(omx, cfg, down):
    """`qkv`, `h` and `h2` as one decode step from a 37-token prompt leaves them, the step's token and logits, the forms"""
    sizes = {"qkv": _qkv_size(cfg), "h": cfg.hidden_size, "h2": cfg.hidden_size}
    with _env("OMX_ATTN_DOWN", down):
        m = _engine(cfg)
        first = m.prefill(synth.prompt_ids(37, cfg.vocab_size))
        toks = np.concatenate([[first], m.decode(1)])
        logits = m.last_logits().copy()
        bufs = {name: _bits(m, omx, name, n).copy() for name, n in sizes.items()}
        forms = m.step_forms()
        m.close()
    return bufs, toks, logits, forms


@pytest.mark.parametrize("wiring", list(WIRINGS))
def test_rows_bit_for_bit(omx, wiring):
    """After one decode step the last fused launch's q/k/v rows (`qkv`: the bias epilogue and the clamped surplus rows on the Qwen2 wiring)
    and both hidden buffers equal those of the two-launch layer, bit for bit."""
    _needs_resident(omx)
    cfg = WIRINGS[wiring]
    want, want_toks, want_logits, off = _buffers_after_one_step(omx, cfg, "0")
    got, got_toks, got_logits, on = _buffers_after_one_step(omx, cfg, None)
    assert not off["attn_down"], off
    assert on["attn_down"] and not on["attn_gateup_gave_up"] and not on["down_qkv_gave_up"], on
    for name in want:
        assert np.isfinite(_f32(want[name])).all(), name
        diff = int((got[name] != want[name]).sum())
        print(f"{wiring} {name}: {diff} of {want[name].size} values differ")
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    np.testing.assert_array_equal(got_toks, want_toks)
    np.testing.assert_array_equal(got_logits, want_logits)


def _repeats(cfg, starts, down, no_graph, repeats):
    """{start: [(tokens, last logits)] * repeats} of ONE engine, reset between the runs, and its forms at the end"""
    prompt = synth.prompt_ids(1100, cfg.vocab_size)
    with _env("OMX_ATTN_DOWN", down), _env("OMX_NO_GRAPH", "1" if no_graph else None):
        m = _engine(cfg)
        out = {s: [_continuation(m, prompt, starts[s]) for _ in range(repeats)] for s in STARTS}
        forms, path = m.step_forms(), m.decode_path()
        m.close()
    return out, forms, path


@pytest.fixture(scope="module")
def two_launch(omx, starts):
    """the reference, once per wiring and mode: {(wiring, no_graph): {start: (tokens, last logits)}} with OMX_ATTN_DOWN=0"""
    ref = {}
    for wiring, cfg in WIRINGS.items():
        for ng in (False, True):
            out, forms, _ = _repeats(cfg, starts, "0", ng, 1)
            assert not forms["attn_down"], forms
            ref[(wiring, ng)] = {s: out[s][0] for s in STARTS}
    return ref


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "no_graph"])
@pytest.mark.parametrize("wiring", list(WIRINGS))
def test_twenty_continuations_equal_the_two_launch_layer(omx, two_launch, starts, wiring, no_graph):
    """Twenty 24-step continuations on one engine from each of the two starts -- the waves meet the residual row's sweep in whatever order
    the hardware schedules them -- equal OMX_ATTN_DOWN=0 bit for bit, tokens and last logits; the form is taken and nothing gave up."""
    _needs_resident(omx)
    got, forms, path = _repeats(WIRINGS[wiring], starts, None, no_graph, REPEATS)
    assert path.startswith("eager" if no_graph else "graph"), path
    assert forms["attn_down"] and not forms["attn_gateup_gave_up"] and not forms["down_qkv_gave_up"], forms
    for s in STARTS:
        want = two_launch[(wiring, no_graph)][s]
        for toks, logits in got[s]:
            np.testing.assert_array_equal(toks, want[0])
            np.testing.assert_array_equal(logits, want[1])


def test_stamp_order(omx, monkeypatch):
    """Per fused layer and block of the traced instantiation: first unit reduced (word 12) <= residual row swept (13) <= rows stored (14);
    the counts read 48 pairs, 32 units and 24 rows."""
    monkeypatch.delenv("OMX_ATTN_DOWN", raising=False)
    _needs_resident(omx)
    m = _engine(WIDE3)
    m.prefill(synth.prompt_ids(37, WIDE3.vocab_size))
    m.decode(2)
    L = WIDE3.num_hidden_layers
    buf = np.zeros(L * 256 * TRACE_WORDS, np.uint64)
    nb = ctypes.c_int()
    omx.check(omx.lib.omx_qwen3_debug_trace_step(m._h, buf.ctypes.data, buf.size, ctypes.byref(nb)))
    m.close()
    assert nb.value == 256
    t = buf.reshape(L, 256, TRACE_WORDS)[:L - 1].astype(np.int64)
    assert (t[:, :, [12, 13, 14]] > 0).all(), "a stamp is missing"
    chain = [("first unit", t[:, :, 12]), ("row swept", t[:, :, 13]), ("rows stored", t[:, :, 14])]
    t0 = t[:, :, 0].min(axis=1, keepdims=True)
    for name, v in chain:
        print(f"{name:12s} median {np.median(v - t0) / 100.0:6.2f} us after the launch's first block start")
    for (na, va), (nb_, vb) in zip(chain, chain[1:]):
        assert (va <= vb).all(), f"'{na}' after '{nb_}' in {int((va > vb).sum())} blocks"
    np.testing.assert_array_equal(t[:, :, 10], np.full_like(t[:, :, 10], BLOCK_PAIRS))
    np.testing.assert_array_equal(t[:, :, 15] & 0xFFFFFFFF, np.full_like(t[:, :, 15], BLOCK_UNITS))
    np.testing.assert_array_equal(t[:, :, 15] >> 32, np.full_like(t[:, :, 15], BLOCK_QKV_ROWS))


def test_stale_qkv_is_never_read(omx, monkeypatch):
    """`qkv` filled with a bf16 NaN pattern before EACH of three consecutive steps: every step gives the token and logits of the clean run
    and leaves `qkv` finite -- the rows the attention phase reads are the ones the launch before it stored, wherever they were asked for."""
    monkeypatch.delenv("OMX_ATTN_DOWN", raising=False)
    _needs_resident(omx)
    cfg = WIDE3
    n = _qkv_size(cfg)
    prompt = synth.prompt_ids(37, cfg.vocab_size)
    m = _engine(cfg)
    m.reset()
    want_toks, want_logits = [m.prefill(prompt)] + list(m.decode(2)), []
    for _ in range(3):
        want_toks += list(m.decode(1))
        want_logits.append(m.last_logits().copy())
    m.reset()
    got = [m.prefill(prompt)] + list(m.decode(2))
    assert m.step_forms()["attn_down"]
    poison = np.full(n, NAN16, np.uint16)
    for step in range(3):
        omx.check(omx.lib.omx_qwen3_debug_write(m._h, b"qkv", poison.ctypes.data, n))
        np.testing.assert_array_equal(_bits(m, omx, "qkv", n), poison)
        got += list(m.decode(1))
        np.testing.assert_array_equal(m.last_logits(), want_logits[step])
        v = _f32(_bits(m, omx, "qkv", n))
        assert np.isfinite(v).all(), f"step {step}: {int((~np.isfinite(v)).sum())} of {v.size} values of qkv were not rewritten"
    forms = m.step_forms()
    m.close()
    assert not forms["attn_gateup_gave_up"] and not forms["down_qkv_gave_up"], forms
    np.testing.assert_array_equal(np.array(got, np.uint32), np.array(want_toks, np.uint32))
