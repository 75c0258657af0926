"""Hop three of the layer launch (csrc/attn_step.hip gateup_phase): an O block stores its O rows as granules BEFORE its waves ask for their
first (gate, up) pair, and wave 0's first pass over the hidden row goes out without a watch in front of it (EXPERIMENTS C-7).
Only the point at which a store and loads are issued moves, so everything is compared BIT FOR BIT with the separate gate/up launch
(OMX_ATTN_GATEUP=0) and with the two-launch layer (OMX_ATTN_DOWN=0), and the traced instantiation's stamps must stay in the order of the
phases.
The form is gated on the widths, so the models are the 3-layer wide ones of tests/test_gpu_layer_launch.py (two layers take the form)."""
import ctypes

import numpy as np
import pytest

from oracle import synth
from test_gpu_attn_gateup import _engine, _resident, starts   # noqa: F401  (starts: the module-scoped fixture)
from test_gpu_hop_five import _qkv_size
from test_gpu_hop_four import BLOCK_PAIRS, BLOCK_QKV_ROWS, BLOCK_UNITS
from test_gpu_hop_issue import _env
from test_gpu_layer_launch import NAN16, TRACE_WORDS, WIDE3, WIDE3_BIAS, _bits, _continuation, _f32

pytestmark = pytest.mark.gpu

REPEATS = 20
STARTS = ["second_batch", "chunk_edge"]
WIRINGS = {"qwen3": WIDE3, "qwen2": WIDE3_BIAS}
CONSUMER_BLOCKS = 32      # one per query head, the launch's first blocks; the 224 behind them hold the O rows and publish them


def _needs_resident(omx):
    if not _resident(omx):
        pytest.skip("the 256-block grid is not resident on this device: the form is never taken")


def _buffers_after_one_step(cfg, omx, switch):
    """both hidden buffers, the gate/up output and `qkv` as one decode step from a 37-token prompt leaves them; the step's token, its
    logits and the forms.  `switch`: the environment variable set to 0 for the run (None: the default, the layer launch)"""
    sizes = {"h": cfg.hidden_size, "h2": cfg.hidden_size, "act": cfg.intermediate_size, "qkv": _qkv_size(cfg)}
    with _env(switch or "OMX_ATTN_DOWN", "0" if switch else None):
        m = _engine(cfg)
        first = m.prefill(synth.prompt_ids(37, cfg.vocab_size))
        toks = np.concatenate([[first], m.decode(1)])
        logits = m.last_logits().copy()
        bufs = {name: _bits(m, omx, name, n).copy() for name, n in sizes.items()}
        forms = m.step_forms()
        m.close()
    return bufs, toks, logits, forms


@pytest.mark.parametrize("wiring", list(WIRINGS))
def test_buffers_bit_for_bit_after_one_step(omx, monkeypatch, wiring):
    """After one decode step `h`, `h2`, `act` and `qkv`, the token and the logits of the layer launch equal those of the step with gate/up
    as a launch of its own and those of the two-launch layer, bit for bit, and are finite."""
    for name in ("OMX_ATTN_DOWN", "OMX_ATTN_GATEUP"):
        monkeypatch.delenv(name, raising=False)
    _needs_resident(omx)
    cfg = WIRINGS[wiring]
    got, got_toks, got_logits, on = _buffers_after_one_step(cfg, omx, None)
    assert on["attn_down"] and on["attn_gateup"] and not on["attn_gateup_gave_up"] and not on["down_qkv_gave_up"], on
    assert np.isfinite(got_logits).all()
    for switch, form in (("OMX_ATTN_GATEUP", "attn_gateup"), ("OMX_ATTN_DOWN", "attn_down")):
        want, want_toks, want_logits, off = _buffers_after_one_step(cfg, omx, switch)
        assert not off[form] and not off["attn_down"], (switch, off)
        for name in want:
            assert np.isfinite(_f32(got[name])).all(), name
            diff = int((got[name] != want[name]).sum())
            print(f"{wiring} against {switch}=0, {name}: {diff} of {want[name].size} values differ")
            np.testing.assert_array_equal(got[name], want[name], err_msg=f"{name} against {switch}=0")
        np.testing.assert_array_equal(got_toks, want_toks)
        np.testing.assert_array_equal(got_logits, want_logits)


def _repeats(cfg, starts, gateup, no_graph, repeats):
    """{start: [(tokens, last logits)] * repeats} of ONE engine, reset between the runs, its forms and its path at the end"""
    prompt = synth.prompt_ids(1100, cfg.vocab_size)
    with _env("OMX_ATTN_GATEUP", gateup), _env("OMX_NO_GRAPH", "1" if no_graph else None):
        m = _engine(cfg)
        out = {s: [_continuation(m, prompt, starts[s]) for _ in range(repeats)] for s in STARTS}
        forms, path = m.step_forms(), m.decode_path()
        m.close()
    return out, forms, path


@pytest.fixture(scope="module")
def separate_gateup(omx, starts):
    """the reference, once per wiring and mode: {(wiring, no_graph): {start: (tokens, last logits)}} with OMX_ATTN_GATEUP=0"""
    ref = {}
    if not _resident(omx):
        return ref
    for wiring, cfg in WIRINGS.items():
        for ng in (False, True):
            out, forms, _ = _repeats(cfg, starts, "0", ng, 1)
            assert not forms["attn_gateup"] and not forms["attn_down"], forms
            ref[(wiring, ng)] = {s: out[s][0] for s in STARTS}
    return ref


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "no_graph"])
@pytest.mark.parametrize("wiring", list(WIRINGS))
def test_twenty_continuations_equal_the_separate_gateup_launch(omx, monkeypatch, separate_gateup, starts, wiring, no_graph):
    """Twenty 24-step continuations on one engine from each of the two starts -- the blocks publish, and the waves meet the hidden row's
    sweep, in whatever order the hardware schedules them -- equal OMX_ATTN_GATEUP=0 bit for bit, tokens and last logits; the form is
    taken and nothing gave up."""
    for name in ("OMX_ATTN_DOWN", "OMX_ATTN_GATEUP"):
        monkeypatch.delenv(name, raising=False)
    _needs_resident(omx)
    got, forms, path = _repeats(WIRINGS[wiring], starts, None, no_graph, REPEATS)
    assert path.startswith("eager" if no_graph else "graph"), path
    assert forms["attn_down"] and forms["attn_gateup"] and not forms["attn_gateup_gave_up"] and not forms["down_qkv_gave_up"], forms
    for s in STARTS:
        want = separate_gateup[(wiring, no_graph)][s]
        assert len(got[s]) == REPEATS
        for toks, logits in got[s]:
            np.testing.assert_array_equal(toks, want[0])
            np.testing.assert_array_equal(logits, want[1])


def test_stamp_order(omx, monkeypatch):
    """Per fused layer and block of the traced instantiation: O rows stored (word 6, O blocks) <= hidden row swept (4, O blocks) <= first
    pair reduced (7) <= last pair of wave 0 (8); in every block, the consumers included, the first-pair stamp is not later than the
    last-pair stamp; the counts read 48 pairs, 32 units and 24 rows."""
    for name in ("OMX_ATTN_DOWN", "OMX_ATTN_GATEUP"):
        monkeypatch.delenv(name, raising=False)
    _needs_resident(omx)
    m = _engine(WIDE3)
    m.prefill(synth.prompt_ids(37, WIDE3.vocab_size))
    m.decode(2)
    L = WIDE3.num_hidden_layers
    buf = np.zeros(L * 256 * TRACE_WORDS, np.uint64)
    nb = ctypes.c_int()
    omx.check(omx.lib.omx_qwen3_debug_trace_step(m._h, buf.ctypes.data, buf.size, ctypes.byref(nb)))
    forms = m.step_forms()
    m.close()
    assert nb.value == 256
    assert forms["attn_down"] and not forms["attn_gateup_gave_up"] and not forms["down_qkv_gave_up"], forms
    t = buf.reshape(L, 256, TRACE_WORDS)[:L - 1].astype(np.int64)
    assert (t[:, :, [7, 8]] > 0).all() and (t[:, CONSUMER_BLOCKS:, [4, 6]] > 0).all(), "a stamp is missing"
    o = t[:, CONSUMER_BLOCKS:]
    chain = [("O rows stored", o[:, :, 6]), ("hidden row swept", o[:, :, 4]), ("first pair reduced", o[:, :, 7]),
             ("last pair of wave 0", o[:, :, 8])]
    t0 = t[:, :, 0].min(axis=1, keepdims=True)
    for name, v in chain:
        print(f"{name:20s} median {np.median(v - t0) / 100.0:6.2f} us after the launch's first block start")
    for (na, va), (nb_, vb) in zip(chain, chain[1:]):
        assert (va <= vb).all(), f"'{na}' after '{nb_}' in {int((va > vb).sum())} blocks"
    assert (t[:, :, 7] <= t[:, :, 8]).all(), f"first pair after the last in {int((t[:, :, 7] > t[:, :, 8]).sum())} blocks"
    np.testing.assert_array_equal(t[:, :, 10], np.full_like(t[:, :, 10], BLOCK_PAIRS))
    np.testing.assert_array_equal(t[:, :, 15] & 0xFFFFFFFF, np.full_like(t[:, :, 15], BLOCK_UNITS))
    np.testing.assert_array_equal(t[:, :, 15] >> 32, np.full_like(t[:, :, 15], BLOCK_QKV_ROWS))


def test_three_poisoned_steps(omx, monkeypatch):
    """`h2` -- the hidden buffer the O rows are stored to: every layer enters on `h` and the O projection writes its ping-pong partner --
    and `act` filled with a bf16 NaN pattern before EACH of three consecutive steps: every step gives the token and logits of the clean
    run and leaves both buffers finite -- the hidden row every block normalises arrives inside the launch, published first or not."""
    for name in ("OMX_ATTN_DOWN", "OMX_ATTN_GATEUP"):
        monkeypatch.delenv(name, raising=False)
    _needs_resident(omx)
    cfg = WIDE3
    sizes = {"h2": cfg.hidden_size, "act": cfg.intermediate_size}
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
    for step in range(3):
        for name, n in sizes.items():
            poison = np.full(n, NAN16, np.uint16)
            omx.check(omx.lib.omx_qwen3_debug_write(m._h, name.encode(), poison.ctypes.data, n))
            np.testing.assert_array_equal(_bits(m, omx, name, n), poison)
        got += list(m.decode(1))
        np.testing.assert_array_equal(m.last_logits(), want_logits[step])
        for name, n in sizes.items():
            v = _f32(_bits(m, omx, name, n))
            assert np.isfinite(v).all(), f"step {step}: {int((~np.isfinite(v)).sum())} of {v.size} values of {name} were not rewritten"
    forms = m.step_forms()
    m.close()
    assert not forms["attn_gateup_gave_up"] and not forms["down_qkv_gave_up"], forms
    np.testing.assert_array_equal(np.array(got, np.uint32), np.array(want_toks, np.uint32))
