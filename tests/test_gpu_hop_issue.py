"""Weight loads queued behind the sweeps of the decode step's two fused launches, and (gate, up) pairs drawn from a ticket counter inside
the block (csrc/attn_step.hip oproj_await_vector / gateup_phase, csrc/gemv_chain.hip phase B).  Nothing of that changes what is computed --
a pair's value depends on its two weight rows and the row in LDS, not on the wave that reduces it or on when its loads were asked for --
so everything is compared BIT FOR BIT with the separate launches (OMX_ATTN_GATEUP=0, OMX_DOWN_QKV=0).  tests/test_gpu_attn_gateup.py and
tests/test_gpu_down_qkv_chain.py hold one run of each form to that; this file adds what one run cannot see: a pair nobody drew, a pair
drawn twice, a result that depends on the order the waves drew in, and the give-up path through the phase's barriers.  The forms are
taken at one shape only (hidden 4096, intermediate 12288, 32 / 8 heads of 128, a 256-block split plan, at least 256 CUs): the models are
those of the two files."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ref_qwen3 as rq
from oracle import synth
from test_gpu_attn_gateup import CAP, STEPS, WIDE, _engine, _resident, starts   # noqa: F401  (starts: the module-scoped fixture)
from test_gpu_down_qkv_chain import WIDE_BIAS

pytestmark = pytest.mark.gpu

CASES = ["one_split", "second_batch", "chunk_edge", "bucket_edge"]
REPEATS = 20
BLOCK_PAIRS = 48          # (gate, up) pairs per block of the fused launch: 12 288 over 256 blocks
TRACE_WORDS = 16          # words per block of omx_qwen3_debug_trace_step; word 10: the pairs the block's waves reduced
ONE_LAYER = rq.Qwen3Config(4096, 1, 12288, 32, 8, 128, 1024, 1e-6, 1e6, False)


class _env:
    """os.environ[name] = value (None: unset) for a with-block"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.saved = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.saved


def _skip_unless_resident(omx):
    if not _resident(omx):
        pytest.skip("the 256-block grid is not resident on this device: the forms are never taken")


def _continuation(m, prompt, start):
    m.reset()
    first = m.prefill(prompt[:start])
    return np.concatenate([[first], m.decode(STEPS)]), m.last_logits()


def _bits(m, omx, name, n):
    raw = np.empty(n, np.uint16)
    omx.check(omx.lib.omx_qwen3_debug_read(m._h, name.encode(), raw.ctypes.data, n))
    return raw


def test_every_pair_is_written_exactly_once(omx):
    """One decode step of a one-layer engine on an `act` buffer poisoned with a bf16 NaN pattern: all 12 288 values come back finite (a
    pair nobody drew leaves NaN) and bit-equal to the same step with gate/up as its own launch.  A pair drawn twice is written twice with
    the same bits, so it is caught by a count instead: the traced instantiation reports per block the pairs its waves reduced, 48."""
    _skip_unless_resident(omx)
    I = ONE_LAYER.intermediate_size
    prompt = synth.prompt_ids(37, ONE_LAYER.vocab_size)
    poison = np.full(I, 0x7FC1, np.uint16)
    acts = {}
    for mode in ("0", None):
        with _env("OMX_ATTN_GATEUP", mode):
            m = _engine(ONE_LAYER)
            m.prefill(prompt)
            m.decode(2)
            assert m.step_forms()["attn_gateup"] == (mode is None)
            omx.check(omx.lib.omx_qwen3_debug_write(m._h, b"act", poison.ctypes.data, I))
            np.testing.assert_array_equal(_bits(m, omx, "act", I), poison)
            m.decode(1)
            acts[mode] = _bits(m, omx, "act", I)
            if mode is None:
                # the traced launch of the next step: poisoned again, every block reports its count
                omx.check(omx.lib.omx_qwen3_debug_write(m._h, b"act", poison.ctypes.data, I))
                buf = np.zeros(ONE_LAYER.num_hidden_layers * 256 * TRACE_WORDS, np.uint64)
                nb = ctypes.c_int()
                omx.check(omx.lib.omx_qwen3_debug_trace_step(m._h, buf.ctypes.data, buf.size, ctypes.byref(nb)))
                assert nb.value == 256
                counts = buf.reshape(-1, 256, TRACE_WORDS)[:, :, 10]
                print("pairs reduced per block: min", counts.min(), "max", counts.max())
                np.testing.assert_array_equal(counts, np.full_like(counts, BLOCK_PAIRS))
                traced = _bits(m, omx, "act", I)
                assert np.isfinite((traced.astype(np.uint32) << np.uint32(16)).view(np.float32)).all()
            m.close()
    on = (acts[None].astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert np.isfinite(on).all(), f"{int((~np.isfinite(on)).sum())} of {I} activations were not written"
    np.testing.assert_array_equal(acts["0"], acts[None])


@pytest.fixture(scope="module")
def gateup_runs(omx, starts):
    """{case: (two-launch result, [REPEATS results of ONE engine with the form on])}, a result = (tokens, last-step logits)"""
    prompt = synth.prompt_ids(1100, WIDE.vocab_size)
    out = {}
    with _env("OMX_ATTN_GATEUP", "0"):
        m = _engine(WIDE)
        for case in CASES:
            out[case] = [_continuation(m, prompt, starts[case]), []]
        assert not m.step_forms()["attn_gateup"]
        m.close()
    with _env("OMX_ATTN_GATEUP", None):
        m = _engine(WIDE)
        for case in CASES:
            for _ in range(REPEATS):
                out[case][1].append(_continuation(m, prompt, starts[case]))
        out["forms"] = m.step_forms()
        m.close()
    return out


@pytest.mark.parametrize("case", CASES)
def test_claim_order_does_not_matter(omx, gateup_runs, case):
    """The same 24-step greedy continuation 20 times on one engine (reset between runs): the waves draw their pairs in whatever order
    the hardware schedules them, tokens and last-step logits are the two-launch step's every time."""
    _skip_unless_resident(omx)
    assert gateup_runs["forms"]["attn_gateup"] == _resident(omx) and not gateup_runs["forms"]["attn_gateup_gave_up"], gateup_runs["forms"]
    want, got = gateup_runs[case]
    assert len(got) == REPEATS
    for toks, logits in got:
        np.testing.assert_array_equal(toks, want[0])
        np.testing.assert_array_equal(logits, want[1])


def test_give_up_passes_every_barrier(omx, monkeypatch):
    """The give-up word raised from the host (the condition of test_give_up_takes_the_first_rung, nothing beyond it): the decode call
    returns, decode_path() names the first rung, and the replayed tokens and logits are those of an engine that ran on the separate
    launches from the start."""
    monkeypatch.delenv("OMX_ATTN_GATEUP", raising=False)
    monkeypatch.delenv("OMX_DOWN_QKV", raising=False)
    _skip_unless_resident(omx)
    prompt = synth.prompt_ids(64, WIDE.vocab_size)
    with _env("OMX_ATTN_GATEUP", "0"), _env("OMX_DOWN_QKV", "0"):
        a = _engine(WIDE)
        want = np.concatenate([[a.prefill(prompt)], a.decode(14)])
        want_logits = a.last_logits()
        forms = a.step_forms()
        assert not forms["attn_gateup"] and not forms["down_qkv"], forms
        a.close()
    b = _engine(WIDE)
    got = [b.prefill(prompt)] + list(b.decode(4))
    assert b.step_forms()["attn_gateup"] and b.step_forms()["down_qkv"] and "disabled" not in b.decode_path()
    b.raise_give_up()
    got += list(b.decode(6))
    assert b.decode_path().endswith(" gateup_disabled chain_disabled"), b.decode_path()
    forms = b.step_forms()
    assert not forms["attn_gateup"] and forms["attn_gateup_gave_up"] and forms["attn_oproj"], forms
    got += list(b.decode(4))
    np.testing.assert_array_equal(np.array(got, np.uint32), want.astype(np.uint32))
    np.testing.assert_array_equal(b.last_logits(), want_logits)
    b.close()


@pytest.fixture(scope="module")
def chain_runs(omx, starts):
    """the same on the down -> q/k/v edge: the Qwen2-wired model (q/k/v bias, no q/k norm), OMX_DOWN_QKV=0 against the default"""
    prompt = synth.prompt_ids(1100, WIDE_BIAS.vocab_size)
    out = {}
    with _env("OMX_DOWN_QKV", "0"):
        m = _engine(WIDE_BIAS)
        for case in CASES:
            out[case] = [_continuation(m, prompt, starts[case]), []]
        assert not m.step_forms()["down_qkv"]
        m.close()
    with _env("OMX_DOWN_QKV", None):
        m = _engine(WIDE_BIAS)
        for case in CASES:
            for _ in range(REPEATS):
                out[case][1].append(_continuation(m, prompt, starts[case]))
        out["forms"] = m.step_forms()
        m.close()
    return out


@pytest.mark.parametrize("case", CASES)
def test_chain_edge_repeats(omx, chain_runs, case):
    """q/k/v rows asked for behind the residual row's sweep: 20 repeats of the continuation on one engine equal the two-launch step."""
    _skip_unless_resident(omx)   # (256 CUs hold the chain's 512 workgroups as well)
    assert chain_runs["forms"]["down_qkv"] and not chain_runs["forms"]["down_qkv_gave_up"], chain_runs["forms"]
    want, got = chain_runs[case]
    assert len(got) == REPEATS
    for toks, logits in got:
        np.testing.assert_array_equal(toks, want[0])
        np.testing.assert_array_equal(logits, want[1])
