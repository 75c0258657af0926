"""CPU: the rule module tests/qwen3_asr_rule.py held to the frozen decoder oracle, so that the yardstick of the embedding-row prompt
pass is itself checked: forward_from_rows fed the oracle's own embedding rows IS Qwen3Oracle.forward."""
import numpy as np
import pytest

import qwen3_asr_rule as rule
from oracle import ref_core as rc
from oracle import ref_qwen3 as rq
from oracle import synth

CFG = rq.Qwen3Config(128, 2, 256, 4, 2, 32, 512, 1e-6, 1e6, True)


def _oracle(kind):
    if kind == "bf16":
        return rq.Qwen3Oracle(CFG, rq.synth_weights(CFG))
    if kind == "f16":
        return rq.Qwen3Oracle(CFG, rq.synth_weights(CFG, dt="f16"), dt="f16")
    return rq.Qwen3Oracle(CFG, rq.quantize_weights(CFG, rq.synth_weights(CFG), 4, 64), quant=(4, 64))


@pytest.mark.parametrize("kind", ["bf16", "f16", "q4"])
def test_forward_from_rows_on_own_rows_is_forward(kind):
    oracle = _oracle(kind)
    ids = synth.prompt_ids(19, CFG.vocab_size)
    pre, ids = ids[:5], ids[5:]
    # empty cache
    want = oracle.forward(ids[None, :], [])
    got = rule.forward_from_rows(oracle, rule.embed_rows(oracle, ids), [])
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # on top of cached tokens, and a single row (no mask)
    ca, cb = [], []
    oracle.forward(pre[None, :], ca)
    rule.forward_from_rows(oracle, rule.embed_rows(oracle, pre), cb)
    for chunk in (ids[:13], ids[13:]):
        want = oracle.forward(chunk[None, :], ca)
        got = rule.forward_from_rows(oracle, rule.embed_rows(oracle, chunk)[None], cb)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert ca[0].offset() == cb[0].offset() == 19
    # and the greedy loop from rows is the oracle's own
    want_t, want_l = oracle.generate(ids, 5, return_logits=True)
    got_t, got_l = rule.generate_from_rows(oracle, rule.embed_rows(oracle, ids), 5)
    np.testing.assert_array_equal(got_t, want_t)
    np.testing.assert_array_equal(got_l.view(np.uint32), want_l.view(np.uint32))


def test_forward_from_rows_casts_once_to_nearest_even():
    """Rows that are not on the activation grid are cast like as_dtype casts them (model.rs:759): the result is the pre-rounded rows'."""
    oracle = _oracle("bf16")
    g = np.random.default_rng(3)
    rows = (0.02 * g.standard_normal((6, CFG.hidden_size))).astype(np.float32)
    bits = rc.bf16_round(rows).view(np.uint32) + np.uint32(0x8000)          # exact ties above a bf16 value
    ties = bits.view(np.float32)
    even = rc.bf16_round(ties)
    assert (even.view(np.uint32) & 0x10000 == 0).all() and (even != ties).all()
    a = rule.forward_from_rows(oracle, ties, [])
    b = rule.forward_from_rows(oracle, even, [])
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, rule.forward_from_rows(oracle, rows, []))


# ---- the audio tower's rule, against brute force and literal ports ----

def test_length_formula_is_the_convolutions_arithmetic():
    """feat_extract_output_lengths(F) for F = 1..400 against counting: chunks of 100 frames, each through three kernel-3 stride-2
    padding-1 convolutions, positions counted by brute force."""
    def brute(n):                                   # outputs o whose taps [2o - 1, 2o + 1] lie inside the padded input [-1, n]
        return len([o for o in range(n + 1) if 2 * o + 1 <= n])
    for n in range(1, 120):
        assert rule.conv_len(n) == brute(n)
    for F in range(1, 401):
        want = sum(brute(brute(brute(min(100, F - s)))) for s in range(0, F, 100))
        assert rule.feat_extract_output_lengths(F) == want, F
    assert rule.feat_extract_output_lengths(100) == 13 and rule.feat_extract_output_lengths(3000) == 390


def test_block_mask_is_the_literal_port():
    def literal(seq_len, boundaries):               # create_block_attention_mask, encoder.rs:439-458, loop for loop
        n = seq_len
        data = [-1e9] * (n * n)
        for w in range(max(len(boundaries) - 1, 0)):
            start, end = boundaries[w], boundaries[w + 1]
            for i in range(start, min(end, n)):
                for j in range(start, min(end, n)):
                    data[i * n + j] = 0.0
        return np.array(data).reshape(n, n)
    for n, window in [(1, 104), (13, 104), (104, 104), (105, 104), (215, 104), (33, 26), (52, 26)]:
        b = rule.window_boundaries(n, window)
        assert b[0] == 0 and b[-1] == n
        np.testing.assert_array_equal(rule.block_mask(n, b), literal(n, b))


def test_gelu_is_the_erf_form():
    import math
    xs = np.concatenate([np.linspace(-6, 6, 241), [0.0, 1e-8, -1e-8, 30.0, -30.0]])
    want = np.array([0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0))) for x in xs])
    np.testing.assert_allclose(rule.gelu(xs), want, rtol=1e-15, atol=1e-300)
    tanh_form = 0.5 * xs * (1 + np.tanh(math.sqrt(2 / math.pi) * (xs + 0.044715 * xs ** 3)))
    assert np.abs(rule.gelu(xs) - tanh_form).max() > 1e-4       # and not the approximation


@pytest.mark.parametrize("n,window,heads", [(1, 104, 2), (104, 104, 2), (105, 104, 2), (215, 104, 2), (5, 26, 2), (33, 26, 2), (52, 26, 2)])
def test_window_attention_is_masked_full_attention(n, window, heads):
    g = np.random.default_rng(n)
    q, k, v = (g.standard_normal((n, heads * 64)) for _ in range(3))
    full = rule.masked_attention(q, k, v, heads, rule.block_mask(n, rule.window_boundaries(n, window)))
    np.testing.assert_allclose(rule.window_attention(q, k, v, heads, window), full, rtol=0, atol=1e-13)
