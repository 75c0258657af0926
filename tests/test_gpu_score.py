"""Scoring a text on the engine (engine.Model.score; csrc/engine_score.hip omx_qwen3_score): per-token log-probabilities from one
batched prompt pass against the oracle's [L, V] logits, on a peaked checkpoint, under another panel width, its cache bookkeeping
against prefill, MoE / packed-head models against the engine's own prefill logits, and the refusals."""
import functools

import numpy as np
import pytest

from logprob_rule import logprob64
from oracle import ref_core as rc, ref_qwen3 as rq, synth
from test_gpu_batch_decode import _build
from test_gpu_speculative import TARGET, WIDE, _engine

pytestmark = pytest.mark.gpu

N = 200
CTX = 256


def _bound(cfg, logits):
    return 2.0 ** -7 * np.abs(logits).max() * np.sqrt(cfg.num_hidden_layers)


@functools.lru_cache(maxsize=None)
def _oracle_rows(name):
    """the oracle's logits [N, V] of the N-token synthetic text (computed once per config, shared, read-only)"""
    cfg = {"narrow": TARGET, "wide": WIDE}[name]
    ids = synth.prompt_ids(N, cfg.vocab_size)
    ref = rq.Qwen3Oracle(cfg, rq.synth_weights(cfg)).forward(ids[None], [])[0].astype(np.float32)
    ref.setflags(write=False)
    return ids, ref


def _check_against_oracle(cfg, ids, ref, lp, greedy, what):
    """|lp - lp_ref| <= 2 * 1.5 * bound (a log-prob is a logit minus a soft maximum of logits, each within 1.5 bound of the oracle's);
    greedy[t] the oracle's argmax unless the oracle's margin there is <= 2 bound; at most half of the rows such near-ties."""
    n = len(ids)
    bound = _bound(cfg, ref)
    lp_ref, _ = logprob64(ref[:n - 1], ids[1:])
    worst = np.abs(lp - lp_ref).max()
    print(f"{what}: worst |lp - lp_ref| = {worst:.4f} = {worst / bound:.3f} bound (bound {bound:.4f})")
    assert worst <= 2 * 1.5 * bound
    if greedy is not None:
        margins = rc.argmax_margin(ref)
        near = 0
        for t in range(n):
            if int(greedy[t]) != int(np.argmax(ref[t])):
                assert margins[t] <= 2 * bound, f"row {t}: greedy {greedy[t]} vs the oracle's {np.argmax(ref[t])} at margin {margins[t]:.4f}"
            near += margins[t] <= 2 * bound
        print(f"{what}: {near} of {n} rows are near-ties of the oracle")
        assert near <= n // 2


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_score_matches_the_oracle(omx, name):
    """200 tokens of synth.prompt_ids in one score() call against oracle.forward's logits at every position.  bound = 2^-7 max|ref
    logits| sqrt(L), the bound the prompt tests hold logits to (near-ties of the oracle alone: 96 narrow, 57 wide)."""
    ids, ref = _oracle_rows(name)
    cfg, m, _ = _build(name, CTX)
    lp, greedy = m.score(ids, return_greedy=True)
    assert lp.dtype == np.float32 and lp.shape == (N - 1,) and greedy.shape == (N,) and m.offset() == N
    _check_against_oracle(cfg, ids, ref, lp, greedy, name)
    pass_ms, head_ms = m.last_score_ms()
    assert pass_ms > 0 and head_ms > 0
    m.close()


def test_score_on_the_peaked_checkpoint(omx):
    """synth_weights(peaked=True): the greedy successor of token t is t - 1.  A countdown text scores a mean NLL below 0.5, the same
    ids shuffled above 5 (the oracle: about 0.09 and about 10) -- on the engine and on the oracle."""
    cfg = TARGET
    V = cfg.vocab_size
    down = ((1500 - np.arange(N)) % V).astype(np.uint32)
    mixed = np.random.default_rng(3).permutation(down).astype(np.uint32)
    from ominix_mlx_amd import engine
    m = engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                     num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                     vocab_size=V, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, max_context=CTX)
    m.synth_weights(peaked=True)
    oracle = rq.Qwen3Oracle(cfg, rq.synth_weights(cfg, peaked=True))
    for ids, ok in ((down, lambda v: v < 0.5), (mixed, lambda v: v > 5.0)):
        m.reset()
        nll = -float(m.score(ids).astype(np.float64).mean())
        ref = oracle.forward(ids[None], [])[0]
        nll_ref = -float(logprob64(ref[:N - 1], ids[1:])[0].mean())
        print(f"mean NLL: engine {nll:.4f}, oracle {nll_ref:.4f}")
        assert ok(nll_ref) and ok(nll)
    m.close()


def test_score_does_not_depend_on_the_panel_width(omx, monkeypatch):
    """OMX_SCORE_PANEL=1024 (two panels over the vocabulary of 2 048) returns the float32 bits and the greedy tokens of the default
    (one panel of 2 048)"""
    ids, _ = _oracle_rows("narrow")
    _, m, _ = _build("narrow", CTX)
    lp0, g0 = m.score(ids, next_token=7, return_greedy=True)
    monkeypatch.setenv("OMX_SCORE_PANEL", "1024")
    m.reset()
    lp1, g1 = m.score(ids, next_token=7, return_greedy=True)
    np.testing.assert_array_equal(lp1.view(np.uint32), lp0.view(np.uint32))
    np.testing.assert_array_equal(g1, g0)
    monkeypatch.setenv("OMX_SCORE_PANEL", "1000")
    m.reset()
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: OMX_SCORE_PANEL=1000 must be a positive multiple of 1024"):
        m.score(ids)
    m.close()


def test_score_leaves_the_cache_prefill_leaves(omx):
    """score(P); trim(0, X); decode(4) against prefill(P); trim(0, X); decode(4) on a second model of the same weights: identical
    tokens, last_logits() bits and offset (both ran the same batched pass).  And scoring in two pieces -- the second on top of the first's
    cached rows -- matches the oracle within the one-piece tolerance; offset() advances by n."""
    ids, ref = _oracle_rows("narrow")
    cfg, a, _ = _build("narrow", CTX)
    _, b, _ = _build("narrow", CTX)
    X = 321
    a.score(ids)
    assert a.offset() == N
    a.trim(0, X)
    b.prefill(ids)
    b.trim(0, X)
    ta, tb = a.decode(4), b.decode(4)
    np.testing.assert_array_equal(ta, tb)
    np.testing.assert_array_equal(a.last_logits().view(np.uint32), b.last_logits().view(np.uint32))
    assert a.offset() == b.offset() == N + 4
    b.close()
    a.reset()
    lp1 = a.score(ids[:120], next_token=int(ids[120]))
    assert lp1.shape == (120,) and a.offset() == 120
    lp2, g2 = a.score(ids[120:], return_greedy=True)
    assert lp2.shape == (N - 121,) and a.offset() == N
    _check_against_oracle(cfg, ids, ref, np.concatenate([lp1, lp2]), None, "two pieces")
    nxt = a.decode(1)                       # the pending token after score is its last row's argmax
    assert a.offset() == N + 1 and nxt.shape == (1,)
    a.close()


def _moe_model(omx):
    from test_gpu_moe_engine import CONFIGS, _engine as moe_engine
    cfg = CONFIGS["mixtral"]
    return cfg, moe_engine(omx, cfg, max_context=CTX)


@pytest.mark.parametrize("name", ["mixtral", "narrow_q4"])
def test_score_on_moe_and_packed_head_matches_prefill_logits(omx, name):
    """A bf16 sparse-MoE model and a 4-bit model (packed head, dequantised a panel at a time): for rows t in {0, 57, 199} the engine's own
    prefill(ids[:t + 1]) + last_logits(), log-softmaxed on the host in float64, against score's lp[t] -- within 2 * 1.5 * bound,
    bound = 2^-7 max|those logits| sqrt(L)."""
    if name == "mixtral":
        cfg, m = _moe_model(omx)
    else:
        cfg, m, _ = _build(name, CTX)
    ids = synth.prompt_ids(N + 1, cfg.vocab_size)
    lp, greedy = m.score(ids[:N], next_token=int(ids[N]), return_greedy=True)
    assert lp.shape == (N,)
    for t in (0, 57, 199):
        m.reset()
        first = m.prefill(ids[:t + 1])
        logits = m.last_logits().astype(np.float32)
        bound = _bound(cfg, logits)
        want = logprob64(logits[None], ids[t + 1:t + 2])[0][0]
        print(f"{name} row {t}: |lp - prefill's| = {abs(lp[t] - want):.4f} = {abs(lp[t] - want) / bound:.3f} bound")
        assert abs(lp[t] - want) <= 2 * 1.5 * bound
        assert int(greedy[t]) == int(first) or rc.argmax_margin(logits[None])[0] <= 2 * bound
    m.close()


def test_refusals_by_name(omx):
    from ominix_mlx_amd import engine

    def model(cfg, **kw):
        return engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                            num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                            vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, max_context=CTX, **kw)

    ids = synth.prompt_ids(16, TARGET.vocab_size)
    m = model(TARGET, tp_size=2)
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: tensor / expert parallel models are not supported"):
        m.score(ids)
    m.close()
    m = model(WIDE, dtype="float16")
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: float16 models"):
        m.score(ids)
    m.close()
    m = _engine(TARGET, CTX)
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: 0 tokens"):
        m.score(np.zeros(0, np.uint32), next_token=1)
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: .* exceed max_context 256"):
        m.score(synth.prompt_ids(CTX, TARGET.vocab_size))
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: .* exceed max_context 256"):
        m.score(synth.prompt_ids(CTX + 1, TARGET.vocab_size))
    m.score(ids)
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: 16 cached \\+ 240 tokens exceed max_context 256"):
        m.score(synth.prompt_ids(240, TARGET.vocab_size))
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: token id 2048 out of range"):
        m.score([TARGET.vocab_size, 1])
    with pytest.raises(omx.OmxError, match="omx_qwen3_score: target id 2048 out of range"):
        m.score(ids[:4], next_token=TARGET.vocab_size)
    assert m.offset() == 16                 # a refused call changes nothing
    m.close()
