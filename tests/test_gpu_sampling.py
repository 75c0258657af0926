"""GPU: filtered sampling (csrc/sample_filter.hip) -- the op, the engine's in-step sampler and mlx_topk_axis on long axes -- against
the numpy restatement of the rule in tests/sampling_rule.py.

  * penalties and top-k: every step is one float32 operation or a comparison -> token, threshold and kept count EXACT;
  * top-p: the device sums the masses exactly (fixed point) but exp(y - max) through expf, the rule here in float64.  With
    delta = 2^-10 in mass the device's kept set must lie between the float64 rule's sets for p - delta and p + delta (sums chained
    over <= 4096 float32 terms on three levels plus expf's few ulp stay under 3 * 4096 * 2^-24 ~ 7e-4 < 2^-10 relative; exact sums
    are well inside), and the token must be the numpy draw restricted to the device's own set, exactly.
"""
import itertools

import numpy as np
import pytest

from oracle import mlx_rng as rng
from oracle import ref_core as rc
from oracle import ref_qwen3 as rq
from oracle import synth
import sampling_rule as sr
from test_gpu_qwen3 import CONFIGS, _engine

pytestmark = pytest.mark.gpu

DELTA = 2.0 ** -10
DTYPES = ("bf16", "f16", "f32")


def _round(x, dtype):
    if dtype == "bf16":
        return rc.bf16_round(x)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    return x.astype(np.float32)


def _row(V, dtype, seed, sigma=3.0):
    """N(0, sigma^2) on the dtype's grid with ties PLANTED at the ranks top-k 20 and 50 cut at (three more copies of each value)."""
    g = np.random.default_rng(seed)
    x = _round((sigma * g.standard_normal(V)).astype(np.float32), dtype)
    for k in (20, 50):
        if V > 4 * k:
            order = np.argsort(-x, kind="stable")
            x[g.choice(order[2 * k:], 3, replace=False)] = x[order[k - 1]]
    return x


def _device(omx, x, dtype, key_seed, temperature, seen_ids=(), **kw):
    T = omx.ops.Tensor
    seen = None
    if len(seen_ids):
        s = np.zeros(x.size, np.uint8)
        s[np.asarray(seen_ids)] = 1
        seen = T.from_numpy(s, "u8")
    tok, thr, kept = omx.ops.sample_filtered(T.from_numpy(x[None, :], dtype), omx.ops.random_key(key_seed), temperature, seen=seen, **kw)
    return int(tok.numpy()[0]), np.float32(thr.numpy()[0]), int(kept.numpy()[0])


# ---- 1. top-k and penalties: exact ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [151936, 5000, 777, 2, 1])
def test_topk_and_penalties_are_exact(omx, V, dtype):
    x = _row(V, dtype, seed=V + len(dtype))
    g = np.random.default_rng(V)
    temperature, key_seed = 0.6, 1234 + V
    noise = rng.gumbel((1, V), rng.key(key_seed))[0]
    for n_seen, r, q in itertools.product((0, 1, 4000), (1.0, 1.35), (0.0, 1.5)):
        seen_ids = np.sort(g.choice(V, min(n_seen, V), replace=False))
        if n_seen == 1 and V > 50:
            seen_ids = np.array([int(np.argmax(x))])          # the penalty moves the top entry across the thresholds
        y = sr.scaled(x, temperature, seen_ids, r, q)
        for k in (1, 20, 50, V - 1, V):
            thr, mask = sr.topk_threshold(y, k)
            want = int(np.argmax(np.where(mask, (y + noise).astype(np.float32), np.float32(-np.inf))))
            got = _device(omx, x, dtype, key_seed, temperature, seen_ids, top_k=k, repetition_penalty=r, presence_penalty=q)
            assert got == (want, thr, int(mask.sum())), (V, dtype, n_seen, r, q, k)
    # temperature 0 with a penalty: the argmax of the penalised logits; everything off: omx_random_categorical bit for bit
    seen_ids = [int(np.argmax(x))]
    got = _device(omx, x, dtype, 0, 0.0, seen_ids, repetition_penalty=1.35, presence_penalty=1.5)
    assert got[0] == int(np.argmax(sr.scaled(x, 0.0, seen_ids, 1.35, 1.5)))
    T = omx.ops.Tensor
    plain = omx.ops.random_categorical(T.from_numpy(x[None, :], dtype), omx.ops.random_key(key_seed), inv_temp=float(np.float32(1.0) / np.float32(temperature)))
    assert _device(omx, x, dtype, key_seed, temperature) == (int(plain.numpy()[0]), np.float32(-np.inf), V)


def test_topk_counts_planted_ties(omx):
    """the planted copies sit exactly at the thresholds: more than k entries survive"""
    x = _row(151936, "f32", seed=9)
    y = sr.scaled(x, 1.0)
    for k in (20, 50):
        thr, mask = sr.topk_threshold(y, k)
        assert mask.sum() == k + 3
        assert _device(omx, x, "f32", 5, 1.0, top_k=k)[1:] == (thr, k + 3)


# ---- 2. top-p: sandwich, then exact ----

def _sandwich(y, top_k, p, pinned=True):
    """the float64 rule's sets for p - delta and p + delta; pinned: the inputs must hold the two within 10 % of the larger, so that the
    sandwich cannot hide a wrong threshold (asserted on the inputs before anything is asked of the device)"""
    _, surv = sr.topk_threshold(y, top_k)
    lo, hi = sr.topp_mask(y, surv, p - DELTA), sr.topp_mask(y, surv, p + DELTA)
    assert (hi | ~lo).all()                                                         # nested
    if pinned:
        assert hi.sum() - lo.sum() <= 0.10 * hi.sum(), "the inputs do not pin the threshold: the bounding sets differ by more than 10 %"
    return lo, hi


@pytest.mark.parametrize("p", [0.5, 0.8, 0.95])
@pytest.mark.parametrize("temperature", [0.6, 1.0])
@pytest.mark.parametrize("sigma", [1.0, 2.0, 3.0, 4.0])
def test_topp_set_lies_between_the_float64_sets(omx, sigma, temperature, p):
    V = 151936
    # (generator seed 0: rows whose p -+ delta sets differ by 0 - 5.6 % over these cases, checked with the float64 rule on the CPU;
    #  _sandwich asserts it again before the device is asked anything)
    x = rc.bf16_round((sigma * np.random.default_rng(0).standard_normal(V)).astype(np.float32))
    _check_sandwich(omx, x, "bf16", temperature, 0, p, f"sigma {sigma}")


def _check_sandwich(omx, x, dtype, temperature, top_k, p, label):
    y = sr.scaled(x, temperature)
    lo, hi = _sandwich(y, top_k, p)
    key_seed = 77 + top_k
    tok, thr, kept = _device(omx, x, dtype, key_seed, temperature, top_k=top_k, top_p=p)
    dev = y >= thr
    print(f"{label} T {temperature} p {p} top_k {top_k}: float64 sets {lo.sum()} .. {hi.sum()}, device {dev.sum()}")
    assert (dev | ~lo).all(), "an entry of the p - delta set is missing"
    assert (hi | ~dev).all(), "an entry outside the p + delta set was kept"
    assert dev.sum() == kept
    assert tok == sr.draw(y, dev, rng.key(key_seed))


@pytest.mark.parametrize("top_k,p", [(1000, 0.9), (5000, 0.5), (20000, 0.95)])
def test_topp_on_the_survivors_of_topk(omx, top_k, p):
    """top-k then top-p on float32 rows (no ties: the survivors are exactly k, Z is their mass alone)"""
    x = (2.0 * np.random.default_rng(top_k).standard_normal(151936)).astype(np.float32)
    _check_sandwich(omx, x, "f32", 0.8, top_k, p, "f32 row")


def test_topp_keeps_the_maximum_for_a_tiny_p_and_with_penalties(omx):
    x = _row(5000, "bf16", seed=3)
    y = sr.scaled(x, 0.7)
    tok, thr, kept = _device(omx, x, "bf16", 1, 0.7, top_p=1e-6)
    assert (tok, thr, kept) == (int(np.argmax(y)), y.max(), int((y == y.max()).sum()))
    seen_ids = np.argsort(-x)[:7]
    y = sr.scaled(x, 0.7, seen_ids, 1.35, 0.0)
    lo, hi = sr.topp_mask(y, np.ones(y.shape, bool), 0.6 - DELTA), sr.topp_mask(y, np.ones(y.shape, bool), 0.6 + DELTA)
    tok, thr, kept = _device(omx, x, "bf16", 2, 0.7, seen_ids, top_p=0.6, repetition_penalty=1.35)
    dev = y >= thr
    assert (dev | ~lo).all() and (hi | ~dev).all() and dev.sum() == kept and tok == sr.draw(y, dev, rng.key(2))


# ---- 3. distribution ----

def test_filtered_draws_follow_the_restricted_distribution(omx):
    """20 000 draws (rows of one call) from one 64-entry row, top-k 8 then top-p 0.9: nothing outside the kept set, the kept tokens'
    frequencies within 4 sigma of the renormalised probabilities (the bound of test_categorical_follows_the_distribution)."""
    V, n = 64, 20000
    x = np.linspace(-2.0, 3.0, V).astype(np.float32)[np.random.default_rng(1).permutation(V)]
    y = sr.scaled(x, 0.9)
    thr, mask = sr.kept_mask(y, top_k=8, top_p=0.9)
    lo, hi = _sandwich(y, 8, 0.9)
    assert (lo == hi).all() and (lo == mask).all() and 2 <= mask.sum() <= 8
    T = omx.ops.Tensor
    tok, thr_d, kept = omx.ops.sample_filtered(T.from_numpy(np.tile(x, (n, 1)), "f32"), omx.ops.random_key(123), 0.9, top_k=8, top_p=0.9)
    tok = tok.numpy().ravel()
    assert (thr_d.numpy() == thr).all() and (kept.numpy() == mask.sum()).all()
    assert mask[tok].all(), "a token outside the kept set was drawn"
    prob = np.where(mask, np.exp(y.astype(np.float64) - y.max()), 0.0)
    prob /= prob.sum()
    freq = np.bincount(tok, minlength=V) / n
    assert (np.abs(freq - prob) <= 4 * np.sqrt(prob * (1 - prob) / n)).all()


# ---- 4. the engine, from its own logits ----

CASES = {
    "a_topk": dict(top_k=20),
    "b_topk_presence": dict(top_k=20, presence_penalty=1.5),
    "c_repetition": dict(repetition_penalty=1.35),
    "d_topk_topp": dict(top_k=50, top_p=0.9),
}


def _expected_tokens(y, kw, key):
    """the tokens the rule allows: one for the exact cases, the draws of every threshold set between the p -+ delta sets with top-p"""
    p = kw.get("top_p", 1.0)
    if p >= 1.0:
        _, mask = sr.topk_threshold(y, kw.get("top_k", 0))
        return {sr.draw(y, mask, key)}
    lo, hi = _sandwich(y, kw.get("top_k", 0), p, pinned=False)
    out = set()
    for t in np.unique(y[hi & (y <= y[lo].min())]):
        out.add(sr.draw(y, y >= t, key))
    return out


def _run_filtered(m, prompt, temp, seed, kw, steps=12):
    m.set_sampler(temp, seed, **kw)
    toks, logits = [m.prefill(prompt)], [m.last_logits()]
    for _ in range(steps):
        toks.append(int(m.decode(1)[0]))
        logits.append(m.last_logits())
    return toks, logits


def _check_against_rule(toks, logits, temp, seed, kw):
    state = rng.RandomState(seed)
    for i, l in enumerate(logits):
        y = sr.scaled(l, temp, sorted(set(toks[:i])), kw.get("repetition_penalty", 1.0), kw.get("presence_penalty", 0.0))
        assert toks[i] in _expected_tokens(y, kw, state.next()), f"token {i}"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ["gqa2_d64", "gqa4_d128"])
def test_engine_filtered_sampling_draws_what_the_rule_draws_from_the_same_logits(omx, name, case):
    cfg, kw = CONFIGS[name], CASES[case]
    temp, seed = 0.8, 11
    prompt = synth.prompt_ids(32, cfg.vocab_size)
    m = _engine(omx, cfg)
    toks, logits = _run_filtered(m, prompt, temp, seed, kw)
    assert m.decode_path() == "graph"
    _check_against_rule(toks, logits, temp, seed, kw)
    # one decode(12) call equals the twelve decode(1) calls; the same seed replays
    m2 = _engine(omx, cfg)
    m2.set_sampler(temp, seed, **kw)
    assert [m2.prefill(prompt)] + [int(t) for t in m2.decode(12)] == toks
    # not the unfiltered stream where a filter prunes ...
    plain = _engine(omx, cfg)
    plain.set_sampler(temp, seed)
    unfiltered = [plain.prefill(prompt)] + [int(t) for t in plain.decode(12)]
    if "top_k" in kw:      # (a repetition penalty alone need not move a draw within 12 tokens of these flat synthetic models)
        assert unfiltered != toks
    # ... which set_sampler(T, seed) brings back bit for bit on the engine that ran filtered
    m2.reset()
    m2.set_sampler(temp, seed)
    assert [m2.prefill(prompt)] + [int(t) for t in m2.decode(12)] == unfiltered
    # and a new prefill starts a new history: the filtered stream again
    m2.reset()
    m2.set_sampler(temp, seed, **kw)
    assert [m2.prefill(prompt)] + [int(t) for t in m2.decode(12)] == toks


def test_engine_greedy_with_a_penalty_is_the_argmax_of_the_penalised_logits(omx):
    cfg = CONFIGS["gqa2_d64"]
    prompt = synth.prompt_ids(32, cfg.vocab_size)
    m = _engine(omx, cfg)
    toks, logits = _run_filtered(m, prompt, 0.0, 0, dict(repetition_penalty=1.35, presence_penalty=1.5))
    assert m.decode_path() == "graph"
    for i, l in enumerate(logits):
        assert toks[i] == int(np.argmax(sr.scaled(l, 0.0, sorted(set(toks[:i])), 1.35, 1.5)))
    assert len(set(toks)) == len(toks)          # (1.5 off every emitted token: no repeats on this model)


def test_packed_and_float16_engines_run_topk(omx):
    from ominix_mlx_amd import engine
    from test_gpu_dense_f16 import _cfg, _kw
    cfg = CONFIGS["gqa4_d128"]
    kw = CASES["a_topk"]
    q4 = engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                      num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                      vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                      tie_word_embeddings=cfg.tie_word_embeddings, rope_scaling=cfg.rope_scaling, max_context=256,
                      quantization={"bits": 4, "group_size": 64})
    q4.synth_weights()
    toks, logits = _run_filtered(q4, synth.prompt_ids(16, cfg.vocab_size), 0.7, 5, kw, steps=6)
    assert q4.decode_path() == "graph"
    _check_against_rule(toks, logits, 0.7, 5, kw)
    fcfg = _cfg(True)
    f16 = engine.Model(dtype="float16", **_kw(fcfg))
    f16.load_weights({k: v.astype(np.float16) for k, v in rq.synth_weights(fcfg, dt="f16").items()})
    assert f16.f16
    toks, logits = _run_filtered(f16, synth.prompt_ids(40, fcfg.vocab_size), 0.7, 5, kw, steps=6)
    assert f16.decode_path() == "graph"
    _check_against_rule(toks, logits, 0.7, 5, kw)


@pytest.mark.parametrize("quantization", [None, {"bits": 4, "group_size": 64}])
def test_moe_engines_run_topk_with_a_presence_penalty(omx, quantization):
    import test_gpu_moe_engine as tm
    cfg = tm.CONFIGS["qwen3_moe"]
    kw = CASES["b_topk_presence"]
    m = tm._engine(omx, cfg, quantization=quantization)
    toks, logits = _run_filtered(m, synth.prompt_ids(24, cfg.vocab_size), 0.7, 9, kw, steps=6)
    assert m.decode_path() == "graph"
    _check_against_rule(toks, logits, 0.7, 9, kw)


# ---- 5. refusals ----

def test_filtered_sampling_refusals_name_the_reason(omx):
    from ominix_mlx_amd import engine
    cfg = CONFIGS["gqa4_d128"]
    shard = engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                         num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                         vocab_size=cfg.vocab_size, tie_word_embeddings=cfg.tie_word_embeddings, max_context=256, tp_rank=0, tp_size=2)
    with pytest.raises(omx.OmxError, match="tensor parallelism"):
        shard.set_sampler(0.7, 1, top_k=20)
    shard.set_sampler(0.7, 1)                                   # the plain sampler still is accepted
    m = _engine(omx, cfg)
    prompt = synth.prompt_ids(24, cfg.vocab_size)
    m.set_sampler(0.7, 1, top_k=20)
    first = m.prefill(prompt)
    with pytest.raises(omx.OmxError, match="omx_qwen3_verify: filtered sampling"):
        m.verify([first, 1, 2])
    with pytest.raises(omx.OmxError, match="omx_qwen3_trim: filtered sampling"):
        m.trim(1, 3)
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(repetition_penalty=0.0), dict(presence_penalty=float("inf"))):
        with pytest.raises(omx.OmxError):
            m.set_sampler(0.7, 1, **bad)
    m.set_sampler(0.7, 1)                                       # filters off: verify and trim work again
    m.reset()
    first = m.prefill(prompt)
    m.verify([first, 1, 2])
    m.trim(1, 3)


# ---- 6. the handle ABI: mlx_topk_axis beyond the sort kernels' 65 536, and the reference's sample_top_k_p call by call ----

def test_mlx_topk_axis_on_long_axes(omx):
    from ominix_mlx_amd import mlx_c as mx
    g = np.random.default_rng(8)
    for shape, k, dtype, code in [((1, 151936), 20, "bf16", mx.BFLOAT16), ((4, 70000), 20, "f32", mx.FLOAT32), ((4, 70000), 50, "f16", mx.FLOAT16),
                                  ((1, 151936), 1, "f32", mx.FLOAT32)]:
        x = _round((3.0 * g.standard_normal(shape)).astype(np.float32), dtype)
        got = mx.topk(mx.Array.from_numpy(x, code), k, -1).numpy().astype(np.float32)
        np.testing.assert_array_equal(got, np.sort(x, axis=-1)[..., -k:])
    x = _round((3.0 * g.standard_normal((3, 777))).astype(np.float32), "bf16")      # a short axis: the sort path, as before
    a = mx.Array.from_numpy(x, mx.BFLOAT16)
    got = mx.topk(a, 20, -1).numpy()
    np.testing.assert_array_equal(got, mx.slice(mx.sort_axis(a, -1), [0, 757], [3, 777]).numpy())
    np.testing.assert_array_equal(got.astype(np.float32), np.sort(x, axis=-1)[..., -20:])
    with pytest.raises(omx.OmxError):
        mx.topk(a, 778, -1)


def test_sample_top_k_p_op_sequence_through_the_handle_abi(omx):
    """funasr-qwen4b-mlx/src/model.rs:1333-1383 call by call at a Qwen vocabulary: subtract the penalty row, multiply by 1/T, topk_axis,
    index the k-th largest (position 0 of this project's ascending result), ge, where(-inf), categorical -- the token of the rule."""
    from ominix_mlx_amd import mlx_c as mx
    V, k, temperature, q, key_seed = 151936, 20, 0.6, 1.5, 31
    x = _row(V, "bf16", seed=12)
    generated = [int(i) for i in np.argsort(-x)[:5]]
    penalty = np.zeros((1, V), np.float32)
    penalty[0, generated] = q
    modified = mx.subtract(mx.Array.from_numpy(x[None, :], mx.BFLOAT16), mx.Array.from_numpy(penalty, mx.FLOAT32))
    modified = mx.multiply(modified, mx.Array.from_numpy(np.array(np.float32(1.0) / np.float32(temperature), np.float32), mx.FLOAT32))
    topk_vals = mx.topk(modified, k, -1)
    threshold = mx.reshape(mx.slice(topk_vals, [0, 0], [1, 1]), [1, 1])
    mask = mx.greater_equal(modified, threshold)
    modified = mx.where(mask, modified, mx.Array.from_numpy(np.array(-np.inf, np.float32), mx.FLOAT32))
    token = int(np.asarray(mx.random_categorical(modified, -1, None, mx.random_key(key_seed)).numpy()).ravel()[0])
    want, thr, kept = sr.sample(x, temperature, rng.key(key_seed), top_k=k, presence_penalty=q, seen_ids=generated)
    assert np.float32(np.asarray(threshold.numpy()).ravel()[0]) == thr and int(np.asarray(mask.numpy()).sum()) == kept
    assert token == want
    assert token == _device(omx, x, "bf16", key_seed, temperature, generated, top_k=k, presence_penalty=q)[0]
