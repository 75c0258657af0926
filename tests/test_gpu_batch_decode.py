"""Batched decode of up to eight independent sequences on one loaded Qwen3 model (engine.Batch; csrc/engine_batch.hip,
omx_qwen3_batch_*): the ragged step -- per-slot embedding gather, cache append, split-KV attention and sampler around the rows
launches of the verify pass -- against the oracle, against itself under different neighbours and row counts, against the
single-sequence engine on the same model object, and its bookkeeping, sampler and refusals."""
import numpy as np
import pytest

from oracle import mlx_rng, ref_core as rc, ref_qwen3 as rq, synth
from test_gpu_quant_verify import _qmodel, _quantized
from test_gpu_speculative import TARGET, WIDE, _engine

pytestmark = pytest.mark.gpu

CTX = 512
# (config, quantization (bits, group) or None)
VARIANTS = {"narrow": (TARGET, None), "wide": (WIDE, None), "narrow_q4": (TARGET, (4, 64)), "narrow_q6": (TARGET, (6, 64))}
PROMPT_LENS = [5, 33, 64, 130, 250, 17, 96, 200]      # slot 4 crosses the 256-token slab step while decoding


def _build(name, max_context=CTX):
    """(cfg, engine model, oracle) of a variant: synthetic bf16 weights, or their packed form the way test_gpu_quant_verify builds it"""
    cfg, quant = VARIANTS[name]
    if quant is None:
        return cfg, _engine(cfg, max_context), rq.Qwen3Oracle(cfg, rq.synth_weights(cfg))
    w, oracle = _quantized(cfg, *quant)
    m = _qmodel(cfg, quant[0], quant[1], max_context)
    m.load_weights(w)
    return cfg, m, oracle


def _prompt(n, V, shift=None):
    return ((synth.prompt_ids(n, V).astype(np.int64) + (n if shift is None else shift)) % V).astype(np.uint32)


def _bound(cfg, ref_logits):
    return 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(cfg.num_hidden_layers)


# ---- 1. ragged batch against the oracle, teacher-forced ----

@pytest.mark.parametrize("name", list(VARIANTS))
def test_ragged_batch_matches_the_oracle_teacher_forced(omx, name):
    """Eight sequences of 5 .. 250 prompt tokens, 12 positions each (the prompt's last and 11 decode steps over all eight slots), the
    oracle's token forced after every step.  bound = 2^-7 max|ref logits| sqrt(L), the bound test_gpu_speculative holds the same rows
    kernels to: logits within 1.5 bound, the engine's own token the oracle's unless the oracle's margin there is <= 2 bound, and at
    most half of the 96 positions such near-ties (the oracle alone: 39 narrow, 33 wide, 44 narrow_q4, 36 narrow_q6)."""
    cfg, m, oracle = _build(name)
    V, n_pos = cfg.vocab_size, 12
    prompts = [_prompt(n, V) for n in PROMPT_LENS]
    refs = [oracle.generate(p, n_pos, return_logits=True) for p in prompts]
    b = m.batch(8, CTX)
    near, worst = 0, 0.0
    got = [[int(b.prefill(s, prompts[s]))] for s in range(8)]
    logits = [[b.logits(s)] for s in range(8)]
    for i in range(1, n_pos):
        for s in range(8):
            b.trim(s, 0, int(refs[s][0][i - 1]))
        step = b.decode(1)
        for s in range(8):
            got[s].append(int(step[0, s]))
            logits[s].append(b.logits(s))
    for s in range(8):
        assert b.offset(s) == PROMPT_LENS[s] + n_pos - 1
        ref_tokens, ref_logits = refs[s]
        bound = _bound(cfg, ref_logits)
        margins = rc.argmax_margin(ref_logits)
        for i in range(n_pos):
            err = float(np.abs(logits[s][i] - ref_logits[i]).max())
            worst = max(worst, err / bound)
            print(f"{name} slot {s} pos {i}: err {err:.4f} bound {bound:.4f} margin {margins[i]:.4f} token {got[s][i]} ref {int(ref_tokens[i])}")
            assert err <= 1.5 * bound, f"slot {s} position {i}: logits off by {err:.4f} (1.5 x bound = {1.5 * bound:.4f})"
            assert got[s][i] == int(ref_tokens[i]) or margins[i] <= 2 * bound, f"slot {s} position {i}: token {got[s][i]} vs {int(ref_tokens[i])}"
            near += int(margins[i] <= 2 * bound)
    print(f"{name}: worst error {worst:.3f} x bound, {near} of {8 * n_pos} positions are near-ties of the oracle")
    assert near <= 8 * n_pos // 2
    b.close(); m.close()


# ---- 1b. every instantiation of the split kernel against the oracle ----

WIDTH_CTX = 1024
WIDTH_LENS = [5, 250, 255, 600]
# (head_dim, query heads, KV heads): batch_attn_kernel<D, GT> for D = 64 / 128 and GT = 1 / 2 / 4 / 8, and 3 query heads per KV head
WIDTHS = [(128, 8, 2), (128, 4, 4), (128, 4, 2), (128, 8, 1), (64, 4, 4), (64, 4, 2), (64, 8, 2), (64, 8, 1), (64, 6, 2)]


@pytest.mark.parametrize("D,H,Hkv", WIDTHS, ids=lambda v: str(v))
def test_every_width_matches_the_oracle(omx, D, H, Hkv):
    """batch_attn_kernel<D, GT> at both head widths and 1 / 2 / 4 / 8 query heads per KV head, and at 3 (GT = 4 with the last head
    repeated in the spare column, a merge loop of 3 D elements), on one-layer models of hidden 512: four slots whose prompts are the
    ways a split can end -- 5 tokens (three of the four waves see no token and merge with m = -inf), 250 (a clamped ragged tail,
    and the sequence grows into a second split while decoding), 255 (pos + 1 lands exactly on the chunk boundary), 600 (three splits, the
    last one ragged) -- 12 positions each, the oracle's token forced after every step.  The rules of
    test_ragged_batch_matches_the_oracle_teacher_forced with L = 1: logits within 1.5 bound, the engine's token the oracle's unless
    the oracle's margin is <= 2 bound, at most half of the 48 positions such near-ties (the oracle alone, in WIDTHS' order:
    11, 9, 10, 13, 11, 8, 8, 14, 6)."""
    cfg = rq.Qwen3Config(512, 1, 1024, H, Hkv, D, 2048, 1e-6, 1e6, False)
    m, oracle = _engine(cfg, WIDTH_CTX), rq.Qwen3Oracle(cfg, rq.synth_weights(cfg))
    V, n_pos, n = cfg.vocab_size, 12, len(WIDTH_LENS)
    prompts = [_prompt(k, V) for k in WIDTH_LENS]
    refs = [oracle.generate(p, n_pos, return_logits=True) for p in prompts]
    b = m.batch(n, WIDTH_CTX)
    got = [[int(b.prefill(s, prompts[s]))] for s in range(n)]
    logits = [[b.logits(s)] for s in range(n)]
    for i in range(1, n_pos):
        for s in range(n):
            b.trim(s, 0, int(refs[s][0][i - 1]))
        step = b.decode(1)
        for s in range(n):
            got[s].append(int(step[0, s]))
            logits[s].append(b.logits(s))
    near, worst = 0, 0.0
    for s in range(n):
        assert b.offset(s) == WIDTH_LENS[s] + n_pos - 1
        ref_tokens, ref_logits = refs[s]
        bound = _bound(cfg, ref_logits)
        margins = rc.argmax_margin(ref_logits)
        for i in range(n_pos):
            err = float(np.abs(logits[s][i] - ref_logits[i]).max())
            worst = max(worst, err / bound)
            print(f"({D}, {H}, {Hkv}) slot {s} pos {i}: err {err:.4f} bound {bound:.4f} margin {margins[i]:.4f} token {got[s][i]} ref {int(ref_tokens[i])}")
            assert err <= 1.5 * bound, f"slot {s} position {i}: logits off by {err:.4f} (1.5 x bound = {1.5 * bound:.4f})"
            assert got[s][i] == int(ref_tokens[i]) or margins[i] <= 2 * bound, f"slot {s} position {i}: token {got[s][i]} vs {int(ref_tokens[i])}"
            near += int(margins[i] <= 2 * bound)
    print(f"({D}, {H}, {Hkv}): worst error {worst:.3f} x bound, {near} of {n * n_pos} positions are near-ties of the oracle")
    assert near <= n * n_pos // 2
    b.close(); m.close()


# ---- 2. neighbours do not change a sequence ----

def _run_a(b, slot_a, prompt_a, neighbours, order, steps=16, disturb=None):
    """A in slot_a beside `neighbours` {slot: prompt}; `steps` greedy single-step calls over `order`; -> (tokens, logits) of A.
    disturb = (step, slot, prompt): that neighbour is reset and prefilled again before that step."""
    toks, logits = [int(b.prefill(slot_a, prompt_a))], [b.logits(slot_a)]
    for s, p in neighbours.items():
        b.prefill(s, p)
    col = list(order).index(slot_a)
    for i in range(steps):
        if disturb is not None and disturb[0] == i:
            b.reset(disturb[1])
            b.prefill(disturb[1], disturb[2])
        toks.append(int(b.decode(1, order)[0, col]))
        logits.append(b.logits(slot_a))
    return np.asarray(toks), np.stack(logits)


@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
def test_neighbours_do_not_change_a_sequence(omx, name):
    """The same sequence A, 16 greedy steps at M = 8: in slot 0 beside seven long neighbours; in slot 5, listed last, beside seven
    different short ones; beside a neighbour that is reset and prefilled again mid-run -- tokens and logits bit for bit."""
    cfg, m, _ = _build(name)
    V = cfg.vocab_size
    A = _prompt(70, V, 3)
    long_n = {s: _prompt(300 + 20 * s, V, 100 + s) for s in range(1, 8)}
    short_n = {s: _prompt(3 + 5 * i, V, 900 + s) for i, s in enumerate([0, 1, 2, 3, 4, 6, 7])}
    mid_n = {s: _prompt(90 + 11 * s, V, 500 + s) for s in [0, 1, 3, 4, 5, 6, 7]}
    b = m.batch(8, CTX)
    ta, la = _run_a(b, 0, A, long_n, list(range(8)))
    b.close()
    b = m.batch(8, CTX)
    tb, lb = _run_a(b, 5, A, short_n, [0, 1, 2, 3, 4, 6, 7, 5])
    b.close()
    b = m.batch(8, CTX)
    tc, lc = _run_a(b, 2, A, mid_n, [7, 6, 2, 5, 4, 3, 1, 0], disturb=(8, 4, _prompt(41, V, 77)))
    b.close()
    np.testing.assert_array_equal(ta, tb)
    np.testing.assert_array_equal(ta, tc)
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(la, lc)
    assert len(set(ta.tolist())) > 4, "a degenerate stream would not show a difference"
    m.close()


# ---- 3. row count ----

@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4", "narrow_q6"])
def test_a_sequence_alone_equals_itself_among_eight(omx, name):
    """M = 1 against M = 8, bit for bit.  Packed: row t of qgemv_rows is the one-row kernel for every M.  bf16: row t of
    gemv_rows_kernel<T> accumulates acc[r][t] over the same (chunk, vector, lane) order whatever T, its in-launch RMSNorm (M <= 4)
    is rownorm_kernel's arithmetic to the bit, and below the rows route's size the 64-row tile holds all M rows in one tile."""
    cfg, m, _ = _build(name)
    V = cfg.vocab_size
    A = _prompt(70, V, 3)
    b = m.batch(8, CTX)
    t1, l1 = _run_a(b, 3, A, {}, [3])
    b.close()
    b = m.batch(8, CTX)
    t8, l8 = _run_a(b, 3, A, {s: _prompt(20 + 30 * s, V, 200 + s) for s in [0, 1, 2, 4, 5, 6, 7]}, list(range(8)))
    b.close()
    np.testing.assert_array_equal(t1, t8)
    np.testing.assert_array_equal(l1, l8)
    m.close()


# ---- 4. against the single-sequence engine, on the same model object ----

@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
def test_batch_matches_the_single_sequence_engine_and_leaves_it_alone(omx, name):
    cfg, m, oracle = _build(name)
    V, n_pos = cfg.vocab_size, 10
    P = _prompt(48, V, 9)
    ref_tokens, ref_logits = oracle.generate(P, n_pos, return_logits=True)
    bound, margins = _bound(cfg, ref_logits), rc.argmax_margin(ref_logits)
    b = m.batch(2, CTX)
    # both teacher-forced with the oracle's tokens, so that a near-tie cannot cascade
    mt, ml = [int(m.prefill(P))], [m.last_logits()]
    bt, bl = [int(b.prefill(1, P))], [b.logits(1)]
    for i in range(1, n_pos):
        m.trim(0, int(ref_tokens[i - 1]))
        mt.append(int(m.decode(1)[0])); ml.append(m.last_logits())
        b.trim(1, 0, int(ref_tokens[i - 1]))
        bt.append(int(b.decode(1, [1])[0, 0])); bl.append(b.logits(1))
    for i in range(n_pos):
        err = float(np.abs(bl[i] - ml[i]).max())
        print(f"{name} pos {i}: batch vs model {err:.4f}, batch vs oracle {float(np.abs(bl[i] - ref_logits[i]).max()):.4f}, bound {bound:.4f}")
        assert err <= 1.5 * bound
        assert np.abs(bl[i] - ref_logits[i]).max() <= 1.5 * bound
        assert bt[i] == mt[i] or margins[i] <= 2 * bound
        assert bt[i] == int(ref_tokens[i]) or margins[i] <= 2 * bound
    assert m.offset() == b.offset(1) == 48 + n_pos - 1
    # the model's own sequence with a batch at work in between: bit for bit the undisturbed run
    m.reset()
    want = np.concatenate([[m.prefill(P)], m.decode(16)])
    m.reset()
    got = np.concatenate([[m.prefill(P)], m.decode(8)])
    b.reset(0); b.reset(1)
    b.prefill(0, _prompt(100, V, 5)); b.prefill(1, _prompt(300, V, 6))
    b.decode(5)
    got = np.concatenate([got, m.decode(8)])
    np.testing.assert_array_equal(got, want)
    assert m.offset() == 48 + 16 and b.offset(0) == 105 and b.offset(1) == 305
    b.close(); m.close()


# ---- 5. subsets and bookkeeping ----

@pytest.mark.parametrize("name", ["narrow", "narrow_q4"])
def test_subsets_leave_the_other_slots_alone(omx, name):
    cfg, m, _ = _build(name)
    V = cfg.vocab_size
    prompts = [_prompt(n, V) for n in PROMPT_LENS]
    b, ctl = m.batch(8, CTX), m.batch(8, CTX)
    for s in range(8):
        assert b.prefill(s, prompts[s]) == ctl.prefill(s, prompts[s])
    before = {s: (b.offset(s), b.logits(s)) for s in range(8)}
    sub = b.decode(3, [6, 1, 3])
    assert sub.shape == (3, 3)
    for s in [0, 2, 4, 5, 7]:
        assert b.offset(s) == before[s][0] == PROMPT_LENS[s]
        np.testing.assert_array_equal(b.logits(s), before[s][1])
    for s in [6, 1, 3]:
        assert b.offset(s) == PROMPT_LENS[s] + 3
    # the columns follow the listed order: the control decodes the same three slots listed the other way round
    c = ctl.decode(3, [1, 3, 6])
    np.testing.assert_array_equal(sub, c[:, [2, 0, 1]])
    # ... and the untouched slots go on exactly as in the control, whose slots 1, 3, 6 advanced in another call: pending tokens,
    # positions and caches were not disturbed
    rest = [0, 2, 4, 5, 7]
    np.testing.assert_array_equal(b.decode(4, rest), ctl.decode(4, rest))
    for s in rest:
        np.testing.assert_array_equal(b.logits(s), ctl.logits(s))
        assert b.offset(s) == PROMPT_LENS[s] + 4
    b.close(); ctl.close(); m.close()


@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
def test_append_prefill_and_trim(omx, name):
    cfg, m, oracle = _build(name)
    V = cfg.vocab_size
    P = _prompt(75, V, 21)
    ref_tokens, ref_logits = oracle.generate(P, 1, return_logits=True)
    bound, margins = _bound(cfg, ref_logits), rc.argmax_margin(ref_logits)
    b = m.batch(3, CTX)
    whole = b.prefill(0, P)
    b.prefill(1, P[:40])
    assert b.offset(1) == 40
    parts = b.prefill(1, P[40:])                    # appended at offset 40
    b.prefill(2, P[:74])
    one = b.prefill(2, P[74:])                      # a one-token prompt on top of 74 cached tokens
    for slot, tok in [(0, whole), (1, parts), (2, one)]:
        assert b.offset(slot) == 75
        err = float(np.abs(b.logits(slot) - ref_logits[0]).max())
        print(f"{name} slot {slot}: err {err:.4f} bound {bound:.4f}")
        assert err <= 1.5 * bound
        assert tok == int(ref_tokens[0]) or margins[0] <= 2 * bound
    # trim, the form of test_trim_forgets_tokens: decode 8, drop the last 3 cached tokens, re-feed the token that followed
    b.reset(1); b.reset(2)
    b.prefill(1, P)
    b.prefill(2, P)
    want = np.concatenate([[whole], b.decode(16, [0, 1])[:, 0]])
    b.reset(0); b.reset(1)
    assert b.offset(0) == 0
    first = b.prefill(0, P)
    b.prefill(1, P)
    got = np.concatenate([[first], b.decode(8, [0, 1])[:, 0]])
    assert b.offset(0) == 75 + 8
    b.trim(0, 3, int(got[5]))
    assert b.offset(0) == 75 + 5 and b.offset(1) == 75 + 8
    rest = b.decode(11, [0, 1])[:, 0]
    np.testing.assert_array_equal(np.concatenate([got[:6], rest]), want)
    with pytest.raises(omx.OmxError, match="cannot drop"):
        b.trim(0, 10_000, 0)
    b.close(); m.close()


def test_one_token_prompt_on_an_empty_slot(omx):
    cfg, m, oracle = _build("narrow")
    P = _prompt(1, cfg.vocab_size, 333)
    ref_tokens, ref_logits = oracle.generate(P, 3, return_logits=True)
    bound, margins = _bound(cfg, ref_logits), rc.argmax_margin(ref_logits)
    b = m.batch(1, CTX)
    got = [int(b.prefill(0, P))]
    logits = [b.logits(0)]
    for i in range(1, 3):
        b.trim(0, 0, int(ref_tokens[i - 1]))
        got.append(int(b.decode(1)[0, 0]))
        logits.append(b.logits(0))
    assert b.offset(0) == 3
    for i in range(3):
        assert np.abs(logits[i] - ref_logits[i]).max() <= 1.5 * bound
        assert got[i] == int(ref_tokens[i]) or margins[i] <= 2 * bound
    b.close(); m.close()


# ---- 6. sampler ----

def test_every_slot_draws_from_its_own_key_sequence(omx):
    """Two slots at different temperatures and seeds, one greedy: each token is what oracle/mlx_rng's categorical draws from THAT
    slot's read-back logits with THAT slot's key sequence (the method of test_engine_temperature_sampling_draws_what_the_oracle_
    draws_from_the_same_logits), and a slot's draws do not depend on its neighbours."""
    cfg, m, _ = _build("narrow")
    V = cfg.vocab_size
    prompts = [_prompt(32, V, 1), _prompt(50, V, 2), _prompt(20, V, 3)]
    samplers = [(0.8, 3), (1.3, 11), (0.0, 0)]
    b = m.batch(3, CTX)
    for s, (t, seed) in enumerate(samplers):
        b.set_sampler(s, t, seed)
    toks = [[int(b.prefill(s, prompts[s]))] for s in range(3)]
    logits = [[b.logits(s)] for s in range(3)]
    for _ in range(10):
        step = b.decode(1)
        for s in range(3):
            toks[s].append(int(step[0, s]))
            logits[s].append(b.logits(s))
    for s, (t, seed) in enumerate(samplers):
        state = mlx_rng.RandomState(seed)
        want = [int(rc.sample(l[None, :], t, state.next() if t else None)[0]) for l in logits[s]]
        assert toks[s] == want, f"slot {s}"
    assert toks[0] != [int(np.argmax(l)) for l in logits[0]], "temperature 0.8 gave the greedy stream"
    # the same sequence and sampler in another slot, listed first, beside other neighbours with other samplers (same M): the same draws,
    # in one decode call
    b2 = m.batch(3, CTX)
    b2.set_sampler(2, 0.8, 3); b2.set_sampler(0, 0.5, 99); b2.set_sampler(1, 2.0, 5)
    b2.prefill(0, _prompt(44, V, 7)); b2.prefill(1, _prompt(9, V, 8))
    again = [int(b2.prefill(2, prompts[0]))] + [int(t) for t in b2.decode(10, [2, 1, 0])[:, 0]]
    assert again == toks[0]
    # another seed: another stream
    b2.reset(2)
    b2.set_sampler(2, 0.8, 4)
    other = [int(b2.prefill(2, prompts[0]))] + [int(t) for t in b2.decode(10, [2, 1, 0])[:, 0]]
    assert other != toks[0]
    with pytest.raises(omx.OmxError, match="must be >= 0"):
        b.set_sampler(0, -1.0, 0)
    b.close(); b2.close(); m.close()


# ---- 7. refusals ----

def test_refusals(omx):
    from ominix_mlx_amd import engine
    moe = engine.Model(hidden_size=1024, num_hidden_layers=1, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                       vocab_size=1024, max_context=256, num_experts=4, num_experts_per_tok=2, moe_intermediate_size=512)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_create: models with experts \(MoE\) are not supported"):
        moe.batch(2)
    moe.close()
    f16 = engine.Model(hidden_size=1024, num_hidden_layers=1, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                       vocab_size=1024, max_context=256, dtype="float16")
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_create: dense float16 models \(float16_weights\) are not supported"):
        f16.batch(2)
    f16.close()
    f16q = engine.Model(hidden_size=1024, num_hidden_layers=1, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                        vocab_size=1024, max_context=256, quantization={"bits": 4, "group_size": 64, "scales_dtype": "float16"})
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_create: float16 triplets"):
        f16q.batch(2)
    f16q.close()
    tp = engine.Model(hidden_size=1024, num_hidden_layers=1, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                      vocab_size=1024, max_context=256, tp_size=2, tp_rank=0)
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_create: tensor / expert parallel models are not supported"):
        tp.batch(2)
    tp.close()

    cfg, m, _ = _build("narrow", max_context=256)
    V = cfg.vocab_size
    m.set_sampler(0.7, 1, top_k=20)
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_create: filtered sampling"):
        m.batch(2)
    m.set_sampler(0.0)
    for n in (0, 9):
        with pytest.raises(omx.OmxError, match=rf"omx_qwen3_batch_create: {n} slots \(1\.\.8\)"):
            m.batch(n)
    with pytest.raises(omx.OmxError, match="exceeds the model's"):
        m.batch(2, 4096)
    b = m.batch(3)                                   # max_context 0: the model's 256
    P = _prompt(20, V)
    with pytest.raises(omx.OmxError, match=r"slot 3 out of range \(0\.\.2\)"):
        b.prefill(3, P)
    with pytest.raises(omx.OmxError, match=r"slot -1 out of range"):
        b.logits(-1)
    with pytest.raises(omx.OmxError, match=rf"token id {V} out of range"):
        b.prefill(0, [1, 2, V])
    with pytest.raises(omx.OmxError, match="slot 0 has not been prefilled"):
        b.decode(1, [0])
    b.prefill(0, P); b.prefill(1, P)
    with pytest.raises(omx.OmxError, match="slot 1 listed twice"):
        b.decode(1, [1, 0, 1])
    with pytest.raises(omx.OmxError, match="slot 2 has not been prefilled"):
        b.decode(1, [0, 2])
    with pytest.raises(omx.OmxError, match=r"slot 5 out of range"):
        b.decode(1, [0, 5])
    with pytest.raises(omx.OmxError, match=r"4 slots listed \(1\.\.3\)"):
        b.decode(1, [0, 1, 2, 0])
    with pytest.raises(omx.OmxError, match=rf"token id {V + 5} out of range"):
        b.trim(0, 0, V + 5)
    with pytest.raises(omx.OmxError, match="exceed max_context 256"):
        b.prefill(2, _prompt(256, V))
    # offset + n_steps beyond the capacity: refused before anything runs -- offsets, logits and the continuation are what they were
    keep = (b.offset(0), b.offset(1), b.logits(0), b.logits(1))
    with pytest.raises(omx.OmxError, match=r"slot 0: 20 cached \+ 237 new tokens exceed max_context 256"):
        b.decode(237, [0, 1])
    assert (b.offset(0), b.offset(1)) == keep[:2] == (20, 20)
    np.testing.assert_array_equal(b.logits(0), keep[2])
    np.testing.assert_array_equal(b.logits(1), keep[3])
    ctl = m.batch(2)
    ctl.prefill(0, P); ctl.prefill(1, P)
    np.testing.assert_array_equal(b.decode(236, [0, 1]), ctl.decode(236))      # ... and 236 steps fill the slabs to the last row
    assert b.offset(0) == 256
    with pytest.raises(omx.OmxError, match="exceed max_context 256"):
        b.decode(1, [0])
    b.close(); ctl.close(); m.close()


# ---- 8. real width, plumbing ----

def test_real_width_eight_slots_count_down(omx):
    """Qwen3-8B's shapes with 4 layers on the PEAKED synthetic checkpoint (the greedy successor of token t is t - 1 by construction
    of the embedding and the head, include/omx.h): 8 slots with prompts of 40 .. 2 100 tokens, 24 steps -- every slot's tokens are its
    exact countdown.  Plumbing at real width (the rows launches at hidden 4096 / vocabulary 151 936, eight slabs, the ragged attention
    over 9 splits), not a numerics test."""
    from ominix_mlx_amd import engine
    V = 151936
    m = engine.Model(hidden_size=4096, num_hidden_layers=4, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8,
                     head_dim=128, vocab_size=V, max_context=2304)
    m.synth_weights(peaked=True)
    lens = [40, 2100, 300, 1000, 77, 1500, 513, 256]
    prompts = [_prompt(n, V) for n in lens]
    b = m.batch(8)
    firsts = [int(b.prefill(s, prompts[s])) for s in range(8)]
    steps = np.concatenate([b.decode(16), b.decode(8)])
    for s in range(8):
        got = [firsts[s]] + [int(t) for t in steps[:, s]]
        assert got == [(int(prompts[s][-1]) - 1 - i) % V for i in range(25)], f"slot {s}"
        assert b.offset(s) == lens[s] + 24
    b.close(); m.close()
