"""Per-slot top-k, top-p and repetition / presence penalties inside the batched decode step (engine.Batch.set_sampler's keywords;
omx_qwen3_batch_set_sampling, launch_batch_filtered in csrc/sample_filter.hip): every slot's token is what the rule of
tests/sampling_rule.py draws from THAT slot's read-back logits with THAT slot's key sequence and history (the method of
test_gpu_sampling.py section 4: exact for top-k and penalties, the float64 sandwich with DELTA = 2^-10 for top-p), a slot does not
depend on its neighbours' settings, "off" is the plain sampler bit for bit, and the history follows prefill / reset / set_sampler /
fork.  The V = 2 048 models take the one-block-per-row launch, the V = 151 936 model ("big": 1 layer, hidden 512) the launch per
level with one grid row per sequence."""
import numpy as np
import pytest

from oracle import mlx_rng as rng
import sampling_rule as sr
from test_gpu_speculative import TARGET, WIDE, _engine  # noqa: F401  (the tiny models _build puts together)
from test_gpu_batch_decode import _build, _prompt
from test_gpu_sampling import CASES, _expected_tokens, _check_against_rule  # noqa: F401

pytestmark = pytest.mark.gpu

CTX = 512
BIG_V = 151936
STEPS = 8
CARD = dict(top_k=20, top_p=0.95)                 # the Qwen3 model card's filters, at its temperature 0.6
GREEDY_PEN = dict(repetition_penalty=1.35, presence_penalty=1.5)
# (temperature, seed, filters) of six slots that decode in the SAME steps
SETTINGS = [(0.6, 101, dict(top_k=20)), (0.6, 102, CARD), (0.6, 103, dict(top_p=0.9)), (0.6, 104, dict(top_k=20, presence_penalty=1.5)),
            (0.6, 105, {}), (0.0, 0, GREEDY_PEN)]
LENS = [20, 33, 50, 27, 41, 24]


@pytest.fixture(scope="module")
def models():
    """name -> (vocabulary, engine model), built on first use and closed with the module"""
    made = {}

    def get(name):
        if name not in made:
            if name == "big":
                from ominix_mlx_amd import engine
                m = engine.Model(hidden_size=512, num_hidden_layers=1, intermediate_size=1536, num_attention_heads=8, num_key_value_heads=2,
                                 head_dim=64, vocab_size=BIG_V, max_context=CTX)
                m.synth_weights()
                made[name] = (BIG_V, m)
            else:
                cfg, m, _ = _build(name, CTX)
                made[name] = (cfg.vocab_size, m)
        return made[name]

    yield get
    for _, m in made.values():
        m.close()


def _set(b, slot, setting):
    temp, seed, kw = setting
    b.set_sampler(slot, temp, seed, **kw)


def _run(b, slots, prompts, steps=STEPS, order=None):
    """prefill every slot of `slots` with its prompt, then `steps` single-step calls over `order` -> {slot: tokens}, {slot: logits}"""
    order = list(slots) if order is None else order
    toks = {s: [int(b.prefill(s, prompts[s]))] for s in slots}
    logits = {s: [b.logits(s)] for s in slots}
    for _ in range(steps):
        step = b.decode(1, order)
        for c, s in enumerate(order):
            toks[s].append(int(step[0, c]))
            logits[s].append(b.logits(s))
    return toks, logits


def _check_slot(toks, logits, setting):
    temp, seed, kw = setting
    if temp == 0.0:
        for i, l in enumerate(logits):
            assert toks[i] == int(np.argmax(sr.scaled(l, 0.0, sorted(set(toks[:i])), kw.get("repetition_penalty", 1.0), kw.get("presence_penalty", 0.0)))), f"token {i}"
    else:
        _check_against_rule(toks, logits, temp, seed, kw)


# ---- 1. each slot draws what the rule draws from its own logits ----

@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4", "big"])
def test_each_slot_draws_what_the_rule_draws_from_its_own_logits(omx, models, name):
    V, m = models(name)
    prompts = {s: _prompt(LENS[s], V, 10 + s) for s in range(6)}
    b = m.batch(6, CTX)
    for s in range(6):
        _set(b, s, SETTINGS[s])
    toks, logits = _run(b, range(6), prompts)
    b.close()
    for s in range(6):
        _check_slot(toks[s], logits[s], SETTINGS[s])
    assert len(set(toks[5])) == len(toks[5]), "the greedy slot repeated a token under a presence penalty of 1.5"
    # a fresh batch, ONE decode(n) call: the same tokens -- marks and key advances are ordered on the device
    b = m.batch(6, CTX)
    for s in range(6):
        _set(b, s, SETTINGS[s])
    firsts = [int(b.prefill(s, prompts[s])) for s in range(6)]
    rest = b.decode(STEPS)
    for s in range(6):
        assert [firsts[s]] + [int(t) for t in rest[:, s]] == toks[s], f"slot {s}"
    b.close()


# ---- 2. neighbours do not change a slot ----

@pytest.mark.parametrize("name", ["narrow", "big"])
def test_neighbours_do_not_change_a_slot(omx, models, name):
    V, m = models(name)
    A, card = _prompt(37, V, 3), (0.6, 7, CARD)
    others = {s: _prompt(21 + 6 * s, V, 40 + s) for s in range(4)}

    def run(slot_a, neighbours, order, setting_a=card):
        """A in slot_a under setting_a beside `neighbours` {slot: setting} at M = 4 -> (tokens, logits) of A"""
        b = m.batch(4, CTX)
        _set(b, slot_a, setting_a)
        for s, st in neighbours.items():
            _set(b, s, st)
        prompts = {s: others[s] for s in neighbours}
        prompts[slot_a] = A
        toks, logits = _run(b, [slot_a] + list(neighbours), prompts, order=order)
        b.close()
        return toks[slot_a], np.stack(logits[slot_a])

    base_t, base_l = run(0, {1: SETTINGS[0], 2: SETTINGS[3], 3: SETTINGS[5]}, [0, 1, 2, 3])
    variants = [
        run(0, {1: (0.9, 55, dict(top_p=0.5)), 2: (1.3, 56, dict(top_k=5, repetition_penalty=1.2)), 3: (0.6, 57, CARD)}, [0, 1, 2, 3]),   # other settings, other seeds
        run(2, {0: SETTINGS[3], 1: SETTINGS[5], 3: SETTINGS[0]}, [3, 1, 0, 2]),                                                          # another slot, another listed order
        run(0, {1: (0.7, 1, {}), 2: (0.0, 0, {}), 3: (1.1, 2, {})}, [0, 1, 2, 3]),                                                       # every neighbour plain
    ]
    for i, (t, l) in enumerate(variants):
        assert t == base_t, f"variant {i}"
        np.testing.assert_array_equal(l, base_l)
    _check_slot(base_t, list(base_l), card)
    # a PLAIN slot beside filtered neighbours (the filtered route) draws what it draws in an all-plain batch (the plain kernel)
    plain = (0.8, 31, {})
    mixed_t, mixed_l = run(1, {0: SETTINGS[1], 2: SETTINGS[3], 3: SETTINGS[5]}, [0, 1, 2, 3], plain)
    alone_t, alone_l = run(1, {0: (0.7, 1, {}), 2: (0.0, 0, {}), 3: (1.1, 2, {})}, [0, 1, 2, 3], plain)
    assert mixed_t == alone_t
    np.testing.assert_array_equal(mixed_l, alone_l)
    assert len(set(mixed_t)) > 3, "a degenerate stream would not show a difference"


# ---- 3. off means off ----

@pytest.mark.parametrize("name", ["narrow", "big"])
def test_off_means_off(omx, models, name):
    V, m = models(name)
    P, temp, seed = _prompt(30, V, 5), 0.8, 21

    def stream(b, **kw):
        b.reset(0)
        b.set_sampler(0, temp, seed, **kw)
        return [int(b.prefill(0, P))] + [int(t) for t in b.decode(STEPS, [0])[:, 0]]

    b = m.batch(2, CTX)
    b.set_sampler(0, temp, seed)
    unfiltered = [int(b.prefill(0, P))] + [int(t) for t in b.decode(STEPS, [0])[:, 0]]
    assert stream(b, top_k=0, top_p=1.0) == unfiltered
    assert stream(b, top_k=V) == unfiltered
    assert stream(b, top_k=V + 5) == unfiltered
    filtered = stream(b, top_k=20)
    assert filtered != unfiltered
    assert stream(b) == unfiltered, "a plain set_sampler after a filtered run did not bring the plain stream back"
    assert stream(b, top_k=20) == filtered
    b.close()


# ---- 4. history lifecycle ----

@pytest.mark.parametrize("name", ["narrow", "big"])
def test_history_lifecycle(omx, models, name):
    V, m = models(name)
    P, Q = _prompt(26, V, 8), _prompt(9, V, 9)
    setting = (0.6, 104, dict(top_k=20, presence_penalty=1.5))
    greedy = (0.0, 0, GREEDY_PEN)
    b = m.batch(2, CTX)
    _set(b, 0, setting)
    _set(b, 1, greedy)
    first, first_l = _run(b, [0, 1], {0: P, 1: P})
    # reset + prefill replays the first stream (the sampler set again: the key sequence restarts; the history is empty again)
    for s in (0, 1):
        b.reset(s)
    _set(b, 0, setting)
    again, _ = _run(b, [0, 1], {0: P, 1: P})
    assert again == first
    # an appending prefill starts an EMPTY history: the rule with the history restarted (and, for slot 0, the key sequence going on)
    t0 = [int(b.prefill(0, Q))]
    t1 = [int(b.prefill(1, Q))]
    l0, l1 = [b.logits(0)], [b.logits(1)]
    for _ in range(4):
        step = b.decode(1)
        t0.append(int(step[0, 0])); l0.append(b.logits(0))
        t1.append(int(step[0, 1])); l1.append(b.logits(1))
    _check_slot(t1, l1, greedy)
    state = rng.RandomState(setting[1])
    for _ in range(1 + STEPS):
        state.next()
    for i, l in enumerate(l0):
        y = sr.scaled(l, setting[0], sorted(set(t0[:i])), 1.0, 1.5)
        assert t0[i] in _expected_tokens(y, setting[2], state.next()), f"token {i} after the appending prefill"
    # ... and the greedy slot is free to repeat what it emitted before that prefill, which a kept history would forbid: its first
    # token after the appended prompt is the plain argmax
    assert t1[0] == int(np.argmax(l1[0]))
    # set_sampler clears the history: the next token is the rule's with an empty history, not with the five tokens just sampled
    _set(b, 1, greedy)
    tok = int(b.decode(1, [1])[0, 0])
    assert tok == int(np.argmax(b.logits(1)))
    b.close()


# ---- 5. fork ----

@pytest.mark.parametrize("name", ["narrow", "big"])
def test_forked_siblings_draw_under_their_own_settings(omx, models, name):
    V, m = models(name)
    P, temp, seed = _prompt(44, V, 12), 0.6, 300
    kw = dict(top_k=20, top_p=0.95, presence_penalty=1.5)
    b = m.batch(4, CTX)
    b.set_sampler(0, temp, seed, **kw)
    toks = {0: [int(b.prefill(0, P))]}
    owner_logits = b.logits(0)
    for s in (1, 2, 3):
        b.set_sampler(s, temp, seed + s, **kw)
        toks[s] = [int(b.fork(0, s, True))]
        np.testing.assert_array_equal(b.logits(s), owner_logits)
    logits = {s: [owner_logits] for s in range(4)}
    for _ in range(STEPS):
        step = b.decode(1)
        for s in range(4):
            toks[s].append(int(step[0, s]))
            logits[s].append(b.logits(s))
    for s in range(4):      # first token: the OWNER's prefill logits, the sibling's first key, an empty history; then its own history
        _check_against_rule(toks[s], logits[s], temp, seed + s, kw)
    assert len({tuple(toks[s]) for s in range(4)}) == 4
    b.close()


def test_fork_without_resample_copies_the_history(omx, models):
    V, m = models("narrow")
    P = _prompt(31, V, 14)
    b = m.batch(2, CTX)
    b.set_sampler(0, 0.0, 0, **GREEDY_PEN)
    b.set_sampler(1, 0.0, 0, **GREEDY_PEN)
    seen = [int(b.prefill(0, P))] + [int(t) for t in b.decode(4, [0])[:, 0]]
    assert int(b.fork(0, 1, False)) == seen[-1]
    for i in range(STEPS):
        step = b.decode(1)
        assert int(step[0, 0]) == int(step[0, 1]), f"step {i}: the sibling left its source"
        seen.append(int(step[0, 0]))
        np.testing.assert_array_equal(b.logits(0), b.logits(1))
    assert len(set(seen)) == len(seen)           # (the history is at work: no token comes back)
    b.close()


def test_generate_batch_with_filters_is_reproducible(omx, models):
    from ominix_mlx_amd import generate
    V, m = models("narrow")
    prompts = [list(_prompt(23, V, 1)), list(_prompt(35, V, 2))]

    def run(seed):
        b = m.batch(8, CTX)
        outs = generate.generate_batch(b, prompts, 10, chunk=4, n=4,
                                       before_sibling=lambda p, k, slot: b.set_sampler(slot, 0.6, seed + k, presence_penalty=1.5, **CARD))
        b.close()
        return outs

    a, again, other = run(5), run(5), run(6)
    assert a == again and a != other
    for p in range(2):
        assert len({tuple(o) for o in a[4 * p:4 * p + 4]}) == 4, "siblings drew the same completion"


# ---- 6. refusals ----

def test_refusals_name_the_reason(omx, models):
    V, m = models("narrow")
    P = _prompt(20, V)
    b = m.batch(3, CTX)
    b.set_sampler(0, 0.6, 1, presence_penalty=1.5)
    first = b.prefill(0, P)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_trim: slot 0 has a repetition / presence penalty on"):
        b.trim(0, 0, first)
    b.set_sampler(1, 0.6, 2, **CARD)             # top-k / top-p only: trim works as before
    b.prefill(1, P)
    b.trim(1, 1, int(P[-1]))
    assert b.offset(1) == 19
    b.decode(2, [0])
    b.set_sampler(2, 0.6, 3, presence_penalty=1.5)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_fork: destination slot 2 has a repetition / presence penalty on and source slot 0 has decoded 2"):
        b.fork(0, 2, True)
    b.fork(0, 2, False)                          # the history is copied: accepted
    b.reset(2)
    b.set_sampler(2, 0.6, 3, **CARD)             # no penalty on dst: a resample past the prefill is accepted as before
    b.fork(0, 2, True)
    for bad, why in [(dict(top_p=0.0), "top_p"), (dict(top_k=-1), "top_k"), (dict(repetition_penalty=0.0), "repetition_penalty")]:
        with pytest.raises(omx.OmxError, match=rf"omx_qwen3_batch_set_sampling: {why}"):
            b.set_sampler(0, 0.6, 1, **bad)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_set_sampling: slot 3 out of range \(0\.\.2\)"):
        b.set_sampler(3, 0.6, 1, top_k=20)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_set_sampling: slot -1 out of range"):
        b.set_sampler(-1, 0.6, 1, top_k=20)
    b.close()
