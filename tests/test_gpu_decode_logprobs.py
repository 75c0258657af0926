"""Per-token log-probabilities and top-n alternatives inside the decode steps (omx_qwen3_set_logprobs / _decode_logprobs /
_last_logprobs and their omx_qwen3_batch_ forms; engine.Model / engine.Batch / engine.Generate): every reported value against a
float64 log-softmax of exactly the row the engine returns for that step, one call against many, graph against eager, on against
off, against the oracle, a slot against its company, forks, subsets and the refusals."""
import numpy as np
import pytest

from logprob_rule import logprob64, logsumexp64
from oracle import ref_qwen3 as rq, synth
from test_gpu_batch_decode import PROMPT_LENS, _build, _prompt
from test_gpu_logprob import TOL
from test_gpu_logprob_top import _host_top
from test_gpu_score import _moe_model
from test_gpu_speculative import TARGET, WIDE

pytestmark = pytest.mark.gpu

CTX = 512


def _model(omx, name):
    if name == "mixtral":
        return _moe_model(omx)
    cfg, m, _ = _build(name, CTX)
    return cfg, m


def _check(row, token, lp, ids, tlp, what):
    """one token's values against float64 on `row` (float32-widened bf16 logits): logprob and top_logprobs within TOL = 1e-4 (the
    bound of test_gpu_logprob.py: the logit is exact, the f32 lse within ~1e-6, one f32 subtraction), top_ids exactly"""
    lse = logsumexp64(row[None])[0]
    assert abs(float(lp) - (float(row[int(token)]) - lse)) <= TOL, f"{what}: logprob {lp} vs {float(row[int(token)]) - lse}"
    np.testing.assert_array_equal(ids, _host_top(row[None], len(ids))[0], err_msg=what)
    assert np.abs(tlp.astype(np.float64) - (row[ids.astype(np.int64)].astype(np.float64) - lse)).max() <= TOL, what


@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4", "mixtral"])
def test_model_values_are_those_of_the_steps_own_row(omx, name):
    """greedy, top_n = 5: the prefill's first token through last_logprobs(), then 12 steps of decode(1, return_logprobs=True), each
    against last_logits() of that step; the drawn token is top_ids[0]"""
    cfg, m = _model(omx, name)
    m.set_logprobs(5)
    first = m.prefill(synth.prompt_ids(33, cfg.vocab_size))
    lp, ids, tlp = m.last_logprobs()
    _check(m.last_logits(), first, lp, ids, tlp, f"{name} prefill")
    assert int(ids[0]) == int(first)
    for i in range(12):
        tok, lp, ids, tlp = m.decode(1, return_logprobs=True)
        assert tok.shape == (1,) and lp.shape == (1,) and ids.shape == (1, 5) and tlp.shape == (1, 5)
        _check(m.last_logits(), tok[0], lp[0], ids[0], tlp[0], f"{name} step {i}")
        assert int(ids[0, 0]) == int(tok[0])
        last = m.last_logprobs()
        assert last[0].view(np.uint32) == lp.view(np.uint32)[0] and np.array_equal(last[1], ids[0])
    m.close()


def test_one_call_or_many_graph_or_eager(omx, monkeypatch):
    """decode(16, return_logprobs=True) in one call (graph replay) = 16 calls of decode(1) = one call under OMX_NO_GRAPH=1, as bits"""
    cfg = TARGET
    prompt = synth.prompt_ids(33, cfg.vocab_size)
    runs = []
    for mode in ("one", "many", "eager"):
        if mode == "eager":
            monkeypatch.setenv("OMX_NO_GRAPH", "1")
        _, m = _model(omx, "narrow")
        m.set_logprobs(5)
        m.prefill(prompt)
        if mode == "many":
            parts = [m.decode(1, return_logprobs=True) for _ in range(16)]
            out = [np.concatenate([p[k] for p in parts]) for k in range(4)]
        else:
            out = list(m.decode(16, return_logprobs=True))
        assert m.decode_path().startswith("eager" if mode == "eager" else "graph")
        runs.append(out)
        m.close()
    assert len(set(runs[0][0].tolist())) > 4, "a degenerate stream would not show a difference"
    for other, what in ((runs[1], "16 calls"), (runs[2], "eager")):
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


SAMPLER = dict(temperature=0.8, seed=5, top_k=20, top_p=0.95)


@pytest.mark.parametrize("sampler", [None, SAMPLER], ids=["greedy", "filtered"])
def test_off_means_off(omx, sampler):
    """tokens and last_logits() bits of a model with logprobs on equal those of a model that never heard of them: greedy, and under
    temperature 0.8 / top_k 20 / top_p 0.95 at one seed.  Under the sampler the drawn token's logprob is still the raw row's, and on
    at least one step it is below top_logprobs[0] (the draw was not the argmax)."""
    cfg = TARGET
    prompt = synth.prompt_ids(33, cfg.vocab_size)
    _, plain = _model(omx, "narrow")
    _, on = _model(omx, "narrow")
    on.set_logprobs(5)
    for m in (plain, on):
        if sampler:
            m.set_sampler(sampler["temperature"], sampler["seed"], top_k=sampler["top_k"], top_p=sampler["top_p"])
    assert plain.prefill(prompt) == on.prefill(prompt)
    below = 0
    for i in range(12):
        want = plain.decode(1)
        tok, lp, ids, tlp = on.decode(1, return_logprobs=True)
        np.testing.assert_array_equal(tok, want)
        row = on.last_logits()
        np.testing.assert_array_equal(row.view(np.uint32), plain.last_logits().view(np.uint32))
        _check(row, tok[0], lp[0], ids[0], tlp[0], f"step {i}")
        below += bool(lp[0] < tlp[0, 0])
        if not sampler:
            assert int(ids[0, 0]) == int(tok[0])
    np.testing.assert_array_equal(on.decode(8), plain.decode(8))
    np.testing.assert_array_equal(on.last_logits().view(np.uint32), plain.last_logits().view(np.uint32))
    # ... and switched off again, the model goes on as the other does
    on.set_logprobs(None)
    np.testing.assert_array_equal(on.decode(4), plain.decode(4))
    with pytest.raises(omx.OmxError, match="omx_qwen3_decode_logprobs: log-probabilities are off"):
        on.decode(1, return_logprobs=True)
    if sampler:
        print(f"filtered: the draw was below the row's best on {below} of 12 steps")
        assert below >= 1
    plain.close(); on.close()


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_against_the_oracle(omx, name):
    """The 33-token prompt plus the engine's 24 greedy tokens, teacher-forced through Qwen3Oracle.forward: |lp - lp_ref| <= 2 * 1.5 *
    bound, bound = 2^-7 max|ref| sqrt(L) -- the argument and margin of test_gpu_score._check_against_oracle (a log-prob is a logit
    minus a soft maximum of logits, each within 1.5 bound of the oracle's)."""
    cfg, m, oracle = _build(name, CTX)
    prompt = synth.prompt_ids(33, cfg.vocab_size)
    m.set_logprobs(0)
    first = m.prefill(prompt)
    lp0 = m.last_logprobs()
    toks, lps = m.decode(23, return_logprobs=True)
    gen = np.concatenate([[first], toks]).astype(np.uint32)
    lp = np.concatenate([[lp0], lps])
    ids = np.concatenate([prompt, gen]).astype(np.uint32)
    ref = oracle.forward(ids[None], [])[0].astype(np.float32)
    bound = 2.0 ** -7 * np.abs(ref).max() * np.sqrt(cfg.num_hidden_layers)
    lp_ref, _ = logprob64(ref[32:32 + 24], gen)
    worst = np.abs(lp - lp_ref).max()
    print(f"{name}: worst |lp - lp_ref| = {worst:.4f} = {worst / bound:.3f} bound (bound {bound:.4f})")
    assert worst <= 2 * 1.5 * bound
    m.close()


def _bits(*arrays):
    return [np.asarray(a).view(np.uint32) for a in arrays]


@pytest.mark.parametrize("name,kv_bits", [("narrow", 0), ("narrow_q4", 0), ("narrow", 8)], ids=["narrow", "narrow_q4", "narrow_kv8"])
def test_batch_values_neighbours_forks_and_subsets(omx, name, kv_bits):
    """Eight slots with PROMPT_LENS, top_n = 3: every prefill's first token and 6 steps of decode(1, all slots) against
    Batch.logits(slot) of that step.  Slot 3's bits alone (M = 1) and under a permuted slot order equal those among eight.  A
    fork(resample=True) sibling at temperature 0.7 reports its OWN token over the source's kept row; fork(resample=False) the source's
    values.  A subset decode leaves the other slots' last values alone."""
    cfg, m, _ = _build(name, CTX)
    V = cfg.vocab_size
    prompts = [_prompt(n, V) for n in PROMPT_LENS]
    A = 3

    def run(slots, order):
        b = m.batch(8, CTX, kv_bits=kv_bits)
        b.set_logprobs(3)
        out = {s: [] for s in slots}
        for s in slots:
            first = b.prefill(s, prompts[s])
            lp, ids, tlp = b.last_logprobs(s)
            _check(b.logits(s), first, lp, ids, tlp, f"slot {s} prefill")
            out[s].append((np.uint32(first), lp, ids, tlp))
        for i in range(6):
            tok, lp, ids, tlp = b.decode(1, order, return_logprobs=True)
            assert lp.shape == (1, len(order)) and ids.shape == (1, len(order), 3)
            for col, s in enumerate(order):
                _check(b.logits(s), tok[0, col], lp[0, col], ids[0, col], tlp[0, col], f"slot {s} step {i}")
                out[s].append((tok[0, col], lp[0, col], ids[0, col], tlp[0, col]))
        return b, out

    b, among = run(list(range(8)), list(range(8)))
    b1, alone = run([A], [A])
    b2, mixed = run(list(range(8)), [5, 0, 7, 3, 1, 6, 2, 4])
    for other, what in ((alone, "alone"), (mixed, "permuted")):
        for step, (x, y) in enumerate(zip(among[A], other[A])):
            for p, q in zip(_bits(*x), _bits(*y)):
                np.testing.assert_array_equal(p, q, err_msg=f"slot {A} {what}, entry {step}")
    b2.close()

    # forks, on the batch that holds slot A alone
    src_row = b1.logits(A)
    b1.set_sampler(5, 0.7, 11)
    tok = b1.fork(A, 5, True)
    lp, ids, tlp = b1.last_logprobs(5)
    _check(src_row, tok, lp, ids, tlp, "resampled sibling")
    tok = b1.fork(A, 6, False)
    for p, q in zip(_bits(*b1.last_logprobs(6)), _bits(*b1.last_logprobs(A))):
        np.testing.assert_array_equal(p, q, err_msg="a sibling that shares the source's token")
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_last_logprobs: slot 7 has sampled no token"):
        b1.last_logprobs(7)
    b1.close()

    # a subset decode
    before = {s: _bits(*b.last_logprobs(s)) for s in range(8)}
    tok, lp, ids, tlp = b.decode(2, [6, 1, 3], return_logprobs=True)
    for s in [0, 2, 4, 5, 7]:
        for p, q in zip(_bits(*b.last_logprobs(s)), before[s]):
            np.testing.assert_array_equal(p, q, err_msg=f"slot {s} was not listed")
    for col, s in enumerate([6, 1, 3]):
        last = b.last_logprobs(s)
        _check(b.logits(s), tok[1, col], last[0], last[1], last[2], f"slot {s} after the subset")
        for p, q in zip(_bits(*last), _bits(lp[1, col], ids[1, col], tlp[1, col])):
            np.testing.assert_array_equal(p, q)
    # off again: the plain call, and the logprobs call refused by name
    b.set_logprobs(None)
    assert b.decode(1).shape == (1, 8)
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_decode_logprobs: log-probabilities are off"):
        b.decode(1, return_logprobs=True)
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_set_logprobs: top_n = 21 is outside"):
        b.set_logprobs(21)
    b.close(); m.close()


def test_generate_reports_what_it_yields(omx):
    """Generate(..., logprobs=2) yields the tokens Generate yields without it; .logprobs / .top_logprobs cover exactly the tokens
    yielded so far, the greedy token leading its alternatives"""
    from ominix_mlx_amd import engine
    cfg = TARGET
    prompt = synth.prompt_ids(33, cfg.vocab_size)
    _, m = _model(omx, "narrow")
    want = [t for _, t in zip(range(9), engine.Generate(m, 0.0, prompt, chunk=4))]
    m.reset()
    g = engine.Generate(m, 0.0, prompt, chunk=4, logprobs=2)
    got = [t for _, t in zip(range(9), g)]
    assert got == want and len(g.logprobs) == 9 and len(g.top_logprobs) == 9
    assert all(alts[0][0] == t and abs(alts[0][1] - lp) == 0 and len(alts) == 2 for t, lp, alts in zip(got, g.logprobs, g.top_logprobs))
    assert all(lp <= 0 for lp in g.logprobs)
    m.close()


def test_refusals_by_name(omx):
    """(top_n = V + 1 is refused on the raw op, test_gpu_logprob_top.test_refusals_by_name: the engine's smallest vocabulary is far
    above 20, where the limit of 20 refuses first)"""
    from ominix_mlx_amd import engine

    def model(cfg, **kw):
        return engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                            num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                            vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, max_context=256, **kw)

    m = model(TARGET, tp_size=2)
    with pytest.raises(omx.OmxError, match="omx_qwen3_set_logprobs: tensor / expert parallel models are not supported"):
        m.set_logprobs(5)
    m.set_logprobs(None)                    # switching off what is off is no error
    m.close()
    m = model(WIDE, dtype="float16")
    with pytest.raises(omx.OmxError, match="omx_qwen3_set_logprobs: float16 models"):
        m.set_logprobs(0)
    m.close()
    _, m = _model(omx, "narrow")
    for n in (21, -2):
        with pytest.raises(omx.OmxError, match=f"omx_qwen3_set_logprobs: top_n = {n} is outside -1..min\\(20, V = 2048\\)"):
            m.set_logprobs(n)
    m.prefill(synth.prompt_ids(8, TARGET.vocab_size))
    with pytest.raises(omx.OmxError, match="omx_qwen3_decode_logprobs: log-probabilities are off"):
        m.decode(1, return_logprobs=True)
    with pytest.raises(omx.OmxError, match="omx_qwen3_last_logprobs: log-probabilities are off"):
        m.last_logprobs()
    m.set_logprobs(5)
    with pytest.raises(omx.OmxError, match="omx_qwen3_last_logprobs: no token has been sampled since"):
        m.last_logprobs()
    tok, lp, ids, tlp = m.decode(2, return_logprobs=True)
    assert int(ids[1, 0]) == int(tok[1]) and m.last_logprobs()[0] == lp[1]
    m.close()
