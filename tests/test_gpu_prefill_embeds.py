"""A prompt pass whose rows the caller supplies (omx_qwen3_prefill_embeds, omx_qwen3_embed_tokens; Model.prefill(embeds=, embeds_at=),
Model.embed_tokens) -- the reference's forward_embeddings(inputs_embeds, cache), qwen3-asr-mlx/src/model.rs:720-769, 782 -- on tiny Qwen3
models in bf16, float16 and 4-bit group 64 (and one mixed-format table).

Bounds (cited, not chosen here): logits against the oracle under the prompt-pass bounds of tests/test_gpu_qwen3.py --
  bf16     2^-7  * max|logit| * sqrt(layers)        (test_greedy_decode_matches_oracle)
  4-bit    2^-7  * max|logit| * sqrt(2 * layers)    (test_quantized_checkpoint_decode_matches_oracle)
  float16  2^-10 * max|logit| * sqrt(2 * layers)    (test_f16_triplets..., tests/test_gpu_dense_f16.py _bound)
Everything else here is bit equality."""
import ctypes
import functools

import numpy as np
import pytest

import mixed_quant_helpers as mq
import qwen3_asr_rule as rule
from oracle import ref_core as rc
from oracle import ref_qwen3 as rq
from oracle import synth

pytestmark = pytest.mark.gpu

KINDS = ("bf16", "f16", "q4")
N_PROMPT = 24          # above the float16 model's 16-row token-serial threshold
PAD = 7                # the id the caller leaves at overridden positions
SPANS = [(0, 24), (0, 7), (9, 17), (15, 24), (11, 12)]   # whole prompt, start, middle, end with the last row, one row
U32P = ctypes.POINTER(ctypes.c_uint32)


def _cfg(kind):
    if kind == "f16":   # (a dense float16 model needs head_dim 128)
        return rq.Qwen3Config(1024, 2, 3072, 8, 2, 128, 4096, 1e-6, 1e6, True)
    return rq.Qwen3Config(512, 2, 1536, 8, 4, 64, 2048, 1e-6, 1e6, False)


def _kw(cfg, max_context=128):
    return dict(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                tie_word_embeddings=cfg.tie_word_embeddings, max_context=max_context)


@functools.lru_cache(maxsize=None)
def _host(kind):
    """(cfg, checkpoint, oracle, activation dtype, logit bound factor) -- built once per kind"""
    cfg = _cfg(kind)
    L = cfg.num_hidden_layers
    if kind == "bf16":
        w = rq.synth_weights(cfg)
        return cfg, w, rq.Qwen3Oracle(cfg, w), "bf16", 2.0 ** -7 * np.sqrt(L)
    if kind == "f16":
        w = rq.synth_weights(cfg, dt="f16")
        return cfg, w, rq.Qwen3Oracle(cfg, w, dt="f16"), "f16", 2.0 ** -10 * np.sqrt(2 * L)
    w = rq.quantize_weights(cfg, rq.synth_weights(cfg), 4, 64)
    return cfg, w, rq.Qwen3Oracle(cfg, w, quant=(4, 64)), "bf16", 2.0 ** -7 * np.sqrt(2 * L)


_MODELS = {}


def _model(kind):
    """one resident model per kind, handed out reset and greedy"""
    from ominix_mlx_amd import engine
    if kind not in _MODELS:
        cfg, w, _, _, _ = _host(kind)
        if kind == "f16":
            m = engine.Model(dtype="float16", **_kw(cfg))
            m.load_weights({k: v.astype(np.float16) for k, v in w.items()})
        elif kind == "q4":
            m = engine.Model(quantization={"bits": 4, "group_size": 64}, **_kw(cfg))
            m.load_weights(w)
        else:
            m = engine.Model(**_kw(cfg))
            m.load_weights(w)
        _MODELS[kind] = m
    m = _MODELS[kind]
    m.set_sampler(0.0)
    m.reset()
    return m


def _ids(cfg):
    ids = synth.prompt_ids(N_PROMPT, cfg.vocab_size).astype(np.uint32)
    assert not (ids == PAD).any()
    return ids


def _run(m, ids, pre=None, n_new=8, **kw):
    """(first token, last_logits bits, the next n_new greedy tokens, offset) of one prompt on a reset model"""
    m.reset()
    if pre is not None:
        m.prefill(pre)
    first = m.prefill(ids, **kw)
    logits = m.last_logits().copy()
    rest = m.decode(n_new)
    return int(first), logits.view(np.uint32), rest.astype(np.uint32), m.offset()


def _padded(ids, a, b):
    out = ids.copy()
    out[a:b] = PAD
    return out


@pytest.mark.parametrize("cached", [0, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_own_rows_given_back_are_the_plain_prompt_pass(omx, kind, cached):
    """prefill(ids with PAD over [a, b), embeds=embed_tokens(ids[a:b]), embeds_at=a) IS prefill(ids): first token, logits bits, the next 8
    greedy tokens and offset() -- on an empty cache and on top of 5 cached tokens.  The PAD ids make the identity depend on the rows
    being taken from the caller: a pass that ignored them would gather PAD's row."""
    cfg = _host(kind)[0]
    m = _model(kind)
    ids = _ids(cfg)
    pre = synth.prompt_ids(40, cfg.vocab_size)[35:40] if cached else None
    want = _run(m, ids, pre)
    assert want[3] == cached + N_PROMPT + 8
    for a, b in SPANS:
        rows = m.embed_tokens(ids[a:b])
        got = _run(m, _padded(ids, a, b), pre, embeds=rows, embeds_at=a)
        assert got[0] == want[0] and got[3] == want[3], f"span [{a}, {b})"
        np.testing.assert_array_equal(got[1], want[1], err_msg=f"logits bits, span [{a}, {b})")
        np.testing.assert_array_equal(got[2], want[2], err_msg=f"greedy tokens, span [{a}, {b})")
    # and the PAD ids alone, without the rows, are another prompt (the identity above is not vacuous)
    other = _run(m, _padded(ids, 9, 17), pre)
    assert not np.array_equal(other[1], want[1])


def test_mixed_format_table_own_rows(omx):
    """A mixed-precision checkpoint (base 3-bit, an 8-bit embedding table, every kind of matrix in its own format): the same identity,
    and embed_tokens in the table's own format."""
    from ominix_mlx_amd import engine, ops
    cfg = _cfg("q4")
    base, table = mq.table_b(cfg)
    wm, _, _ = mq.checkpoints(cfg, base, table)
    m = engine.Model(quantization=mq.quantization(base, table), **_kw(cfg))
    m.load_weights(wm)
    ids = _ids(cfg)
    want = _run(m, ids)
    for a, b in [(0, 24), (9, 17)]:
        got = _run(m, _padded(ids, a, b), embeds=m.embed_tokens(ids[a:b]), embeds_at=a)
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
    T = ops.Tensor
    p = "model.embed_tokens."
    own = ops.dequantize(T.from_numpy(wm[p + "weight"][ids], "u32"), T.from_numpy(wm[p + "scales"][ids]), T.from_numpy(wm[p + "biases"][ids]),
                         64, 8).numpy()
    np.testing.assert_array_equal(m.embed_tokens(ids).numpy().view(np.uint32), own.view(np.uint32))
    m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_embed_tokens_bits(omx, kind):
    """bf16 / float16 table: the oracle's gather, bit for bit.  Packed table: the rows the device prompt pass makes for itself -- its
    launches (gather the triplet rows, omx_dequantize) driven from here."""
    from ominix_mlx_amd import ops
    cfg, w, oracle, dt, _ = _host(kind)
    m = _model(kind)
    ids = _ids(cfg)
    got = m.embed_tokens(ids)
    assert got.shape == (N_PROMPT, cfg.hidden_size) and got.dtype == (omx.FLOAT16 if kind == "f16" else omx.BFLOAT16)
    if kind == "q4":
        T = ops.Tensor
        p = "model.embed_tokens."
        own = ops.dequantize(T.from_numpy(w[p + "weight"][ids], "u32"), T.from_numpy(w[p + "scales"][ids]), T.from_numpy(w[p + "biases"][ids]), 64, 4)
        np.testing.assert_array_equal(got.numpy().view(np.uint32), own.numpy().view(np.uint32))
        # (the oracle's dequantise of the gathered rows is the same arithmetic in float64, rounded once: within one bf16 ulp)
        ref = rule.embed_rows(oracle, ids)
        assert np.abs(got.numpy() - ref).max() <= 2.0 ** -8 * np.abs(ref).max()
    else:
        np.testing.assert_array_equal(got.numpy().view(np.uint32), np.ascontiguousarray(w["model.embed_tokens.weight"][ids], dtype=np.float32).view(np.uint32))
    assert m.offset() == 0     # neither the cache nor the sampler is touched
    with pytest.raises(omx.OmxError, match="out of range"):
        m.embed_tokens([cfg.vocab_size])


@functools.lru_cache(maxsize=None)
def _random_rows(hidden):
    """rows at the embedding table's scale (std 0.02), float32 with all 24 mantissa bits in play"""
    return (0.02 * np.random.default_rng(20240607).standard_normal((14, hidden))).astype(np.float32)


@pytest.mark.parametrize("given", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
def test_arbitrary_rows_match_forward_from_rows(omx, kind, given):
    """Random rows over positions [10, 24) -- the last row included, which then goes through the end of the step from the row buffer --
    given as float32, bf16 and float16, against forward_from_rows on the oracle fed the given VALUES (the rule casts them to the
    activation dtype).  The check is test_greedy_decode_matches_oracle's (tests/test_gpu_qwen3.py), term for term: 12 greedy tokens,
    the bound from the largest reference logit of those 12 rows, the prompt's logits under it, tokens equal outside the near-tie
    guard, the last step's logits when nothing diverged.
    (The first version of this test took the bound from the prompt's row alone -- narrower than the cited test -- and missed it in one
    of nine cases, bf16 model with float16 rows: error 0.015625 = two bf16 ulps of a logit in [1, 2), bound 0.015537 at max|logit|
    1.406.  Measured beside it: the plain prompt pass of the same model sits at 0.013184 of 0.016745; the pass over the caller's rows
    is that pass bit for bit, test_own_rows_given_back_are_the_plain_prompt_pass.)"""
    from ominix_mlx_amd import ops
    cfg, _, oracle, dt, factor = _host(kind)
    m = _model(kind)
    ids = _ids(cfg)
    a, b, n_new = 10, 24, 12
    values = rc.rnd(_random_rows(cfg.hidden_size), given)            # what the caller's buffer holds, exactly
    h = np.array(rule.embed_rows(oracle, ids), dtype=np.float32)
    h[a:b] = values
    ref_tokens, ref_logits = rule.generate_from_rows(oracle, h, n_new)
    m.reset()
    first = m.prefill(_padded(ids, a, b), embeds=ops.Tensor.from_numpy(values, given), embeds_at=a)
    logits0 = m.last_logits()
    got = np.concatenate([[first], m.decode(n_new - 1)]).astype(np.uint32)
    assert m.offset() == N_PROMPT + n_new - 1
    err, bound = np.abs(logits0 - ref_logits[0]).max(), factor * np.abs(ref_logits).max()
    print(f"{kind} rows given as {given}: max |logit error| {err:.6f}, bound {bound:.6f}, max |logit| of the prompt's row {np.abs(ref_logits[0]).max():.4f}")
    assert err <= bound
    margins = rc.argmax_margin(ref_logits)
    for i in range(n_new):
        if got[i] != ref_tokens[i]:
            assert margins[i] <= 2 * bound, f"token {i}: got {got[i]} want {ref_tokens[i]} with margin {margins[i]:.4f} > {2*bound:.4f}"
            break
    else:
        assert np.abs(m.last_logits() - ref_logits[-1]).max() <= bound


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_float32_rows_round_to_nearest_even(omx, kind):
    """float32 rows lying between two values of the activation dtype -- exact ties, one float32 ulp either side of a tie, a quarter of
    the way -- land where round-to-nearest-even puts them: the pass over them is, bit for bit, the pass over the pre-rounded rows."""
    from ominix_mlx_amd import ops
    cfg, _, _, dt, _ = _host(kind)
    m = _model(kind)
    ids = _ids(cfg)
    a, b = 4, 20
    e = m.embed_tokens(ids[a:b]).numpy().astype(np.float32)
    half = 0x8000 if dt == "bf16" else 0x1000                        # half an ulp of the 16-bit format, in float32 bits
    deltas = np.array([half, half + 1, half - 1, half // 2], dtype=np.uint32)
    bits = e.view(np.uint32) + deltas[np.arange(e.size) % 4].reshape(e.shape)
    r32 = bits.view(np.float32)
    want_rows = rc.rnd(r32, dt)
    assert np.isfinite(r32).all()
    trunc = (bits & ~np.uint32(2 * half - 1)).view(np.float32)
    ties = (np.arange(e.size) % 4 == 0).reshape(e.shape)
    assert (want_rows[ties] == trunc[ties]).any() and (want_rows[ties] != trunc[ties]).any()   # ties go both ways: to even
    assert (want_rows != trunc).mean() > 0.3
    want = _run(m, _padded(ids, a, b), n_new=4, embeds=ops.Tensor.from_numpy(want_rows, dt), embeds_at=a)
    got = _run(m, _padded(ids, a, b), n_new=4, embeds=ops.Tensor.from_numpy(r32, "f32"), embeds_at=a)
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    # truncated rows are another prompt: the comparison above can tell the roundings apart
    cut = _run(m, _padded(ids, a, b), n_new=4, embeds=ops.Tensor.from_numpy(trunc, dt), embeds_at=a)
    assert not np.array_equal(cut[1], want[1])


def _raw_prefill_embeds(omx, m, ids, rows_ptr, dtype, first_row, n_rows):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    first = ctypes.c_uint32()
    omx.check(omx.lib.omx_qwen3_prefill_embeds(m._h, ids.ctypes.data_as(U32P), ids.size, rows_ptr, dtype, first_row, n_rows, ctypes.byref(first)))
    return first.value


def test_refusals_are_named(omx, monkeypatch):
    from ominix_mlx_amd import engine
    cfg = _host("bf16")[0]
    m = _model("bf16")
    ids = _ids(cfg)
    rows = m.embed_tokens(ids[:10])
    with pytest.raises(omx.OmxError, match="lie outside the prompt"):
        m.prefill(ids, embeds=rows, embeds_at=20)
    with pytest.raises(omx.OmxError, match="lie outside the prompt"):
        m.prefill(ids, embeds=rows, embeds_at=-1)
    with pytest.raises(omx.OmxError, match="n_rows -1 is negative"):
        _raw_prefill_embeds(omx, m, ids, rows.ptr, omx.BFLOAT16, 0, -1)
    with pytest.raises(omx.OmxError, match="null rows with n_rows 3"):
        _raw_prefill_embeds(omx, m, ids, None, omx.BFLOAT16, 0, 3)
    with pytest.raises(omx.OmxError, match="rows of dtype"):
        _raw_prefill_embeds(omx, m, ids, rows.ptr, omx.UINT32, 0, 3)
    with pytest.raises(omx.OmxError, match="ShapeMismatch"):
        m.prefill(ids, embeds=np.zeros((3, cfg.hidden_size + 8), np.float32))
    with pytest.raises(omx.OmxError, match="out of range"):          # the ids under the rows are still checked
        m.prefill(np.concatenate([[cfg.vocab_size], ids[1:]]), embeds=rows, embeds_at=0)
    # where omx_qwen3_prefill would go through the decode step, the rows are refused, never dropped
    with pytest.raises(omx.OmxError, match="InvalidConfig.*one-row prompt"):
        m.prefill(ids[:1], embeds=m.embed_tokens(ids[:1]))
    for switch in ("OMX_PREFILL_SERIAL", "OMX_PREFILL_TAIL_STEP"):
        monkeypatch.setenv(switch, "1")
        with pytest.raises(omx.OmxError, match=f"InvalidConfig.*{switch}=1"):
            m.prefill(ids, embeds=rows, embeds_at=0)
        monkeypatch.delenv(switch)
    assert m.offset() == 0                                           # a refused call appended nothing
    f = _model("f16")
    fcfg = _host("f16")[0]
    fids = _ids(fcfg)[:16]
    with pytest.raises(omx.OmxError, match="InvalidConfig.*float16 model.*16 rows or fewer"):
        f.prefill(fids, embeds=f.embed_tokens(fids[:4]), embeds_at=2)
    # sharded and sparse-MoE engines (refused before any weight is looked at)
    z = np.zeros((2, cfg.hidden_size), np.float32)
    tp = engine.Model(tp_rank=0, tp_size=2, **_kw(cfg))
    with pytest.raises(omx.OmxError, match="tensor-parallel"):
        tp.prefill(ids, embeds=z, embeds_at=3)
    with pytest.raises(omx.OmxError, match="tensor-parallel"):
        tp.embed_tokens(ids)
    tp.close()
    moe = engine.Model(num_experts=4, num_experts_per_tok=2, moe_intermediate_size=256, **_kw(cfg))
    with pytest.raises(omx.OmxError, match="sparse-MoE"):
        moe.prefill(ids, embeds=z, embeds_at=3)
    moe.close()


@pytest.mark.parametrize("kind", KINDS)
def test_no_rows_is_omx_qwen3_prefill(omx, kind):
    """n_rows = 0 through the new entry (rows NULL) is omx_qwen3_prefill bit for bit under a filtered sampler: tokens, logits, the
    sampler's key state and -- through the repetition penalty on the tokens that follow -- the penalty history.  A one-row prompt and
    the serial switch are accepted, as omx_qwen3_prefill accepts them."""
    cfg = _host(kind)[0]
    m = _model(kind)
    ids = _ids(cfg)

    def run(new_entry, prompt):
        m.reset()
        m.set_sampler(0.8, seed=11, top_k=40, top_p=0.95, repetition_penalty=1.3, presence_penalty=0.2)
        first = _raw_prefill_embeds(omx, m, prompt, None, omx.FLOAT32, 0, 0) if new_entry else m.prefill(prompt)
        logits = m.last_logits().view(np.uint32).copy()
        rest = m.decode(8)
        return int(first), logits, rest.astype(np.uint32), m.sampler_state(), m.offset()

    for prompt in (ids, ids[:1]):
        a, b = run(False, prompt), run(True, prompt)
        assert a[0] == b[0] and a[3] == b[3] and a[4] == b[4]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])
    m.set_sampler(0.0)
