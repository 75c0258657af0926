"""Batch.prefill(slot, prompt, embeds=, embeds_at=) -- omx_qwen3_batch_prefill_embeds, the span of omx_qwen3_prefill_embeds taken by the
batch's prompt pass -- on the tiny dense model of tests/test_gpu_batch_decode.py, bf16 and 4-bit, K/V slabs bf16 and kv_bits = 8.
The prompt is 19 tokens with a 7-row span at position 5.  Everything here is bit equality with the plain Batch.prefill."""
import functools

import numpy as np
import pytest

from oracle import synth
from test_gpu_quant_verify import _qmodel, _quantized
from test_gpu_speculative import TARGET, _engine

pytestmark = pytest.mark.gpu

N_PROMPT, A, B = 19, 5, 12
PAD = 7
KINDS = ("bf16", "q4")
_MODELS = {}


def _model(kind):
    if kind not in _MODELS:
        if kind == "bf16":
            m = _engine(TARGET, 256)
        else:
            m = _qmodel(TARGET, 4, 64, 256)
            m.load_weights(_quantized(TARGET, 4, 64)[0])
        _MODELS[kind] = m
    m = _MODELS[kind]
    m.set_sampler(0.0)
    m.reset()
    return m


@functools.lru_cache(maxsize=None)
def _ids():
    ids = synth.prompt_ids(N_PROMPT, TARGET.vocab_size).astype(np.uint32)
    other = ((synth.prompt_ids(40, TARGET.vocab_size)[20:20 + B - A].astype(np.int64) + 3) % TARGET.vocab_size).astype(np.uint32)
    assert not (ids == PAD).any() and not (other == PAD).any() and not np.array_equal(other, ids[A:B])
    return ids, other


def _padded(ids):
    out = ids.copy()
    out[A:B] = PAD
    return out


def _kv_bits(b, slot):
    """every cached row of the slot, every layer, as raw bits"""
    out = []
    for layer in range(TARGET.num_hidden_layers):
        k, v = b.kv_rows(slot, layer)
        for part in (k, v):
            out.extend(np.ascontiguousarray(a).view(np.uint32).copy() for a in (part if isinstance(part, tuple) else (part,)))
    return out


def _one(m, kv_bits, prompt, n_new=6, **kw):
    """(first token, K/V bits after the prompt, the next n_new greedy tokens) of slot 1 of a fresh 3-slot batch"""
    b = m.batch(3, 128, kv_bits=kv_bits)
    first = b.prefill(1, prompt, **kw)
    kv = _kv_bits(b, 1)
    rest = b.decode(n_new, [1]).reshape(-1).astype(np.uint32)
    b.close()
    return int(first), kv, rest


def _same(got, want, what):
    assert got[0] == want[0], what
    assert len(got[1]) == len(want[1])
    for g, w in zip(got[1], want[1]):
        np.testing.assert_array_equal(g, w, err_msg=f"K/V bits: {what}")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"greedy tokens: {what}")


@pytest.mark.parametrize("kv_bits", [0, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_own_rows_given_back_are_the_plain_batch_prefill(omx, kind, kv_bits):
    """rows = model.embed_tokens(ids[5:12]) over PAD ids, as the activation dtype and widened to float32: first token, the slot's
    kv_rows and the tokens that follow are the plain Batch.prefill's, bit for bit.  The PAD ids alone are another prompt."""
    from ominix_mlx_amd import ops
    m = _model(kind)
    ids, _ = _ids()
    want = _one(m, kv_bits, ids)
    rows = m.embed_tokens(ids[A:B])
    _same(_one(m, kv_bits, _padded(ids), embeds=rows, embeds_at=A), want, "bf16 rows")
    wide = ops.Tensor.from_numpy(rows.numpy().astype(np.float32), "f32")
    _same(_one(m, kv_bits, _padded(ids), embeds=wide, embeds_at=A), want, "float32 rows")
    _same(_one(m, kv_bits, _padded(ids), embeds=rows.numpy().astype(np.float32), embeds_at=A), want, "numpy float32 rows")
    pad_only = _one(m, kv_bits, _padded(ids))
    assert any(not np.array_equal(g, w) for g, w in zip(pad_only[1], want[1]))


@pytest.mark.parametrize("kv_bits", [0, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_other_rows_are_the_prompt_with_those_ids(omx, kind, kv_bits):
    m = _model(kind)
    ids, other = _ids()
    swapped = ids.copy()
    swapped[A:B] = other
    want = _one(m, kv_bits, swapped)
    _same(_one(m, kv_bits, _padded(ids), embeds=m.embed_tokens(other), embeds_at=A), want, "rows of other ids")
    plain = _one(m, kv_bits, ids)
    assert any(not np.array_equal(g, w) for g, w in zip(plain[1], want[1]))


@pytest.mark.parametrize("kind", KINDS)
def test_a_neighbour_does_not_change_the_slot(omx, kind):
    """slot 1 prefilled over caller rows and decoded alone, against the same beside a neighbour that was prefilled (plain, and over rows
    of its own) and decodes in the same steps"""
    m = _model(kind)
    ids, other = _ids()
    alone = _one(m, 0, _padded(ids), n_new=8, embeds=m.embed_tokens(ids[A:B]), embeds_at=A)
    b = m.batch(3, 128)
    b.prefill(0, synth.prompt_ids(33, TARGET.vocab_size).astype(np.uint32))
    first = b.prefill(1, _padded(ids), embeds=m.embed_tokens(ids[A:B]), embeds_at=A)
    b.prefill(2, _padded(ids), embeds=m.embed_tokens(other), embeds_at=A)
    toks = b.decode(8, [0, 1, 2]).astype(np.uint32)
    b.close()
    assert int(first) == alone[0]
    np.testing.assert_array_equal(toks[:, 1], alone[2])


def test_refusals_carry_over(omx):
    from ominix_mlx_amd import engine
    from test_gpu_prefill_embeds import _cfg, _kw
    m = _model("bf16")
    ids, _ = _ids()
    rows = m.embed_tokens(ids[A:B])
    b = m.batch(2, 128)
    with pytest.raises(omx.OmxError, match="InvalidConfig.*one-row prompt"):
        b.prefill(0, ids[:1], embeds=m.embed_tokens(ids[:1]))
    with pytest.raises(omx.OmxError, match="lie outside the prompt"):
        b.prefill(0, ids, embeds=rows, embeds_at=13)
    with pytest.raises(omx.OmxError, match="lie outside the prompt"):
        b.prefill(0, ids, embeds=rows, embeds_at=-1)
    with pytest.raises(omx.OmxError, match="ShapeMismatch"):
        b.prefill(0, ids, embeds=np.zeros((3, TARGET.hidden_size + 8), np.float32))
    with pytest.raises(omx.OmxError, match="out of range"):
        b.prefill(0, np.concatenate([[TARGET.vocab_size], ids[1:]]), embeds=rows, embeds_at=A)
    assert b.offset(0) == 0                                          # a refused call appended nothing
    b.close()
    # the few-row packed route of a packed model cannot take rows
    q = _model("q4")
    bq = q.batch(2, 128)
    with pytest.raises(omx.OmxError, match="InvalidConfig.*few-row packed"):
        bq.prefill(0, ids[:8], embeds=q.embed_tokens(ids[2:5]), embeds_at=2)
    assert bq.offset(0) == 0
    bq.close()
    cfg = _cfg("bf16")
    moe = engine.Model(num_experts=4, num_experts_per_tok=2, moe_intermediate_size=256, **_kw(cfg))
    with pytest.raises(omx.OmxError, match="MoE"):                   # (a sparse-MoE model has no batch at all: refused at create)
        moe.batch(2, 64)
    moe.close()
