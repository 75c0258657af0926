"""The 8-bit K/V cache rule of a kv_bits = 8 batch (include/omx.h, omx_qwen3_batch_create_kv) restated on the oracle, shared by
tests/test_kv_quant_rule.py (CPU) and tests/test_gpu_batch_kv8.py (GPU): every K row (after q/k norm and RoPE) and V row is stored as
MLX affine codes -- rc.quantize(x, 64, 8) on the bf16 row, scales and biases rounded to bf16 -- and every attention reads
code * scale + bias.  KV8Cache is rc.KVCache with that round trip on the way in; Qwen3Oracle.generate takes a list of them as it is."""
import functools

import numpy as np

from oracle import ref_core as rc, ref_qwen3 as rq

GROUP, BITS = 64, 8


def kv8_triplet(x):
    """(codes uint32 [..., D / 4], scales, biases float32 on the bf16 grid [..., D / 64]) of rows x [..., D]"""
    q, s, b = rc.quantize(x, GROUP, BITS)
    return q, rc.bf16_round(s), rc.bf16_round(b)


def kv8_round_trip(x) -> np.ndarray:
    """what a kv8 cache returns for the rows x it was handed: float32, not rounded to bf16"""
    return rc.dequantize(*kv8_triplet(x), GROUP, BITS, "f32").astype(np.float32)


def dequantize64(q, s, b) -> np.ndarray:
    """float64 code * scale + bias of a triplet (scales / biases as stored: bf16 values)"""
    q = np.asarray(q, dtype=np.uint32)
    codes = ((q[..., None] >> (np.arange(4, dtype=np.uint32) * np.uint32(8))) & np.uint32(0xFF)).reshape(*q.shape[:-1], -1)
    sc = np.repeat(np.asarray(s, dtype=np.float64), GROUP, axis=-1)
    bi = np.repeat(np.asarray(b, dtype=np.float64), GROUP, axis=-1)
    return codes.astype(np.float64) * sc + bi


class KV8Cache(rc.KVCache):
    """rc.KVCache whose rows pass through the 8-bit round trip as they are appended: stored and returned dequantised (float32)."""

    def update_and_fetch(self, keys, values):
        return super().update_and_fetch(kv8_round_trip(keys), kv8_round_trip(values))


def kv8_caches(cfg):
    return [KV8Cache() for _ in range(cfg.num_hidden_layers)]


# ---- the teacher-forced protocol of test_gpu_batch_decode on the kv8 oracle: references computed once per variant and shared ----

PROMPT_LENS = [5, 33, 64, 130, 250, 17, 96, 200]      # test_gpu_batch_decode.PROMPT_LENS
N_POS = 12


def prompt(n, V, shift=None):
    """test_gpu_batch_decode._prompt"""
    from oracle import synth
    return ((synth.prompt_ids(n, V).astype(np.int64) + (n if shift is None else shift)) % V).astype(np.uint32)


def bound(cfg, ref_logits):
    """test_gpu_batch_decode._bound"""
    return 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(cfg.num_hidden_layers)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """(cfg, oracle, checkpoint or None) of a variant of test_gpu_batch_decode.VARIANTS, without a device"""
    from test_gpu_batch_decode import VARIANTS
    cfg, quant = VARIANTS[name]
    if quant is None:
        return cfg, rq.Qwen3Oracle(cfg, rq.synth_weights(cfg)), None
    w = rq.quantize_weights(cfg, rq.synth_weights(cfg), *quant)
    return cfg, rq.Qwen3Oracle(cfg, w, quant=quant), w


@functools.lru_cache(maxsize=None)
def kv8_refs(name):
    """[(tokens, logits)] of the kv8 oracle for the eight prompts of PROMPT_LENS, N_POS positions each.  Read-only."""
    cfg, oracle, _ = oracle_of(name)
    out = []
    for n in PROMPT_LENS:
        toks, logits = oracle.generate(prompt(n, cfg.vocab_size), N_POS, caches=kv8_caches(cfg), return_logits=True)
        toks, logits = np.asarray(toks), np.asarray(logits)
        toks.setflags(write=False); logits.setflags(write=False)
        out.append((toks, logits))
    return tuple(out)


def near_ties(name):
    """positions of kv8_refs(name) whose top-1 / top-2 margin is within 2 x bound: where a token may legitimately differ"""
    cfg = oracle_of(name)[0]
    return sum(int((rc.argmax_margin(logits) <= 2 * bound(cfg, logits)).sum()) for _, logits in kv8_refs(name))
