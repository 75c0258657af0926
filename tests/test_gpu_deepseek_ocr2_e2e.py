"""GPU: DeepSeek-OCR-2 image to text -- deepseek_ocr2.DeepseekOCR2.ocr(): encode_image -> the rows over the prompt's image span -> the
prompt pass over caller rows -> decode, at the tiny tower widths of tests/test_gpu_deepencoder.py (a 1024 px view: 256 rows + the
separator) and the tiny decoder of tests/test_gpu_deepseek_engine.py.  The decoder is held to the rule of tests/deepseek_moe_rule.py fed
the DEVICE's image rows (the towers have their own tests), at the engine bound: |logits - ref| <= 2^-7 * max|ref| * sqrt(layers) * 2,
tokens under the margin rule."""
import functools

import numpy as np
import pytest

import deepencoder_rule as vr
import deepseek_moe_rule as dr
from oracle import ref_core as rc

pytestmark = pytest.mark.gpu
LLM = dict(hidden_size=256, num_hidden_layers=3, intermediate_size=448, num_attention_heads=2, num_key_value_heads=2, head_dim=128,
           vocab_size=1024, rms_norm_eps=1e-6, rope_theta=10000.0, qk_norm=False, num_experts=16, num_experts_per_tok=6,
           moe_intermediate_size=192, moe_mode="deepseek", norm_topk_prob=True, first_k_dense_replace=1, n_shared_experts=2,
           routed_scaling_factor=1.0)
IMAGE_ID, SEED = 1023, 0x0C0FFEE5


class Chars:
    """one id per character, inside the tiny vocabulary and clear of BOS / EOS / the placeholder"""
    def encode(self, text, add_special_tokens=False):
        return [2 + (ord(ch) * 7) % 1000 for ch in text]


@functools.lru_cache(maxsize=None)
def _weights(peaked=False):
    w = dict(vr.synth_weights(vr.TINY_SAM, vr.TINY_VCF, seed=51, neck=vr.TINY_NECK, out_dim=LLM["hidden_size"]))
    cfg = dr.tiny_decoder_config()
    w.update(dr.decoder_weights(cfg, 1, 2, SEED))
    return w, cfg


def _model(w):
    from ominix_mlx_amd import deepseek_ocr2
    m = deepseek_ocr2.DeepseekOCR2.from_weights(w, LLM, vr.TINY_SAM, vr.TINY_VCF, tokenizer=Chars(), max_context=512)
    m.image_token_id = IMAGE_ID
    return m


def test_ocr_against_the_rule_fed_the_device_rows(omx):
    from ominix_mlx_amd import deepseek_ocr2 as d
    w, cfg = _weights()
    view = vr.synth_images(1, 1024, 52)[0]
    m = _model(w)
    prompt, n_new = "<image>\nFree OCR.", 6
    got = m.ocr(view, None, prompt, max_tokens=n_new)
    logits0 = None
    # the same call by hand, to read the prompt's logits
    ids, mask = d.tokenize_prompt(Chars(), prompt, True, 1024, 0, (1, 1), IMAGE_ID)
    rows = m.encoder.encode_image(view)
    assert rows.shape == (257, 256) and d.image_span(mask) == (1 + len("<|User|>: "), 257)
    again = m.generate_ids(ids, mask, rows, max_tokens=1)
    logits0 = m.llm.last_logits()
    assert again[0] == got[0]
    # the rule: the device's rows (rounded to bf16 as the prompt pass takes them) as extra rows of the embedding table
    table = np.concatenate([w["model.embed_tokens.weight"], rc.bf16_round(rows.numpy())])
    at, n = d.image_span(mask)
    ref_ids = np.array(ids, np.int64)
    ref_ids[at:at + n] = LLM["vocab_size"] + np.arange(n)
    o = dr.make_oracle(cfg, dict(w, **{"model.embed_tokens.weight": table}), 1, 2, 1.0)
    ref_tokens, ref_logits = o.generate(ref_ids, n_new, return_logits=True)
    bound = 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(3) * 2
    print(f"e2e: {len(ids)} prompt positions, prompt logits off by {np.abs(logits0 - ref_logits[0]).max():.4e}, bound {bound:.4e}")
    assert np.abs(logits0 - ref_logits[0]).max() <= bound
    margins = rc.argmax_margin(ref_logits)
    assert len(got) <= n_new
    for i, t in enumerate(got):
        if t != ref_tokens[i]:
            assert margins[i] <= 2 * bound, f"token {i}: got {t} want {ref_tokens[i]} with margin {margins[i]:.4f}"
            break
    m.close()


def test_generation_stops_on_eos_and_on_a_repeating_ngram(omx):
    """peaked weights (oracle/ref_qwen3.py synth_weights(peaked=True)): the greedy successor of token t is t - 1, so a text prompt ending
    in token 5 counts 4, 3, 2, 1 and stops AFTER the EOS (1), which is returned; with a head that maps every token of a 4-cycle to the
    next one, generation stops by is_repeating() once the cycle stood three times, before max_tokens"""
    from oracle import synth
    from ominix_mlx_amd import deepseek_ocr2 as d
    w, cfg = _weights()
    shape = w["model.embed_tokens.weight"].shape
    table = synth.tensor("model.embed_tokens.weight", shape, 64.0, 0.0, "bf16")
    head = synth.tensor("model.embed_tokens.weight", shape, 0.02, 0.0, "bf16")
    peaked = dict(w, **{"model.embed_tokens.weight": table, "lm_head.weight": np.roll(head, -1, axis=0)})
    m = _model(peaked)
    out = m.generate_ids([0, 9, 8, 7, 6, 5], max_tokens=40)
    assert out == [4, 3, 2, 1]
    m.close()
    cyc = head.copy()                       # successor of 10 is 11, of 11 is 12, of 12 is 13, of 13 is 10
    lm = np.roll(head, -1, axis=0)
    for a, b in ((10, 11), (11, 12), (12, 13), (13, 10)):
        lm[b] = head[a]
    lm[9], lm[12 + 2] = head[200], head[201]     # the rows that pointed INTO the cycle the counting-down way now point elsewhere
    m = _model(dict(peaked, **{"lm_head.weight": lm}))
    out = m.generate_ids([0, 20, 10], max_tokens=40)
    assert d.is_repeating(out) and len(out) == 12 and out[:4] == [11, 12, 13, 10]
    m.close()
