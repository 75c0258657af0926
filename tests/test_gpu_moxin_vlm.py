"""Moxin-VLM end to end on the device (ominix_mlx_amd/moxin_vlm.py): tiny towers -> projector -> the visual rows over the placeholder span
behind BOS -> Model.prefill(embeds=, embeds_at=1) on a tiny Mistral-wired decoder (no q/k norm, no bias, theta 1e4, eps 1e-5) -> decode.
The decoder stage is held to qwen3_asr_rule.forward_from_rows fed THE DEVICE'S OWN rows on the bound of tests/test_gpu_qwen3.py
(2^-7 max|logit| sqrt(layers), sqrt(2 layers) for the packed model); the rows are held to tests/vit_rule.py on the float32 rule (1e-4)."""
import numpy as np
import pytest

import qwen3_asr_rule as asr_rule
import vit_rule as rule

pytestmark = pytest.mark.gpu

TOL = 1e-4
HIDDEN = 512
PROJ = (272, 544, HIDDEN, HIDDEN)


def _ratio(got, ref, what):
    r = np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max()
    print(f"{what}: worst error / largest magnitude = {r:.3e}")
    return r


def _vision():
    from ominix_mlx_amd import vision
    dw, sw, pw = rule.synth_weights(rule.TINY_DINO, seed=1), rule.synth_weights(rule.TINY_SIGLIP, seed=2), rule.projector_synth_weights(PROJ, seed=3)
    dino, siglip, proj = vision.ViTEncoder(**rule.TINY_DINO), vision.ViTEncoder(**rule.TINY_SIGLIP), vision.Projector()
    dino.load_weights(dw)
    siglip.load_weights(sw)
    proj.load_weights(pw)
    return (dino, siglip, proj), (dw, sw, pw)


def _text(kind, synth=False):
    from ominix_mlx_amd import engine
    from oracle import ref_qwen3 as rq
    tcfg = rq.Qwen3Config(HIDDEN, 2, 1536, 8, 4, 64, 2048, 1e-5, 1e4, False, qk_norm=False)
    kw = dict(hidden_size=HIDDEN, num_hidden_layers=2, intermediate_size=1536, num_attention_heads=8, num_key_value_heads=4, head_dim=64,
              vocab_size=2048, rms_norm_eps=1e-5, rope_theta=1e4, tie_word_embeddings=False, qk_norm=False, attention_bias=False, max_context=256)
    m = engine.Model(quantization={"bits": 4, "group_size": 64}, **kw) if kind == "q4" else engine.Model(**kw)
    if synth:
        m.synth_weights()
        return m, None, None
    w = rq.synth_weights(tcfg)
    L = tcfg.num_hidden_layers
    if kind == "q4":
        w = rq.quantize_weights(tcfg, w, 4, 64)
        oracle, factor = rq.Qwen3Oracle(tcfg, w, quant=(4, 64)), 2.0 ** -7 * np.sqrt(2 * L)
    else:
        oracle, factor = rq.Qwen3Oracle(tcfg, w), 2.0 ** -7 * np.sqrt(L)
    m.load_weights(w)
    return m, oracle, factor


class FakeTokenizer:
    """BOS id 1 when asked for special tokens, every character one id"""

    def __init__(self, bos=True):
        self.bos = bos

    def encode(self, text, add_special_tokens=True):
        return ([1] if add_special_tokens and self.bos else []) + [10 + ord(c) % 1000 for c in text]

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(t)) for t in ids)


@pytest.mark.parametrize("kind", ["bf16", "q4"])
def test_visual_rows_through_the_prompt_pass(omx, kind):
    from ominix_mlx_amd import moxin_vlm
    from oracle import ref_core as rc
    (dino, siglip, proj), (dw, sw, pw) = _vision()
    m, oracle, factor = _text(kind)
    vlm = moxin_vlm.MoxinVLM(m, dino, siglip, proj, FakeTokenizer(), image_token_id=1999)
    img = rule.synth_image(56, 5)
    rows = vlm.visual_rows(img)
    P = rows.shape[0]
    assert rows.shape == (16, HIDDEN)
    assert _ratio(rows.numpy(), rule.visual_rows(img, dw, rule.TINY_DINO, sw, rule.TINY_SIGLIP, pw), "visual rows") <= TOL

    ids = vlm.prompt_ids("what is this")
    assert ids[0] == 1 and (ids[1:1 + P] == 1999).all() and ids.size == 1 + P + len("In: what is this\nOut:")
    n_new = 12
    m.reset()
    first = m.prefill(ids, embeds=rows, embeds_at=1)
    logits0 = m.last_logits()
    got = np.concatenate([[first], m.decode(n_new - 1)]).astype(np.uint32)
    assert m.offset() == ids.size + n_new - 1
    h = np.array(asr_rule.embed_rows(oracle, ids), dtype=np.float32)
    h[1:1 + P] = rows.numpy()
    ref_tokens, ref_logits = asr_rule.generate_from_rows(oracle, h, n_new)
    err, bound = np.abs(logits0 - ref_logits[0]).max(), factor * np.abs(ref_logits).max()
    print(f"{kind}: prompt logits max error {err:.6f}, bound {bound:.6f}")
    assert err <= bound
    margins = rc.argmax_margin(ref_logits)
    for i in range(n_new):
        if got[i] != ref_tokens[i]:
            assert margins[i] <= 2 * bound, f"token {i}: got {got[i]} want {ref_tokens[i]} with margin {margins[i]:.4f}"
            break
    vlm.close()


@pytest.mark.parametrize("kind", ["bf16", "q4"])
def test_generate_ids_is_the_stages_by_hand(omx, kind):
    """MoxinVLM.generate_ids / describe give the ids of the stages done by hand (towers into one buffer, projector, the prompt's ids,
    Model.prefill(embeds=, embeds_at=1), decode, the EOS rule of examples/generate.rs: the EOS id ends the stream and is not emitted).  A
    prompt whose placeholder span is not the towers' row count raises."""
    from ominix_mlx_amd import moxin_vlm, ops
    (dino, siglip, proj), _ = _vision()
    m, _, _ = _text(kind, synth=True)
    tok = FakeTokenizer()
    img = rule.synth_image(56, 6)
    n_new = 12

    fused = ops.Tensor((16, 272), "f32")
    dino.forward(img, out=fused, column=0)
    siglip.forward(img, out=fused, column=128)
    rows = proj.forward(fused)
    body = tok.encode("In: look\nOut:", add_special_tokens=True)
    ids = np.asarray(body[:1] + [1999] * 16 + body[1:], np.uint32)
    m.reset()
    first = m.prefill(ids, embeds=rows, embeds_at=1)
    stream = [int(first)] + [int(t) for t in m.decode(n_new + 4)]
    eos = stream[5]                                                  # an id the greedy stream does reach: the loop must stop there
    hand = stream[:stream.index(eos)]
    assert len(hand) <= 5

    vlm = moxin_vlm.MoxinVLM(m, dino, siglip, proj, tok, image_token_id=1999, eos_id=eos)
    assert vlm.generate_ids(img, "look", max_tokens=n_new, chunk=4) == hand
    assert vlm.describe(img, "look", max_tokens=n_new) == " ".join(str(t) for t in hand)
    t = vlm.last_times
    assert t["prompt_rows"] == ids.size and t["tokens"] == len(hand) and t["launches"] == dino.launches() + siglip.launches() + 3
    assert all(k in t for k in ("towers_ms", "projector_ms", "prompt_pass_ms", "per_token_ms"))
    vlm.eos_id = 2047                                                # without an EOS in reach: max_tokens ids, the by-hand stream's
    assert vlm.generate_ids(img, "look", max_tokens=n_new) == stream[:n_new]

    class Doubled(FakeTokenizer):                                    # a tokenizer that itself emits a placeholder id
        def encode(self, text, add_special_tokens=True):
            return super().encode(text, add_special_tokens) + [1999]

    short = moxin_vlm.MoxinVLM(m, dino, siglip, proj, Doubled(), image_token_id=1999, eos_id=eos)
    with pytest.raises(omx.OmxError, match="holds 17 placeholder ids but the towers made 16 rows"):
        short.generate_ids(img, "look")
    with pytest.raises(omx.OmxError, match="placeholder id 4000 outside the vocabulary"):
        moxin_vlm.MoxinVLM(m, dino, siglip, proj, tok, image_token_id=4000)
    vlm.close()


def test_quantize_packs_the_decoder_for_the_engine(omx):
    """MoxinVLM.load(quantize=4)'s packing step (moxin_vlm.quantize_text_weights, the device's mlx quantize): the same tensors, shapes and
    dtypes an MLX-quantized checkpoint of the model holds (embedding included, norms untouched); the engine loads them and its prompt
    logits are held to the oracle ON THOSE TRIPLETS with the packed model's bound (tests/test_gpu_qwen3.py: 2^-7 max|logit| sqrt(2 layers))."""
    from ominix_mlx_amd import engine, moxin_vlm
    from oracle import ref_qwen3 as rq, synth
    tcfg = rq.Qwen3Config(HIDDEN, 2, 1536, 8, 4, 64, 2048, 1e-5, 1e4, False, qk_norm=False)
    w = rq.synth_weights(tcfg)
    wq = moxin_vlm.quantize_text_weights(w, 4, 64)
    want = rq.quantize_weights(tcfg, w, 4, 64)
    assert sorted(wq) == sorted(want)
    for k, v in want.items():
        assert wq[k].shape == v.shape and (wq[k].dtype == np.uint32) == (v.dtype == np.uint32), k
    np.testing.assert_array_equal(wq["model.norm.weight"], w["model.norm.weight"])
    m, _, _ = _text("q4", synth=True)
    m.load_weights(wq)
    ids = synth.prompt_ids(24, tcfg.vocab_size)
    m.prefill(ids)
    _, ref_logits = rq.Qwen3Oracle(tcfg, wq, quant=(4, 64)).generate(ids, 1, return_logits=True)
    err, bound = np.abs(m.last_logits() - ref_logits[0]).max(), 2.0 ** -7 * np.sqrt(2 * 2) * np.abs(ref_logits).max()
    print(f"device-quantised decoder: prompt logits max error {err:.6f}, bound {bound:.6f}")
    assert err <= bound
    m.close()
