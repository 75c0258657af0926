"""The Qwen3-ASR audio tower on the device (csrc/audio_encoder.hip; audio.AudioEncoder, audio.window_attention_f32) against its
numpy float64 restatement (tests/qwen3_asr_rule.py, written from qwen3-asr-mlx/src/encoder.rs).

Tolerance: the form tests/test_gpu_paraformer.py uses for the float32 path -- error <= 1e-4 x the largest magnitude of the float64
result (TOL["f32"] there) -- at every stage.  Each test prints its measured worst ratio (error / largest magnitude)."""
import functools

import numpy as np
import pytest

import qwen3_asr_rule as rule

pytestmark = pytest.mark.gpu

TOL = 1e-4

TINY = dict(num_mel_bins=16, downsample_hidden_size=32, d_model=128, encoder_attention_heads=2, encoder_ffn_dim=256, encoder_layers=2,
            output_dim=128, n_window=50, n_window_infer=200, max_source_positions=1500)


def _ratio(got, ref, what):
    r = np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max()
    print(f"{what}: worst error / largest magnitude = {r:.3e}")
    return r


def _mel(n_mels, F, seed):
    """a mel in the range the Whisper frontend writes ((log10 power + 4) / 4: roughly [-1, 2])"""
    return (0.5 + 0.6 * np.random.default_rng(seed).standard_normal((n_mels, F))).astype(np.float32)


def _encoder(cfg, w):
    from ominix_mlx_amd import audio
    e = audio.AudioEncoder(**cfg)
    e.load_weights(w)
    return e


@pytest.mark.parametrize("heads,window,sizes", [(16, 104, (1, 7, 13, 104, 105, 117, 208, 215)), (2, 26, (5, 26, 33, 52))])
def test_window_attention_against_the_explicit_forms(omx, heads, window, sizes):
    """The attention kernel alone: a window of one row, a last window shorter than a query tile, N an exact multiple of the window and one
    past it; q | k | v read in place from a stacked projection whose rows are longer than 3 * d_model.  Against the rule's per-window
    form and against the reference's form, full attention under the -1e9 additive mask, both in float64."""
    from ominix_mlx_amd import audio, ops
    d = heads * 64
    ld = 3 * d + 8
    for n in sizes:
        g = np.random.default_rng(1000 * heads + n)
        qkv = g.standard_normal((n, ld)).astype(np.float32)
        qkv[:, :d] *= 0.125                                        # q arrives scaled by head_dim^-0.5, the kernel's scale is 1
        q, k, v = (qkv[:, i * d:(i + 1) * d].astype(np.float64) for i in range(3))
        got = audio.window_attention_f32(ops.Tensor.from_numpy(qkv, "f32"), heads, window).numpy()
        ref = rule.window_attention(q, k, v, heads, window)
        masked = rule.masked_attention(q, k, v, heads, rule.block_mask(n, rule.window_boundaries(n, window)))
        assert np.abs(ref - masked).max() <= 1e-12
        assert _ratio(got, ref, f"window attention heads {heads} window {window} N {n}") <= TOL
        assert _ratio(got, masked, "  ... against the masked full form") <= TOL


@functools.lru_cache(maxsize=None)
def _real_width_stem():
    """the stem at the real widths with no transformer layer: weights, and the rule's stages for F = 150 (one full chunk, one padded 50)"""
    cfg = dict(num_mel_bins=128, downsample_hidden_size=480, d_model=1024, encoder_attention_heads=16, encoder_ffn_dim=4096,
               encoder_layers=0, output_dim=64, n_window=50, n_window_infer=800, max_source_positions=1500)
    w = rule.tower_synth_weights(cfg, seed=5)
    return cfg, w


@pytest.mark.parametrize("F", [150, 37])
def test_stem_at_the_real_width(omx, F):
    """n_mels 128, ds 480: F = 150 is one full chunk and one of 50 frames padded to 100 (the padded frames go through bias and GELU and
    reach valid outputs near the edge); F = 37 a single chunk whose padding target is 37.  Every layer's output, the assembled rows
    and the tail."""
    cfg, w = _real_width_stem()
    mel = _mel(128, F, F)
    st = rule.tower(mel, w, cfg)
    e = _encoder(cfg, w)
    out = e.forward(mel).numpy()
    assert e.tokens(F) == st["rows"].shape[0] == out.shape[0]
    for name in ("x1", "x2", "x3"):
        assert _ratio(e.debug_read(name, st[name].shape), st[name], f"stem F {F} {name}") <= TOL
    assert _ratio(e.debug_read("h", st["rows"].shape), st["rows"], f"stem F {F} assembled rows") <= TOL
    assert _ratio(out, st["out"], f"stem F {F} tail") <= TOL
    e.close()


def test_one_layer_at_the_real_width(omx):
    """d_model 1024, 16 heads, FFN 4096 at N = 117 (a window of 104 and one of 13): LayerNorms, the stacked q | k | v, the windowed
    attention, GELU and both residuals of one layer.  A narrow stem (n_mels 16, ds 32) carries the rows in: F = 900."""
    cfg = dict(num_mel_bins=16, downsample_hidden_size=32, d_model=1024, encoder_attention_heads=16, encoder_ffn_dim=4096,
               encoder_layers=1, output_dim=64, n_window=50, n_window_infer=800, max_source_positions=1500)
    w = rule.tower_synth_weights(cfg, seed=9)
    mel = _mel(16, 900, 900)
    st = rule.tower(mel, w, cfg)
    assert st["rows"].shape[0] == 117
    e = _encoder(cfg, w)
    out = e.forward(mel).numpy()
    h = rule.encoder_layer(st["rows"], w, "layers.0.", 16, 104)
    assert _ratio(e.debug_read("h", h.shape), h, "one real-width layer, hidden rows") <= TOL
    assert _ratio(out, st["out"], "one real-width layer, tail") <= TOL
    e.close()


@functools.lru_cache(maxsize=None)
def _tiny():
    return rule.tower_synth_weights(TINY, seed=1)


@pytest.mark.parametrize("F", [37, 100, 201, 250, 400])
def test_tiny_tower_end_to_end(omx, F):
    """F = 201 leaves a remainder chunk of one frame, F = 400 no remainder window; row counts equal the rule's."""
    w = _tiny()
    mel = _mel(16, F, F)
    st = rule.tower(mel, w, TINY)
    e = _encoder(TINY, w)
    assert e.tokens(F) == st["out"].shape[0] == rule.feat_extract_output_lengths(F)
    out = e.forward(mel).numpy()
    assert out.shape == st["out"].shape
    assert _ratio(out, st["out"], f"tiny tower F {F}") <= TOL
    e.close()


def test_one_handle_reused(omx):
    """F = 250, 37, 400, 250 through one handle: each result is a fresh handle's, bit for bit (the scratch grows per role and is reused)."""
    w = _tiny()
    one = _encoder(TINY, w)
    for F in (250, 37, 400, 250):
        mel = _mel(16, F, F)
        fresh = _encoder(TINY, w)
        np.testing.assert_array_equal(one.forward(mel).numpy().view(np.uint32), fresh.forward(mel).numpy().view(np.uint32))
        fresh.close()
    one.close()


def test_refusals_are_named(omx):
    from ominix_mlx_amd import audio
    with pytest.raises(omx.OmxError, match="InvalidConfig.*head width 32"):
        audio.AudioEncoder(**dict(TINY, encoder_attention_heads=4))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*multiple of 64"):
        audio.AudioEncoder(**dict(TINY, d_model=96))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*n_window_infer 250 must be a multiple of the chunk"):
        audio.AudioEncoder(**dict(TINY, n_window_infer=250))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*max_source_positions"):
        audio.AudioEncoder(**dict(TINY, max_source_positions=8))
    e = _encoder(TINY, _tiny())
    mel = _mel(16, 120, 3)
    mel[5, 77] = np.nan
    with pytest.raises(omx.OmxError, match="mel holds a NaN"):
        e.forward(mel)
    with pytest.raises(omx.OmxError, match="ShapeMismatch"):
        e.forward(_mel(17, 120, 3))
    e.close()
    bare = audio.AudioEncoder(**TINY)
    with pytest.raises(omx.OmxError, match="WeightNotFound: audio_tower.conv2d1.weight"):
        bare.forward(_mel(16, 120, 3))
    bare.close()


@pytest.mark.parametrize("kind", ["bf16", "q4"])
def test_audio_rows_through_the_prompt_pass(omx, kind):
    """The stages of a transcription chained on the device: 2.5 s of seeded noise -> audio.WhisperMelFrontend -> the tower -> its float32
    rows over the <|audio_pad|> span of a prompt (Model.prefill(embeds=, embeds_at=)) -> decode.  The prompt's logits are held to
    forward_from_rows fed THE DEVICE'S OWN audio rows, so the decoder stage is judged on its own bound (tests/test_gpu_qwen3.py:
    2^-7 max|logit| sqrt(layers), sqrt(2 layers) for the packed model) and the tower's float32 error is not counted twice; the tower's
    rows are held to the rule separately."""
    from ominix_mlx_amd import audio, engine
    from oracle import ref_core as rc, ref_qwen3 as rq, synth
    tcfg = rq.Qwen3Config(512, 2, 1536, 8, 4, 64, 2048, 1e-6, 1e6, True)
    acfg = dict(TINY, num_mel_bins=128, output_dim=tcfg.hidden_size)
    aw = rule.tower_synth_weights(acfg, seed=4)
    samples = (0.1 * np.random.default_rng(77).standard_normal(40000)).astype(np.float32)
    mel = audio.WhisperMelFrontend(n_mels=128).compute_mel_spectrogram(samples)
    F = mel.shape[1]
    enc = _encoder(acfg, aw)
    rows = enc.forward(mel)
    N = enc.tokens(F)
    assert rows.shape == (N, tcfg.hidden_size) and N == rule.feat_extract_output_lengths(F)
    ref_rows = rule.tower(mel.numpy(), aw, acfg)["out"]
    assert _ratio(rows.numpy(), ref_rows, f"tower on a device mel, F {F}") <= TOL

    w = rq.synth_weights(tcfg)
    L = tcfg.num_hidden_layers
    kw = dict(hidden_size=tcfg.hidden_size, num_hidden_layers=L, intermediate_size=tcfg.intermediate_size,
              num_attention_heads=tcfg.num_attention_heads, num_key_value_heads=tcfg.num_key_value_heads, head_dim=tcfg.head_dim,
              vocab_size=tcfg.vocab_size, tie_word_embeddings=True, max_context=256)
    if kind == "q4":
        w = rq.quantize_weights(tcfg, w, 4, 64)
        oracle, factor = rq.Qwen3Oracle(tcfg, w, quant=(4, 64)), 2.0 ** -7 * np.sqrt(2 * L)
        m = engine.Model(quantization={"bits": 4, "group_size": 64}, **kw)
    else:
        oracle, factor = rq.Qwen3Oracle(tcfg, w), 2.0 ** -7 * np.sqrt(L)
        m = engine.Model(**kw)
    m.load_weights(w)
    pad, head, tail = 1999, synth.prompt_ids(9, tcfg.vocab_size), synth.prompt_ids(16, tcfg.vocab_size)[9:]
    ids = np.concatenate([head, np.full(N, pad), tail]).astype(np.uint32)
    n_new = 12
    first = m.prefill(ids, embeds=rows, embeds_at=len(head))
    logits0 = m.last_logits()
    got = np.concatenate([[first], m.decode(n_new - 1)]).astype(np.uint32)
    assert m.offset() == ids.size + n_new - 1
    h = np.array(rule.embed_rows(oracle, ids), dtype=np.float32)
    h[len(head):len(head) + N] = rows.numpy()
    ref_tokens, ref_logits = rule.generate_from_rows(oracle, h, n_new)
    err, bound = np.abs(logits0 - ref_logits[0]).max(), factor * np.abs(ref_logits).max()
    print(f"{kind}: prompt logits max error {err:.6f}, bound {bound:.6f}")
    assert err <= bound
    margins = rc.argmax_margin(ref_logits)
    for i in range(n_new):
        if got[i] != ref_tokens[i]:
            assert margins[i] <= 2 * bound, f"token {i}: got {got[i]} want {ref_tokens[i]} with margin {margins[i]:.4f}"
            break
    with pytest.raises(omx.OmxError, match="lie outside the prompt"):
        m.reset()
        m.prefill(ids[:len(head) + 3], embeds=rows, embeds_at=len(head))
    m.close()
    enc.close()


class FakeTokenizer:
    """the template's special tokens as single ids, every other character as one id -- enough of a tokenizer for ids in, ids out"""
    SPECIAL = {"<|im_start|>": 1990, "<|im_end|>": 1991, "<|audio_start|>": 1992, "<|audio_end|>": 1993, "<asr_text>": 1994, "<|audio_pad|>": 1999}

    def __init__(self, drop_pads=0):
        self.drop_pads = drop_pads

    def encode(self, text, add_special_tokens=True):
        import re
        ids = []
        for part in re.split(r"(<\|[a-z_]+\|>|<asr_text>)", text):
            if part in self.SPECIAL:
                ids.append(self.SPECIAL[part])
            else:
                ids.extend(10 + ord(c) % 1000 for c in part)
        for _ in range(self.drop_pads):
            ids.remove(1999)
        return ids

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(t)) for t in ids)


@pytest.mark.parametrize("kind", ["bf16", "q4"])
def test_transcribe_is_the_stages_by_hand(omx, kind):
    """Qwen3ASR.transcribe_ids / transcribe_samples on 2.5 s of seeded noise (tiny synthetic tower and text model) give the ids of the
    stages done by hand: WhisperMelFrontend, AudioEncoder, the template's ids, Model.prefill(embeds=, embeds_at=), decode, the stop
    rule.  A prompt whose <|audio_pad|> count is not the tower's row count raises."""
    from ominix_mlx_amd import audio, engine, qwen3_asr
    from oracle import ref_qwen3 as rq
    tcfg = rq.Qwen3Config(512, 2, 1536, 8, 4, 64, 2048, 1e-6, 1e6, True)
    acfg = dict(TINY, num_mel_bins=128, output_dim=tcfg.hidden_size)
    enc = _encoder(acfg, rule.tower_synth_weights(acfg, seed=4))
    kw = dict(hidden_size=tcfg.hidden_size, num_hidden_layers=2, intermediate_size=tcfg.intermediate_size, num_attention_heads=8,
              num_key_value_heads=4, head_dim=64, vocab_size=tcfg.vocab_size, tie_word_embeddings=True, max_context=256)
    m = engine.Model(quantization={"bits": 4, "group_size": 64}, **kw) if kind == "q4" else engine.Model(**kw)
    m.synth_weights()
    front = audio.WhisperMelFrontend(n_mels=128)
    tok = FakeTokenizer()
    config = qwen3_asr.Qwen3ASRConfig(audio_config=acfg, audio_token_id=1999)
    samples = (0.1 * np.random.default_rng(78).standard_normal(40000)).astype(np.float32)
    n_new = 12

    rows = enc.forward(front.compute_mel_spectrogram(samples))
    ids = np.asarray(tok.encode(qwen3_asr.prompt_text(rows.shape[0], "English"), add_special_tokens=False), np.uint32)
    at = int(np.nonzero(ids == 1999)[0][0])
    m.reset()
    first = m.prefill(ids, embeds=rows, embeds_at=at)
    stream = [int(first)] + [int(t) for t in m.decode(n_new + 4)]
    eos = stream[5]                                                  # an id the greedy stream does reach: the loop must stop there
    def loop(tokens, max_tokens, eos_ids):                           # model.rs:794-810, one token per turn
        out, recent = [], []
        for t in tokens[:max_tokens]:
            if t in eos_ids:
                break
            recent = (recent + [t])[-10:]
            if len(recent) >= 10 and all(r == t for r in recent):
                break
            out.append(t)
        return out

    hand = loop(stream, n_new, (eos,))
    assert len(hand) <= 5

    asr = qwen3_asr.Qwen3ASR(config, m, enc, front, tok, eos_ids=(eos,))
    assert asr.transcribe_ids(samples, "English", max_tokens=n_new, chunk=4) == hand
    assert asr.transcribe_samples(samples, "English", max_tokens=n_new) == " ".join(str(t) for t in hand)
    assert asr.last_times["audio_rows"] == rows.shape[0] and asr.last_times["prompt_rows"] == ids.size
    # without an EOS in reach: max_tokens ids, the by-hand stream's
    asr.eos_ids = [2047]
    assert asr.transcribe_ids(samples, "English", max_tokens=n_new) == loop(stream, n_new, (2047,))
    short = qwen3_asr.Qwen3ASR(config, m, enc, front, FakeTokenizer(drop_pads=1), eos_ids=(eos,))
    with pytest.raises(omx.OmxError, match=f"holds {rows.shape[0] - 1} <.audio_pad.> ids but the tower made {rows.shape[0]} rows"):
        short.transcribe_ids(samples, "English")
    m.close()
    enc.close()
