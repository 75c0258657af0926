"""Fun-ASR-Nano end to end on the device with synthetic weights and no tokenizer: three clips of different length through the mel
frontend, one joint tower pass, and one Batch -- against the decoder oracle fed the device's own adapted rows, compared the way
tests/test_gpu_prefill_embeds.py (test_arbitrary_rows_match_forward_from_rows) compares Model.prefill(embeds=): the bf16 prompt-pass
bound 2^-7 * max|logit| * sqrt(layers) on the prompt's logits, tokens equal outside the near-tie guard."""
import numpy as np
import pytest

import funasr_nano_rule as tower_rule
import qwen3_asr_rule as rule
from oracle import ref_core as rc
from oracle import ref_qwen3 as rq

pytestmark = pytest.mark.gpu

LLM = rq.Qwen3Config(1024, 2, 3072, 16, 8, 128, 2048, 1e-6, 1e6, False)
TOWER = dict(lfr_dim=560, output_size=256, attention_heads=2, linear_units=512, num_blocks=2, tp_blocks=1, kernel_size=11,
             encoder_dim=256, ffn_dim=256, llm_dim=1024, n_layer=1)
N_NEW = 8


def _build():
    from ominix_mlx_amd import audio, engine, funasr_nano as fn
    w = rq.synth_weights(LLM)
    m = engine.Model(hidden_size=LLM.hidden_size, num_hidden_layers=LLM.num_hidden_layers, intermediate_size=LLM.intermediate_size,
                     num_attention_heads=LLM.num_attention_heads, num_key_value_heads=LLM.num_key_value_heads, head_dim=LLM.head_dim,
                     vocab_size=LLM.vocab_size, rms_norm_eps=LLM.rms_norm_eps, rope_theta=LLM.rope_theta,
                     tie_word_embeddings=LLM.tie_word_embeddings, max_context=256)
    m.load_weights(w)
    enc = audio.FunASRNanoEncoder(**TOWER)
    enc.load_weights(tower_rule.synth_weights(TOWER, 11))
    markers = fn.Markers(im_start=2001, im_end=2002, eos=2000, speech_start=2003, speech_end=2004)
    prompt = fn.Prompt([2001, 17, 5, 99, 2002, 5, 2001, 23, 5, 400, 401], [2002, 5, 2001, 31, 5], markers)
    return fn.FunASRNano(m, enc, audio.SenseVoiceMelFrontend(), None, prompt, joint_tower=True), rq.Qwen3Oracle(LLM, w), fn


def test_three_clips_match_the_decoder_oracle(omx):
    nano, oracle, fn = _build()
    g = np.random.default_rng(31)
    clips = [(0.1 * g.standard_normal(n)).astype(np.float32) for n in (8000, 12800, 17600)]
    cfg = fn.SamplingConfig(max_tokens=N_NEW)
    got = nano.transcribe_ids_batch(clips, cfg)
    rows = nano.encode_audio(clips)
    lengths = [r.shape[0] for r in rows]
    assert len(set(lengths)) == 3 and all(r.shape[1] == LLM.hidden_size for r in rows)
    factor = 2.0 ** -7 * np.sqrt(LLM.num_hidden_layers)
    b = nano._batch(3)
    for slot, r in enumerate(rows):
        ids, at = nano.prompt.ids(r.shape[0])
        h = np.array(rule.embed_rows(oracle, ids), dtype=np.float32)
        h[at:at + r.shape[0]] = r.numpy()
        ref_tokens, ref_logits = rule.generate_from_rows(oracle, h, N_NEW)
        bound = factor * np.abs(ref_logits).max()
        b.reset(slot)
        b.set_sampler(slot, 0.0)
        first = b.prefill(slot, ids, embeds=r, embeds_at=at)
        err = np.abs(b.logits(slot) - ref_logits[0]).max()
        print(f"clip {slot}: {r.shape[0]} rows, prompt of {ids.size}: max |logit error| {err:.6f}, bound {bound:.6f}")
        assert err <= bound
        stop = fn.StopRule(nano.markers, N_NEW)
        want = [int(t) for t in ref_tokens if stop.push(t)]
        margins = rc.argmax_margin(ref_logits)
        assert first == got[slot][0] if got[slot] else True
        for i in range(min(len(want), len(got[slot]))):
            if got[slot][i] != want[i]:
                assert margins[i] <= 2 * bound, f"clip {slot} token {i}: got {got[slot][i]} want {want[i]} with margin {margins[i]:.4f}"
                break
        else:
            assert len(got[slot]) == len(want)
    # the per-utterance tower gives the same tokens outside near-ties; at least it runs the same path end to end
    nano.joint_tower = False
    loop = nano.transcribe_ids_batch(clips, cfg)
    assert [len(t) > 0 for t in loop] == [len(t) > 0 for t in got]
    # and one clip through engine.Model is the batch's slot
    alone = nano.generate_ids(rows[1], cfg)
    assert alone[0] == got[1][0]
