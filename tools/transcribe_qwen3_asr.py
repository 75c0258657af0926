#!/usr/bin/env python3
"""Transcribe a WAV with a Qwen3-ASR checkpoint, or (--synthetic) time the device stages of a transcription at the real shapes with
synthetic weights: mel, audio tower, the prompt pass over the tower's rows, decode steps.

    python tools/transcribe_qwen3_asr.py <model_dir> <wav> [--language English]
    python tools/transcribe_qwen3_asr.py --synthetic [--seconds 30] [--reps 10] [--quant]

--synthetic:

Qwen3-ASR-1.7B (qwen3-asr-mlx/README.md): tower of 24 layers, d_model 1024, 16 heads, FFN 4096, stem width 480, output 2048; text decoder
Qwen3 with 28 layers, hidden 2048, 16 / 8 heads of 128, intermediate 6144, tied head, vocabulary 151 936.  No tokenizer and no
checkpoint: the prompt is a template's worth of ids around the <|audio_pad|> span, so the tokens mean nothing and the times are real.
Host clock around a device synchronise for mel and tower (median of --reps after warm-ups), device events for the prompt pass and the
decode steps.

"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import  # noqa: E402

omx = omx_import.load_package()
from ominix_mlx_amd import audio, engine  # noqa: E402

TOWER = dict(num_mel_bins=128, encoder_layers=24, encoder_attention_heads=16, encoder_ffn_dim=4096, d_model=1024, max_source_positions=1500,
             n_window=50, output_dim=2048, n_window_infer=800, downsample_hidden_size=480)


def tower_weights(cfg, seed=0):
    g = np.random.default_rng(seed)
    ds, d, ffn = cfg["downsample_hidden_size"], cfg["d_model"], cfg["encoder_ffn_dim"]
    f3 = cfg["num_mel_bins"]
    for _ in range(3):
        f3 = (f3 - 1) // 2 + 1
    shapes = {"conv2d1.weight": (ds, 3, 3, 1), "conv2d1.bias": (ds,), "conv2d2.weight": (ds, 3, 3, ds), "conv2d2.bias": (ds,),
              "conv2d3.weight": (ds, 3, 3, ds), "conv2d3.bias": (ds,), "conv_out.weight": (d, ds * f3), "ln_post.weight": (d,),
              "ln_post.bias": (d,), "proj1.weight": (d, d), "proj1.bias": (d,), "proj2.weight": (cfg["output_dim"], d),
              "proj2.bias": (cfg["output_dim"],)}
    for l in range(cfg["encoder_layers"]):
        p = f"layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            shapes[p + f"self_attn.{n}.weight"], shapes[p + f"self_attn.{n}.bias"] = (d, d), (d,)
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            shapes[p + n + ".weight"] = shapes[p + n + ".bias"] = (d,)
        shapes[p + "fc1.weight"], shapes[p + "fc1.bias"], shapes[p + "fc2.weight"], shapes[p + "fc2.bias"] = (ffn, d), (ffn,), (d, ffn), (d,)
    out = {}
    for name, shape in shapes.items():
        if name.endswith("norm.weight") or name == "ln_post.weight":
            out[name] = np.ones(shape, np.float32)
        elif name.endswith(".bias"):
            out[name] = np.zeros(shape, np.float32)
        else:
            out[name] = (g.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))).astype(np.float32)
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        omx.check(omx.lib.omx_synchronize(None))
        t0 = time.perf_counter()
        r = fn()
        omx.check(omx.lib.omx_synchronize(None))
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model_dir", nargs="?")
    ap.add_argument("wav", nargs="?")
    ap.add_argument("--language", default="English")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--quant", action="store_true", help="text decoder in MLX 4-bit group 64 instead of bf16")
    a = ap.parse_args()
    if not a.synthetic:
        if not (a.model_dir and a.wav):
            ap.error("give <model_dir> <wav>, or --synthetic")
        from ominix_mlx_amd import qwen3_asr
        asr = qwen3_asr.Qwen3ASR.load(a.model_dir)
        print(asr.transcribe(a.wav, a.language))
        t = asr.last_times
        print(f"{t['frames']} frames -> {t['audio_rows']} audio rows, prompt of {t['prompt_rows']} rows; to the first token {t['to_first_token_s'] * 1e3:.1f} ms "
              f"(prompt pass {t['prompt_pass_ms']:.2f} ms on the device), {t['tokens']} tokens in {t['decode_s'] * 1e3:.1f} ms", file=sys.stderr)
        return
    samples = (0.1 * np.random.default_rng(0).standard_normal(int(a.seconds * 16000))).astype(np.float32)
    dev_samples = omx.ops.Tensor.from_numpy(samples, "f32")
    front = audio.WhisperMelFrontend()
    enc = audio.AudioEncoder(**TOWER)
    enc.load_weights(tower_weights(TOWER))
    V = 151936
    m = engine.Model(hidden_size=2048, num_hidden_layers=28, intermediate_size=6144, num_attention_heads=16, num_key_value_heads=8,
                     head_dim=128, vocab_size=V, tie_word_embeddings=True, max_context=1024,
                     quantization={"bits": 4, "group_size": 64} if a.quant else None)
    m.synth_weights()
    for _ in range(3):                                  # warm-ups of every shape the timed windows use
        mel = front.compute_mel_spectrogram(dev_samples)
        rows = enc.forward(mel)
    mel, mel_ms, mel_lo, mel_hi = timed(lambda: front.compute_mel_spectrogram(dev_samples), a.reps)
    rows, tw_ms, tw_lo, tw_hi = timed(lambda: enc.forward(mel), a.reps)
    n = rows.shape[0]
    ids = np.concatenate([(np.arange(9) * 7919 + 13) % V, np.full(n, 151676), (np.arange(6) * 104729 + 7) % V]).astype(np.uint32)
    pf, dec = [], []
    for i in range(a.reps + 2):
        m.reset()
        m.prefill(ids, embeds=rows, embeds_at=9)
        m.decode(a.tokens)
        if i >= 2:
            pf.append(m.last_prefill_ms())
            dec.append(m.last_decode_ms() / a.tokens)
    print(f"{a.seconds:g} s of audio: {mel.shape[1]} frames -> {n} audio rows, prompt of {ids.size} rows; text decoder {'4-bit' if a.quant else 'bf16'}; {a.reps} runs")
    print(f"  mel          median {mel_ms:8.3f} ms  (min {mel_lo:.3f}, max {mel_hi:.3f})   host clock around a device synchronise")
    print(f"  tower        median {tw_ms:8.3f} ms  (min {tw_lo:.3f}, max {tw_hi:.3f})   host clock around a device synchronise")
    print(f"  prompt pass  median {np.median(pf):8.3f} ms  (min {min(pf):.3f}, max {max(pf):.3f})   device events")
    print(f"  per token    median {np.median(dec):8.4f} ms  (min {min(dec):.4f}, max {max(dec):.4f})   device events over {a.tokens} steps")


if __name__ == "__main__":
    main()
