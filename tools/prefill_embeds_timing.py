#!/usr/bin/env python3
"""Time the prompt pass over caller-supplied rows (Model.prefill(embeds=)) beside the plain one, alternating, on one model.

The shapes are Qwen3-ASR-1.7B's text decoder (hidden 2048, 28 layers, 16 / 8 heads of 128, intermediate 6144, tied head) with
synthetic weights; the prompt is what 30 s of audio makes: 390 audio rows inside a 405-token template.  Device events
(Model.last_prefill_ms), warm-ups first, then --reps alternating pairs; reports the median and the spread of each form.

    python tools/prefill_embeds_timing.py [--reps 15] [--quant]      # on a GPU box
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import  # noqa: E402

omx_import.load_package()
from ominix_mlx_amd import engine, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rows", type=int, default=390)
    ap.add_argument("--prompt", type=int, default=405)
    ap.add_argument("--quant", action="store_true", help="MLX 4-bit group 64 instead of bf16")
    a = ap.parse_args()
    hd, V = 2048, 151936
    m = engine.Model(hidden_size=hd, num_hidden_layers=28, intermediate_size=6144, num_attention_heads=16, num_key_value_heads=8,
                     head_dim=128, vocab_size=V, tie_word_embeddings=True, max_context=a.prompt + 64,
                     quantization={"bits": 4, "group_size": 64} if a.quant else None)
    m.synth_weights()
    ids = ((np.arange(a.prompt, dtype=np.uint32) * 7919 + 13) % V).astype(np.uint32)
    at = 9
    rows32 = (0.02 * np.random.default_rng(1).standard_normal((a.rows, hd))).astype(np.float32)
    forms = {"plain": None, "f32 rows": ops.Tensor.from_numpy(rows32, "f32"), "bf16 rows": ops.Tensor.from_numpy(rows32, "bf16")}
    times = {k: [] for k in forms}

    def once(rows):
        m.reset()
        m.prefill(ids) if rows is None else m.prefill(ids, embeds=rows, embeds_at=at)
        return m.last_prefill_ms()

    for _ in range(3):
        for rows in forms.values():
            once(rows)
    for _ in range(a.reps):
        for k, rows in forms.items():
            times[k].append(once(rows))
    print(f"{'4-bit' if a.quant else 'bf16'} model, prompt {a.prompt} tokens, {a.rows} caller rows, {a.reps} alternating runs, device ms")
    for k, t in times.items():
        t = np.array(t)
        print(f"  {k:10s} median {np.median(t):8.4f}  min {t.min():8.4f}  max {t.max():8.4f}")
    m.close()


if __name__ == "__main__":
    main()
