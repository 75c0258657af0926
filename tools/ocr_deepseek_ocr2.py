#!/usr/bin/env python3
"""Image to text with a DeepSeek-OCR-2 checkpoint, or (--synthetic) time the language decoder at the real shapes.

    python tools/ocr_deepseek_ocr2.py <model_dir> global.npy [--crops crops.npy] "<image>\\nFree OCR."
    python tools/ocr_deepseek_ocr2.py --synthetic

global.npy is the [1024, 1024, 3] global view, crops.npy the [n, 768, 768, 3] crops (n <= 6): float in [-1, 1], or uint8.  Resizing and
cropping are the caller's.  Needs the `tokenizers` package and the checkpoint's tokenizer.json; prints the generated ids and the text.

--synthetic:

The decoder alone (12 layers, hidden 1280, 10 / 10 heads of 128, layer 0 dense at 6848, 64 experts of 896, top-6, 2 shared, vocabulary
129 280) with synthetic weights: the tokens mean nothing and the times are real.  The prompt pass over 257 image rows (a 1024 px view and
the separator; the towers' own times: tools/encode_deepseek_ocr2.py --synthetic) plus the text, then ms per decoded token with the shared
experts as pseudo-expert slots (the default) and as launches of their own (OMX_MOE_SHARED_SLOTS=0), against the bytes a token streams.
Median of three timed windows after a warm-up, device events around calls that return when the device is done.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import  # noqa: E402

omx = omx_import.load_package()
from ominix_mlx_amd import deepseek_ocr2 as ds, engine, loader  # noqa: E402


def event_ms(fn, reps=3):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return r, float(np.median(ts))


def synthetic(n_decode=64):
    args = loader.deepseek_ocr2_args({})
    L, k, ns = args["num_hidden_layers"], args["num_experts_per_tok"], args["n_shared_experts"]
    n_moe = L - args["first_k_dense_replace"]
    text = 24
    ids = np.concatenate([[0], np.full(10, 5), np.full(257, ds.IMAGE_TOKEN_ID), np.full(text - 11, 7)]).astype(np.uint32)
    rows = np.random.default_rng(0).standard_normal((257, args["hidden_size"])).astype(np.float32)
    print("DeepSeek-OCR-2 decoder, real shapes, synthetic weights; median of 3 windows after a warm-up")
    for env, name in (("1", "shared experts as slots (default)"), ("0", "shared experts as launches of their own (OMX_MOE_SHARED_SLOTS=0)")):
        os.environ["OMX_MOE_SHARED_SLOTS"] = env
        m = engine.Model(**args, max_context=1024)
        m.synth_weights()

        def prompt():
            m.reset()
            return m.prefill(ids, embeds=rows, embeds_at=11)

        _, ms_p = event_ms(prompt)
        _, ms_d = event_ms(lambda: m.decode(n_decode))
        form = omx.lib.omx_moe_deepseek_form(1, args["hidden_size"], args["moe_intermediate_size"], k, ns, ns if env == "1" else 0, 1)
        ffn = 2 * args["first_k_dense_replace"] + n_moe * (4 if form == 0 else 4 + 2 * (ns > 0))
        gb = m.step_bytes(len(ids) + n_decode // 2) / 1e9
        print(f"  {name}:")
        print(f"    prompt pass, {len(ids)} positions (257 image rows): median {ms_p:8.3f} ms")
        print(f"    decode: median {ms_d / n_decode:7.4f} ms per token over {n_decode} tokens, path {m.decode_path()}; {gb:.3f} GB per token -> "
              f"{gb / (ms_d / n_decode) * 1e3:7.1f} GB/s; feed-forward launches per token: {ffn} ({n_moe} MoE layers x {4 if form == 0 else 6}, "
              f"{args['first_k_dense_replace']} dense x 2)")
        m.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model_dir", nargs="?")
    ap.add_argument("global_view", nargs="?")
    ap.add_argument("prompt", nargs="?", default="<image>\nFree OCR.")
    ap.add_argument("--crops")
    ap.add_argument("--max-tokens", type=int, default=1024)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--repetition-context-size", type=int, default=20)
    ap.add_argument("--synthetic", action="store_true")
    a = ap.parse_args()
    if a.synthetic:
        return synthetic()
    if not (a.model_dir and a.global_view):
        ap.error("give <model_dir> global.npy [--crops crops.npy] [prompt], or --synthetic")
    m = ds.DeepseekOCR2.load(a.model_dir)
    out = m.ocr(np.load(a.global_view), np.load(a.crops) if a.crops else None, a.prompt, max_tokens=a.max_tokens, temperature=a.temperature,
                repetition_penalty=a.repetition_penalty, repetition_context_size=a.repetition_context_size)
    print(out)
    if m.tokenizer is not None:
        print(m.tokenizer.decode([t for t in out if t != ds.EOS_TOKEN_ID]))
    m.close()


if __name__ == "__main__":
    main()
