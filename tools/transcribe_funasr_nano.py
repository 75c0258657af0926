#!/usr/bin/env python3
"""Fun-ASR-Nano on the device.

    python tools/transcribe_funasr_nano.py <model_dir> a.wav [b.wav ...]     # one file: engine.Model; several: groups of 8 through one Batch
    python tools/transcribe_funasr_nano.py --synthetic                       # the real shapes with synthetic weights: times per stage

--synthetic measures 1 and 8 utterances of 5 s and of 30 s: mel + LFR, the tower with its adaptor in ONE pass over the stacked utterances
against the same code called once per utterance, the prompt passes, and the batched decode step.  Times are host clocks around work that
ends in a device synchronise, each shape warmed up first."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import  # noqa: E402

QWEN3_0_6B = dict(hidden_size=1024, num_hidden_layers=28, intermediate_size=3072, num_attention_heads=16, num_key_value_heads=8, head_dim=128,
                  vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True)


def _timed(omx, fn, reps):
    fn()
    omx.ops.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    omx.ops.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def synthetic(omx, reps):
    from ominix_mlx_amd import audio, engine, funasr_nano as fn
    cfg = fn.parse_config(None)
    g = np.random.default_rng(1)
    w = {}
    for name, shape in fn.tower_weight_shapes(cfg).items():
        if ".norm" in name or "_norm." in name:
            w[name] = (1.0 + 0.1 * g.standard_normal(shape) if name.endswith("weight") else 0.05 * g.standard_normal(shape)).astype(np.float32)
        elif name.endswith(".bias"):
            w[name] = (0.02 * g.standard_normal(shape)).astype(np.float32)
        else:
            w[name] = (g.standard_normal(shape) / np.sqrt(shape[-1])).astype(np.float32)
    enc = audio.FunASRNanoEncoder(**cfg)
    enc.load_weights(w)
    model = engine.Model(max_context=1024, **QWEN3_0_6B)
    model.synth_weights()
    markers = fn.Markers(im_start=151644, im_end=151645, eos=151643, speech_start=151646, speech_end=151647)
    prompt = fn.Prompt([151644, 8948, 198, 2610, 525, 264, 10950, 17847, 13, 151645, 198, 151644, 872, 198, 105761, 46670, 61443, 12857, 104811, 5122],
                       [151645, 198, 151644, 77091, 198], markers)
    nano = fn.FunASRNano(model, enc, audio.SenseVoiceMelFrontend(), None, prompt)
    out = []
    for seconds in (5, 30):
        for n in (1, 8):
            clips = [(0.1 * g.standard_normal(16000 * seconds)).astype(np.float32) for _ in range(n)]
            feats = [nano.lfr_rows(c) for c in clips]
            lengths = [f.shape[0] for f in feats]
            stacked = omx.ops.Tensor.from_numpy(np.concatenate([f.numpy() for f in feats]), "f32")
            r = {"seconds": seconds, "utterances": n, "rows_each": lengths[0]}
            r["mel_lfr_ms"] = _timed(omx, lambda: [nano.lfr_rows(c) for c in clips], reps)
            # the two forms alternate, three rounds each; the median round is reported and the spread of the rounds beside it
            joint, loop = [], []
            for _ in range(3):
                joint.append(_timed(omx, lambda: enc.forward(stacked, lengths), reps))
                loop.append(_timed(omx, lambda: [enc.forward(f, [f.shape[0]]) for f in feats], reps))
            r["tower_joint_ms"], r["tower_loop_ms"] = float(np.median(joint)), float(np.median(loop))
            r["tower_joint_spread_ms"], r["tower_loop_spread_ms"] = max(joint) - min(joint), max(loop) - min(loop)
            nano.joint_tower = True
            rows = nano.encode_audio(clips)
            b = nano._batch(n)
            ms = []
            for slot, x in enumerate(rows):
                ids, at = prompt.ids(x.shape[0])
                b.reset(slot)
                b.set_sampler(slot, 0.0)
                omx.ops.synchronize()
                t = time.perf_counter()
                b.prefill(slot, ids, embeds=x, embeds_at=at)
                ms.append((time.perf_counter() - t) * 1e3)
            r["prompt_rows"] = int(prompt.ids(rows[0].shape[0])[0].size)
            r["prompt_pass_ms_each"] = float(np.median(ms))
            b.decode(8, list(range(n)))
            t = time.perf_counter()
            b.decode(64, list(range(n)))
            r["decode_step_ms"] = (time.perf_counter() - t) / 64 * 1e3
            r["decode_ms_per_token"] = r["decode_step_ms"] / n
            if n == 1:
                ids, at = prompt.ids(rows[0].shape[0])
                model.reset()
                model.set_sampler(0.0)
                model.prefill(ids, embeds=rows[0], embeds_at=at)
                r["model_prompt_pass_ms"] = model.last_prefill_ms()
                model.decode(8)
                t = time.perf_counter()
                model.decode(64)
                r["model_decode_ms_per_token"] = (time.perf_counter() - t) / 64 * 1e3
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
            out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_dir", nargs="?")
    ap.add_argument("wavs", nargs="*")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kv-bits", type=int, default=0, choices=(0, 8))
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--max-tokens", type=int, default=256)
    a = ap.parse_args()
    omx = omx_import.load_package()
    if a.synthetic:
        synthetic(omx, a.reps)
        return
    if not a.model_dir or not a.wavs:
        ap.error("model_dir and at least one wav, or --synthetic")
    from ominix_mlx_amd import audio, funasr_nano as fn
    nano = fn.FunASRNano.load(a.model_dir, kv_bits=a.kv_bits)
    cfg = fn.SamplingConfig(temperature=a.temperature, max_tokens=a.max_tokens)
    if len(a.wavs) == 1:
        print(nano.transcribe(a.wavs[0], cfg))
        return
    for path, text in zip(a.wavs, nano.transcribe_samples_batch([audio.load_wav(p) for p in a.wavs], cfg)):
        print(f"{path}\t{text}")


if __name__ == "__main__":
    main()
