"""Decode speed of a Qwen3-8B-shaped model on dense float16 weights against bf16 (synthetic weights, one process):

    f16_decode.py [--ctx 2048] [--steps 100] [--warmup 10] [--windows 3]

Three models one after the other: bf16 (default step: O projection inside the attention launch), bf16 with OMX_ATTN_OPROJ=0 (O as its
own GEMV launch, the float16 model's step shape), and float16 (Model(dtype="float16")).  For each: the prompt of `ctx` tokens, `warmup`
decode steps, then `windows` windows of `steps` steps timed on the device (Model.last_decode_ms), and the per-kernel microseconds of
omx_qwen3_time_step_kernels.  Last line: one JSON object with every figure."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import  # noqa: E402

omx = omx_import.load_package()
from ominix_mlx_amd import engine  # noqa: E402

SHAPE = dict(hidden_size=4096, num_hidden_layers=36, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
             vocab_size=151936)


def measure(label, dtype, oproj, a):
    if oproj is None:
        os.environ.pop("OMX_ATTN_OPROJ", None)
    else:
        os.environ["OMX_ATTN_OPROJ"] = oproj
    m = engine.Model(max_context=a.ctx + a.warmup + a.windows * a.steps + 64, dtype=dtype, **SHAPE)
    m.synth_weights()
    m.prefill(((np.arange(a.ctx, dtype=np.uint32) * 7919) + 13) % SHAPE["vocab_size"])
    m.decode(a.warmup)
    tps = []
    for _ in range(a.windows):
        m.decode(a.steps)
        tps.append(a.steps / (m.last_decode_ms() / 1e3))
    kern = m.time_step_kernels(4)
    m.close()
    res = {"tok_s": tps, "tok_s_median": float(np.median(tps)), "kernel_us": kern}
    print(f"{label:12s} tok/s {' '.join(f'{t:.1f}' for t in tps)}  (median {res['tok_s_median']:.1f})", flush=True)
    print(f"{'':12s} us/launch " + "  ".join(f"{k} {v:.2f}" for k, v in kern.items() if v > 0), flush=True)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ctx", type=int, default=2048)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--windows", type=int, default=3)
    a = p.parse_args()
    out = {"ctx": a.ctx, "steps": a.steps, "windows": a.windows}
    out["bf16"] = measure("bf16", "bfloat16", None, a)
    out["bf16_oproj0"] = measure("bf16 oproj=0", "bfloat16", "0", a)
    out["f16"] = measure("float16", "float16", None, a)
    os.environ.pop("OMX_ATTN_OPROJ", None)
    ref, f = out["bf16_oproj0"], out["f16"]
    out["f16_vs_bf16_oproj0"] = f["tok_s_median"] / ref["tok_s_median"]
    out["f16_vs_bf16"] = f["tok_s_median"] / out["bf16"]["tok_s_median"]
    out["gemv_ratio"] = {k: f["kernel_us"][k] / ref["kernel_us"][k] for k in ("qkv", "o", "gate_up", "down", "lm_head") if ref["kernel_us"][k] > 0}
    print("float16 / bf16(oproj=0) per launch: " + "  ".join(f"{k} {v:.3f}" for k, v in out["gemv_ratio"].items()))
    print(f"float16 step: {out['f16_vs_bf16_oproj0']:.3f}x bf16 with OMX_ATTN_OPROJ=0, {out['f16_vs_bf16']:.3f}x default bf16")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
