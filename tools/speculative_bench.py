"""Cost of the speculative-decoding verify pass (Model.verify: n tokens batched on top of the cache, [n, V] lm_head GEMM, per-row argmax)
against n ordinary decode steps, Qwen3-8B shapes, 2048 tokens of context.  With synthetic weights a draft model cannot agree with the
target (flat logits), so this reports the MECHANISM's ceiling: tokens per second if every draft token were accepted, draft cost excluded.
--bits B [--group G]: the same on a packed (MLX affine B-bit, group G = 64) checkpoint -- verify runs the few-row packed GEMV
(csrc/qgemv_rows.hip) and is timed against B-bit decode steps.
usage: python tools/speculative_bench.py [--bits B [--group G]] [n ...]      (default n = 2 3 5 9 17)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import omx_import  # noqa: E402

omx = omx_import.load_package()
from ominix_mlx_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, default=0, help="packed checkpoint width (2, 3, 4, 5, 6, 8); 0 = bf16")
ap.add_argument("--group", type=int, default=64)
ap.add_argument("n", type=int, nargs="*")
args = ap.parse_args()
cfg = dict(bench.QWEN3_8B)
quant = {"bits": args.bits, "group_size": args.group} if args.bits else None
m = engine.Model(max_context=2048 + 512, quantization=quant, **cfg)
m.synth_weights()
prompt = bench.prompt_ids(2048, cfg["vocab_size"])
m.prefill(prompt)
t0 = time.perf_counter(); m.decode(32); step_ms = (time.perf_counter() - t0) * 1e3 / 32
print(f"{'bf16' if not args.bits else f'{args.bits}-bit group {args.group}'}: decode step {step_ms:.3f} ms")
for n in (args.n or (2, 3, 5, 9, 17)):
    toks = [int(t) for t in prompt[:n]]
    m.verify(toks); m.trim(n, toks[0])              # warm (buffers, kernels)
    t0 = time.perf_counter()
    reps = 8
    for _ in range(reps):
        m.verify(toks)
        m.trim(n, toks[0])
    ms = (time.perf_counter() - t0) * 1e3 / reps
    print(f"verify {n:2d} tokens: {ms:7.3f} ms  = {ms / step_ms:4.2f} decode steps  -> {n / ms * 1e3:7.1f} tok/s if all {n - 1} drafts are accepted "
          f"(plain decode {1e3 / step_ms:.1f})")
m.close()
