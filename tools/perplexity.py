"""Perplexity of a token sequence under a checkpoint, through engine.Model.score (one batched pass per window, the head over every
position in vocabulary panels -- no [T, V] logits):

    python tools/perplexity.py <model_dir> (--tokens ids.npy | --text file) [--ctx 2048] [--stride S]
    python tools/perplexity.py --synthetic [--bits 4] [--prefill]

Prints ONE JSON line: tokens, nll, ppl, tok_per_s, pass_ms, head_ms (device ms of the last window's prompt pass and head).
--text needs the `tokenizers` package generate.load_tokenizer uses; without it the tool says so and exits non-zero.
--synthetic: no checkpoint -- a Qwen3-8B-shape model with synthetic weights (bf16, or MLX 4-bit with --bits 4) and the timing of
score() over 2 048 synthetic tokens: 3 warm-up calls, 10 timed ones, the median of each device time.  --prefill adds the median
last_prefill_ms of prefill() over the same tokens."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic(args):
    import omx_import
    omx_import.load_package()
    import bench
    from ominix_mlx_amd import engine
    cfg = bench.MODELS["qwen3-8b"]
    n = args.ctx
    quant = {"bits": args.bits, "group_size": 64} if args.bits else None
    m = engine.Model(max_context=n + 64, quantization=quant, **cfg)
    m.synth_weights()
    ids = bench.prompt_ids(n, cfg["vocab_size"])
    pass_ms, head_ms, wall = [], [], []
    nll = 0.0
    for i in range(3 + 10):
        m.reset()
        t0 = time.perf_counter()
        lp = m.score(ids)
        dt = time.perf_counter() - t0
        if i >= 3:
            a, b = m.last_score_ms()
            pass_ms.append(a); head_ms.append(b); wall.append(dt)
            nll = -float(lp.astype("float64").sum())
    out = {"workload": f"qwen3-8b {'bf16' if not args.bits else str(args.bits) + '-bit'} score of {n} synthetic tokens",
           "panel": os.environ.get("OMX_SCORE_PANEL", "default"), "tokens": n - 1, "nll": round(nll, 3),
           "ppl": round(math.exp(nll / (n - 1)), 3), "tok_per_s": round(n / statistics.median(wall), 1),
           "pass_ms": round(statistics.median(pass_ms), 3), "head_ms": round(statistics.median(head_ms), 3),
           "pass_ms_min_max": [round(min(pass_ms), 3), round(max(pass_ms), 3)], "head_ms_min_max": [round(min(head_ms), 3), round(max(head_ms), 3)]}
    if args.prefill:
        pf = []
        for i in range(3 + 10):
            m.reset()
            m.prefill(ids)
            if i >= 3:
                pf.append(m.last_prefill_ms())
        out["prefill_ms"] = round(statistics.median(pf), 3)
        out["prefill_ms_min_max"] = [round(min(pf), 3), round(max(pf), 3)]
    m.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("model_dir", nargs="?")
    ap.add_argument("--tokens", help="token ids as a .npy file (any integer dtype)")
    ap.add_argument("--text", help="a UTF-8 text file, encoded with the checkpoint's tokenizer.json")
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--stride", type=int, default=None)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--bits", type=int, default=0, help="--synthetic: 4 = MLX 4-bit weights (default bf16)")
    ap.add_argument("--prefill", action="store_true", help="--synthetic: also time prefill() of the same tokens")
    args = ap.parse_args()
    if args.synthetic:
        return synthetic(args)
    if not args.model_dir or (args.tokens is None) == (args.text is None):
        ap.error("a model directory and exactly one of --tokens / --text are needed (or --synthetic)")
    import numpy as np
    if args.text is not None:
        try:
            import tokenizers  # noqa: F401
        except ImportError:
            print("perplexity: --text needs the `tokenizers` package (generate.load_tokenizer); it is not importable here -- "
                  "pass --tokens ids.npy instead", file=sys.stderr)
            return 2
    import omx_import
    omx_import.load_package()
    from ominix_mlx_amd import generate, loader
    if args.text is not None:
        ids = generate.load_tokenizer(args.model_dir).encode(open(args.text, encoding="utf-8").read(), add_special_tokens=True).ids
    else:
        ids = [int(t) for t in np.load(args.tokens).ravel()]
    model = loader.load_model(args.model_dir, max_context=args.ctx + 64)
    t0 = time.perf_counter()
    res = generate.perplexity(model, ids, ctx=args.ctx, stride=args.stride)
    dt = time.perf_counter() - t0
    pass_ms, head_ms = model.last_score_ms()
    res.update(tok_per_s=round(res["tokens"] / dt, 1), pass_ms=round(pass_ms, 3), head_ms=round(head_ms, 3))
    model.close()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
