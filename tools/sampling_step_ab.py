"""Cost of filtered sampling inside the decode step: the Qwen3-8B-shaped bf16 step (synthetic weights, 151 936-entry vocabulary) timed
with plain temperature sampling and with the filters of csrc/sample_filter.hip, in ONE process on ONE model, the modes interleaved
round by round (switching the sampler re-captures the step graph; every timed window follows a warm-up of its own).

    python tools/sampling_step_ab.py [--prompt 512] [--steps 128] [--rounds 4] [--modes temperature,topk_topp,topp,topk_presence]
    python tools/sampling_step_ab.py --json out.json ...          # the table as JSON as well
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sampling_step_ab.py --fresh-models --layers 4 --rounds 1 --steps 64
                                                                  # the sampler's launches (their time does not depend on the layers)

The yardstick of a change to the sampler is the PARENT commit's temperature step: build that commit's library as a variant
(`make -C ominix-mlx_amd/csrc VARIANT=parent` in a checkout of it, the .so copied beside this one) and run
`OMX_LIB_VARIANT=parent python tools/sampling_step_ab.py --modes temperature` in the same GPU visit.  Run each invocation under its own
`timeout` and chain them with `&&`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import omx_import  # noqa: E402
omx = omx_import.load_package()
from ominix_mlx_amd import engine  # noqa: E402

CFG = dict(hidden_size=4096, num_hidden_layers=36, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
           vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False)
MODES = {
    "greedy": (0.0, {}),
    "temperature": (0.6, {}),
    "topk": (0.6, dict(top_k=20)),
    "topk_topp": (0.6, dict(top_k=20, top_p=0.95)),                     # the Qwen3 model card's settings
    "topp": (0.6, dict(top_p=0.95)),                                     # the worst case of the noise pass: 10^4 - 10^5 survivors
    "topk_presence": (0.6, dict(top_k=20, presence_penalty=1.5)),        # funasr-qwen4b's sample_top_k_p
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--modes", default="temperature,topk_topp,topp,topk_presence")
    ap.add_argument("--json", default=None)
    ap.add_argument("--layers", type=int, default=CFG["num_hidden_layers"], help="fewer layers: a short run for a kernel trace of the sampler")
    ap.add_argument("--fresh-models", action="store_true",
                    help="one model per mode, its sampler set before the first step (no step graph is dropped and re-captured: for profiler runs)")
    args = ap.parse_args()
    modes = args.modes.split(",")
    prompt = np.random.default_rng(0).integers(0, CFG["vocab_size"], args.prompt).astype(np.uint32)
    cfg = dict(CFG, num_hidden_layers=args.layers)

    def new_model(mode=None):
        m = engine.Model(max_context=args.prompt + (args.steps + 8) * args.rounds * len(modes) + 64, **cfg)
        m.synth_weights()
        if mode is not None:
            m.set_sampler(MODES[mode][0], 1, **MODES[mode][1])
        m.prefill(prompt)
        return m

    shared = None if args.fresh_models else new_model()
    times = {k: [] for k in modes}
    for r in range(args.rounds):
        for k in modes:
            temp, kw = MODES[k]
            if args.fresh_models:
                m = new_model(k)
            else:
                m = shared
                m.set_sampler(temp, 1 + r, **kw)
            m.decode(8)                  # graph capture + warm-up of this mode
            omx.check(omx.lib.omx_synchronize(m.stream()))
            t0 = time.perf_counter()
            m.decode(args.steps)
            omx.check(omx.lib.omx_synchronize(m.stream()))
            times[k].append((time.perf_counter() - t0) / args.steps * 1e6)
            assert m.decode_path() == "graph"
    base = min(times[modes[0]])
    out = {"library": os.path.basename(omx.LIB_PATH), "prompt": args.prompt, "steps": args.steps, "rounds": args.rounds, "modes": {}}
    for k in modes:
        best, med = min(times[k]), float(np.median(times[k]))
        out["modes"][k] = {"best_us_per_step": round(best, 2), "median_us_per_step": round(med, 2), "rounds_us": [round(t, 2) for t in times[k]],
                           "best_minus_first_mode_us": round(best - base, 2)}
        print(f"{k:16s} best {best:9.2f} us/step  median {med:9.2f}  (+{best - base:7.2f} us vs {modes[0]})  rounds {[round(t, 1) for t in times[k]]}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
