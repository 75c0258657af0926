"""Batched decode (engine.Batch) of the Qwen3-8B-shaped synthetic model: aggregate tokens per second against the batch size.

    python tools/batch_decode.py [--bits 0 4] [--ctx 2048] [--steps 128] [--windows 3]
        per weight format (0 = bf16, 4 = 4-bit group 64): the single-sequence Model.decode rate, then B = 1, 2, 4, 8 slots each prefilled
        with --ctx tokens, then 8 slots with ragged contexts (ctx/8 .. ctx); every figure is the median of --windows windows of --steps
        steps after a warm-up, timed with device events on the engine's stream (Model.last_decode_ms / Batch.last_decode_ms).
        One JSON line per row, then the table.  --batch-sizes 1 8 keeps those rows only (and drops the single-sequence and ragged rows).
        --temperature T [--top-k K] [--top-p P] [--presence-penalty Q]: every slot samples with these settings (Batch.set_sampler,
        seed = its slot) instead of greedily -- the cost of the per-slot filters is the difference between two such runs.  They
        apply to --trace too.  --logprobs K (0..20): per-token log-probabilities on (Model.set_logprobs / Batch.set_logprobs) in the
        single-sequence row, every batch row and --trace -- the cost of the two extra launches is the difference to a run without it.
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/batch_decode.py --trace --bits 0 [--ctx 2048] [--steps 16]
        8 slots prefilled, --steps steps at B = 8 and nothing else at that row count: the trace's last steps give the per-launch times
        of a B = 8 step (python tools/batch_decode.py --stats DIR [--steps 32] prints them; pass rocprofv3 -f csv).
    python tools/batch_decode.py --fork [--fork-ctx 2048 8192] [--steps 128] [--windows 3]
        bf16: eight slots forked from one prompt (Batch.fork) against eight slots prefilled independently with prompts of the same
        length, at every --fork-ctx, each with the grouped read of the shared span on and off (OMX_BATCH_SHARE=1 / 0) in a child
        process of its own; same windows, same device events.  One JSON line per row, then the table.  With --trace: one
        configuration only (--fork-ctx C, OMX_BATCH_SHARE from the environment), eight forked slots, for a kernel trace.
    python tools/batch_decode.py --kv-bits 0 8 [--bits 0 4] [--ctx 2048 16384] [--steps 128] [--windows 3]
        the K/V storage of the batch (Model.batch(kv_bits=...): 0 = bf16 slabs, 8 = 8-bit MLX affine rows read packed): per weight
        format and context, B = 8 with every --kv-bits value in turn, each line in a child process of its own.  To reach a long
        context quickly one slot is prefilled and forked seven times with OMX_BATCH_SHARE=0: the fork copies the rows and nothing is
        shared, so every slot reads its own slab.  Same windows, same device events; the JSON lines carry the slab bytes
        (Batch.kv_bytes) and the algorithmic K/V bytes a step's attention reads.  With --trace: the first --bits / --ctx / --kv-bits
        only, filled the same way, for a kernel trace (--stats prints it)."""
import argparse, csv, glob, json, os, subprocess, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--bits", type=int, nargs="+", default=[0, 4])
ap.add_argument("--ctx", type=int, nargs="+", default=[2048], help="context per slot; the modes that take one use the first")
ap.add_argument("--kv-bits", type=int, nargs="+", help="K/V storage of the batch (0 = bf16, 8 = 8-bit rows): the comparison described above")
ap.add_argument("--kv-child", type=int, nargs=3, metavar=("BITS", "CTX", "KV_BITS"), help=argparse.SUPPRESS)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--layers", type=int, default=36)
ap.add_argument("--trace", action="store_true", help="only prefill 8 slots and run --steps steps at B = 8 (for a kernel trace)")
ap.add_argument("--stats", metavar="DIR", help="print the per-launch times of the last --steps steps of a --trace run's kernel_trace.csv under DIR")
ap.add_argument("--fork", action="store_true", help="eight forked slots against eight independent ones, shared-span read on and off")
ap.add_argument("--fork-ctx", type=int, nargs="+", default=[2048, 8192])
ap.add_argument("--fork-child", type=int, metavar="CTX", help=argparse.SUPPRESS)
ap.add_argument("--batch-sizes", type=int, nargs="+", help="only these slot counts (1..8), no single-sequence and no ragged row")
ap.add_argument("--temperature", type=float, default=0.0, help="every slot's sampler (0 = greedy)")
ap.add_argument("--top-k", type=int, default=0)
ap.add_argument("--top-p", type=float, default=1.0)
ap.add_argument("--presence-penalty", type=float, default=0.0)
ap.add_argument("--logprobs", type=int, default=None, help="log-probabilities of the generated tokens with K alternatives (off by default)")
args = ap.parse_args()
ctx_list, args.ctx = args.ctx, args.ctx[0]

if args.kv_bits and not args.trace and not args.kv_child:
    table = []
    for bits in args.bits:
        for ctx in ctx_list:
            for kvb in args.kv_bits:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kv-child", str(bits), str(ctx), str(kvb), "--steps", str(args.steps),
                                    "--windows", str(args.windows), "--layers", str(args.layers)], env=dict(os.environ, OMX_BATCH_SHARE="0"),
                                   stdout=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL)
                if p.returncode:
                    sys.exit(f"--kv-child {bits} {ctx} {kvb} failed with status {p.returncode}")
                for ln in p.stdout.splitlines():
                    if ln.startswith("{"):
                        print(ln, flush=True)
                        table.append(json.loads(ln))
    print(f"\n{'format':<12} {'context':>8} {'kv_bits':>8} {'ms/step':>9} {'tok/s':>9} {'slabs GB':>9} {'K/V read MB/layer':>18}")
    for r in table:
        print(f"{r['format']:<12} {r['ctx']:>8} {r['kv_bits']:>8} {r['ms_per_step']:>9.3f} {r['tok_s']:>9.1f} {r['kv_bytes'] / 1e9:>9.2f} "
              f"{r['kv_read_bytes_per_layer'] / 1e6:>18.1f}")
    sys.exit(0)

if args.fork and not args.trace:
    # every (context, switch) in a process of its own: the switch is read when the batch is created, and no run inherits another's state
    table = []
    for ctx in args.fork_ctx:
        for share in ("1", "0"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--fork-child", str(ctx), "--steps", str(args.steps), "--windows",
                                str(args.windows), "--layers", str(args.layers)], env=dict(os.environ, OMX_BATCH_SHARE=share),
                               stdout=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL)
            if p.returncode:
                sys.exit(f"--fork-child {ctx} (OMX_BATCH_SHARE={share}) failed with status {p.returncode}")
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    print(ln, flush=True)
                    table.append(json.loads(ln))
    print(f"\n{'slots':<14} {'prompt':>7} {'share':>6} {'ms/step':>9} {'tok/s':>9} {'fork / prefill ms':>18}")
    for r in table:
        print(f"{r['slots']:<14} {r['ctx']:>7} {r['share']:>6} {r['ms_per_step']:>9.3f} {r['tok_s']:>9.1f} {r['setup_ms']:>18.1f}")
    sys.exit(0)

if args.stats:
    # the dispatches of the last --steps steps of the trace: a step begins with its embedding gather
    import re, statistics
    f = glob.glob(args.stats + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))))
    starts = [i for i, r in enumerate(rows) if "batch_embed_kernel" in r[2]]
    steps = min(args.steps, len(starts) - 1)
    rows = rows[starts[-steps - 1]:starts[-1]]        # (the very last step is left out: it has no successor to end it)
    by = {}
    for s0, e0, name in rows:
        name = re.sub(r"\(anonymous namespace\)::|omx::|^void ", "", name)
        by.setdefault(re.sub(r"\(.*\)$", "", name)[:78], []).append((e0 - s0) / 1e3)
    print(f"{'kernel':<78} {'launches/step':>13} {'median us':>10} {'us/step':>9}")
    for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print(f"{name:<78} {len(v) / steps:>13.1f} {statistics.median(v):>10.2f} {sum(v) / steps:>9.1f}")
    busy = sum(sum(v) for v in by.values()) / steps
    print(f"{steps} steps: {len(rows) / steps:.0f} launches per step, kernel time {busy:.1f} us per step, "
          f"first start to last end {(rows[-1][1] - rows[0][0]) / 1e3 / steps:.1f} us per step")
    sys.exit(0)

import omx_import
omx = omx_import.load_package()
from ominix_mlx_amd import engine

V = 151936


def prompt(n, shift):
    return ((np.arange(n, dtype=np.int64) * 7919 + 13 + shift) % V).astype(np.uint32)


def median_ms(run, read_ms, steps, windows):
    ms = []
    for _ in range(windows):
        run(steps)
        ms.append(read_ms() / steps)
    return float(np.median(ms)), ms


if args.kv_child or (args.kv_bits and args.trace):
    bits, ctx, kvb = args.kv_child or (args.bits[0], args.ctx, args.kv_bits[0])
    m = engine.Model(hidden_size=4096, num_hidden_layers=args.layers, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8,
                     head_dim=128, vocab_size=V, max_context=ctx + 8 + args.steps * args.windows + 16,
                     quantization={"bits": bits, "group_size": 64} if bits else None)
    m.synth_weights()
    fmt = f"{bits}-bit g64" if bits else "bf16"
    b = m.batch(8, kv_bits=kvb)
    b.prefill(0, prompt(ctx, 0))
    for s in range(1, 8):
        b.fork(0, s)
    assert b.shared(1)[1] == 0, "run with OMX_BATCH_SHARE=0: the slots are meant to share nothing"
    if args.trace:
        b.decode(args.steps)
        print(f"{fmt}, kv_bits {kvb}, 8 slots of {ctx} tokens: {b.last_decode_ms() / args.steps:.3f} ms per step", flush=True)
    else:
        b.decode(8)
        ms, raw = median_ms(b.decode, b.last_decode_ms, args.steps, args.windows)
        # a step's attention reads every cached row of every slot once per KV head: K and V, mid-run length
        rows = 8 * 8 * (ctx + 8 + args.steps * args.windows // 2)
        per_row = 2 * (128 * 2 if kvb == 0 else 128 + 4 * 128 // 64)
        print(json.dumps({"format": fmt, "B": 8, "ctx": ctx, "kv_bits": kvb, "ms_per_step": ms, "tok_s": 8e3 / ms, "kv_bytes": b.kv_bytes(),
                          "kv_read_bytes_per_layer": rows * per_row, "windows_ms": raw}), flush=True)
    b.close(); m.close()
    sys.exit(0)

if args.fork_child or (args.fork and args.trace):
    import time
    ctx = args.fork_child or args.fork_ctx[0]
    share = os.environ.get("OMX_BATCH_SHARE", "1")
    m = engine.Model(hidden_size=4096, num_hidden_layers=args.layers, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8,
                     head_dim=128, vocab_size=V, max_context=ctx + 8 + args.steps * args.windows + 16)
    m.synth_weights()
    b = m.batch(8)
    for forked in ((True,) if args.trace else (True, False)):
        for s in range(8):
            b.reset(s)
        b.prefill(0, prompt(ctx, 0))
        t0 = time.perf_counter()
        for s in range(1, 8):
            b.fork(0, s) if forked else b.prefill(s, prompt(ctx, s))
        setup = (time.perf_counter() - t0) * 1e3 / 7          # (both calls wait for the device)
        if args.trace:
            b.decode(args.steps)
            print(f"bf16, 8 forked slots of {ctx} tokens, OMX_BATCH_SHARE={share}: {b.last_decode_ms() / args.steps:.3f} ms per step", flush=True)
            break
        b.decode(8)
        ms, raw = median_ms(b.decode, b.last_decode_ms, args.steps, args.windows)
        print(json.dumps({"slots": "8 forked" if forked else "8 independent", "ctx": ctx, "share": int(share), "shared_len": b.shared(1)[1],
                          "ms_per_step": ms, "tok_s": 8e3 / ms, "setup_ms": setup, "windows_ms": raw}), flush=True)
    b.close(); m.close()
    sys.exit(0)

table = []
for bits in args.bits:
    room = 8 + args.steps * args.windows + 16
    m = engine.Model(hidden_size=4096, num_hidden_layers=args.layers, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8,
                     head_dim=128, vocab_size=V, max_context=args.ctx + room, quantization={"bits": bits, "group_size": 64} if bits else None)
    m.synth_weights()
    fmt = f"{bits}-bit g64" if bits else "bf16"
    b = m.batch(8)
    if args.logprobs is not None:
        m.set_logprobs(args.logprobs)
        b.set_logprobs(args.logprobs)
    sampler = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, presence_penalty=args.presence_penalty, logprobs=args.logprobs)
    filters = {k: v for k, v, off in (("top_k", args.top_k, 0), ("top_p", args.top_p, 1.0), ("presence_penalty", args.presence_penalty, 0.0)) if v != off}
    if args.temperature != 0.0 or filters:
        for s in range(8):
            b.set_sampler(s, args.temperature, s, **filters)
    if args.trace:
        for s in range(8):
            b.prefill(s, prompt(args.ctx, s))
        b.decode(args.steps)
        print(f"{fmt}: {args.steps} steps at B = 8, {b.last_decode_ms() / args.steps:.3f} ms per step", flush=True)
        b.close(); m.close()
        continue
    base = float("nan")
    if not args.batch_sizes:
        m.prefill(prompt(args.ctx, 100))
        m.decode(8)
        base, raw = median_ms(m.decode, m.last_decode_ms, args.steps, args.windows)
        row = {"format": fmt, "B": "single", "ctx": args.ctx, "ms_per_step": base, "tok_s": 1e3 / base, "ratio": 1.0, "windows_ms": raw}
        print(json.dumps(row), flush=True)
        table.append(row)
    runs = [(B, [args.ctx] * B) for B in (1, 2, 4, 8)] + [(8, [args.ctx * (i + 1) // 8 for i in range(8)])]
    if args.batch_sizes:
        runs = [(B, [args.ctx] * B) for B in args.batch_sizes]
    for B, ctxs in runs:
        slots = list(range(B))
        for s in slots:
            b.reset(s)
            b.prefill(s, prompt(ctxs[s], s))
        b.decode(8, slots)
        ms, raw = median_ms(lambda n: b.decode(n, slots), b.last_decode_ms, args.steps, args.windows)
        ragged = len(set(ctxs)) > 1
        row = {"format": fmt, "B": B, "ctx": f"{ctxs[0]}..{ctxs[-1]}" if ragged else args.ctx, "ms_per_step": ms, "tok_s": B * 1e3 / ms,
               "ratio": B * base / ms, "windows_ms": raw, "sampler": sampler}
        print(json.dumps(row), flush=True)
        table.append(row)
    b.close(); m.close()

if table:
    print(f"\n{'format':<12} {'B':>6} {'context':>10} {'ms/step':>9} {'tok/s':>9} {'x single':>9}")
    for r in table:
        print(f"{r['format']:<12} {str(r['B']):>6} {str(r['ctx']):>10} {r['ms_per_step']:>9.3f} {r['tok_s']:>9.1f} {r['ratio']:>9.2f}")
