"""qwen3-mlx/examples/generate_qwen3.rs on the MI355X engine:
    python tools/generate_qwen3.py <model_dir> [prompt] [--temperature T] [--top-k K] [--top-p P] [--repetition-penalty R]
                                   [--presence-penalty Q] [--seed S] [--max-tokens N]
    python tools/generate_qwen3.py <model_dir> --prompts-file FILE [--slots N] [--temperature T] [--seed S] [--max-tokens N] [--kv-bits 8]
    python tools/generate_qwen3.py <model_dir> [prompt] --samples N [--temperature T] [--seed S] [--max-tokens N] [--kv-bits 8]
(the filter flags --top-k / --top-p / --repetition-penalty / --presence-penalty apply to all three forms)
--prompts-file: one prompt per line, decoded together over N slots of one loaded model (engine.Batch), every slot with these settings.
--samples N: N completions (1..8) of the prompt -- or of every line of --prompts-file -- from ONE prefill: the prompt's slot is forked
N - 1 times (Batch.fork); sibling i of every prompt draws with a fresh key sequence of seed S + i (Batch.set_sampler before its fork).
--kv-bits 8 (the two batched forms): the batch keeps its K/V cache as 8-bit MLX affine rows (MLX's kv_bits; 0 = bf16, the default).
Without flags: the example's plain temperature 0.7.  The Qwen3 model card's settings are --temperature 0.6 --top-k 20 --top-p 0.95."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import
omx_import.load_package()
from ominix_mlx_amd import generate, loader

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("model_dir")
ap.add_argument("prompt", nargs="?", default="Hello, I am a language model,")
ap.add_argument("--temperature", type=float, default=0.7)
ap.add_argument("--top-k", type=int, default=0, help="keep the k most likely tokens, ties included (0 = off)")
ap.add_argument("--top-p", type=float, default=1.0, help="nucleus mass on the survivors of top-k (1 = off)")
ap.add_argument("--repetition-penalty", type=float, default=1.0, help="x > 0 ? x / r : x * r on generated tokens (1 = off)")
ap.add_argument("--presence-penalty", type=float, default=0.0, help="x - q on generated tokens (0 = off)")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--max-tokens", type=int, default=100)
ap.add_argument("--prompts-file", help="one prompt per line: all of them through generate_batch over --slots slots")
ap.add_argument("--slots", type=int, default=8, help="sequences decoded together (1..8)")
ap.add_argument("--samples", type=int, default=1, help="completions per prompt from one prefill (1..8)")
ap.add_argument("--kv-bits", type=int, default=0, choices=[0, 8], help="K/V cache of the batched forms: 0 = bf16, 8 = 8-bit rows")
args = ap.parse_args()
if not 1 <= args.samples <= 8:
    ap.error("--samples must be 1..8")
if args.kv_bits and not (args.prompts_file or args.samples > 1):
    ap.error("--kv-bits applies to --prompts-file and --samples (the batched forms)")
tokenizer = generate.load_tokenizer(args.model_dir)
model = loader.load_model(args.model_dir)
if args.prompts_file or args.samples > 1:
    import json, time
    if args.prompts_file:
        with open(args.prompts_file, encoding="utf-8") as fh:
            texts = [ln.rstrip("\n") for ln in fh if ln.strip()]
    else:
        texts = [args.prompt]
    prompts = [list(tokenizer.encode(t, add_special_tokens=True).ids) for t in texts]
    eos = []
    gen_cfg = os.path.join(args.model_dir, "generation_config.json")
    if os.path.exists(gen_cfg):
        e = json.load(open(gen_cfg)).get("eos_token_id", [])
        eos = [int(t) for t in (e if isinstance(e, list) else [e])]
    n = args.samples
    filters = dict(top_k=args.top_k, top_p=args.top_p, repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty)
    batch = model.batch(max(n, min(args.slots, len(prompts) * n)), kv_bits=args.kv_bits)
    if n == 1:
        for slot in range(batch.n_slots):
            batch.set_sampler(slot, args.temperature, args.seed + slot, **filters)
    start = time.perf_counter()
    # --samples: sibling i of EVERY prompt starts a fresh key sequence of seed + i, set on its slot right before its prefill / fork, so
    # a prompt's samples do not depend on where it stands in the file or on which slots were free
    outs = generate.generate_batch(batch, prompts, args.max_tokens, eos_ids=eos, n=n, before_sibling=None if n == 1 else
                                   lambda p, k, slot: batch.set_sampler(slot, args.temperature, args.seed + k, **filters))
    seconds = time.perf_counter() - start
    for i, toks in enumerate(outs):
        head = f"Prompt: {texts[i // n]}" + (f"  [sample {i % n}]" if n > 1 else "")
        print(f"{head}\n---\n{tokenizer.decode(toks, skip_special_tokens=True)}\n===")
    total = sum(len(t) for t in outs)
    print(f"Generated {total} tokens for {len(prompts)} prompts over {batch.n_slots} slots in {seconds:.2f}s ({total / seconds:.1f} tok/s)")
    sys.exit(0)
print(f"Prompt: {args.prompt}\n---")
out = generate.generate_text(model, tokenizer, args.prompt, temperature=args.temperature, max_tokens=args.max_tokens, seed=args.seed,
                             emit=lambda t: print(t, end="", flush=True), top_k=args.top_k, top_p=args.top_p,
                             repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty)
print(f"\n---\nGenerated {len(out['tokens'])} tokens in {out['seconds']:.2f}s ({out['tokens_per_sec']:.1f} tok/s)")
