"""qwen3-mlx/examples/generate_qwen3.rs on the MI355X engine:
    python tools/generate_qwen3.py <model_dir> [prompt] [--temperature T] [--top-k K] [--top-p P] [--repetition-penalty R]
                                   [--presence-penalty Q] [--seed S] [--max-tokens N]
    python tools/generate_qwen3.py <model_dir> --prompts-file FILE [--slots N] [--temperature T] [--seed S] [--max-tokens N] [--kv-bits 8]
    python tools/generate_qwen3.py <model_dir> [prompt] --samples N [--temperature T] [--seed S] [--max-tokens N] [--kv-bits 8]
(the filter flags --top-k / --top-p / --repetition-penalty / --presence-penalty apply to all three forms)
--logprobs K (0..20): print every generated token's log-probability under the model's raw logits and its K most likely alternatives.
--best-of M (beside --samples N, N <= M <= 8): M siblings are forked per prompt, the N with the highest mean token log-probability shown.
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
ap.add_argument("--logprobs", type=int, default=None, help="report each token's log-probability and K alternatives (0..20)")
ap.add_argument("--best-of", type=int, default=None, help="fork M siblings per prompt, keep the --samples best by mean log-probability")
args = ap.parse_args()
if args.best_of is not None and not args.samples <= args.best_of <= 8:
    ap.error("--best-of must be in --samples..8")
if args.logprobs is not None and not 0 <= args.logprobs <= 20:
    ap.error("--logprobs must be 0..20")
if not 1 <= args.samples <= 8:
    ap.error("--samples must be 1..8")
batched = bool(args.prompts_file) or args.samples > 1 or args.best_of is not None
if args.kv_bits and not batched:
    ap.error("--kv-bits applies to --prompts-file and --samples (the batched forms)")
tokenizer = generate.load_tokenizer(args.model_dir)
model = loader.load_model(args.model_dir)
if batched:
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
    n, m = args.samples, args.best_of or args.samples   # completions shown / siblings decoded per prompt
    filters = dict(top_k=args.top_k, top_p=args.top_p, repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty)
    batch = model.batch(max(m, min(args.slots, len(prompts) * m)), kv_bits=args.kv_bits)
    if args.logprobs is not None:
        batch.set_logprobs(0)   # (the batched forms print each token's log-probability; alternatives are the single-prompt form's)
    if m == 1:
        for slot in range(batch.n_slots):
            batch.set_sampler(slot, args.temperature, args.seed + slot, **filters)
    start = time.perf_counter()
    # --samples: sibling i of EVERY prompt starts a fresh key sequence of seed + i, set on its slot right before its prefill / fork, so
    # a prompt's samples do not depend on where it stands in the file or on which slots were free
    with_lp = args.logprobs is not None or args.best_of is not None
    outs = generate.generate_batch(batch, prompts, args.max_tokens, eos_ids=eos, n=n, before_sibling=None if m == 1 else
                                   lambda p, k, slot: batch.set_sampler(slot, args.temperature, args.seed + k, **filters),
                                   return_logprobs=with_lp, best_of=args.best_of)
    outs, lps = outs if with_lp else (outs, None)
    seconds = time.perf_counter() - start
    for i, toks in enumerate(outs):
        head = f"Prompt: {texts[i // n]}" + (f"  [sample {i % n}]" if n > 1 else "")
        if lps is not None:
            head += f"  [mean logprob {sum(lps[i]) / len(lps[i]):.4f}]"
        print(f"{head}\n---\n{tokenizer.decode(toks, skip_special_tokens=True)}\n===")
        if args.logprobs is not None:
            print(" ".join(f"{t}:{v:.4f}" for t, v in zip(toks, lps[i])) + "\n===")
    total = sum(len(t) for t in outs)
    print(f"Generated {total} tokens for {len(prompts)} prompts over {batch.n_slots} slots in {seconds:.2f}s ({total / seconds:.1f} tok/s)")
    sys.exit(0)
print(f"Prompt: {args.prompt}\n---")
out = generate.generate_text(model, tokenizer, args.prompt, temperature=args.temperature, max_tokens=args.max_tokens, seed=args.seed,
                             emit=lambda t: print(t, end="", flush=True), top_k=args.top_k, top_p=args.top_p,
                             repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty, logprobs=args.logprobs)
print(f"\n---\nGenerated {len(out['tokens'])} tokens in {out['seconds']:.2f}s ({out['tokens_per_sec']:.1f} tok/s)")
if args.logprobs is not None:
    for tok, lp, alts in zip(out["tokens"], out["logprobs"], out["top_logprobs"]):
        shown = "  ".join(f"{tokenizer.decode([i], skip_special_tokens=False)!r} {v:.4f}" for i, v in alts)
        print(f"{tokenizer.decode([tok], skip_special_tokens=False)!r:>16} {lp:9.4f}" + (f"   | {shown}" if alts else ""))
