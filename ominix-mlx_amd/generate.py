"""Generation front-end either side of the decode engine, host side only:

    load_tokenizer                       mlx-rs-core/src/lib.rs:73-76 (HF `tokenizer.json` through the `tokenizers` library)
    load_model_chat_template_from_*      mlx-rs/mlx-lm-utils/src/tokenizer.rs:242-258 (`chat_template` of tokenizer_config.json)
    apply_chat_template                  tokenizer.rs:430-530 (Jinja render of `messages`, add_generation_prompt,
                                         continue_final_message; the reference uses minijinja + pycompat, this uses jinja2)
    generate_text                        qwen3-mlx/examples/generate_qwen3.rs:31-101 (encode with special tokens,
                                         Generate at `temperature`, decode + emit every 10 tokens, flush the rest)

    generate_batch                       many prompts over the slots of an `engine.Batch` (the reference batches through the [B, L]
                                         ids of Model::forward; here the sequences are ragged and retire one by one)
    perplexity                           the strided log-likelihood evaluation of a token sequence over `engine.Model.score` (the
                                         reference's Model::forward returns the [B, L, V] logits it would be taken from)

The model side is `engine.Model` / `engine.Generate` / `engine.Batch` (the HIP decode engine); nothing here touches the GPU."""
from __future__ import annotations

import json
import os
import time
from typing import Callable, Iterable, List, Optional, Sequence


def load_tokenizer(model_dir):
    from tokenizers import Tokenizer
    path = os.path.join(os.fspath(model_dir), "tokenizer.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"Tokenizer: {path} not found")
    return Tokenizer.from_file(path)


def load_model_chat_template_from_str(content: str) -> Optional[str]:
    value = json.loads(content)
    tpl = value.get("chat_template") if isinstance(value, dict) else None
    return tpl if isinstance(tpl, str) else None


def load_model_chat_template_from_file(path) -> Optional[str]:
    with open(path, "r", encoding="utf-8") as fh:
        return load_model_chat_template_from_str(fh.read())


_ENV = None


def _jinja_env():
    global _ENV
    if _ENV is None:
        import jinja2
        from jinja2.sandbox import ImmutableSandboxedEnvironment

        def raise_exception(message):
            raise jinja2.exceptions.TemplateError(message)

        _ENV = ImmutableSandboxedEnvironment(trim_blocks=True, lstrip_blocks=True)
        _ENV.globals["raise_exception"] = raise_exception
        _ENV.filters["tojson"] = lambda x, **kw: json.dumps(x, ensure_ascii=False, **{k: v for k, v in kw.items() if k == "indent"})
    return _ENV


def apply_chat_template(model_template: str, conversations: Sequence[Sequence[dict]], documents=None,
                        add_generation_prompt: Optional[bool] = None, continue_final_message: Optional[bool] = None) -> List[str]:
    """One rendered string per conversation (a conversation = list of {"role", "content"} messages)."""
    add_generation_prompt = bool(add_generation_prompt)
    continue_final_message = bool(continue_final_message)
    if add_generation_prompt and continue_final_message:
        raise ValueError("continue_final_message and add_generation_prompt are not compatible")
    template = _jinja_env().from_string(model_template)
    out = []
    for chat in conversations:
        chat = [dict(m) for m in chat]
        rendered = template.render(messages=chat, documents=documents, add_generation_prompt=add_generation_prompt)
        if continue_final_message:
            final = str(chat[-1]["content"])
            loc = rendered.rfind(final.strip())
            if loc < 0:
                raise ValueError("continue_final_message is set but the final message does not appear in the chat after "
                                 "applying the chat template")
            keep = len(final.lstrip())
            # the template kept the message's trailing spacing (or it has none): cut after it; otherwise after the trimmed text
            rendered = rendered[:loc + keep] if rendered[loc:loc + keep] == final else rendered[:loc + len(final.strip())]
        out.append(rendered)
    return out


def apply_chat_template_and_encode(tokenizer, model_template: str, conversations, **kw):
    """tokenizer.rs:128-160: render, then encode each string WITHOUT adding special tokens (the template wrote them)."""
    return [tokenizer.encode(text, add_special_tokens=False) for text in apply_chat_template(model_template, conversations, **kw)]


def generate_text(model, tokenizer, prompt: str, temperature: float = 0.7, max_tokens: int = 100, seed: int = 0,
                  emit: Optional[Callable[[str], None]] = None, flush_every: int = 10,
                  stop_token_ids: Optional[Iterable[int]] = None, prompt_ids: Optional[Sequence[int]] = None, *, top_k: int = 0,
                  top_p: float = 1.0, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                  logprobs: Optional[int] = None) -> dict:
    """generate_qwen3.rs:31-101.  Returns {"text", "tokens", "prompt_tokens", "seconds", "tokens_per_sec"}; `emit` receives
    each decoded chunk as the example prints it.  `stop_token_ids` (not in the example, which always runs max_tokens)
    ends the stream after such a token.  top_k / top_p / repetition_penalty / presence_penalty: Model.set_sampler's filters (off by default).
    logprobs = k (0..20): the dict also has "logprobs" (a float per token) and "top_logprobs" (per token, its k alternatives as
    (id, logprob) pairs, best first), from the model's raw logits (Model.set_logprobs)."""
    from .engine import Generate
    ids = list(prompt_ids) if prompt_ids is not None else list(tokenizer.encode(prompt, add_special_tokens=True).ids)
    if not ids:
        raise ValueError("generate_text: the prompt encodes to no tokens")
    stop = set(int(t) for t in stop_token_ids) if stop_token_ids is not None else set()
    start = time.perf_counter()
    pending: List[int] = []
    all_tokens: List[int] = []
    pieces: List[str] = []

    def flush():
        if pending:
            text = tokenizer.decode(pending, skip_special_tokens=True)
            pieces.append(text)
            if emit is not None:
                emit(text)
            pending.clear()

    more = {} if logprobs is None else {"logprobs": int(logprobs)}
    gen = Generate(model, temperature, ids, chunk=flush_every, seed=seed, top_k=top_k, top_p=top_p,
                   repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, **more)
    for i, token in enumerate(gen):
        token = int(token)
        pending.append(token)
        all_tokens.append(token)
        if len(pending) % flush_every == 0:
            flush()
        if token in stop or i >= max_tokens - 1:
            break
    flush()
    seconds = time.perf_counter() - start
    out = {"text": "".join(pieces), "tokens": all_tokens, "prompt_tokens": len(ids), "seconds": seconds,
           "tokens_per_sec": len(all_tokens) / seconds if seconds > 0 else 0.0}
    if logprobs is not None:
        out["logprobs"], out["top_logprobs"] = list(gen.logprobs), list(gen.top_logprobs)
    return out


def generate_batch(batch, prompts: Sequence[Sequence[int]], max_new_tokens: int, eos_ids: Iterable[int] = (), chunk: int = 16,
                   n: int = 1, before_sibling=None, return_logprobs: bool = False, best_of: Optional[int] = None):
    """Any number of token-id prompts over the slots of an `engine.Batch`: free slots are prefilled with waiting prompts, the active
    slots decode together `chunk` tokens at a time, a sequence retires at its first token in `eos_ids` (which it keeps) or at
    max_new_tokens -- what its slot decoded past that point inside the chunk is dropped -- and its slot is reset and handed to the next
    waiting prompt.  Returns the generated tokens per prompt, in prompt order.  Drives `batch` through prefill / decode / reset and,
    with n > 1, fork.
    n > 1: n completions of every prompt.  A prompt starts when n slots are free; it is prefilled ONCE and its slot forked n - 1 times,
    every sibling drawing its first token from the prompt's logits with its own slot's sampler (`Batch.fork`).  A forked sibling's
    slot is reset and free again as soon as it retires.  The prompt's own slot stops decoding when its sequence retires but is reset
    only after its last sibling has: resetting the owner ends what its children share with it (`Batch.shared`).  Returns n lists per
    prompt, prompt-major: completion k of prompt i is [i * n + k].
    before_sibling(i, k, slot), if given, is called before completion k of prompt i is prefilled (k = 0) or forked into `slot` --
    the place to give the slot its sampler (`Batch.set_sampler(slot, temperature, seed + k)`).
    Samplers are the caller's: whatever `Batch.set_sampler` was given per slot -- its top_k / top_p / repetition_penalty /
    presence_penalty filters included -- applies to the prefill's first token, to a fork's and to every decoded one; a slot's penalty
    history starts empty at its prefill or fork and is cleared by the reset that frees the slot.
    return_logprobs: returns (outputs, logprobs), logprobs[i][t] being the log-probability of outputs[i][t] under the model's raw
    logits (`Batch.set_logprobs`, switched on with no alternatives if the batch has it off), truncated with the tokens.
    best_of = m (n <= m <= batch.n_slots): m siblings are forked per prompt and the n with the highest mean token log-probability are
    returned, best first, ties going to the lower sibling index."""
    if max_new_tokens < 1 or chunk < 1:
        raise ValueError("generate_batch: max_new_tokens and chunk must be positive")
    if n < 1 or n > batch.n_slots:
        raise ValueError(f"generate_batch: n = {n} completions per prompt need 1..{batch.n_slots} slots")
    if best_of is not None and not n <= best_of <= batch.n_slots:
        raise ValueError(f"generate_batch: best_of = {best_of} must be in n = {n}..{batch.n_slots} (the batch's slots)")
    keep, n = n, (n if best_of is None else int(best_of))   # from here on n = the siblings decoded per prompt
    with_lp = return_logprobs or best_of is not None
    if with_lp and batch.logprobs_top is None:
        batch.set_logprobs(0)
    eos = set(int(t) for t in eos_ids)
    outputs: List[List[int]] = [[] for _ in range(len(prompts) * n)]
    logprobs: List[List[float]] = [[] for _ in range(len(prompts) * n)]
    waiting = list(range(len(prompts)))
    free = list(range(batch.n_slots))
    active = {}                                   # slot -> output index
    owner = {}                                    # prompt index -> the slot it was prefilled in, until its last sibling retires
    left = {}                                     # prompt index -> siblings still decoding

    def finished(i):
        return len(outputs[i]) >= max_new_tokens or (outputs[i] and outputs[i][-1] in eos)

    def release(slot):
        batch.reset(slot)
        free.append(slot)

    def retire(slot, i):
        del active[slot]
        p = i // n
        if slot != owner[p]:
            release(slot)
        left[p] -= 1
        if left[p] == 0:
            release(owner.pop(p))

    while waiting or active:
        while waiting and len(free) >= n:
            p = waiting.pop(0)
            if len(prompts[p]) == 0:
                raise ValueError(f"generate_batch: prompt {p} is empty")
            slots = [free.pop(0) for _ in range(n)]
            owner[p], left[p] = slots[0], n
            for k, slot in enumerate(slots):
                if before_sibling is not None:
                    before_sibling(p, k, slot)
                first = batch.prefill(slot, prompts[p]) if k == 0 else batch.fork(slots[0], slot, True)
                outputs[p * n + k].append(int(first))
                if with_lp:
                    last = batch.last_logprobs(slot)
                    logprobs[p * n + k].append(float(last[0] if isinstance(last, tuple) else last))
                active[slot] = p * n + k
            for k, slot in reversed(list(enumerate(slots))):   # (the owner last: it is released with its last sibling)
                if finished(p * n + k):           # EOS as the first token, or max_new_tokens == 1
                    retire(slot, p * n + k)
        if not active:
            continue
        slots = sorted(active)
        steps = min(chunk, min(max_new_tokens - len(outputs[active[s]]) for s in slots))
        tokens, lps = batch.decode(steps, slots, return_logprobs=True)[:2] if with_lp else (batch.decode(steps, slots), None)
        for col, slot in enumerate(slots):
            i = active[slot]
            for step in range(steps):
                outputs[i].append(int(tokens[step][col]))
                if with_lp:
                    logprobs[i].append(float(lps[step][col]))
                if finished(i):
                    break
            if finished(i):
                retire(slot, i)
    if best_of is not None:
        order = []
        for p in range(len(prompts)):
            mean = lambda i: sum(logprobs[i]) / len(logprobs[i])
            ranked = sorted(range(p * n, p * n + n), key=lambda i: (-mean(i), i))   # best first, ties to the lower sibling index
            order.extend(ranked[:keep])
        outputs, logprobs = [outputs[i] for i in order], [logprobs[i] for i in order]
    return (outputs, logprobs) if return_logprobs else outputs


def perplexity(model, ids: Sequence[int], ctx: int = 2048, stride: Optional[int] = None) -> dict:
    """Perplexity of a token sequence, the standard strided evaluation: windows ids[b : b + ctx] at b = 0, stride, 2 stride, ... each
    scored from an empty cache (model.reset(), then ONE model.score pass; the token behind the window, where the text has one, is the
    target of the window's last position), and of every window only the targets no earlier window counted enter the sum -- so each of
    the len(ids) - 1 targets is counted exactly once, conditioned on at least ctx - stride + 1 tokens where the text has them.  stride
    defaults to ctx (windows side by side).  Returns {"tokens": targets counted, "nll": their summed negative log-likelihood in nats,
    "ppl": exp(nll / tokens)}.  Pure host logic over model.reset / model.score."""
    import math
    ids = [int(t) for t in ids]
    stride = ctx if stride is None else int(stride)
    if len(ids) < 2:
        raise ValueError("perplexity: a text of at least 2 tokens is needed (the first token has no context to be predicted from)")
    if ctx < 1 or stride < 1 or stride > ctx:
        raise ValueError(f"perplexity: ctx = {ctx} must be positive and stride = {stride} in 1..ctx")
    n = len(ids)
    nll, done, begin = 0.0, 0, 0            # done: the targets ids[1 .. done] are counted (ids[0] is nobody's target)
    while done < n - 1:
        end = min(begin + ctx, n)
        model.reset()
        # lp[i] = log p(ids[begin + i + 1] | ids[begin : begin + i + 1]); with a token behind the window, also the last position's
        lp = model.score(ids[begin:end], next_token=ids[end] if end < n else None)
        last = min(end, n - 1)
        for t in range(done + 1, last + 1):
            nll -= float(lp[t - begin - 1])
        done = last
        begin += stride
    return {"tokens": n - 1, "nll": nll, "ppl": math.exp(nll / (n - 1))}
