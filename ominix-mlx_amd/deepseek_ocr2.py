"""The vision side of DeepSeek-OCR-2 on the device (deepseek-ocr2-mlx/src/lib.rs `DeepseekOCR2::encode_image`, :467-497): views -> SAM
ViT-B tower (float32, csrc/sam_encoder.hip) -> visual-causal-flow encoder (csrc/vcf_encoder.hip) -> Linear projector -> the rows that
`prepare_inputs` scatters over the image placeholders, the learned separator row last -- and `DeepseekOCR2`, those rows into the language
decoder (a DeepSeek-V2 style MoE on engine.Model, moe_mode="deepseek"): prompt layout, scatter, the prompt pass over caller rows, the
reference's `Generate` loop.  Host logic only; every hot path is a device call of vision.py / engine.py."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np

from . import OmxError, check, lib

SAM_PREFIX, VCF_PREFIX = "model.sam_model", "model.qwen2_model"                   # load_model (lib.rs:959-965)
PROJECTOR_WEIGHT, PROJECTOR_BIAS, SEPARATOR = "model.projector.layers.weight", "model.projector.layers.bias", "model.view_seperator"
SAM_DEFAULTS = dict(embed_dim=768, depth=12, num_heads=12, mlp_dim=3072, window=14, global_attn_indexes=(2, 5, 8, 11), patch_size=16)
VCF_DEFAULTS = dict(hidden=896, layers=24, heads=14, kv_heads=2, intermediate=4864, rope_theta=1e6, eps=1e-6)
MAX_CROPS = 6                                                                     # find_best_crop_ratio(w, h, 2, 6)


def find_best_crop_ratio(width: int, height: int, min_num: int, max_num: int) -> Tuple[int, int]:
    """lib.rs:873-900: the (columns, rows) whose aspect is nearest the image's among min_num <= columns * rows <= max_num; the first
    candidate in the reference's loop order wins a tie"""
    aspect = float(width) / float(height)
    best, best_diff = (1, 1), float("inf")
    for n in range(min_num, max_num + 1):
        for i in range(1, n + 1):
            for j in range(1, n + 1):
                if min_num <= i * j <= max_num:
                    diff = abs(aspect - float(i) / float(j))
                    if diff < best_diff:
                        best_diff, best = diff, (i, j)
    return best


def image_token_count(base_size: int, image_size: int, crop_ratio, patch_size: int = 16, downsample_ratio: int = 4) -> int:
    """tokenize_prompt (lib.rs:823-843): (base / 64)^2 rows of the global view, the separator, and (image_size / 64)^2 per crop when the
    ratio is not (1, 1)"""
    nb, nq = base_size // patch_size // downsample_ratio, image_size // patch_size // downsample_ratio
    w, h = crop_ratio
    return nb * nb + 1 + (nq * w * nq * h if (w > 1 or h > 1) else 0)


def row_plan(base_size: int, image_size: int = 0, n_crops: int = 0, patch_size: int = 16, downsample_ratio: int = 4):
    """where each view's rows lie in what encode_image returns (lib.rs:487-493): [(name, first row, rows)] -- "crop<i>" in the order
    given, "global", "separator" -- with the row counts tokenize_prompt assumes, (size / 64)^2 per view"""
    nb, nq = base_size // patch_size // downsample_ratio, (image_size // patch_size // downsample_ratio) if n_crops else 0
    plan, at = [], 0
    for i in range(n_crops):
        plan.append((f"crop{i}", at, nq * nq))
        at += nq * nq
    plan.append(("global", at, nb * nb))
    plan.append(("separator", at + nb * nb, 1))
    return plan


def image_array(image) -> np.ndarray:
    """[..., S, S, 3] float in [-1, 1] as it is, or uint8 mapped by v / 127.5 - 1 in float32 (examples/infer.rs:97-100); resizing is
    the caller's"""
    a = np.asarray(image)
    if a.ndim < 3 or a.shape[-1] != 3 or a.shape[-2] != a.shape[-3]:
        raise OmxError(f"ShapeMismatch: image has shape {a.shape}, [S, S, 3] is expected")
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a.astype(np.float32) / np.float32(127.5) - np.float32(1.0))
    if a.dtype.kind != "f":
        raise OmxError(f"image dtype {a.dtype}: uint8 or floating point in [-1, 1]")
    return np.ascontiguousarray(a, dtype=np.float32)


def _behind(weights: Dict[str, np.ndarray], prefix: str) -> Dict[str, np.ndarray]:
    return {k[len(prefix) + 1:]: v for k, v in weights.items() if k.startswith(prefix + ".")}


class DeepEncoder:
    """`load(model_dir)` / `from_weights(dict, sam_cfg, vcf_cfg)`; `encode_image(global_image, crops=None)` -> device f32 [n, out_dim]."""

    def __init__(self, sam, vcf, proj_w, proj_b, separator):
        self.sam, self.vcf, self.proj_w, self.proj_b, self.separator = sam, vcf, proj_w, proj_b, separator
        self.out_dim, self.hidden = proj_w.shape
        if self.hidden != vcf.cfg.hidden or proj_b.size != self.out_dim or separator.size != self.out_dim:
            raise OmxError(f"ShapeMismatch: projector {proj_w.shape} / bias {proj_b.shape} / separator {separator.shape} against an encoder of {vcf.cfg.hidden}")

    @staticmethod
    def from_weights(weights: Dict[str, np.ndarray], sam_cfg: Optional[dict] = None, vcf_cfg: Optional[dict] = None, keep_stages: bool = False) -> "DeepEncoder":
        """weights under the checkpoint's full names (model.sam_model.*, model.qwen2_model.*, model.projector.layers.{weight,bias},
        model.view_seperator); the configs default to the reference's"""
        from . import ops, vision
        for key in (PROJECTOR_WEIGHT, PROJECTOR_BIAS, SEPARATOR):
            if key not in weights:
                raise OmxError(f"WeightNotFound: {key}")
        sam = vision.SamEncoder(**dict(SAM_DEFAULTS, **(sam_cfg or {})), prefix=SAM_PREFIX, keep_stages=keep_stages)
        sam.load_weights(_behind(weights, SAM_PREFIX))
        vcf = vision.VisualCausalEncoder(**dict(VCF_DEFAULTS, **(vcf_cfg or {})), prefix=VCF_PREFIX, keep_stages=keep_stages)
        vcf.load_weights(_behind(weights, VCF_PREFIX))
        T = lambda k: ops.Tensor.from_numpy(vision.widen(weights[k]), "f32")
        pw = T(PROJECTOR_WEIGHT)
        if len(pw.shape) != 2:
            raise OmxError(f"ShapeMismatch: {PROJECTOR_WEIGHT} is not a matrix")
        return DeepEncoder(sam, vcf, pw, T(PROJECTOR_BIAS), T(SEPARATOR))

    @staticmethod
    def load(model_dir: str) -> "DeepEncoder":
        """the vision tensors of load_model (lib.rs:946-974), read through loader.py's safetensors reader"""
        from . import loader
        weights = loader.load_all_weights(model_dir)
        keep = (SAM_PREFIX + ".", VCF_PREFIX + ".", "model.projector.", SEPARATOR)
        return DeepEncoder.from_weights({k: v for k, v in weights.items() if k.startswith(keep)})

    def close(self) -> None:
        self.sam.close()
        self.vcf.close()

    def rows_for(self, image_size: int) -> int:
        """rows one view of that size contributes"""
        _, n_img, _ = self.sam.tokens(image_size)
        return self.vcf.tokens(n_img)[0]

    def _views(self, images, rows, row: int) -> int:
        """stacked views of one size -> their query rows into rows[row:]; returns the count"""
        from . import ops
        t = images if isinstance(images, ops.Tensor) else ops.Tensor.from_numpy(images, "f32")
        feat = self.sam.forward(t)
        self.vcf.forward(feat, images=t.shape[0], out=rows, row=row)
        return t.shape[0] * self.rows_for(t.shape[1])

    def encode_image(self, global_image, crops=None):
        """encode_image (lib.rs:467-497): the crops' rows in the order given (all crops in ONE stacked pass), the global view's rows, the
        separator.  global_image [S, S, 3], crops [n, s, s, 3] (n <= 6) or None; float in [-1, 1] or uint8."""
        from . import ops
        g = image_array(global_image)
        if g.ndim != 3:
            raise OmxError(f"ShapeMismatch: the global view has shape {g.shape}, [S, S, 3] is expected")
        c = None
        if crops is not None and len(crops):
            c = image_array(crops)
            if c.ndim != 4:
                raise OmxError(f"ShapeMismatch: crops have shape {c.shape}, [n, S, S, 3] is expected")
            if c.shape[0] > MAX_CROPS:
                raise OmxError(f"InvalidConfig: {c.shape[0]} crops (at most {MAX_CROPS}: find_best_crop_ratio(w, h, 2, 6))")
        n = self.rows_for(g.shape[0]) + (c.shape[0] * self.rows_for(c.shape[1]) if c is not None else 0)
        plan = row_plan(g.shape[0], c.shape[1] if c is not None else 0, c.shape[0] if c is not None else 0, self.sam.cfg.patch_size)
        if plan[-1][1] != n:
            raise OmxError(f"ShapeMismatch: the query tables make {n} rows for these views, the prompt's placeholders assume {plan[-1][1]}")
        rows = ops.Tensor((n, self.hidden), "f32")
        at = self._views(c, rows, 0) if c is not None else 0
        at += self._views(g[None], rows, at)
        out = ops.Tensor((n + 1, self.out_dim), "f32")
        check(lib.omx_gemm_f32_epilogue(out.ptr, rows.ptr, self.proj_w.ptr, self.proj_b.ptr, None, None, n, self.out_dim, self.hidden, 0, None))
        check(lib.omx_memcpy_d2d(ctypes.c_void_p(out.ptr + 4 * n * self.out_dim), ctypes.c_void_p(self.separator.ptr), 4 * self.out_dim, None))
        return out

    def launches(self) -> int:
        """of the last view that went through the towers, + the projector's one"""
        return self.sam.launches() + self.vcf.launches() + 1


IMAGE_TOKEN_ID, BOS_TOKEN_ID, EOS_TOKEN_ID = 128815, 0, 1                         # lib.rs:787, :129-130


def _encode(tokenizer, text: str):
    """ids of `text` without special tokens: a `tokenizers.Tokenizer` (encode(text, False).ids) or any callable / object with
    encode(text) -> list of ids"""
    if callable(tokenizer) and not hasattr(tokenizer, "encode"):
        return [int(t) for t in tokenizer(text)]
    try:
        enc = tokenizer.encode(text, False)
    except TypeError:
        enc = tokenizer.encode(text)
    return [int(t) for t in (enc.ids if hasattr(enc, "ids") else enc)]


def tokenize_prompt(tokenizer, prompt: str, has_image: bool, base_size: int, image_size: int, crop_ratio=(1, 1),
                    image_token_id: int = IMAGE_TOKEN_ID):
    """tokenize_prompt (lib.rs:791-870), literally: the text is framed as "<|User|>: {prompt}\n\n<|Assistant|>:" and split at "<image>";
    with an image and a placeholder, the ids are [text before] [IMAGE_TOKEN_ID x (base / 64)^2: the global view] [one more: the separator]
    [x (image_size / 64)^2 * w * h: the crops, when the ratio is not (1, 1)] [text after, further "<image>" kept as text]; otherwise the
    whole frame as text.  BOS (0) goes in front.  -> (ids, mask), mask True over the image span.  (image_token_id: a model with a smaller
    vocabulary than the checkpoint's names its own placeholder; the engine checks every id against the vocabulary.)

    The id sequence lists the global block, the separator, then the crops; the ROWS that `encode_image` returns are in another order --
    crops, global view, separator -- and `prepare_inputs` lays them over the span in the order they come.  That is the reference's own
    behaviour (every placeholder carries the same id, so only the count matters to it); it is kept, not corrected."""
    formatted = f"<|User|>: {prompt}\n\n<|Assistant|>:"
    splits = formatted.split("<image>")
    ids, mask = [], []
    if has_image and len(splits) > 1:
        pre = _encode(tokenizer, splits[0])
        ids += pre
        mask += [False] * len(pre)
        n = image_token_count(base_size, image_size, crop_ratio)
        ids += [int(image_token_id)] * n
        mask += [True] * n
        post = _encode(tokenizer, "<image>".join(splits[1:]))
        ids += post
        mask += [False] * len(post)
    else:
        ids = _encode(tokenizer, formatted)
        mask = [False] * len(ids)
    return [BOS_TOKEN_ID] + ids, [False] + mask


def image_span(mask) -> Tuple[int, int]:
    """(first position, length) of the image span of a tokenize_prompt mask -- (0, 0) without one.  tokenize_prompt writes ONE
    contiguous run, so the scatter is one block of rows; anything else is refused."""
    m = np.asarray(mask, dtype=bool)
    on = np.flatnonzero(m)
    if on.size == 0:
        return 0, 0
    if on[-1] - on[0] + 1 != on.size:
        raise OmxError("InvalidConfig: the image placeholders are not one contiguous span")
    return int(on[0]), int(on.size)


def is_repeating(tokens) -> bool:
    """Generate::is_repeating (lib.rs:675-698): from 12 generated tokens on, true when the last n tokens (n = 4 .. min(32, len / 3))
    stand three times in a row at the end"""
    t = [int(v) for v in tokens]
    n_tok = len(t)
    if n_tok < 12:
        return False
    for n in range(4, min(32, n_tok // 3) + 1):
        tail, repeats, pos = t[n_tok - n:], 1, n_tok - n
        while pos >= n:
            pos -= n
            if t[pos:pos + n] != tail:
                break
            repeats += 1
            if repeats >= 3:
                return True
    return False


def penalty_window(generated, repetition_context_size: int):
    """the tokens the repetition penalty sees (lib.rs:631-639): the last repetition_context_size generated ones (all of them when the size
    is 0 or not yet exceeded), each once, in order of first appearance"""
    g = [int(v) for v in generated]
    if repetition_context_size > 0 and len(g) > repetition_context_size:
        g = g[len(g) - repetition_context_size:]
    return list(dict.fromkeys(g))


def penalize(logits: np.ndarray, ids, penalty: float) -> np.ndarray:
    """apply_repetition_penalty (lib.rs:650-660): a positive logit is divided by the penalty, any other multiplied"""
    out = np.array(logits, dtype=np.float32)
    for t in ids:
        if 0 <= t < out.size:
            out[t] = out[t] / np.float32(penalty) if out[t] > 0 else out[t] * np.float32(penalty)
    return out


class DeepseekOCR2:
    """`load(model_dir)` / `from_weights(weights, llm_args, ...)`: DeepEncoder + engine.Model (moe_mode="deepseek").
    `ocr(global_image, crops, prompt)` -> generated ids: encode_image -> scatter -> prompt pass over caller rows -> decode."""

    def __init__(self, encoder: DeepEncoder, llm, tokenizer=None, image_token_id: int = IMAGE_TOKEN_ID):
        self.encoder, self.llm, self.tokenizer, self.image_token_id = encoder, llm, tokenizer, image_token_id

    @staticmethod
    def from_weights(weights: Dict[str, np.ndarray], llm_args: dict, sam_cfg: Optional[dict] = None, vcf_cfg: Optional[dict] = None,
                     tokenizer=None, max_context: int = 8192) -> "DeepseekOCR2":
        """weights under the checkpoint's names (experts per expert or stacked); llm_args: engine.Model's keywords
        (loader.deepseek_ocr2_args(config))"""
        from . import engine, loader
        enc = DeepEncoder.from_weights(weights, sam_cfg, vcf_cfg)
        args = dict(llm_args, max_context=max_context)
        if enc.out_dim != args["hidden_size"]:
            raise OmxError(f"ShapeMismatch: the projector makes rows of {enc.out_dim}, the decoder's hidden size is {args['hidden_size']}")
        llm = engine.Model(**args)
        dec = {k: v for k, v in weights.items() if k.startswith(("model.layers.", "model.embed_tokens.", "model.norm.", "lm_head."))}
        llm.load_weights(loader.stack_deepseek_experts(dec, args["num_hidden_layers"], args["num_experts"]))
        return DeepseekOCR2(enc, llm, tokenizer)

    @staticmethod
    def load(model_dir: str, max_context: int = 8192) -> "DeepseekOCR2":
        """load_model (lib.rs:946-1120): config.json with the reference's defaults, every shard, tokenizer.json when the `tokenizers`
        package is there (else pass ids / a tokenizer of your own to the calls)"""
        import json
        import os
        from . import loader
        with open(os.path.join(model_dir, "config.json")) as f:
            cfg = json.load(f)
        tok = None
        try:
            import tokenizers
            path = os.path.join(model_dir, "tokenizer.json")
            tok = tokenizers.Tokenizer.from_file(path) if os.path.exists(path) else None
        except ImportError:
            pass
        return DeepseekOCR2.from_weights(loader.load_all_weights(model_dir), loader.deepseek_ocr2_args(cfg), tokenizer=tok, max_context=max_context)

    def close(self) -> None:
        self.encoder.close()
        self.llm.close()

    def prepare_inputs(self, ids, mask, visual_rows):
        """prepare_inputs (lib.rs:522-583) as the engine takes it: (embeds, embeds_at) for engine.Model.prefill -- the rows laid over the
        masked span in the order they come.  As in the reference, a row count that differs from the span leaves the text embeddings
        alone (None, 0)."""
        at, n = image_span(mask)
        if n == 0 or visual_rows is None or visual_rows.shape[0] != n:
            return None, 0
        return visual_rows, at

    def generate_ids(self, ids, mask=None, visual_rows=None, max_tokens: int = 512, temperature: float = 0.0, repetition_penalty: float = 1.0,
                     repetition_context_size: int = 20, seed: int = 0, eos_token_id: int = EOS_TOKEN_ID):
        """The reference's `Generate` (lib.rs:613-769): sample with the repetition penalty over the last repetition_context_size GENERATED
        tokens, stop after EOS (returned) or, before a further step, when is_repeating().
        The penalty runs in the device sampler (set_sampler(repetition_penalty=...)), whose history is every token sampled since the
        prefill: it has no window.  While the generated list is no longer than the window the two are the same thing; from there on the
        window is applied where the reference applies it, on the generated list: the step's raw logits are read back, penalised over
        penalty_window() and drawn on the host (greedy, or categorical with numpy's generator at a temperature)."""
        llm = self.llm
        llm.reset()
        llm.set_sampler(temperature, seed, repetition_penalty=repetition_penalty)
        embeds, at = self.prepare_inputs(ids, mask, visual_rows) if mask is not None else (None, 0)
        tok = int(llm.prefill(np.asarray(ids, dtype=np.uint32), embeds=embeds, embeds_at=at))
        out = [tok]
        windowed = repetition_penalty != 1.0 and repetition_context_size > 0
        rng = np.random.default_rng(seed)
        while out[-1] != eos_token_id and len(out) < max_tokens and not is_repeating(out):
            if not (windowed and len(out) > repetition_context_size):
                tok = int(llm.decode(1)[0])
            else:
                llm.decode(1)                                             # the step; its own draw saw the whole history and is replaced
                logits = penalize(llm.last_logits(), penalty_window(out, repetition_context_size), repetition_penalty)
                if temperature == 0.0:
                    tok = int(np.argmax(logits))
                else:
                    z = logits.astype(np.float64) / temperature
                    p = np.exp(z - z.max())
                    tok = int(rng.choice(p.size, p=p / p.sum()))
                llm.trim(0, tok)                                          # the next step's input
            out.append(tok)
        return out

    def ocr(self, global_image, crops=None, prompt: str = "<image>\nFree OCR.", tokenizer=None, crop_ratio=None, **generate):
        """image views + prompt -> generated ids (decode them with the tokenizer).  crop_ratio (w, h) defaults to (n_crops, 1) -- any
        ratio with that many tiles gives the same ids."""
        tok = tokenizer or self.tokenizer
        if tok is None:
            raise OmxError("ocr: no tokenizer (pass tokenizer=, or install `tokenizers` next to a tokenizer.json)")
        g = image_array(global_image)
        n_crops = 0 if crops is None else len(crops)
        ratio = crop_ratio or ((n_crops, 1) if n_crops > 1 else (1, 1))
        image_size = int(np.asarray(crops).shape[1]) if n_crops else 0
        ids, mask = tokenize_prompt(tok, prompt, True, g.shape[0], image_size, ratio, self.image_token_id)
        rows = self.encoder.encode_image(g, crops if n_crops else None)
        return self.generate_ids(ids, mask, rows, **generate)
