"""Moxin-VLM on the device (moxin-vlm-mlx/src/lib.rs): image -> DINOv2 and SigLIP towers (float32, csrc/vit_encoder.hip) writing the two
column ranges of one [256, 2176] buffer -> projector -> the visual rows over the placeholder span behind BOS
(Model.prefill(embeds=, embeds_at=1), the reference's forward_embeddings) -> greedy / sampled decode of the Mistral-wired decoder
(no q/k norm, no bias).  Host logic only; every hot path is a device call of vision.py / engine.py."""
from __future__ import annotations

import json
import os
import time
from typing import Dict, List, Tuple

import numpy as np

from . import OmxError

EOS_ID = 2                                # </s> (examples/generate.rs:113)
MISTRAL_DEFAULTS = dict(hidden_size=4096, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, intermediate_size=14336,
                        vocab_size=32064, rms_norm_eps=1e-5, rope_theta=10000.0, tie_word_embeddings=False)      # lib.rs:93-116
VISION_PREFIXES = (("vision_backbone.featurizer", "vision_backbone.fused_featurizer"),                           # lib.rs:626-636
                   ("vision_backbone.featurizer.0", "vision_backbone.featurizer.1"))
LLM_PREFIXES = ("language_model", "llm_backbone.llm")                                                            # lib.rs:639-643
_LINEARS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def text_model_args(config: dict) -> dict:
    """config.json -> keywords of engine.Model: `text_config` over MistralConfig's defaults (lib.rs:71-116, 613-619)"""
    c = dict(MISTRAL_DEFAULTS, **{k: v for k, v in (config.get("text_config") or {}).items() if k in MISTRAL_DEFAULTS})
    return dict(c, head_dim=c["hidden_size"] // c["num_attention_heads"], qk_norm=False, attention_bias=False)


def split_weights(weights: Dict[str, np.ndarray]) -> Tuple[dict, dict, dict, dict, dict]:
    """The name mapping of load_model (lib.rs:624-758) -> (dino tensors, siglip tensors, projector tensors, text tensors, prefixes).
    Tower tensors lose their prefix; projector tensors become fc1 / fc2 / fc3 (from `projector.fc1/fc2/fc3` or the fallback
    `projector.0/2/4`, projector.rs:60-101); text tensors become engine.Model's `model.*` / `lm_head.*`."""
    hf = any(k.startswith(VISION_PREFIXES[0][0] + ".blocks.") for k in weights)
    dino_p, sig_p = VISION_PREFIXES[0] if hf else VISION_PREFIXES[1]
    llm_p = LLM_PREFIXES[0] if any(k.startswith(LLM_PREFIXES[0] + ".") for k in weights) else LLM_PREFIXES[1]

    def behind(prefix):
        return {k[len(prefix) + 1:]: v for k, v in weights.items() if k.startswith(prefix + ".")}

    dino, siglip = behind(dino_p), behind(sig_p)
    proj = {}
    for name, idx in ((("fc1", "0"), ("fc2", "2"), ("fc3", "4"))):
        for leaf in ("weight", "bias"):
            for key in (f"projector.{name}.{leaf}", f"projector.{idx}.{leaf}"):
                if key in weights:
                    proj[f"{name}.{leaf}"] = weights[key]
                    break
        if f"{name}.weight" not in proj:
            raise OmxError(f"WeightNotFound: projector.{name}.weight or projector.{idx}.weight")
    text = behind(llm_p)
    text = {k: v for k, v in text.items() if k.startswith(("model.", "lm_head."))}
    return dino, siglip, proj, text, dict(dino=dino_p, siglip=sig_p, llm=llm_p)


def build_prompt_ids(tokenizer, text: str, n_rows: int, image_token_id: int) -> np.ndarray:
    """The Prismatic form "In: {prompt}\\nOut:" tokenised with BOS (examples/generate.rs:85-90), and n_rows placeholder ids behind the
    BOS: the positions the visual rows take (lib.rs:318-324)."""
    enc = tokenizer.encode(f"In: {text}\nOut:", add_special_tokens=True)
    ids = [int(t) for t in getattr(enc, "ids", enc)]
    if not ids:
        raise OmxError("moxin-vlm: the tokenizer returned no ids (a BOS id is expected first)")
    return np.asarray(ids[:1] + [int(image_token_id)] * int(n_rows) + ids[1:], dtype=np.uint32)


def placeholder_span(ids, image_token_id: int, n_rows: int) -> int:
    """Index of the first placeholder; the placeholders must be one run of exactly the row count, directly behind the first id"""
    ids = np.asarray(ids)
    at = np.nonzero(ids == image_token_id)[0]
    if at.size != n_rows:
        raise OmxError(f"moxin-vlm: the prompt holds {at.size} placeholder ids but the towers made {n_rows} rows")
    if n_rows and (at[0] != 1 or at[-1] != n_rows):
        raise OmxError("moxin-vlm: the placeholder ids of the prompt are not one span directly behind the BOS id")
    return 1


def quantize_text_weights(text: Dict[str, np.ndarray], bits: int, group_size: int = 64) -> Dict[str, np.ndarray]:
    """MoxinVLM::quantize (lib.rs:366-391) on the device's quantiser (ops.quantize = mlx_rs::ops::quantize): every decoder Linear and the
    head become packed triplets; norms stay.  The engine runs no unquantised matrix inside a packed model, so the embedding table is
    packed in the same format too (the reference keeps it bf16: DESIGN 4.13)."""
    from . import ops
    out = {}
    for k, v in text.items():
        stem = k[:-7] if k.endswith(".weight") else None
        if stem is None or not (stem.endswith(_LINEARS) or stem in ("lm_head", "model.embed_tokens")):
            out[k] = v
            continue
        packed, scales, biases = ops.quantize(ops.Tensor.from_numpy(v, "bf16"), group_size, bits)
        out[k], out[stem + ".scales"], out[stem + ".biases"] = packed.numpy(), scales.numpy(), biases.numpy()
    return out


def read_checkpoint(model_dir: str):
    """The device-free half of load: (config.json or {}, dino tensors, siglip tensors, projector tensors, text tensors, prefixes),
    read through loader.py's safetensors reader."""
    from . import loader
    config = {}
    path = os.path.join(model_dir, "config.json")
    if os.path.exists(path):
        with open(path) as f:
            config = json.load(f)
    return (config,) + split_weights(loader.load_all_weights(model_dir))


class MoxinVLM:
    """MoxinVLM (lib.rs:281-391) with the loop of examples/generate.rs: `load(model_dir, quantize=0)`, `visual_rows(image)`,
    `prompt_ids(text)`, `generate_ids(image, prompt, max_tokens, temperature)`, `describe(image, prompt)`."""

    def __init__(self, model, dino, siglip, projector, tokenizer, image_token_id: int = 32000, eos_id: int = EOS_ID):
        self.model, self.dino, self.siglip, self.projector, self.tokenizer = model, dino, siglip, projector, tokenizer
        self.image_token_id, self.eos_id = int(image_token_id), int(eos_id)
        if dino.rows() != siglip.rows():
            raise OmxError(f"InvalidConfig: the towers make {dino.rows()} and {siglip.rows()} rows")
        fused = dino.cfg.embed_dim + siglip.cfg.embed_dim
        if projector.dims() != (fused, model.cfg.hidden_size):
            raise OmxError(f"ShapeMismatch: projector {projector.dims()} against towers of {fused} columns and a decoder of {model.cfg.hidden_size}")
        if not 0 <= self.image_token_id < model.cfg.vocab_size:
            raise OmxError(f"InvalidConfig: placeholder id {self.image_token_id} outside the vocabulary of {model.cfg.vocab_size}")
        self.last_times = {}
        self._fused = None

    @staticmethod
    def load(model_dir: str, quantize: int = 0, max_context: int = 4096, group_size: int = 64) -> "MoxinVLM":
        """load_model (lib.rs:608-772).  quantize = 4 | 8 packs the decoder only; towers and projector stay float32 (lib.rs:366-391)."""
        from . import engine, generate, vision
        if quantize not in (0, 4, 8):
            raise OmxError(f"InvalidConfig: quantize {quantize} (0, 4 or 8)")
        config, dino_w, sig_w, proj_w, text, prefixes = read_checkpoint(model_dir)
        args = dict(text_model_args(config), max_context=max_context)
        if quantize:
            args["quantization"] = {"bits": quantize, "group_size": group_size}
            text = quantize_text_weights(text, quantize, group_size)
        model = engine.Model(**args)
        model.load_weights({k: v for k, v in text.items() if not (args["tie_word_embeddings"] and k.startswith("lm_head."))})
        dino = vision.ViTEncoder.dinov2_large(prefix=prefixes["dino"])
        dino.load_weights(dino_w)
        siglip = vision.ViTEncoder.siglip_so400m(prefix=prefixes["siglip"])
        siglip.load_weights(sig_w)
        proj = vision.Projector()
        proj.load_weights(proj_w)
        return MoxinVLM(model, dino, siglip, proj, generate.load_tokenizer(model_dir), int(config.get("image_token_index", 32000)))

    def close(self) -> None:
        for h in (self.model, self.dino, self.siglip, self.projector):
            h.close()

    def visual_rows(self, image):
        """lib.rs:306-313: both towers on the image, side by side in one buffer (no concatenation), through the projector ->
        device f32 [rows, hidden].  Records tower / projector milliseconds (host clock around a device synchronisation) in last_times."""
        from . import ops, vision
        S = self.dino.cfg.image_size
        img = image if isinstance(image, ops.Tensor) else ops.Tensor.from_numpy(vision.image_array(image, S), "f32")
        n, d0, d1 = self.dino.rows(), self.dino.cfg.embed_dim, self.siglip.cfg.embed_dim
        if self._fused is None:
            self._fused = ops.Tensor((n, d0 + d1), "f32")
        t0 = time.perf_counter()
        self.dino.forward(img, out=self._fused, column=0)
        self.siglip.forward(img, out=self._fused, column=d0)
        ops.synchronize()
        t1 = time.perf_counter()
        rows = self.projector.forward(self._fused)
        ops.synchronize()
        t2 = time.perf_counter()
        self.last_times.update(towers_ms=1e3 * (t1 - t0), projector_ms=1e3 * (t2 - t1),
                               launches=self.dino.launches() + self.siglip.launches() + 3)
        return rows

    def prompt_ids(self, text: str) -> np.ndarray:
        return build_prompt_ids(self.tokenizer, text, self.dino.rows(), self.image_token_id)

    def generate_ids(self, image, prompt: str, max_tokens: int = 256, temperature: float = 0.0, seed: int = 0, chunk: int = 16) -> List[int]:
        """Generate (lib.rs:456-555) under the loop of examples/generate.rs:119-133: at most max_tokens tokens are drawn, the EOS id ends the
        stream and is not emitted."""
        self.last_times = {}
        rows = self.visual_rows(image)
        ids = self.prompt_ids(prompt)
        at = placeholder_span(ids, self.image_token_id, rows.shape[0])
        self.model.reset()
        self.model.set_sampler(float(temperature), seed)
        tok = int(self.model.prefill(ids, embeds=rows, embeds_at=at))
        t0 = time.perf_counter()
        out: List[int] = []
        pending: List[int] = []
        steps = 0
        for _ in range(max_tokens):
            if tok == self.eos_id:
                break
            out.append(tok)
            if len(out) == max_tokens:
                break
            if not pending:
                pending = [int(t) for t in self.model.decode(min(chunk, max_tokens - len(out)))]
                steps += len(pending)
            tok = pending.pop(0)
        self.last_times.update(prompt_rows=int(ids.size), prompt_pass_ms=self.model.last_prefill_ms(), tokens=len(out),
                               per_token_ms=1e3 * (time.perf_counter() - t0) / steps if steps else 0.0)
        return out

    def describe(self, image, prompt: str, max_tokens: int = 256, temperature: float = 0.0) -> str:
        return self.tokenizer.decode(self.generate_ids(image, prompt, max_tokens, temperature), skip_special_tokens=True)
