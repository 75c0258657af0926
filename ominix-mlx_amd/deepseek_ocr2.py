"""The vision side of DeepSeek-OCR-2 on the device (deepseek-ocr2-mlx/src/lib.rs `DeepseekOCR2::encode_image`, :467-497): views -> SAM
ViT-B tower (float32, csrc/sam_encoder.hip) -> visual-causal-flow encoder (csrc/vcf_encoder.hip) -> Linear projector -> the rows that
`prepare_inputs` scatters over the image placeholders, the learned separator row last.  The language decoder (DeepSeek-V2 MoE) is not
here.  Host logic only; every hot path is a device call of vision.py."""
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
