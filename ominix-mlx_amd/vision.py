"""Host mirror of moxin-vlm-mlx's vision side over the omx_vit_encoder_* / omx_vlm_projector_* C ABI (csrc/vit_encoder.hip):
`ViTEncoder` (vision.rs:244-310; `dinov2_large()` / `siglip_so400m()` are the reference's two configs, :41-70), `Projector`
(projector.rs:14-40), and `attention_f32`, the towers' attention kernel alone.  Everything runs in float32, as the reference does
(a float32 image meets bf16 parameters and MLX promotes); weights are widened once at load."""
from __future__ import annotations

import ctypes
import sys

import numpy as np

from . import OmxError, check, lib, require_device
from .audio import ViTConfig          # the struct and the signatures are bound in audio.AUDIO_SIGNATURES
from .ops import Tensor

c_int, c_void_p, c_int64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # normalize_dino (lib.rs:427-431)
UNIT_MEAN, UNIT_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)                          # normalize_siglip (lib.rs:436-440)


def widen(arr) -> np.ndarray:
    """a checkpoint tensor as contiguous float32 (loader.read_safetensors' Bf16Bits are bit patterns: widened exactly)"""
    if type(arr).__name__ == "Bf16Bits":
        arr = (np.asarray(arr).astype(np.uint32) << np.uint32(16)).view(np.float32)
    return np.ascontiguousarray(arr, dtype=np.float32)


def image_array(image, size: int) -> np.ndarray:
    """[size, size, 3] uint8 (-> / 255) or float32 in [0, 1] -> contiguous float32; anything else is refused by name"""
    a = np.asarray(image)
    if a.shape != (size, size, 3):
        raise OmxError(f"ShapeMismatch: image has shape {a.shape}, the tower expects [{size}, {size}, 3]")
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a.astype(np.float32) / np.float32(255.0))
    if a.dtype.kind != "f":
        raise OmxError(f"image dtype {a.dtype}: uint8 or floating point in [0, 1]")
    return np.ascontiguousarray(a, dtype=np.float32)


class ViTEncoder:
    """ViTEncoder::forward (vision.rs:259-310) in float32 on the device: image [S, S, 3] in [0, 1] -> patch rows [num_patches, embed_dim]
    of block depth - 2.  Keywords are ViTConfig's fields (:26-37), `mean` / `std` the tower's image statistics, `prefix` the checkpoint
    prefix that error texts name."""

    def __init__(self, embed_dim=1024, depth=24, num_heads=16, head_dim=64, intermediate_dim=4096, has_cls_token=True, num_registers=4,
                 has_layer_scale=True, patch_size=14, image_size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, prefix=""):
        require_device()
        if len(prefix.encode()) > 126:
            raise OmxError(f"InvalidConfig: vit encoder prefix of {len(prefix.encode())} bytes (at most 126)")
        self.cfg = ViTConfig(embed_dim, depth, num_heads, head_dim, intermediate_dim, int(bool(has_cls_token)), num_registers,
                             int(bool(has_layer_scale)), patch_size, image_size, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std),
                             prefix.encode())
        self._h = c_void_p()
        check(lib.omx_vit_encoder_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))

    @staticmethod
    def dinov2_large(**kw) -> "ViTEncoder":
        """ViTConfig::dinov2_large (vision.rs:41-54) with the ImageNet statistics of normalize_dino"""
        return ViTEncoder(**dict(dict(embed_dim=1024, depth=24, num_heads=16, head_dim=64, intermediate_dim=4096, has_cls_token=True,
                                      num_registers=4, has_layer_scale=True, patch_size=14, image_size=224, mean=IMAGENET_MEAN,
                                      std=IMAGENET_STD), **kw))

    @staticmethod
    def siglip_so400m(**kw) -> "ViTEncoder":
        """ViTConfig::siglip_so400m (vision.rs:57-70) with the unit statistics of normalize_siglip"""
        return ViTEncoder(**dict(dict(embed_dim=1152, depth=27, num_heads=16, head_dim=72, intermediate_dim=4304, has_cls_token=False,
                                      num_registers=0, has_layer_scale=False, patch_size=14, image_size=224, mean=UNIT_MEAN, std=UNIT_STD),
                                 **kw))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_vit_encoder_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        if sys is not None and not sys.is_finalizing():
            self.close()

    def load_weights(self, weights) -> None:
        """{key behind the prefix: array}, the checkpoint's own layouts (patch_embed.proj.weight [O, 3, P, P])"""
        for name, arr in weights.items():
            a = widen(arr)
            shape = (c_int64 * a.ndim)(*a.shape)
            check(lib.omx_vit_encoder_load(self._h, name.encode(), a.ctypes.data, shape, a.ndim))

    def tokens(self) -> int:
        """rows of the sequence the blocks see: CLS + registers + patches"""
        t, r = c_int(), c_int()
        check(lib.omx_vit_encoder_tokens(self._h, ctypes.byref(t), ctypes.byref(r)))
        return t.value

    def rows(self) -> int:
        """rows that come out: the patches"""
        t, r = c_int(), c_int()
        check(lib.omx_vit_encoder_tokens(self._h, ctypes.byref(t), ctypes.byref(r)))
        return r.value

    def launches(self) -> int:
        n = c_int()
        check(lib.omx_vit_encoder_launches(self._h, ctypes.byref(n)))
        return n.value

    def debug_read(self, name: str, shape) -> np.ndarray:
        """A stage of the last forward as float32 (test hook): "col", "patches", "h", and of the last block run "ln1", "qkv", "attn",
        "ln2", "mlp" (include/omx.h)."""
        out = np.empty(shape, np.float32)
        check(lib.omx_vit_encoder_debug_read(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def forward(self, image, out: Tensor = None, column: int = 0) -> Tensor:
        """image: numpy [S, S, 3] (uint8, or float in [0, 1]) or a device f32 Tensor of that shape.  With `out` (f32 [rows, width]) the
        rows go into its columns [column, column + embed_dim): two towers fill one buffer."""
        S, d = self.cfg.image_size, self.cfg.embed_dim
        img = image if isinstance(image, Tensor) else Tensor.from_numpy(image_array(image, S), "f32")
        if tuple(img.shape) != (S, S, 3):
            raise OmxError(f"ShapeMismatch: image has shape {img.shape}, the tower expects [{S}, {S}, 3]")
        n = self.rows()
        if out is None:
            out, column = Tensor((n, d), "f32"), 0
        if len(out.shape) != 2 or out.shape[0] != n or column < 0 or column + d > out.shape[1]:
            raise OmxError(f"ShapeMismatch: rows [{n}, {d}] at column {column} do not fit a buffer of shape {out.shape}")
        check(lib.omx_vit_encoder_forward(self._h, img.ptr, out.ptr + 4 * column, out.shape[1], None))
        return out


class Projector:
    """FusedMLPProjector (projector.rs:14-40): fc1 -> gelu -> fc2 -> gelu -> fc3 in float32, widths read from the weights."""

    def __init__(self):
        require_device()
        self._h = c_void_p()
        check(lib.omx_vlm_projector_create(ctypes.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_vlm_projector_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        if sys is not None and not sys.is_finalizing():
            self.close()

    def load_weights(self, weights) -> None:
        """{"fc1.weight": ..., "fc1.bias": ..., "fc2...", "fc3..."}"""
        for name, arr in weights.items():
            a = widen(arr)
            shape = (c_int64 * a.ndim)(*a.shape)
            check(lib.omx_vlm_projector_load(self._h, name.encode(), a.ctypes.data, shape, a.ndim))

    def dims(self):
        i, o = c_int(), c_int()
        check(lib.omx_vlm_projector_dims(self._h, ctypes.byref(i), ctypes.byref(o)))
        return i.value, o.value

    def forward(self, x: Tensor) -> Tensor:
        i, o = self.dims()
        if len(x.shape) != 2 or x.shape[1] != i:
            raise OmxError(f"ShapeMismatch: projector input has shape {x.shape}, fc1 takes rows of {i}")
        out = Tensor((x.shape[0], o), "f32")
        check(lib.omx_vlm_projector_forward(self._h, x.ptr, x.shape[0], out.ptr, None))
        return out


def attention_f32(qkv: Tensor, heads: int, width: int, n: int = None) -> Tensor:
    """The towers' attention alone (omx_vit_attention_f32): qkv f32 [N, ld >= 3 * heads * width] holding q | k | v side by side from
    column 0, unmasked, scale width^-0.5; -> [N, heads * width].  width 64 or 72, N <= 1024."""
    d = heads * width
    N, ld = (qkv.shape[0] if n is None else n), qkv.shape[1]
    if ld < 3 * d:
        raise OmxError(f"ShapeMismatch: rows of {ld} floats do not hold q | k | v of {heads} x {width}")
    out = Tensor((max(N, 1), d), "f32")
    check(lib.omx_vit_attention_f32(out.ptr, d, qkv.ptr, qkv.ptr + 4 * d, qkv.ptr + 8 * d, ld, N, heads, width, None))
    return out


def gemm_f32(a: Tensor, w: Tensor, bias: Tensor = None, resid: Tensor = None, col_scale: Tensor = None, gelu: bool = False) -> Tensor:
    """out [M, N] = resid + col_scale * gelu?(a [M, K] . w [N, K]^T + bias): launch_gemm_f32 with its fused epilogues (omx_gemm_f32_epilogue)"""
    (M, K), (N, K2) = a.shape, w.shape
    if K != K2:
        raise OmxError(f"ShapeMismatch: a {a.shape} against w {w.shape}")
    out = Tensor((M, N), "f32")
    p = lambda t: None if t is None else t.ptr
    check(lib.omx_gemm_f32_epilogue(out.ptr, a.ptr, w.ptr, p(bias), p(resid), p(col_scale), M, N, K, int(bool(gelu)), None))
    return out
