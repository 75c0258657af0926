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


# ---- the DeepSeek-OCR-2 vision side (csrc/sam_encoder.hip, csrc/vcf_encoder.hip; deepseek_ocr2.py drives them) ----
from .audio import SamConfig, VcfConfig   # noqa: E402  (bound in audio.AUDIO_SIGNATURES, like ViTConfig)

c_size_t = ctypes.c_size_t


class _Tower:
    """what SamEncoder and VisualCausalEncoder share: the handle, loading by checkpoint key, the counters, debug_read"""
    _family = ""

    def _call(self, name):
        return getattr(lib, f"omx_{self._family}_encoder_{name}")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._call("destroy")(self._h)
            self._h = c_void_p()

    def __del__(self):
        if sys is not None and not sys.is_finalizing():
            self.close()

    def load_weights(self, weights) -> None:
        """{key behind the prefix: array}, the checkpoint's own names and layouts (convolutions [O, I, kh, kw])"""
        for name, arr in weights.items():
            a = widen(arr)
            shape = (c_int64 * a.ndim)(*a.shape)
            check(self._call("load")(self._h, name.encode(), a.ctypes.data, shape, a.ndim))

    def launches(self) -> int:
        n = c_int()
        check(self._call("launches")(self._h, ctypes.byref(n)))
        return n.value

    def scratch_bytes(self) -> int:
        """device scratch the handle holds after its last forward"""
        n = c_size_t()
        check(self._call("scratch_bytes")(self._h, ctypes.byref(n)))
        return n.value

    def debug_read(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, np.float32)
        check(self._call("debug_read")(self._h, name.encode(), out.ctypes.data, out.size))
        return out


def _prefix_bytes(prefix: str, what: str) -> bytes:
    if len(prefix.encode()) > 126:
        raise OmxError(f"InvalidConfig: {what} prefix of {len(prefix.encode())} bytes (at most 126)")
    return prefix.encode()


class SamEncoder(_Tower):
    """ImageEncoderViT::forward (deepseek-ocr2-mlx/src/vision.rs:385-431) in float32 on the device over stacked images [B, S, S, 3] in
    [-1, 1] -> rows [B * (S / 64)^2, 896].  The defaults are the reference's SAM ViT-B (:492-496); the neck and output widths are read
    from the weights.  keep_stages keeps "h0" and every "block<N>" for debug_read (tests)."""
    _family = "sam"

    def __init__(self, embed_dim=768, depth=12, num_heads=12, mlp_dim=3072, window=14, global_attn_indexes=(2, 5, 8, 11), patch_size=16,
                 prefix="", keep_stages=False):
        require_device()
        g = tuple(int(i) for i in global_attn_indexes)
        if len(g) > 16:
            raise OmxError(f"InvalidConfig: sam encoder: {len(g)} global blocks (at most 16)")
        self.cfg = SamConfig(embed_dim, depth, num_heads, mlp_dim, window, patch_size, len(g), int(bool(keep_stages)),
                             (c_int * 16)(*(g + (0,) * (16 - len(g)))), _prefix_bytes(prefix, "sam encoder"))
        self._h = c_void_p()
        check(lib.omx_sam_encoder_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))

    def tokens(self, image_size: int):
        """(grid side, rows per image that come out, their width)"""
        g, r, d = c_int(), c_int(), c_int()
        check(lib.omx_sam_encoder_tokens(self._h, image_size, ctypes.byref(g), ctypes.byref(r), ctypes.byref(d)))
        return g.value, r.value, d.value

    def forward(self, images, out: Tensor = None) -> Tensor:
        """images: device f32 Tensor or numpy [B, S, S, 3] (or [S, S, 3]) in [-1, 1] -> f32 [B * rows, width]"""
        img = images if isinstance(images, Tensor) else Tensor.from_numpy(np.ascontiguousarray(images, np.float32), "f32")
        shape = tuple(img.shape)
        if len(shape) == 3:
            shape = (1,) + shape
        if len(shape) != 4 or shape[1] != shape[2] or shape[3] != 3:
            raise OmxError(f"ShapeMismatch: images have shape {tuple(img.shape)}, the tower expects [B, S, S, 3]")
        B, S = shape[0], shape[1]
        _, rows, width = self.tokens(S)
        if out is None:
            out = Tensor((B * rows, width), "f32")
        if tuple(out.shape) != (B * rows, width):
            raise OmxError(f"ShapeMismatch: rows [{B * rows}, {width}] do not fit a buffer of shape {out.shape}")
        check(lib.omx_sam_encoder_forward(self._h, img.ptr, B, S, out.ptr, None))
        return out


class VisualCausalEncoder(_Tower):
    """Qwen2Encoder::forward_vision (qwen2_encoder.rs:198-244) in float32 on the device: x [B * n_img, hidden] (B images' SAM rows) ->
    the query rows [B * n_query, hidden].  Keys are the checkpoint's behind its prefix ("model.model.layers.3.self_attn.q_proj.weight",
    "model.model.norm.weight", "query_768.weight", "query_1024.weight")."""
    _family = "vcf"

    def __init__(self, hidden=896, layers=24, heads=14, kv_heads=2, intermediate=4864, rope_theta=1e6, eps=1e-6, prefix="", keep_stages=False):
        require_device()
        self.cfg = VcfConfig(hidden, layers, heads, kv_heads, intermediate, int(bool(keep_stages)), rope_theta, eps,
                             _prefix_bytes(prefix, "vcf encoder"))
        self._h = c_void_p()
        check(lib.omx_vcf_encoder_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))

    def tokens(self, n_img: int):
        """(query rows per image, sequence length) for images of n_img rows"""
        q, l = c_int(), c_int()
        check(lib.omx_vcf_encoder_tokens(self._h, n_img, ctypes.byref(q), ctypes.byref(l)))
        return q.value, l.value

    def forward(self, x: Tensor, images: int = 1, out: Tensor = None, row: int = 0) -> Tensor:
        """x f32 [images * n_img, hidden]; with `out` (f32 [rows, hidden]) the query rows go to its rows [row, row + images * n_query)"""
        d = self.cfg.hidden
        if len(x.shape) != 2 or x.shape[1] != d or images < 1 or x.shape[0] % images:
            raise OmxError(f"ShapeMismatch: rows of shape {x.shape} are not {images} images of rows of {d}")
        nq, _ = self.tokens(x.shape[0] // images)
        if out is None:
            out, row = Tensor((images * nq, d), "f32"), 0
        if len(out.shape) != 2 or out.shape[1] != d or row < 0 or row + images * nq > out.shape[0]:
            raise OmxError(f"ShapeMismatch: rows [{images * nq}, {d}] at row {row} do not fit a buffer of shape {out.shape}")
        check(lib.omx_vcf_encoder_forward(self._h, x.ptr, images, x.shape[0] // images, out.ptr + 4 * row * d, None))
        return out


def sam_attention_f32(qkv: Tensor, heads: int, grid, window: int, rel_pos_h: Tensor, rel_pos_w: Tensor, pad_qkv: Tensor = None,
                      images: int = 1) -> Tensor:
    """SAM's attention alone (omx_sam_attention_f32): qkv f32 [images * gh * gw, ld >= 3 * heads * 64] holding q | k | v side by side,
    grid = (gh, gw), window 0 (global, any key count) or the window side; rel_pos_* f32 [len, width]; pad_qkv f32 [3 * heads * 64], the
    padded token's row, required when a grid side is no multiple of the window.  -> [images * gh * gw, heads * 64]."""
    gh, gw = (int(g) for g in grid)
    width = rel_pos_h.shape[1] if len(rel_pos_h.shape) == 2 else 0
    if len(rel_pos_w.shape) != 2 or rel_pos_w.shape[1] != width:
        raise OmxError(f"ShapeMismatch: rel_pos_h {rel_pos_h.shape} against rel_pos_w {rel_pos_w.shape}")
    d = heads * width
    if len(qkv.shape) != 2 or qkv.shape[0] != images * gh * gw or qkv.shape[1] < 3 * d:
        raise OmxError(f"ShapeMismatch: rows of shape {qkv.shape} do not hold q | k | v of {heads} x {width} for {images} grids of {gh} x {gw}")
    if pad_qkv is not None and pad_qkv.size != 3 * d:
        raise OmxError(f"ShapeMismatch: pad_qkv has {pad_qkv.size} elements, a q | k | v row has {3 * d}")
    out = Tensor((qkv.shape[0], d), "f32")
    check(lib.omx_sam_attention_f32(out.ptr, d, qkv.ptr, qkv.shape[1], images, gh, gw, heads, width, window, rel_pos_h.ptr, rel_pos_h.shape[0],
                                    rel_pos_w.ptr, rel_pos_w.shape[0], None if pad_qkv is None else pad_qkv.ptr, None))
    return out


def prefix_causal_attention_f32(qkv: Tensor, heads: int, kv_heads: int, n_prefix: int, images: int = 1, width: int = 64) -> Tensor:
    """The visual-causal-flow attention alone (omx_prefix_causal_attention_f32): qkv f32 [images * L, ld >= (heads + 2 kv_heads) * 64]
    holding the query heads, the key heads, the value heads; row i sees keys j < max(n_prefix, i + 1) of its image.  -> [images * L, heads * 64]."""
    if len(qkv.shape) != 2 or images < 1 or qkv.shape[0] % images or qkv.shape[1] < (heads + 2 * kv_heads) * width:
        raise OmxError(f"ShapeMismatch: rows of shape {qkv.shape} do not hold {heads} + 2 x {kv_heads} heads of {width} for {images} images")
    out = Tensor((qkv.shape[0], heads * width), "f32")
    check(lib.omx_prefix_causal_attention_f32(out.ptr, heads * width, qkv.ptr, qkv.shape[1], images, qkv.shape[0] // images, heads, kv_heads, width,
                                              n_prefix, None))
    return out
