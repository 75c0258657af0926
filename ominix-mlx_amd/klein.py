"""Host mirror of flux-klein-mlx's `FluxKlein` (klein_model.rs:686-870) over omx_klein_*: `compute_rope`
(ids -> cos/sin), `forward_with_rope`, and the Euler denoise loop of examples/generate_klein.rs:431-446."""
from __future__ import annotations

import ctypes
import sys

import numpy as np

from . import BFLOAT16, UINT32, OmxError, check, lib, require_device
from .ops import Tensor

c_int, c_float, c_void_p, c_uint32, c_size_t = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t


class KleinConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("in_channels", "hidden_size", "txt_embed_dim", "num_heads", "depth", "depth_single",
                                     "head_dim", "mlp_hidden", "tp_rank", "tp_size")]


KLEIN_SIGNATURES = {
    "omx_klein_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(KleinConfig)]),
    "omx_klein_destroy": (c_int, [c_void_p]),
    "omx_klein_set_weight": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_klein_synth_weights": (c_int, [c_void_p, c_uint32]),
    "omx_klein_set_quantized_weight": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int]),
    "omx_klein_quantize": (c_int, [c_void_p, c_int, c_int]),
    "omx_klein_weight_bytes": (c_int, [c_void_p, ctypes.POINTER(c_size_t)]),
    "omx_klein_set_comm": (c_int, [c_void_p, c_void_p, c_void_p]),
    "omx_klein_forward_with_rope": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]),
    "omx_klein_euler_step": (c_int, [c_void_p, c_void_p, c_float, c_void_p, ctypes.c_int64, c_void_p]),
    "omx_klein_last_ms": (c_int, [c_void_p, ctypes.POINTER(c_float)]),
    "omx_klein_debug_read": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, c_size_t]),
}
for _n, (_r, _a) in KLEIN_SIGNATURES.items():
    _f = getattr(lib, _n)
    _f.restype, _f.argtypes = _r, _a

AXES_DIM, THETA = (32, 32, 32, 32), 2000.0


def is_linear_weight(name: str) -> bool:
    """The DiT weights QuantizedFluxKlein packs (klein_quantized.rs:498-556): every Linear's `.weight` -- the per-head q / k RmsNorms
    stay bf16 (`norm_out` is the AdaLN Linear and is packed)."""
    return name.endswith(".weight") and not name.endswith(("norm_q.weight", "norm_k.weight"))


def create_txt_ids(seq_len: int) -> np.ndarray:
    """generate_klein.rs:543-556: (0, 0, 0, s)."""
    ids = np.zeros((seq_len, 4), np.float32)
    ids[:, 3] = np.arange(seq_len)
    return ids


def create_img_ids(h: int, w: int) -> np.ndarray:
    """generate_klein.rs:519-535: (0, y, x, 0)."""
    ids = np.zeros((h * w, 4), np.float32)
    ids[:, 1] = np.repeat(np.arange(h), w)
    ids[:, 2] = np.tile(np.arange(w), h)
    return ids


def compute_rope(txt_ids: np.ndarray, img_ids: np.ndarray):
    """FluxKlein::compute_rope / compute_rope_freqs (klein_model.rs:53-110, 786-797): [txt, img] order, every
    frequency duplicated for its interleaved pair.  The tables are tiny ([S, 128]) and position-only, so they are
    built once on the host (f32 angle, as the reference) and uploaded."""
    ids = np.concatenate([txt_ids, img_ids], 0).astype(np.float32)
    cs, sn = [], []
    for axis, dim in enumerate(AXES_DIM):
        half = dim // 2
        inv = (np.float32(1.0) / np.power(np.float32(THETA), np.float32(2.0) * np.arange(half, dtype=np.float32) / np.float32(dim))).astype(np.float32)
        ang = (ids[:, axis:axis + 1] * inv[None, :]).astype(np.float32)
        cs.append(np.repeat(np.cos(ang.astype(np.float64)), 2, axis=1))
        sn.append(np.repeat(np.sin(ang.astype(np.float64)), 2, axis=1))
    return (Tensor.from_numpy(np.concatenate(cs, 1).astype(np.float32), "f32"),
            Tensor.from_numpy(np.concatenate(sn, 1).astype(np.float32), "f32"))


def shard_state_dict(weights: dict, hidden_size: int, mlp_hidden: int, rank: int, world: int) -> dict:
    """Tensor-parallel shard plan of the DiT, shared by `FluxKlein.load_weights`,
    the device generator (`omx_klein_synth_weights`) and the world-size-2 gloo test (tests/test_klein_tp.py).
    Heads are contiguous per rank (width hl = hidden/world), MLP columns too (ml = mlp_hidden/world):
        row split   to_q / to_k / to_v                      rows  [r*hl, +hl)
                    mlp_in  = [gate; up]                    rows  [r*ml, +ml) of each half
                    to_qkv_mlp = [q; k; v; gate; up]        the rank's rows of each of the five parts
        col split   to_out (double), mlp_out                cols  [r*hl, +hl) / [r*ml, +ml)   -> partial sums
                    to_out (single) over [attn | mlp]       cols  [r*hl, +hl) and h + [r*ml, +ml)
        replicated  embedders, time/modulation MLPs, q/k norms, norm_out, proj_out"""
    if world == 1:
        return dict(weights)
    h, mh, r = hidden_size, mlp_hidden, rank
    if h % world or mh % world:
        raise ValueError(f"InvalidConfig: hidden_size={h} / mlp_hidden={mh} not divisible by tp_size={world}")
    hl, ml = h // world, mh // world
    from .loader import keep_kind
    rows = lambda a, segs: keep_kind(a, np.ascontiguousarray(np.concatenate([a[s:s + n] for s, n in segs], 0)))
    cols = lambda a, segs: keep_kind(a, np.ascontiguousarray(np.concatenate([a[:, s:s + n] for s, n in segs], 1)))
    out = {}
    for name, a in weights.items():
        leaf = name.rsplit(".", 2)[-2] if name.endswith(".weight") else name
        if leaf.endswith(("to_q", "to_k", "to_v")):
            a = rows(a, [(r * hl, hl)])
        elif leaf.endswith("mlp_in"):
            a = rows(a, [(r * ml, ml), (mh + r * ml, ml)])
        elif leaf.endswith("mlp_out"):
            a = cols(a, [(r * ml, ml)])
        elif leaf == "to_qkv_mlp":
            a = rows(a, [(r * hl, hl), (h + r * hl, hl), (2 * h + r * hl, hl), (3 * h + r * ml, ml), (3 * h + mh + r * ml, ml)])
        elif leaf.endswith("to_out"):
            a = cols(a, [(r * hl, hl), (h + r * ml, ml)] if name.startswith("single_blocks.") else [(r * hl, hl)])
        out[name] = a
    return out


class FluxKlein:
    def __init__(self, in_channels=128, hidden_size=3072, txt_embed_dim=7680, num_heads=24, depth=5, depth_single=20,
                 head_dim=128, mlp_hidden=9216, tp_rank=0, tp_size=1):
        require_device()
        self.cfg = KleinConfig(in_channels, hidden_size, txt_embed_dim, num_heads, depth, depth_single, head_dim, mlp_hidden,
                               tp_rank, tp_size)
        self._h = c_void_p()
        check(lib.omx_klein_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))
        self._keep = []
        # weight name -> ("bf16" | "packed", the tensors uploaded for it): what load_weights / load_quantized_weights registered
        self._keep_of = {}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.omx_klein_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        if sys is not None and not sys.is_finalizing():   # (module globals are already None late in shutdown)
            self.close()

    def set_comm(self, comm_ptr: int, allreduce_fn_ptr: int) -> None:
        """RCCL communicator + address of ncclAllReduce (comm.rccl_comm), before the first forward."""
        check(lib.omx_klein_set_comm(self._h, comm_ptr, allreduce_fn_ptr))

    def load_weights(self, weights: dict) -> None:
        """Logical (unsharded) tensors by the reference's internal names; sliced here under tensor parallelism."""
        weights = shard_state_dict(weights, self.cfg.hidden_size, self.cfg.mlp_hidden, self.cfg.tp_rank, self.cfg.tp_size)
        for name, arr in weights.items():
            t = arr if isinstance(arr, Tensor) else Tensor.from_numpy(arr, "bf16")   # (a device tensor: single GPU)
            self._keep.append(t)
            self._keep_of[name] = ("bf16", [t])
            check(lib.omx_klein_set_weight(self._h, name.encode(), t.ptr, t.nbytes))

    def _drop(self, name: str) -> None:
        ids = {id(t) for t in self._keep_of.pop(name, (None, []))[1]}
        self._keep = [t for t in self._keep if id(t) not in ids]

    def quantize(self, group_size: int = 64, bits: int = 8) -> None:
        """QuantizedFluxKlein::from_unquantized(flux, group_size, bits) (klein_quantized.rs:498): every Linear registered so far becomes
        a model-owned packed triplet; the bf16 copies this object uploaded for them are released.  Triplets registered by
        load_quantized_weights are already packed: the model keeps reading them, so they stay referenced here."""
        check(lib.omx_klein_quantize(self._h, group_size, bits))
        for name in [n for n, (kind, _) in self._keep_of.items() if kind == "bf16" and is_linear_weight(n)]:
            self._drop(name)

    def load_quantized_weights(self, weights: dict, group_size: int = 64, bits: int = 8) -> None:
        """A pre-quantized checkpoint under the internal names load_weights takes (what sanitize_klein_quantized_weights produces,
        weights.rs:599-): `<lin>.weight` packed uint32 [rows, cols * bits / 32] with `<lin>.scales` / `<lin>.biases` [rows, cols / group],
        and the bf16 norm `.weight`s.  Values are numpy arrays or device Tensors."""
        if self.cfg.tp_size > 1:
            raise OmxError("load_quantized_weights: packed weights with tensor parallelism are not supported")
        if bits not in (4, 8):
            raise OmxError(f"load_quantized_weights: bits must be 4 or 8 (got {bits})")
        def dev(a, code, what):
            if isinstance(a, Tensor):
                if a.dtype != code:
                    raise OmxError(f"load_quantized_weights: {what} is a device tensor of dtype {a.dtype}, expected {code}")
                return a
            if code == UINT32 and np.asarray(a).dtype != np.uint32:
                raise OmxError(f"load_quantized_weights: {what} must hold uint32 packed words (got {np.asarray(a).dtype})")
            return Tensor.from_numpy(a, "u32" if code == UINT32 else "bf16")
        for name in weights:
            if not name.endswith((".weight", ".scales", ".biases")):
                raise OmxError(f"load_quantized_weights: {name}: expected a `.weight`, `.scales` or `.biases` name")
            if name.endswith((".scales", ".biases")) and name.rsplit(".", 1)[0] + ".weight" not in weights:
                raise OmxError(f"load_quantized_weights: {name} has no `.weight` beside it")
        for name, arr in weights.items():
            if not name.endswith(".weight"):
                continue
            base = name[:-len(".weight")]
            if base + ".scales" not in weights:
                t = dev(arr, BFLOAT16, name)
                self._drop(name)
                self._keep.append(t)
                self._keep_of[name] = ("bf16", [t])
                check(lib.omx_klein_set_weight(self._h, name.encode(), t.ptr, t.nbytes))
                continue
            if base + ".biases" not in weights:
                raise OmxError(f"load_quantized_weights: {base}.biases is missing")
            q = dev(arr, UINT32, name)
            sc, bi = dev(weights[base + ".scales"], BFLOAT16, base + ".scales"), dev(weights[base + ".biases"], BFLOAT16, base + ".biases")
            rows, cols = q.shape[0], q.shape[-1] * 32 // bits
            if (len(q.shape) != 2 or cols % group_size or tuple(sc.shape) != (rows, cols // group_size)
                    or tuple(bi.shape) != (rows, cols // group_size)):
                raise OmxError(f"load_quantized_weights: {base}: packed {tuple(q.shape)}, scales {tuple(sc.shape)}, biases {tuple(bi.shape)} "
                               f"do not form one [{rows}, {cols}] matrix at {bits} bits, group {group_size}")
            check(lib.omx_klein_set_quantized_weight(self._h, name.encode(), q.ptr, sc.ptr, bi.ptr, rows, cols, group_size, bits))
            self._drop(name)
            self._keep += [q, sc, bi]
            self._keep_of[name] = ("packed", [q, sc, bi])

    def weight_bytes(self) -> int:
        """Device bytes of the tensors the forward reads (packed words + scales + biases of packed Linears, bf16 tensors)."""
        v = c_size_t()
        check(lib.omx_klein_weight_bytes(self._h, ctypes.byref(v)))
        return v.value

    def synth_weights(self, base_seed: int = 0x0C0FFEE5) -> None:
        check(lib.omx_klein_synth_weights(self._h, base_seed & 0xFFFFFFFF))

    def forward_with_rope(self, img: Tensor, txt: Tensor, timestep: float, rope_cos: Tensor, rope_sin: Tensor) -> Tensor:
        s_img, s_txt = img.shape[-2], txt.shape[-2]
        out = Tensor(img.shape, img.dtype)
        check(lib.omx_klein_forward_with_rope(self._h, out.ptr, img.ptr, txt.ptr, s_img, s_txt, timestep, rope_cos.ptr, rope_sin.ptr))
        return out

    def last_ms(self) -> float:
        v = c_float()
        check(lib.omx_klein_last_ms(self._h, ctypes.byref(v)))
        return v.value
