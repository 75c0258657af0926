"""Host mirror of qwen3-mlx's `Model` + `Generate` (qwen3-mlx/src/model.rs:473-498, 743-844)
over the fused decode engine of libomx_hip.so (include/omx.h, omx_qwen3_*)."""
from __future__ import annotations

import ctypes
import sys
from typing import Dict, Iterator, Optional

import numpy as np

from . import OmxError, Sampling, check, lib, require_device
from .ops import Tensor

c_int, c_float, c_void_p, c_uint32 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32


class Qwen3Config(ctypes.Structure):
    """omx_qwen3_config == the ModelArgs fields the forward uses (model.rs:47-64)."""
    _fields_ = [("hidden_size", c_int), ("num_hidden_layers", c_int), ("intermediate_size", c_int),
                ("num_attention_heads", c_int), ("num_key_value_heads", c_int), ("head_dim", c_int),
                ("vocab_size", c_int), ("rms_norm_eps", c_float), ("rope_theta", c_float), ("rope_scale", c_float),
                ("tie_word_embeddings", c_int), ("max_context", c_int), ("tp_rank", c_int), ("tp_size", c_int),
                ("quant_bits", c_int), ("quant_group", c_int), ("num_experts", c_int), ("num_experts_per_tok", c_int),
                ("moe_intermediate_size", c_int), ("moe_mode", c_int), ("norm_topk_prob", c_int), ("no_qk_norm", c_int),
                ("ep_rank", c_int), ("ep_size", c_int), ("attention_bias", c_int), ("quant_scales_f16", c_int),
                ("float16_weights", c_int)]


class DeepseekPlan(ctypes.Structure):
    """omx_qwen3_deepseek_plan: the DeepSeek-V2 family layer plan that goes beside a mode-2 Qwen3Config (omx_qwen3_create_deepseek)."""
    _fields_ = [("first_k_dense_replace", c_int), ("n_shared_experts", c_int), ("routed_scaling_factor", c_float)]


class GemvEx(ctypes.Structure):
    """omx_gemv_ex: every field of one dense decode GEMV launch (omx_debug_gemv_ex); route_* are filled in by the call."""
    _fields_ = [("out", c_void_p), ("argmax_slot", c_void_p), ("argmax_slot_n", c_int),
                ("x", c_void_p), ("norm_w", c_void_p), ("resid", c_void_p), ("bias", c_void_p),
                ("w0", c_void_p), ("w1", c_void_p), ("w2", c_void_p), ("n0", c_int), ("n1", c_int), ("N", c_int), ("K", c_int),
                ("pro", c_int), ("epi", c_int), ("f16", c_int), ("eps", c_float), ("single_round", c_int),
                ("rows_per_wave", c_int), ("row_offset", c_int),
                ("x_partial", c_void_p), ("x_partial_n", c_int), ("x_out", c_void_p), ("out_scale", c_void_p),
                ("n_batch", c_int), ("x_div", c_int), ("x_bstride", ctypes.c_longlong), ("out_bstride_bytes", ctypes.c_longlong),
                ("w_sel", c_void_p), ("w_estride", ctypes.c_longlong), ("w_sel_lo", c_int), ("w_sel_n", c_int),
                ("dry_run", c_int),
                ("route_nv", c_int), ("route_ksplit", c_int), ("route_tail", c_int), ("route_rows_per_wave", c_int), ("route_blocks", c_int)]


class QGemvMember(ctypes.Structure):
    """omx_qgemv_member: one packed matrix of a launch, with its own format (0: the launch's)"""
    _fields_ = [("w", c_void_p), ("scales", c_void_p), ("biases", c_void_p), ("n", c_int), ("bits", c_int), ("group", c_int)]


class QGemvEx(ctypes.Structure):
    """omx_qgemv_ex: every field of one packed decode GEMV launch (omx_debug_qgemv_ex); route_* are filled in by the call."""
    _fields_ = [("m", QGemvMember * 3),
                ("N", c_int), ("K", c_int), ("group", c_int), ("bits", c_int), ("pro", c_int), ("epi", c_int), ("eps", c_float),
                ("single_round", c_int),
                ("scales_f16", c_int), ("use_sb", c_int), ("use_tiles", c_int), ("mfma", c_int), ("row_offset", c_int), ("rolled_stage", c_int),
                ("n_batch", c_int), ("x_div", c_int), ("w_sel", c_void_p), ("w_estride", ctypes.c_longlong), ("s_estride", ctypes.c_longlong),
                ("w_sel_lo", c_int), ("w_sel_n", c_int), ("n_experts", c_int),
                ("x", c_void_p), ("norm_w", c_void_p), ("resid", c_void_p),
                ("out", c_void_p), ("out_f32", c_void_p), ("argmax_slot", c_void_p), ("argmax_slot_n", c_int),
                ("dry_run", c_int),
                ("route_kernel", c_int), ("route_bits", c_int), ("route_w", c_int), ("route_rb", c_int), ("route_rows_per_wave", c_int),
                ("route_sb", c_int), ("route_f16s", c_int), ("route_blocks", c_int), ("route_lds_bytes", c_int),
                ("route_ks", c_int), ("route_nu", c_int), ("route_nbuf", c_int)]


class AttnStepDbg(ctypes.Structure):
    """omx_attn_step_dbg: one step-attention launch on caller-owned buffers (omx_debug_attn_step); chunk / nsplit / abort_flag
    come back filled in."""
    _fields_ = [("qkv", c_void_p), ("k", c_void_p), ("v", c_void_p), ("H", c_int), ("Hkv", c_int), ("D", c_int), ("cap", c_int),
                ("scale", c_float), ("eps", c_float), ("q_norm_w", c_void_p), ("k_norm_w", c_void_p), ("rope_cur", c_void_p),
                ("granules", c_void_p), ("granules_n", ctypes.c_longlong),
                ("pos", c_int), ("seq", c_uint32), ("tag_mul", c_uint32), ("tag_add", c_uint32), ("f16", c_int),
                ("chunk", c_int), ("nsplit", c_int), ("tk_max", c_int), ("out", c_void_p), ("abort_flag", c_uint32)]


class GemvRowsSeg(ctypes.Structure):
    """omx_gemv_rows_seg: one plain segment of a segmented few-row launch"""
    _fields_ = [("w", c_void_p), ("bias", c_void_p), ("out", c_void_p), ("cols", c_int), ("ld", c_int)]


class GemvRowsDbg(ctypes.Structure):
    """omx_gemv_rows_dbg: one launch of the few-row bf16 Linear (omx_debug_gemv_rows), plain or segmented; route_rpw comes back
    filled in."""
    _fields_ = [("x", c_void_p), ("M", c_int), ("K", c_int), ("segmented", c_int),
                ("w", c_void_p), ("bias", c_void_p), ("resid", c_void_p), ("gate", c_void_p), ("relu", c_int), ("N", c_int), ("out", c_void_p),
                ("seg", GemvRowsSeg * 3), ("n_plain", c_int),
                ("w_gate", c_void_p), ("w_up", c_void_p), ("out_act", c_void_p), ("half", c_int), ("ld_act", c_int), ("act_mode", c_int),
                ("pre_norm_w", c_void_p), ("pre_norm_eps", c_float),
                ("route_rpw", c_int)]


ENGINE_SIGNATURES = {
    "omx_fill_uniform_2d": (c_int, [c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                    ctypes.c_int64, c_uint32, c_float, c_float, c_int, c_void_p]),
    "omx_qwen3_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(Qwen3Config)]),
    "omx_qwen3_create_deepseek": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(Qwen3Config), ctypes.POINTER(DeepseekPlan)]),
    "omx_qwen3_destroy": (c_int, [c_void_p]),
    "omx_qwen3_set_weight": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_qwen3_synth_weights": (c_int, [c_void_p, c_uint32]),
    "omx_qwen3_synth_weights_peaked": (c_int, [c_void_p, c_uint32]),
    "omx_qwen3_set_comm": (c_int, [c_void_p, c_void_p, c_void_p]),
    "omx_qwen3_set_sampler": (c_int, [c_void_p, ctypes.c_float, ctypes.c_uint64]),
    "omx_qwen3_set_sampling": (c_int, [c_void_p, ctypes.POINTER(Sampling), ctypes.c_uint64]),
    "omx_qwen3_sampler_state": (c_int, [c_void_p, c_void_p, c_int]),
    "omx_qwen3_encode": (c_int, [c_void_p, ctypes.POINTER(c_uint32), c_int, c_void_p, ctypes.POINTER(c_int), c_int, c_void_p]),
    "omx_qwen3_reset": (c_int, [c_void_p]),
    "omx_qwen3_offset": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "omx_qwen3_prefill": (c_int, [c_void_p, ctypes.POINTER(c_uint32), c_int, ctypes.POINTER(c_uint32)]),
    # a prompt pass over caller-supplied embedding rows (the reference's forward_embeddings), and the model's own rows
    "omx_qwen3_embed_tokens": (c_int, [c_void_p, ctypes.POINTER(c_uint32), c_int, c_void_p]),
    "omx_qwen3_prefill_embeds": (c_int, [c_void_p, ctypes.POINTER(c_uint32), c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_uint32)]),
    "omx_qwen3_decode": (c_int, [c_void_p, c_int, ctypes.POINTER(c_uint32)]),
    "omx_qwen3_last_logits": (c_int, [c_void_p, c_void_p, c_int]),
    # per-token log-probabilities of the tokens being generated, inside the step (csrc/logprob.hip's top-n form)
    "omx_qwen3_set_logprobs": (c_int, [c_void_p, c_int]),
    "omx_qwen3_decode_logprobs": (c_int, [c_void_p, c_int, ctypes.POINTER(c_uint32), ctypes.POINTER(c_float), c_void_p, c_void_p]),
    "omx_qwen3_last_logprobs": (c_int, [c_void_p, ctypes.POINTER(c_float), c_void_p, c_void_p]),
    "omx_qwen3_last_decode_ms": (c_int, [c_void_p, ctypes.POINTER(c_float)]),
    "omx_qwen3_last_prefill_ms": (c_int, [c_void_p, ctypes.POINTER(c_float)]),
    "omx_qwen3_dequant_bytes": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_size_t)]),
    "omx_qwen3_debug_read": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_qwen3_debug_write": (c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "omx_qwen3_stream": (c_int, [c_void_p, ctypes.POINTER(c_void_p)]),
    "omx_qwen3_step_bytes": (c_int, [c_void_p, c_int, ctypes.POINTER(ctypes.c_double)]),
    "omx_qwen3_decode_path": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "omx_qwen3_debug_trace_step": (c_int, [c_void_p, c_void_p, ctypes.c_size_t, ctypes.POINTER(c_int)]),
    "omx_qwen3_time_step_kernels": (c_int, [c_void_p, c_int, ctypes.POINTER(ctypes.c_float)]),
    "omx_qwen3_debug_trace_engine": (c_int, [c_void_p, c_void_p, ctypes.c_size_t, ctypes.POINTER(c_int)]),
    "omx_qwen3_debug_step_forms": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "omx_qwen3_debug_raise_give_up": (c_int, [c_void_p]),
    "omx_qwen3_verify": (c_int, [c_void_p, ctypes.POINTER(c_uint32), c_int, ctypes.POINTER(c_uint32)]),
    "omx_qwen3_verify_logits": (c_int, [c_void_p, c_int, c_void_p, c_int]),
    "omx_qwen3_trim": (c_int, [c_void_p, c_int, c_uint32]),
    "omx_qwen3_score": (c_int, [c_void_p, ctypes.POINTER(c_uint32), c_int, ctypes.POINTER(c_uint32), ctypes.POINTER(c_float), ctypes.POINTER(c_uint32)]),
    "omx_qwen3_last_score_ms": (c_int, [c_void_p, ctypes.POINTER(c_float), ctypes.POINTER(c_float)]),
    "omx_qwen3_get_weight": (c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_size_t)]),
    # mixed-precision MLX checkpoints: one packed matrix's own (bits, group_size), and the query
    "omx_qwen3_set_quant_format": (c_int, [c_void_p, ctypes.c_char_p, c_int, c_int]),
    "omx_qwen3_quant_format": (c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    # batched decode: up to 8 independent sequences per step on one loaded model (csrc/engine_batch.hip)
    "omx_qwen3_batch_create": (c_int, [ctypes.POINTER(c_void_p), c_void_p, c_int, c_int]),
    "omx_qwen3_batch_destroy": (c_int, [c_void_p]),
    "omx_qwen3_batch_set_sampler": (c_int, [c_void_p, c_int, ctypes.c_float, ctypes.c_uint64]),
    "omx_qwen3_batch_set_sampling": (c_int, [c_void_p, c_int, ctypes.POINTER(Sampling), ctypes.c_uint64]),
    "omx_qwen3_batch_prefill": (c_int, [c_void_p, c_int, ctypes.POINTER(c_uint32), c_int, ctypes.POINTER(c_uint32)]),
    "omx_qwen3_batch_prefill_embeds": (c_int, [c_void_p, c_int, ctypes.POINTER(c_uint32), c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_uint32)]),
    "omx_qwen3_batch_decode": (c_int, [c_void_p, ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(c_uint32)]),
    "omx_qwen3_batch_logits": (c_int, [c_void_p, c_int, c_void_p, c_int]),
    "omx_qwen3_batch_offset": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int)]),
    "omx_qwen3_batch_trim": (c_int, [c_void_p, c_int, c_int, c_uint32]),
    "omx_qwen3_batch_reset": (c_int, [c_void_p, c_int]),
    "omx_qwen3_batch_last_decode_ms": (c_int, [c_void_p, ctypes.POINTER(c_float)]),
    "omx_qwen3_batch_fork": (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_uint32)]),
    "omx_qwen3_batch_shared": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "omx_qwen3_batch_set_logprobs": (c_int, [c_void_p, c_int]),
    "omx_qwen3_batch_decode_logprobs": (c_int, [c_void_p, ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(c_uint32), ctypes.POINTER(c_float),
                                                c_void_p, c_void_p]),
    "omx_qwen3_batch_last_logprobs": (c_int, [c_void_p, c_int, ctypes.POINTER(c_float), c_void_p, c_void_p]),
    # ... with its K/V storage chosen (kv_bits 8: MLX affine rows, quantised on append, read packed), and what reads the slabs back
    "omx_qwen3_batch_create_kv": (c_int, [ctypes.POINTER(c_void_p), c_void_p, c_int, c_int, c_int]),
    "omx_qwen3_batch_kv_bytes": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_size_t)]),
    "omx_qwen3_batch_kv_read": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "omx_qwen3_batch_debug_attention": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int), c_int, c_void_p, c_void_p]),
    # test hook of the dense decode GEMV (csrc/gemv.hip): one launch of a prologue / epilogue form, bf16 or float16
    "omx_debug_gemv": (c_int, [c_void_p] * 9 + [c_int] * 7 + [c_float, c_int, c_void_p]),
    "omx_debug_gemv_grid": (c_int, [c_int, c_int]),
    # ... every field of the launch (rows_per_wave, argmax row_offset, x_partial fold, EPI_F32 out_scale, batched / expert-selected
    # entries) and the route it takes; the step attention (csrc/attn_step.hip) on caller-owned buffers
    "omx_debug_gemv_ex": (c_int, [ctypes.POINTER(GemvEx), c_void_p]),
    "omx_debug_attn_step": (c_int, [ctypes.POINTER(AttnStepDbg), c_void_p]),
    # the packed decode GEMV (csrc/quant.hip, qgemv_mfma.hip): every field of the launch, and the kernel it resolved to
    "omx_debug_qgemv_ex": (c_int, [ctypes.POINTER(QGemvEx), c_void_p]),
    # the few-row bf16 Linear (csrc/gemv_rows.hip), plain or segmented, without the GEMM entry's N * K routing threshold
    "omx_debug_gemv_rows": (c_int, [ctypes.POINTER(GemvRowsDbg), c_void_p]),
    "omx_bench_qwen3_per_op": (c_int, [c_void_p, ctypes.POINTER(Qwen3Config), ctypes.POINTER(c_uint32), c_int, c_int, ctypes.POINTER(c_uint32),
                                       ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
}
for _n, (_r, _a) in ENGINE_SIGNATURES.items():
    _f = getattr(lib, _n)
    _f.restype, _f.argtypes = _r, _a


def rope_scale_from_config(rope_scaling: Optional[dict]) -> float:
    """mlx_rs_core::initialize_rope (utils.rs:52-97): only default / linear are accepted."""
    rope_type = "default"
    if rope_scaling is not None:
        rope_type = rope_scaling.get("type", rope_scaling.get("rope_type", "default"))
    if rope_type == "default":
        return 1.0
    if rope_type == "linear":
        if "factor" not in rope_scaling:
            raise OmxError('key "factor" is not found in scaling config')
        try:
            return 1.0 / float(rope_scaling["factor"])
        except (TypeError, ValueError):
            raise OmxError('key "factor" is not a valid float')
    raise OmxError(f"Unsupported RoPE type {rope_type!r}")


def dense_dtype_is_f16(dtype) -> bool:
    """engine.Model(dtype=...): True for float16, False for bfloat16; anything else is refused."""
    d = str(dtype).lower()
    if d in ("float16", "f16", "half"):
        return True
    if d in ("bfloat16", "bf16"):
        return False
    raise OmxError(f"Model: dtype {dtype!r} (bfloat16 or float16)")


QUANT_BITS, QUANT_GROUPS = (2, 3, 4, 5, 6, 8), (32, 64, 128)
_QUANT_SCALARS = ("bits", "group_size", "mode", "scales_dtype")


def quant_formats(quantization):
    """config.json's "quantization" block -> (base, table): base = (bits, group_size) or None for an unquantised checkpoint, table =
    {module path: (bits, group_size)} for the nested per-module entries a mixed-precision MLX checkpoint carries next to the global
    pair ("model.layers.3.mlp.down_proj": {"group_size": 64, "bits": 6}).  An entry's missing field is the base's.  "mode" is accepted
    only as "affine"; an entry that is False / True (an unquantised or default member inside a packed model) or names another mode is
    refused with the module path.  Pure: no device, no model."""
    if not quantization:
        return None, {}
    q = dict(quantization)
    if str(q.get("mode", "affine")) != "affine":
        raise OmxError(f"InvalidConfig: quantization mode {q['mode']!r} (only MLX's affine mode is supported)")
    base = (int(q.get("bits", 0)), int(q.get("group_size", 64)))
    if base[0] == 0:          # (bits 0 is the config field's "not quantised")
        return None, {}
    if base[0] not in QUANT_BITS:
        raise OmxError(f"InvalidConfig: quantization bits {base[0]} (2, 3, 4, 5, 6, 8)")
    if base[1] not in QUANT_GROUPS:
        raise OmxError(f"InvalidConfig: quantization group_size {base[1]} (32, 64, 128)")
    table = {}
    for prefix, entry in q.items():
        if prefix in _QUANT_SCALARS:
            continue
        if isinstance(entry, bool):
            raise OmxError(f"InvalidConfig: quantization entry {prefix}: {entry} -- a member that is not an affine (bits, group_size) "
                           "format of its own inside a packed model is not supported")
        if not isinstance(entry, dict):
            continue      # (other scalar keys of the block say nothing about a matrix)
        if str(entry.get("mode", "affine")) != "affine":
            raise OmxError(f"InvalidConfig: quantization entry {prefix}: mode {entry['mode']!r} (only MLX's affine mode is supported)")
        bits, group = int(entry.get("bits", base[0])), int(entry.get("group_size", base[1]))
        if bits not in QUANT_BITS:
            raise OmxError(f"InvalidConfig: quantization entry {prefix}: bits {bits} (2, 3, 4, 5, 6, 8)")
        if group not in QUANT_GROUPS:
            raise OmxError(f"InvalidConfig: quantization entry {prefix}: group_size {group} (32, 64, 128)")
        table[prefix] = (bits, group)
    return base, table


def mixed_recipe(recipe: str, num_layers: int):
    """The layers whose v_proj and down_proj an `mlx_lm.convert --quant-predicate mixed_<low>_<high>` checkpoint keeps at the wide
    format, as (low_bits, high_bits, [layer indices]).  The rule is written down FROM MEMORY of mlx_lm (its source is not at hand) and
    nothing in the engine depends on it being mlx_lm's: layer i is wide when i < L // 8 or i >= 7 * L // 8 or (i - L // 8) % 3 == 2;
    lm_head is wide, everything else narrow, group 64."""
    known = {"mixed_2_6": (2, 6), "mixed_3_4": (3, 4), "mixed_3_6": (3, 6), "mixed_4_6": (4, 6)}
    if recipe not in known:
        raise OmxError(f"mixed_recipe: {recipe!r} (one of {', '.join(sorted(known))})")
    low, high = known[recipe]
    L = int(num_layers)
    wide = [i for i in range(L) if i < L // 8 or i >= 7 * L // 8 or (i - L // 8) % 3 == 2]
    return low, high, wide


def mixed_recipe_quantization(recipe: str, num_layers: int, tie_word_embeddings: bool = False, group_size: int = 64) -> dict:
    """mixed_recipe as the config.json "quantization" block such a checkpoint would carry."""
    low, high, wide = mixed_recipe(recipe, num_layers)
    q = {"group_size": group_size, "bits": low}
    for i in wide:
        for sub in ("self_attn.v_proj", "mlp.down_proj"):
            q[f"model.layers.{i}.{sub}"] = {"group_size": group_size, "bits": high}
    if not tie_word_embeddings:
        q["lm_head"] = {"group_size": group_size, "bits": high}
    return q


def expected_shape(c: Qwen3Config, name: str, formats=None, plan=None):
    """Shape the engine will read for checkpoint tensor `name` on THIS rank (after the TP / EP slicing), or None for a
    name the forward does not use.  Mirrors resolve_weights in csrc/engine_weights.hip.  formats: {module path: (bits, group_size)} of
    the matrices that have a format of their own (quant_formats); every other packed matrix has the config's base format.  plan: the
    DeepseekPlan of a moe_mode "deepseek" model (None: every layer routes, no shared experts)."""
    tp, ep = max(c.tp_size, 1), max(c.ep_size, 1)
    hd, D = c.hidden_size, c.head_dim
    H, Hkv, I, V = c.num_attention_heads // tp, max(1, c.num_key_value_heads // tp), c.intermediate_size // tp, c.vocab_size
    Im, E = c.moe_intermediate_size, c.num_experts
    if E > 0 and tp > 1:      # expert tensor parallel: this rank's intermediate columns of every expert
        Im //= tp
    leaf_kind = None
    for suffix in (".weight", ".scales", ".biases", ".bias"):
        if name.endswith(suffix):
            leaf_kind, stem = suffix[1:], name[:-len(suffix)]
            break
    if leaf_kind is None:
        return None
    quant = bool(c.quant_bits)

    def lin(n, k, stack=()):
        """[n, k] Linear: dense, or the packed triplet of a quantized checkpoint."""
        if leaf_kind == "bias":
            return (n,)
        if not quant:
            return tuple(stack) + (n, k) if leaf_kind == "weight" else None
        bits, group = (formats or {}).get(stem, (c.quant_bits, c.quant_group))      # the matrix's own format
        if leaf_kind == "weight":
            return tuple(stack) + (n, k * bits // 32)
        return tuple(stack) + (n, k // group)

    if stem == "model.embed_tokens":
        return lin(V, hd)
    if stem == "lm_head":
        return lin(V // tp, hd)
    if stem == "model.norm":
        return (hd,) if leaf_kind == "weight" else None
    parts = stem.split(".")
    if len(parts) < 4 or parts[0] != "model" or parts[1] != "layers":
        return None
    sub = ".".join(parts[3:])
    table = {"self_attn.q_proj": (H * D, hd), "self_attn.k_proj": (Hkv * D, hd), "self_attn.v_proj": (Hkv * D, hd),
             "self_attn.o_proj": (hd, H * D), "mlp.gate_proj": (I, hd), "mlp.up_proj": (I, hd), "mlp.down_proj": (hd, I)}
    ds = E > 0 and c.moe_mode == MOE_MODES["deepseek"]
    if ds:      # the per-layer plan: a dense prefix, then router + stacks + shared experts; a name its layer does not read has no shape
        plan = plan or DeepseekPlan(0, 0, 1.0)
        is_moe = int(parts[2]) >= plan.first_k_dense_replace
        moe_name = sub == "mlp.gate" or sub.startswith("mlp.switch_mlp.") or sub.startswith("mlp.shared_experts.")
        if (sub in ("mlp.gate_proj", "mlp.up_proj", "mlp.down_proj") and is_moe) or (moe_name and not is_moe):
            return None
        Ws = plan.n_shared_experts * Im
        if Ws and sub in ("mlp.shared_experts.gate_proj", "mlp.shared_experts.up_proj"):
            return lin(Ws, hd)
        if Ws and sub == "mlp.shared_experts.down_proj":
            return lin(hd, Ws)
    if sub in table:
        return lin(*table[sub])
    if sub in ("input_layernorm", "post_attention_layernorm"):
        return (hd,) if leaf_kind == "weight" else None
    if sub in ("self_attn.q_norm", "self_attn.k_norm"):
        return (D,) if leaf_kind == "weight" else None
    if E > 0:
        El = E // ep
        for mp in ("block_sparse_moe.", "mlp."):
            if sub == mp + "gate":
                return lin(E, hd)
            if sub in (mp + "switch_mlp.gate_proj", mp + "switch_mlp.up_proj"):
                return lin(Im, hd, (El,))
            if sub == mp + "switch_mlp.down_proj":
                return lin(hd, Im, (El,))
    return None


MOE_MODES = {"mixtral": 0, "qwen3_moe": 1, "deepseek": 2}


class Model:
    """qwen3_mlx::Model (dense Qwen3) resident on one MI355X (or one TP shard of it)."""

    logprobs_top = None   # set_logprobs: alternatives reported per generated token (None = off)

    def __init__(self, *, hidden_size, num_hidden_layers, intermediate_size, num_attention_heads,
                 num_key_value_heads, head_dim, vocab_size, rms_norm_eps=1e-6, rope_theta=1e6,
                 tie_word_embeddings=False, rope_scaling=None, max_context=4096, tp_rank=0, tp_size=1, quantization=None,
                 num_experts=0, num_experts_per_tok=0, moe_intermediate_size=0, moe_mode="qwen3_moe", norm_topk_prob=False,
                 qk_norm=True, ep_rank=0, ep_size=1, attention_bias=False, dtype="bfloat16", first_k_dense_replace=0,
                 n_shared_experts=0, routed_scaling_factor=1.0, **_ignored):
        """quantization: config.json's {"bits": 2|3|4|5|6|8, "group_size": 64} (model.rs:63) or None for a bf16 checkpoint (2, 3,
        5 and 6 bits: dense single-rank models only); nested entries {module path: {"bits", "group_size"}} give single matrices a
        format of their own (a mixed-precision MLX checkpoint; quant_formats; dense single-rank bf16-triplet models); + "scales_dtype":
        "float16" when the checkpoint's scales / biases are float16 (loader.load_model reads it off the tensors' dtype).
        num_experts > 0: sparse-MoE feed-forward in every layer -- moe_mode "qwen3_moe" (qwen3_moe.rs ModelArgs :60-87) or
        "mixtral" (mixtral-mlx ModelArgs :54-80, with qk_norm=False and moe_intermediate_size = intermediate_size).
        moe_mode "deepseek" (deepseek-ocr2-mlx/src/lib.rs:70-130, the DeepSeek-V2 family): layers [0, first_k_dense_replace) are dense
        MLPs of intermediate_size, the rest route in float32 over num_experts with routed_scaling_factor and add n_shared_experts
        shared experts ("mlp.shared_experts.*" at n_shared_experts * moe_intermediate_size); bf16, one rank, qk_norm=False.
        dtype: the weight dtype of a dense (unquantised) checkpoint -- "bfloat16" (default) or "float16"; a float16 model runs in
        float16 end to end, like MLX runs a checkpoint saved in float16 (single rank, dense MLP, head_dim 128)."""
        require_device()
        q = quantization or {}
        _, table = quant_formats(quantization)
        f16_weights = dense_dtype_is_f16(dtype)
        self.cfg = Qwen3Config(hidden_size, num_hidden_layers, intermediate_size, num_attention_heads,
                               num_key_value_heads, head_dim, vocab_size, rms_norm_eps, rope_theta,
                               rope_scale_from_config(rope_scaling), int(bool(tie_word_embeddings)), max_context,
                               tp_rank, tp_size, int(q.get("bits", 0)), int(q.get("group_size", 64 if q else 0)),
                               int(num_experts), int(num_experts_per_tok), int(moe_intermediate_size),
                               MOE_MODES[moe_mode], int(bool(norm_topk_prob)), int(not qk_norm),
                               int(ep_rank), int(ep_size), int(bool(attention_bias)),
                               int(str(q.get("scales_dtype", "bfloat16")).lower() in ("float16", "f16", "half")),
                               int(f16_weights))
        self._h = c_void_p()
        self.plan = None
        if moe_mode == "deepseek" or first_k_dense_replace or n_shared_experts:      # (on another mode the engine refuses the plan by name)
            self.plan = DeepseekPlan(int(first_k_dense_replace), int(n_shared_experts), float(routed_scaling_factor))
            check(lib.omx_qwen3_create_deepseek(ctypes.byref(self._h), ctypes.byref(self.cfg), ctypes.byref(self.plan)))
        else:
            check(lib.omx_qwen3_create(ctypes.byref(self._h), ctypes.byref(self.cfg)))
        self._keep = []
        # per-matrix formats: what differs from the base goes to the engine (an entry that repeats the base changes nothing; a tied head
        # has the embedding's format, so a stray lm_head entry of a tied model names no matrix)
        base = (self.cfg.quant_bits, self.cfg.quant_group)
        self.quant_table = {p: f for p, f in table.items() if f != base and not (p == "lm_head" and self.cfg.tie_word_embeddings)}
        for prefix, (bits, group) in self.quant_table.items():
            check(lib.omx_qwen3_set_quant_format(self._h, prefix.encode(), bits, group))

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.omx_qwen3_destroy(h)
            self._h = c_void_p()

    def __del__(self):
        # never call into HIP while the interpreter (and possibly the HIP runtime / a profiler
        # layered on it) is being torn down
        if sys is not None and not sys.is_finalizing():   # (module globals are already None late in shutdown)
            self.close()

    @property
    def f16(self) -> bool:
        """The model runs in float16 (a packed checkpoint with float16 triplets, or dense float16 weights)."""
        return bool(self.cfg.quant_scales_f16 or self.cfg.float16_weights)

    @property
    def vocab_local(self) -> int:
        return self.cfg.vocab_size // self.cfg.tp_size

    def load_weights(self, weights: Dict[str, np.ndarray]) -> None:
        """ModuleParametersExt::load_safetensors equivalent for in-memory arrays keyed by HF name."""
        if self.cfg.tp_size > 1:   # slice the logical checkpoint with the shared shard plan (tp.py)
            from . import tp
            weights = tp.shard_state_dict(weights, self.cfg.tp_rank, self.cfg.tp_size, bool(self.cfg.tie_word_embeddings),
                                          self.cfg.num_key_value_heads, self.cfg.head_dim)
        if self.cfg.ep_size > 1:   # expert parallel: this rank keeps its slice of every stacked expert tensor
            from . import ep
            weights = {k: (ep.shard_experts(v, self.cfg.ep_rank, self.cfg.ep_size) if ".switch_mlp." in k else v)
                       for k, v in weights.items()}
        for name, arr in weights.items():
            # the engine takes raw device pointers: a tensor whose shape disagrees with the config would be read past its
            # end, so every known name is checked here (the reference raises a shape error on load)
            want = self.expected_shape(name)
            if want is not None and tuple(arr.shape) != want:
                raise OmxError(f"ShapeMismatch: {name} has shape {tuple(arr.shape)}, the config expects {want}")
            dt = np.asarray(arr).dtype
            if self.cfg.quant_bits and name.endswith((".scales", ".biases")):
                # float16 triplets (an MLX float16 checkpoint) stay float16 on the device: the packed-weight kernels widen each group's
                # scale / bias to its exact float32 value (a host-side rounding to bf16 shifts every weight of a group by the same amount
                # -- measured outside the decoder's logit bound).  The model must have been created for them.
                f16 = dt == np.float16
                if f16 != bool(self.cfg.quant_scales_f16):
                    raise OmxError(f"{name}: {'float16' if f16 else str(dt)} scales / biases, but the model was created with "
                                   f"quantization scales_dtype={'float16' if self.cfg.quant_scales_f16 else 'bfloat16'}")
                if f16:
                    t = Tensor.from_numpy(arr, "f16")
                    self._keep.append(t)
                    check(lib.omx_qwen3_set_weight(self._h, name.encode(), t.ptr, t.nbytes))
                    continue
            if self.cfg.quant_bits and name.endswith(".weight") and name[:-7] + ".scales" in weights and dt != np.uint32:
                raise OmxError(f"{name}: a quantized weight must be packed uint32, found {dt}")
            # quantized checkpoints: "<prefix>.weight" is packed uint32 (ops/quantization.rs:41-84), scales / biases bf16; in a float16
            # checkpoint every other tensor (the norm weights) is float16 too -- the model then runs in float16 end to end, like in MLX
            if self.f16 and dt != np.uint32 and type(arr).__name__ == "Bf16Bits":
                # a BF16 tensor of a checkpoint whose triplets are float16 (loader.read_safetensors hands raw bits): its VALUES go up as float16
                arr = (np.asarray(arr).astype(np.uint32) << np.uint32(16)).view(np.float32)
            t = Tensor.from_numpy(arr, "u32" if dt == np.uint32 else "f16" if self.f16 else "bf16")
            self._keep.append(t)
            check(lib.omx_qwen3_set_weight(self._h, name.encode(), t.ptr, t.nbytes))

    def expected_shape(self, name: str):
        return expected_shape(self.cfg, name, self.quant_table, self.plan)

    def quant_format(self, prefix: str) -> tuple:
        """(bits, group_size) of the packed matrix at module path `prefix`: its own, or the base format (omx_qwen3_quant_format)."""
        bits, group = c_int(), c_int()
        check(lib.omx_qwen3_quant_format(self._h, prefix.encode(), ctypes.byref(bits), ctypes.byref(group)))
        return bits.value, group.value

    def synth_weights(self, base_seed: int = 0x0C0FFEE5, peaked: bool = False) -> None:
        """peaked: embedding std 64 and lm_head[v] = table[(v + 1) mod V] -- greedy tokens count down with top-1 margins far above the
        bf16 bound (full-size parity tests assert token equality; oracle/ref_qwen3.py synth_weights(peaked=True))."""
        fn = lib.omx_qwen3_synth_weights_peaked if peaked else lib.omx_qwen3_synth_weights
        check(fn(self._h, base_seed & 0xFFFFFFFF))

    def set_comm(self, comm_ptr: int, allreduce_fn_ptr: int) -> None:
        check(lib.omx_qwen3_set_comm(self._h, comm_ptr, allreduce_fn_ptr))

    def encode(self, input_ids, attention_mask=None, extract_layers=(8, 17, 26)):
        """Qwen3TextEncoder::encode (flux-klein-mlx/src/qwen3_encoder.rs:403-455): hidden states after the tapped
        layers (0-indexed, raw, no final norm) concatenated on the last axis -> device Tensor [n, len(taps)*hidden]."""
        from .ops import Tensor
        ids = np.ascontiguousarray(np.asarray(input_ids, dtype=np.uint32).ravel())
        taps = (c_int * len(extract_layers))(*[int(t) for t in extract_layers])
        out = Tensor((ids.size, len(extract_layers) * self.cfg.hidden_size), "f16" if self.f16 else "bf16")
        am = None
        if attention_mask is not None:
            am = np.ascontiguousarray(np.asarray(attention_mask).ravel() != 0, dtype=np.uint8)
            if am.size != ids.size:
                raise OmxError("encode: attention_mask and input_ids differ in length")
        check(lib.omx_qwen3_encode(self._h, ids.ctypes.data_as(ctypes.POINTER(c_uint32)), ids.size,
                                   am.ctypes.data if am is not None else None, taps, len(extract_layers), out.ptr))
        return out

    def set_sampler(self, temperature: float, seed: int = 0, *, top_k: int = 0, top_p: float = 1.0, repetition_penalty: float = 1.0,
                    presence_penalty: float = 0.0) -> None:
        """DefaultSampler (mlx-rs-core/src/sampler.rs:9-18): 0 = greedy, otherwise categorical(logits / temperature)
        drawn on the device with the key sequence of `mlx_rs::random::seed(seed)`.
        The keywords put the filters of the reference's generation loops in front of the draw, inside the same device step
        (omx_sample_filtered's rule): repetition_penalty (step-audio2-mlx/src/llm.rs:440-474) and presence_penalty
        (funasr-qwen4b-mlx/src/model.rs:1342-1352) on the tokens sampled since the last prefill, top_k (ties kept, :1357-1372), top_p on
        the survivors.  Their defaults are off: the call is then the plain sampler, bit for bit."""
        if top_k == 0 and top_p == 1.0 and repetition_penalty == 1.0 and presence_penalty == 0.0:
            check(lib.omx_qwen3_set_sampler(self._h, float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF))
            return
        p = Sampling(temperature, top_k, top_p, repetition_penalty, presence_penalty)
        check(lib.omx_qwen3_set_sampling(self._h, ctypes.byref(p), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def sampler_state(self) -> tuple:
        """The two words of the sampler's key sequence (after set_sampler): the reference's speculative loop draws both models' tokens from
        ONE global sequence, which two models reproduce by handing this state over (speculative.py)."""
        st = (c_uint32 * 2)()
        check(lib.omx_qwen3_sampler_state(self._h, st, 0))
        return int(st[0]), int(st[1])

    def set_sampler_state(self, state) -> None:
        st = (c_uint32 * 2)(int(state[0]), int(state[1]))
        check(lib.omx_qwen3_sampler_state(self._h, st, 1))

    def reset(self) -> None:
        check(lib.omx_qwen3_reset(self._h))

    def offset(self) -> int:
        v = c_int()
        check(lib.omx_qwen3_offset(self._h, ctypes.byref(v)))
        return v.value

    def embed_tokens(self, ids):
        """get_token_embeddings (qwen3-asr-mlx/src/model.rs:726): the model's own embedding rows of `ids`, a device Tensor
        [n, hidden] in the activation dtype -- the bits the prompt pass gathers (omx_qwen3_embed_tokens)."""
        from .ops import Tensor
        p = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).ravel())
        out = Tensor((p.size, self.cfg.hidden_size), "f16" if self.f16 else "bf16")
        check(lib.omx_qwen3_embed_tokens(self._h, p.ctypes.data_as(ctypes.POINTER(c_uint32)), p.size, out.ptr))
        return out

    def prefill(self, prompt, embeds=None, embeds_at: int = 0) -> int:
        """The prompt's first sampled token.  embeds: rows [n_rows, hidden] that replace the embedding rows of positions
        [embeds_at, embeds_at + n_rows) -- the reference's forward_embeddings (omx_qwen3_prefill_embeds): a device Tensor (f32, bf16 or
        f16) or a float32 / float16 numpy array; the ids at those positions are still required (the pad token)."""
        p = np.ascontiguousarray(prompt, dtype=np.uint32)
        first = c_uint32()
        if embeds is None:
            check(lib.omx_qwen3_prefill(self._h, p.ctypes.data_as(ctypes.POINTER(c_uint32)), p.size, ctypes.byref(first)))
            return first.value
        from .ops import Tensor
        if not isinstance(embeds, Tensor):
            a = np.asarray(embeds)
            embeds = Tensor.from_numpy(a, "f16" if a.dtype == np.float16 else "f32")
        if len(embeds.shape) != 2 or embeds.shape[1] != self.cfg.hidden_size:
            raise OmxError(f"ShapeMismatch: embeds has shape {embeds.shape}, the model expects [n_rows, {self.cfg.hidden_size}]")
        check(lib.omx_synchronize(None))   # the rows may come from ops on the null stream; the pass runs on the model's own
        check(lib.omx_qwen3_prefill_embeds(self._h, p.ctypes.data_as(ctypes.POINTER(c_uint32)), p.size, embeds.ptr if embeds.shape[0] else None,
                                           embeds.dtype, int(embeds_at), embeds.shape[0], ctypes.byref(first)))
        return first.value

    def set_logprobs(self, top_n=None) -> None:
        """Per-token log-probabilities inside the step (omx_qwen3_set_logprobs): None = off (default), 0 = the drawn token's only,
        1..20 = with that many alternatives.  They are the log-softmax of the RAW logits row (what last_logits() returns): before
        temperature, top-k / top-p and penalties, as score() reports them."""
        check(lib.omx_qwen3_set_logprobs(self._h, -1 if top_n is None else int(top_n)))
        self.logprobs_top = None if top_n is None or int(top_n) < 0 else int(top_n)

    def decode(self, n: int, return_logprobs: bool = False):
        """n further tokens, uint32 [n].  return_logprobs (after set_logprobs): (tokens, logprobs float32 [n]) and, with alternatives
        on, (tokens, logprobs, top_ids uint32 [n, top_n], top_logprobs float32 [n, top_n])."""
        out = np.empty(n, dtype=np.uint32)
        if not return_logprobs:
            check(lib.omx_qwen3_decode(self._h, n, out.ctypes.data_as(ctypes.POINTER(c_uint32))))
            return out
        top = self.logprobs_top or 0
        lp, ids, tlp = np.zeros(n, np.float32), np.zeros((n, top), np.uint32), np.zeros((n, top), np.float32)
        check(lib.omx_qwen3_decode_logprobs(self._h, n, out.ctypes.data_as(ctypes.POINTER(c_uint32)), lp.ctypes.data_as(ctypes.POINTER(c_float)),
                                            ids.ctypes.data if top else None, tlp.ctypes.data if top else None))
        return (out, lp, ids, tlp) if top else (out, lp)

    def last_logprobs(self):
        """Of the most recently sampled token (after a prefill: its first token): logprob, or (logprob, top_ids, top_logprobs)."""
        top = self.logprobs_top or 0
        lp, ids, tlp = c_float(), np.zeros(top, np.uint32), np.zeros(top, np.float32)
        check(lib.omx_qwen3_last_logprobs(self._h, ctypes.byref(lp), ids.ctypes.data if top else None, tlp.ctypes.data if top else None))
        return (np.float32(lp.value), ids, tlp) if top else np.float32(lp.value)

    def verify(self, tokens) -> np.ndarray:
        """speculative.rs:132-161 `verify_draft_tokens`: all tokens in one batched pass on top of the cache; greedy token per position."""
        ids = np.ascontiguousarray(np.asarray(tokens, dtype=np.uint32).ravel())
        out = np.empty(ids.size, dtype=np.uint32)
        check(lib.omx_qwen3_verify(self._h, ids.ctypes.data_as(ctypes.POINTER(c_uint32)), ids.size, out.ctypes.data_as(ctypes.POINTER(c_uint32))))
        return out

    def verify_logits(self, row: int) -> np.ndarray:
        raw = np.empty(self.vocab_local, dtype=np.uint16)
        check(lib.omx_qwen3_verify_logits(self._h, row, raw.ctypes.data, raw.size))
        return (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)

    def trim(self, n: int, next_token: int) -> None:
        """KeyValueCache::trim(n) (missing in the reference, speculative.rs:165-169) + the next step's input token."""
        check(lib.omx_qwen3_trim(self._h, n, int(next_token)))

    def score(self, tokens, next_token=None, return_greedy=False):
        """Per-token log-probabilities of a text from ONE batched pass on top of the cache (omx_qwen3_score): entry i is
        log p(tokens[i + 1] | cache, tokens[:i + 1]), float32 [n - 1] -- or [n] with next_token, the target of the last position.  The n
        tokens are appended to the cache (offset() advances by n); the pending input token becomes the last row's argmax, trim(0, tok)
        sets another.  return_greedy: also the argmax of every one of the n rows, uint32 [n]."""
        ids = np.ascontiguousarray(np.asarray(tokens, dtype=np.uint32).ravel())
        last = 0xFFFFFFFF if next_token is None else int(next_token)
        targets = np.ascontiguousarray(np.concatenate([ids[1:], np.array([last], dtype=np.uint32)]), dtype=np.uint32)
        lp = np.zeros(ids.size, dtype=np.float32)
        greedy = np.zeros(ids.size, dtype=np.uint32)
        u32p = ctypes.POINTER(c_uint32)
        check(lib.omx_qwen3_score(self._h, ids.ctypes.data_as(u32p), ids.size, targets.ctypes.data_as(u32p),
                                  lp.ctypes.data_as(ctypes.POINTER(c_float)), greedy.ctypes.data_as(u32p)))
        if next_token is None:
            lp = lp[:-1]
        return (lp, greedy) if return_greedy else lp

    def last_score_ms(self) -> tuple:
        """Device ms of the last score() call: (the prompt pass, the head: final norm + panel GEMMs + statistics + merge)."""
        a, b = c_float(), c_float()
        check(lib.omx_qwen3_last_score_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def last_decode_ms(self) -> float:
        v = c_float()
        check(lib.omx_qwen3_last_decode_ms(self._h, ctypes.byref(v)))
        return v.value

    def dequant_bytes(self) -> int:
        """Device bytes held for dequantised weights (dequant cache slab + scratch of the prompt pass); 0 for a bf16 model."""
        v = ctypes.c_size_t()
        check(lib.omx_qwen3_dequant_bytes(self._h, ctypes.byref(v)))
        return int(v.value)

    def last_prefill_ms(self) -> float:
        v = c_float()
        check(lib.omx_qwen3_last_prefill_ms(self._h, ctypes.byref(v)))
        return v.value

    def per_op_route(self, prompt, n_new: int) -> dict:
        """The DROP-IN route on this model's weights (csrc/per_op_route.hip): qwen3-mlx's Model::forward + Generate::next replayed call for
        call through the mlx-c handle ABI, as an unmodified crate would drive it -- greedy tokens (the prompt's, then n_new), host
        wall-clock per decoded token, mlx_* calls per token.  Independent of the engine's own KV cache and step graph."""
        ids = np.ascontiguousarray(np.asarray(prompt, dtype=np.uint32).ravel())
        toks = np.zeros(n_new + 1, np.uint32)
        pre, per, calls = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(lib.omx_bench_qwen3_per_op(self._h, ctypes.byref(self.cfg), ids.ctypes.data_as(ctypes.POINTER(c_uint32)), ids.size, n_new,
                                         toks.ctypes.data_as(ctypes.POINTER(c_uint32)), ctypes.byref(pre), ctypes.byref(per), ctypes.byref(calls)))
        return {"tokens": toks, "prefill_ms": pre.value, "ms_per_token": per.value, "calls_per_token": calls.value}

    def per_op_route_forced(self, prompt, forced, logit_steps) -> dict:
        """The same route TEACHER-FORCED (the oracle pins): after the prompt, position i is fed forced[i]; returns the route's own greedy
        token at every step and the float32-widened bf16 logits rows of `logit_steps` (0 = the prompt's last position)."""
        ids = np.ascontiguousarray(np.asarray(prompt, dtype=np.uint32).ravel())
        forced = np.ascontiguousarray(np.asarray(forced, dtype=np.uint32).ravel())
        steps = np.ascontiguousarray(np.asarray(logit_steps, dtype=np.int32).ravel())
        toks = np.zeros(forced.size + 1, np.uint32)
        raw = np.zeros((steps.size, self.cfg.vocab_size), np.uint16)
        fn = lib.omx_bench_qwen3_per_op_ex
        fn.restype = ctypes.c_int
        fn.argtypes = [c_void_p, c_void_p, ctypes.POINTER(c_uint32), c_int, c_int, ctypes.POINTER(c_uint32), c_void_p, c_void_p, c_void_p,
                       ctypes.POINTER(c_uint32), ctypes.POINTER(ctypes.c_int32), c_int, c_void_p]
        pre, per, calls = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(fn(self._h, ctypes.addressof(self.cfg), ids.ctypes.data_as(ctypes.POINTER(c_uint32)), ids.size, forced.size,
                 toks.ctypes.data_as(ctypes.POINTER(c_uint32)), ctypes.addressof(pre), ctypes.addressof(per), ctypes.addressof(calls),
                 forced.ctypes.data_as(ctypes.POINTER(c_uint32)), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), steps.size, raw.ctypes.data))
        return {"tokens": toks, "logits": (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)}

    def last_logits(self) -> np.ndarray:
        raw = np.empty(self.vocab_local, dtype=np.uint16)
        check(lib.omx_qwen3_last_logits(self._h, raw.ctypes.data, raw.size))
        if self.f16:      # a float16 model's logits are float16
            return raw.view(np.float16).astype(np.float32)
        return (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)

    def stream(self) -> int:
        s = c_void_p()
        check(lib.omx_qwen3_stream(self._h, ctypes.byref(s)))
        return s.value or 0

    def decode_path(self) -> str:
        """'graph' | 'eager' | 'aql' (packets on the engine's own HSA queue, OMX_STEP_AQL) once the first step ran ('unbuilt' before);
        followed by the rungs of the fallback ladder a give-up has taken on this engine, e.g. 'graph gateup_disabled'."""
        v = c_int()
        check(lib.omx_qwen3_decode_path(self._h, ctypes.byref(v)))
        path = ("unbuilt", "graph", "eager", "aql")[v.value & 0xFF]
        return path + "".join(" " + name for bit, name in enumerate(("gateup_disabled", "chain_disabled", "engine_disabled", "oproj_disabled"))
                              if v.value >> (8 + bit) & 1)

    KERNEL_CLASSES = ("qkv", "attention", "o", "gate_up", "down", "lm_head", "step_engine")

    def time_step_kernels(self, steps: int = 4) -> dict:
        """Average in-step duration (microseconds) of each per-layer kernel, HIP events on the step's stream around every launch of
        `steps` real (eager) decode steps: each launch's own HIP start / stop events -- omx_qwen3_time_step_kernels."""
        us = (ctypes.c_float * 7)()
        check(lib.omx_qwen3_time_step_kernels(self._h, steps, us))
        return dict(zip(self.KERNEL_CLASSES, (float(v) for v in us)))

    def step_forms(self) -> dict:
        """Which in-launch folds the next decode step would take (test hook, omx_qwen3_debug_step_forms)."""
        f = (c_int * 7)()
        check(lib.omx_qwen3_debug_step_forms(self._h, f))
        return {"down_qkv": bool(f[0]), "attn_oproj": bool(f[1]), "step_engine": int(f[2]), "down_qkv_gave_up": bool(f[3]),
                "attn_gateup": bool(f[4]), "attn_gateup_gave_up": bool(f[5]), "attn_down": bool(f[6])}

    def raise_give_up(self) -> None:
        """Set, from the host, the word a wait inside a launch raises when it gives up (test hook of the fallback ladder)."""
        check(lib.omx_qwen3_debug_raise_give_up(self._h))

    def step_bytes(self, ctx: int) -> float:
        v = ctypes.c_double()
        check(lib.omx_qwen3_step_bytes(self._h, ctx, ctypes.byref(v)))
        return v.value

    def batch(self, n_slots: int, max_context: int = 0, kv_bits: int = 0) -> "Batch":
        """Up to 8 independent sequences decoded together on this model's weights (omx_qwen3_batch_*).  kv_bits = 8: the K/V rows kept
        as 8-bit MLX affine codes (group 64), quantised as they are appended and read packed by the decode attention; 0: bf16 slabs."""
        return Batch(self, n_slots, max_context, kv_bits)


class Batch:
    """n_slots independent sequences on one loaded Model, each with its own KV slabs, position, pending token and sampler; `decode`
    advances any subset of them with one weight stream per Linear.  The model's own prefill / decode / verify keep working beside it;
    calls on a model and its batches must not overlap (they share the model's stream and prompt scratch)."""

    logprobs_top = None   # set_logprobs: alternatives reported per generated token (None = off)

    def __init__(self, model: Model, n_slots: int, max_context: int = 0, kv_bits: int = 0):
        self.model, self.n_slots, self.kv_bits = model, int(n_slots), int(kv_bits)
        self._h = c_void_p()
        if self.kv_bits == 0:
            check(lib.omx_qwen3_batch_create(ctypes.byref(self._h), model._h, int(n_slots), int(max_context)))
        else:
            check(lib.omx_qwen3_batch_create_kv(ctypes.byref(self._h), model._h, int(n_slots), int(max_context), self.kv_bits))

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            m = getattr(self.model, "_h", None)
            if m is not None and m.value:     # (a closed model has freed the stream the batch would wait on)
                lib.omx_qwen3_batch_destroy(h)
            self._h = c_void_p()

    def __del__(self):
        if sys is not None and not sys.is_finalizing():
            self.close()

    def set_sampler(self, slot: int, temperature: float, seed: int = 0, *, top_k: int = 0, top_p: float = 1.0,
                    repetition_penalty: float = 1.0, presence_penalty: float = 0.0) -> None:
        """Model.set_sampler for one slot: 0 = greedy, else categorical(logits / temperature) from the slot's own key sequence.  The
        keywords are Model.set_sampler's filters (omx_sample_filtered's rule) inside the batched step, per slot: the penalties act on
        the tokens THIS slot sampled since its last prefill, top_k keeps ties, top_p acts on the survivors.  Their defaults are off:
        the call is then the plain sampler, bit for bit.  Either form restarts the slot's key sequence and clears its history."""
        if top_k == 0 and top_p == 1.0 and repetition_penalty == 1.0 and presence_penalty == 0.0:
            check(lib.omx_qwen3_batch_set_sampler(self._h, int(slot), float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF))
            return
        p = Sampling(temperature, top_k, top_p, repetition_penalty, presence_penalty)
        check(lib.omx_qwen3_batch_set_sampling(self._h, int(slot), ctypes.byref(p), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def prefill(self, slot: int, prompt, embeds=None, embeds_at: int = 0) -> int:
        """The prompt onto the slot's cache (appended to what the slot holds); returns the slot's first sampled token.  embeds / embeds_at:
        Model.prefill's -- rows [n_rows, hidden] (a device Tensor, f32 / bf16 / f16, or a float32 / float16 numpy array) that replace the
        embedding rows of positions [embeds_at, embeds_at + n_rows) (omx_qwen3_batch_prefill_embeds), with Model.prefill's refusals."""
        p = np.ascontiguousarray(prompt, dtype=np.uint32)
        first = c_uint32()
        if embeds is None:
            check(lib.omx_qwen3_batch_prefill(self._h, int(slot), p.ctypes.data_as(ctypes.POINTER(c_uint32)), p.size, ctypes.byref(first)))
            return first.value
        from .ops import Tensor
        if not isinstance(embeds, Tensor):
            a = np.asarray(embeds)
            embeds = Tensor.from_numpy(a, "f16" if a.dtype == np.float16 else "f32")
        hidden = self.model.cfg.hidden_size
        if len(embeds.shape) != 2 or embeds.shape[1] != hidden:
            raise OmxError(f"ShapeMismatch: embeds has shape {embeds.shape}, the model expects [n_rows, {hidden}]")
        check(lib.omx_synchronize(None))   # the rows may come from ops on the null stream; the pass runs on the model's own
        check(lib.omx_qwen3_batch_prefill_embeds(self._h, int(slot), p.ctypes.data_as(ctypes.POINTER(c_uint32)), p.size,
                                                 embeds.ptr if embeds.shape[0] else None, embeds.dtype, int(embeds_at), embeds.shape[0],
                                                 ctypes.byref(first)))
        return first.value

    def fork(self, src: int, dst: int, resample: bool = True) -> int:
        """The empty slot `dst` becomes what it would be had it been fed `src`'s tokens itself: src's position, kept logits and a copy
        of its K/V rows.  Its pending token is drawn from those logits with dst's own sampler (resample), or is src's.  Returns it.
        With a penalty on, a resampled sibling starts an empty history (fork right after the prefill); resample=False copies src's.
        The slot table records the whole 256-token chunks siblings have in common (`shared`); OMX_BATCH_SHARE_MIN=2..8 makes the decode
        attention read them once per group (bit-identical; slower than the default at every size measured)."""
        first = c_uint32()
        check(lib.omx_qwen3_batch_fork(self._h, int(src), int(dst), int(bool(resample)), ctypes.byref(first)))
        return first.value

    def shared(self, slot: int):
        """(owner, shared_len) of the device's slot table: the decode attention may read tokens [0, shared_len) of `slot` from
        slot `owner`'s slabs, which hold the same bits there."""
        owner, n = c_int(), c_int()
        check(lib.omx_qwen3_batch_shared(self._h, int(slot), ctypes.byref(owner), ctypes.byref(n)))
        return owner.value, n.value

    def set_logprobs(self, top_n=None) -> None:
        """Model.set_logprobs for the batch, one setting for all slots (omx_qwen3_batch_set_logprobs)."""
        check(lib.omx_qwen3_batch_set_logprobs(self._h, -1 if top_n is None else int(top_n)))
        self.logprobs_top = None if top_n is None or int(top_n) < 0 else int(top_n)

    def decode(self, n: int, slots=None, return_logprobs: bool = False):
        """n tokens for each of `slots` (default: all; distinct, prefilled) -> [n, len(slots)], columns in the listed order.
        return_logprobs (after set_logprobs): (tokens, logprobs [n, len(slots)]) and, with alternatives on, (tokens, logprobs,
        top_ids [n, len(slots), top_n], top_logprobs [n, len(slots), top_n])."""
        ids = np.ascontiguousarray(list(range(self.n_slots)) if slots is None else slots, dtype=np.int32).ravel()
        out = np.empty((int(n), ids.size), dtype=np.uint32)
        if not return_logprobs:
            check(lib.omx_qwen3_batch_decode(self._h, ids.ctypes.data_as(ctypes.POINTER(c_int)), ids.size, int(n),
                                             out.ctypes.data_as(ctypes.POINTER(c_uint32))))
            return out
        top = self.logprobs_top or 0
        lp = np.zeros((int(n), ids.size), np.float32)
        tid, tlp = np.zeros((int(n), ids.size, top), np.uint32), np.zeros((int(n), ids.size, top), np.float32)
        check(lib.omx_qwen3_batch_decode_logprobs(self._h, ids.ctypes.data_as(ctypes.POINTER(c_int)), ids.size, int(n),
                                                  out.ctypes.data_as(ctypes.POINTER(c_uint32)), lp.ctypes.data_as(ctypes.POINTER(c_float)),
                                                  tid.ctypes.data if top else None, tlp.ctypes.data if top else None))
        return (out, lp, tid, tlp) if top else (out, lp)

    def last_logprobs(self, slot: int):
        """Of the slot's most recently sampled token (a prefill's or fork's first token, or its last step's): logprob, or
        (logprob, top_ids, top_logprobs)."""
        top = self.logprobs_top or 0
        lp, ids, tlp = c_float(), np.zeros(top, np.uint32), np.zeros(top, np.float32)
        check(lib.omx_qwen3_batch_last_logprobs(self._h, int(slot), ctypes.byref(lp), ids.ctypes.data if top else None,
                                                tlp.ctypes.data if top else None))
        return (np.float32(lp.value), ids, tlp) if top else np.float32(lp.value)

    def logits(self, slot: int) -> np.ndarray:
        """float32-widened bf16 logits of the last prefill or step the slot took part in."""
        raw = np.empty(self.model.vocab_local, dtype=np.uint16)
        check(lib.omx_qwen3_batch_logits(self._h, int(slot), raw.ctypes.data, raw.size))
        return (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)

    def offset(self, slot: int) -> int:
        v = c_int()
        check(lib.omx_qwen3_batch_offset(self._h, int(slot), ctypes.byref(v)))
        return v.value

    def trim(self, slot: int, n: int, next_token: int) -> None:
        """Model.trim for one slot: forget the last n cached tokens; next_token becomes the pending token (n = 0: only that)."""
        check(lib.omx_qwen3_batch_trim(self._h, int(slot), int(n), int(next_token)))

    def reset(self, slot: int) -> None:
        check(lib.omx_qwen3_batch_reset(self._h, int(slot)))

    def kv_bytes(self) -> int:
        """Bytes of K/V storage the batch allocated (the slabs only)."""
        v = ctypes.c_size_t()
        check(lib.omx_qwen3_batch_kv_bytes(self._h, ctypes.byref(v)))
        return v.value

    def kv_rows(self, slot: int, layer: int, first: int = 0, n=None):
        """Cached rows [first, first + n) (default: to the slot's offset) of one layer.  A bf16 batch: (k, v), each float32-widened
        [Hkv, n, D].  A kv_bits = 8 batch: (k, v), each the MLX triplet (codes uint32 [Hkv, n, D / 4], scales, biases float32-widened
        bf16 [Hkv, n, D / 64]) -- what ops.dequantize(..., 64, 8) takes."""
        cfg = self.model.cfg
        Hkv, D = int(cfg.num_key_value_heads), int(cfg.head_dim)
        n = self.offset(slot) - int(first) if n is None else int(n)
        widen = lambda raw: (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)
        if self.kv_bits == 0:
            k, v = (np.empty((Hkv, max(n, 0), D), dtype=np.uint16) for _ in range(2))
            check(lib.omx_qwen3_batch_kv_read(self._h, int(slot), int(layer), int(first), n, k.ctypes.data, v.ctypes.data, None, None, None, None))
            return widen(k), widen(v)
        k, v = (np.empty((Hkv, max(n, 0), D // 4), dtype=np.uint32) for _ in range(2))
        ks, kb, vs, vb = (np.empty((Hkv, max(n, 0), D // 64), dtype=np.uint16) for _ in range(4))
        check(lib.omx_qwen3_batch_kv_read(self._h, int(slot), int(layer), int(first), n, k.ctypes.data, v.ctypes.data, ks.ctypes.data,
                                          kb.ctypes.data, vs.ctypes.data, vb.ctypes.data))
        return (k, widen(ks), widen(kb)), (v, widen(vs), widen(vb))

    def debug_attention(self, layer: int, slots, q) -> np.ndarray:
        """Test hook: the decode attention launch alone.  q [n, H, D] (rounded to bf16) against ALL cached rows of slots[r] at `layer`
        -> float32-widened bf16 [n, H * D].  Touches no slot state."""
        ids = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        qf = np.ascontiguousarray(q, dtype=np.float32)
        H, D = int(self.model.cfg.num_attention_heads), int(self.model.cfg.head_dim)
        if qf.shape != (ids.size, H, D):
            raise ValueError(f"debug_attention: q must be [{ids.size}, {H}, {D}], got {qf.shape}")
        u = qf.view(np.uint32)
        raw = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)   # RNE to bf16
        out = np.empty((ids.size, H * D), dtype=np.uint16)
        check(lib.omx_qwen3_batch_debug_attention(self._h, int(layer), ids.ctypes.data_as(ctypes.POINTER(c_int)), ids.size,
                                                  raw.ctypes.data, out.ctypes.data))
        return (out.astype(np.uint32) << np.uint32(16)).view(np.float32)

    def last_decode_ms(self) -> float:
        """Device time of the steps of the last decode call (HIP events on the model's stream)."""
        v = c_float()
        check(lib.omx_qwen3_batch_last_decode_ms(self._h, ctypes.byref(v)))
        return v.value


class Generate:
    """qwen3_mlx::Generate (model.rs:743-844): iterator yielding sampled tokens; the first `next`
    prefills the prompt.  temp == 0 is the greedy path of sample() (model.rs:733-735); temp != 0 draws
    categorical(logits / temp) (model.rs:736-739) from the key sequence seeded with `seed`.
    logprobs = k (0..20): the same tokens, and `.logprobs` (a float per token yielded so far) / `.top_logprobs` (per token, its k
    alternatives as (id, logprob) pairs, best first) of the model's raw logits (Model.set_logprobs); None leaves the model's setting off."""

    def __init__(self, model: Model, temp: float, prompt_token, chunk: int = 16, seed: int = 0, *, top_k: int = 0, top_p: float = 1.0,
                 repetition_penalty: float = 1.0, presence_penalty: float = 0.0, logprobs=None):
        model.set_sampler(temp, seed, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty, presence_penalty=presence_penalty)
        if logprobs is not None or model.logprobs_top is not None:
            model.set_logprobs(logprobs)
        self.model, self.prompt, self.chunk = model, np.asarray(prompt_token, dtype=np.uint32).ravel(), chunk
        self._prefilled = False
        self._buf = []
        self._with_logprobs = logprobs is not None
        self.logprobs, self.top_logprobs = [], []

    def __iter__(self) -> Iterator[int]:
        return self

    def _record(self, lp, ids=(), tlp=()) -> None:
        self.logprobs.append(float(lp))
        self.top_logprobs.append([(int(i), float(v)) for i, v in zip(ids, tlp)])

    def __next__(self) -> int:
        if not self._prefilled:
            self._prefilled = True
            first = self.model.prefill(self.prompt)
            if self._with_logprobs:
                last = self.model.last_logprobs()
                self._record(*(last if isinstance(last, tuple) else (last,)))
            return first
        if not self._buf:
            if self._with_logprobs:
                toks, lp, *top = self.model.decode(self.chunk, return_logprobs=True)
                ids, tlp = top if top else ([()] * len(toks), [()] * len(toks))
                self._buf = list(zip(toks, lp, ids, tlp))
            else:
                self._buf = [(t,) for t in self.model.decode(self.chunk)]
        tok, *rest = self._buf.pop(0)
        if rest:
            self._record(*rest)
        return int(tok)
