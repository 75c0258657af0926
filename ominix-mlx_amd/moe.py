"""Host mirror of the sparse-MoE block (mixtral-mlx/src/model.rs:280-313 `MixtralSparseMoeBlock`,
qwen3-mlx/src/qwen3_moe.rs:440-508 `MoeBlock`) over omx_moe_forward."""
from __future__ import annotations

import ctypes

import numpy as np

from . import UINT32, check, lib
from .ops import Tensor

c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
MOE_SIGNATURES = {
    "omx_moe_block_partials": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "omx_moe_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_size_t)]),
    "omx_moe_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "omx_moe_block_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "omx_moe_block_forward_q": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p] + [c_void_p] * 12 + [c_int] * 9 + [c_void_p]),
    # the batched expert-parallel block up to the expert outputs (out: struct of four pointers) -> comm.omx_peer_moe_combine
    "omx_moe_block_slots_ep": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_void_p]),
    "omx_moe_block_partial_ep": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "omx_moe_forward_q": (c_int, [c_void_p] * 12 + [c_int] * 9 + [c_void_p, c_void_p, c_void_p]),
    "omx_moe_block_forward_q_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p] + [c_void_p] * 12 + [c_int] * 10 + [c_void_p]),
    # expert tensor parallel (tp_size > 1 on a sparse-MoE engine): this rank's columns of every expert, f32 slot partials, combine
    "omx_moe_block_partial_tp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "omx_moe_combine_slots": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    # the two sharded forms on MLX-packed expert stacks (round 5): partial, x, norm_w, eps, xn, 12 triplet pointers, shapes, shard, format
    "omx_moe_block_partial_ep_q": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p] + [c_void_p] * 12 + [c_int] * 12 + [c_void_p]),
    "omx_moe_block_partial_tp_q": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float] + [c_void_p] * 12 + [c_int] * 10 + [c_void_p]),
    "omx_moe_combine_slots_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    # DeepSeek-V2 family block: float32 router (mode 2), routed + shared experts
    "omx_moe_deepseek_form": (c_int, [c_int] * 7),
    "omx_moe_deepseek_workspace_bytes": (c_int, [c_int] * 6 + [ctypes.POINTER(c_size_t)]),
    "omx_moe_deepseek_forward": (c_int, [c_void_p] * 6 + [c_int] + [c_void_p] * 3 + [c_int] * 7 + [ctypes.c_float, c_void_p, c_void_p, c_void_p]),
    "omx_moe_deepseek_block_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p] + [c_void_p] * 4 + [c_int] +
                                       [c_void_p] * 3 + [c_int] * 7 + [ctypes.c_float, c_void_p]),
    "omx_moe_route_deepseek": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p] + [c_int] * 5 +
                               [ctypes.c_float, c_void_p]),
}
for _n, (_r, _a) in MOE_SIGNATURES.items():
    _f = getattr(lib, _n)
    _f.restype, _f.argtypes = _r, _a


class SparseMoeBlock:
    """gate: Linear [E, hidden]; switch_mlp.{gate,up,down}_proj stacked [E, ...] (model.rs:478-506)."""

    def __init__(self, gate_w: Tensor, w_gate: Tensor, w_up: Tensor, w_down: Tensor, num_experts_per_tok: int,
                 mode: str = "mixtral", norm_topk_prob: bool = True):
        self.gate_w, self.w_gate, self.w_up, self.w_down = gate_w, w_gate, w_up, w_down
        self.E, self.hidden = gate_w.shape
        self.inter = w_gate.shape[1]
        self.k = num_experts_per_tok
        self.mode = {"mixtral": 0, "qwen3_moe": 1}[mode]
        self.norm = int(norm_topk_prob)

    def forward(self, x: Tensor, return_routing: bool = False):
        n = x.size // self.hidden
        out = Tensor(x.shape, x.dtype)
        inds = Tensor((n, self.k), UINT32) if return_routing else None
        scores = Tensor((n, self.k), x.dtype) if return_routing else None
        check(lib.omx_moe_forward(out.ptr, x.ptr, self.gate_w.ptr, self.w_gate.ptr, self.w_up.ptr, self.w_down.ptr, n,
                                  self.hidden, self.inter, self.E, self.k, self.mode, self.norm,
                                  inds.ptr if inds else None, scores.ptr if scores else None, None))
        return (out, inds, scores) if return_routing else out


class QuantizedSparseMoeBlock:
    """MixtralSparseMoeBlock with `QuantizedSwitchLinear` experts (mixtral-mlx/src/model.rs:182-313): each of gate / up / down
    is a (packed u32 [E, out, in*bits/32], scales, biases) triplet of device Tensors; the router gate is bf16 [E, hidden]."""

    def __init__(self, gate_w: Tensor, q_gate, q_up, q_down, num_experts_per_tok: int, group_size: int = 64, bits: int = 4,
                 mode: str = "mixtral", norm_topk_prob: bool = True):
        self.gate_w, self.q_gate, self.q_up, self.q_down = gate_w, tuple(q_gate), tuple(q_up), tuple(q_down)
        self.E, self.hidden = gate_w.shape
        self.inter = self.q_gate[0].shape[1]
        self.k, self.group, self.bits = num_experts_per_tok, group_size, bits
        self.mode = {"mixtral": 0, "qwen3_moe": 1}[mode]
        self.norm = int(norm_topk_prob)

    def forward(self, x: Tensor, return_routing: bool = False):
        n = x.size // self.hidden
        out = Tensor(x.shape, x.dtype)
        inds = Tensor((n, self.k), UINT32) if return_routing else None
        scores = Tensor((n, self.k), x.dtype) if return_routing else None
        ptrs = [t.ptr for trip in (self.q_gate, self.q_up, self.q_down) for t in trip]
        check(lib.omx_moe_forward_q(out.ptr, x.ptr, self.gate_w.ptr, *ptrs, n, self.hidden, self.inter, self.E, self.k, self.mode,
                                    self.norm, self.group, self.bits, inds.ptr if inds else None, scores.ptr if scores else None, None))
        return (out, inds, scores) if return_routing else out


def split_shared_mlp(gate: np.ndarray, up: np.ndarray, down: np.ndarray, n_shared: int):
    """The shared MLP (gate / up [n_shared * I, hidden], down [hidden, n_shared * I]) as n_shared pseudo-experts of width I: row blocks of
    gate / up, the matching column blocks of down.  sum_i down_i(swiglu_i(x)) is down(swiglu(x)) with its contraction split into n_shared
    partial sums -- equal to round-off, which is why the shared width is n_shared * moe_intermediate_size."""
    W, hidden = gate.shape
    assert n_shared >= 1 and W % n_shared == 0 and up.shape == (W, hidden) and down.shape == (hidden, W)
    I = W // n_shared
    return (np.ascontiguousarray(gate.reshape(n_shared, I, hidden)), np.ascontiguousarray(up.reshape(n_shared, I, hidden)),
            np.ascontiguousarray(down.reshape(hidden, n_shared, I).transpose(1, 0, 2)))


class DeepseekMoeBlock:
    """deepseek-ocr2-mlx/src/lib.rs:162-299 `MoEGate` + `MoE`: gate [E, hidden]; experts stacked [E, I, hidden] / [E, hidden, I];
    shared = (gate, up, down) of the shared MLP at width n_shared * I, or None.  All host arrays (float32 holding bf16 values): the
    block appends the shared MLP's pseudo-experts to the stacks it uploads and keeps the whole shared MLP beside them."""

    def __init__(self, gate_w, w_gate, w_up, w_down, num_experts_per_tok: int, shared=None, n_shared_experts: int = 0,
                 norm_topk_prob: bool = False, routed_scaling_factor: float = 1.0):
        T = Tensor.from_numpy
        self.E, self.hidden = gate_w.shape
        self.inter = w_gate.shape[1]
        self.k, self.norm, self.scale = int(num_experts_per_tok), int(bool(norm_topk_prob)), float(routed_scaling_factor)
        self.n_shared = int(n_shared_experts) if shared is not None else 0
        if shared is not None and self.n_shared < 1:
            raise ValueError("DeepseekMoeBlock: shared experts given with n_shared_experts < 1")
        self.gate_w = T(gate_w)
        self.shared = None
        if self.n_shared:
            pg, pu, pd = split_shared_mlp(*shared, self.n_shared)
            if pg.shape[1] != self.inter:
                raise ValueError("DeepseekMoeBlock: the shared width must be n_shared_experts * moe_intermediate_size")
            w_gate, w_up, w_down = np.concatenate([w_gate, pg]), np.concatenate([w_up, pu]), np.concatenate([w_down, pd])
            self.shared = tuple(T(np.ascontiguousarray(a)) for a in shared)
        self.w_gate, self.w_up, self.w_down = T(w_gate), T(w_up), T(w_down)

    def form(self, n_tokens: int) -> int:
        """0: top_k + n_shared slots through the expert-selected GEMVs; 1: the shared MLP as launches of its own; 2: grouped GEMMs."""
        return lib.omx_moe_deepseek_form(n_tokens, self.hidden, self.inter, self.k, self.n_shared, self.n_shared, int(self.shared is not None))

    def route(self, x: Tensor):
        n = x.size // self.hidden
        inds, weights = Tensor((n, self.k), UINT32), Tensor((n, self.k), "f32")
        check(lib.omx_moe_route_deepseek(inds.ptr, weights.ptr, x.ptr, self.gate_w.ptr, None, 0.0, None, n, self.hidden, self.E, self.k,
                                         self.norm, self.scale, None))
        return inds, weights

    def forward(self, x: Tensor, return_routing: bool = False):
        n = x.size // self.hidden
        out = Tensor(x.shape, x.dtype)
        inds = Tensor((n, self.k), UINT32) if return_routing else None
        weights = Tensor((n, self.k), "f32") if return_routing else None
        sh = [t.ptr for t in self.shared] if self.shared else [None] * 3
        check(lib.omx_moe_deepseek_forward(out.ptr, x.ptr, self.gate_w.ptr, self.w_gate.ptr, self.w_up.ptr, self.w_down.ptr, self.n_shared,
                                           *sh, n, self.hidden, self.inter, self.E, self.k, self.n_shared, self.norm, self.scale,
                                           inds.ptr if inds else None, weights.ptr if weights else None, None))
        return (out, inds, weights) if return_routing else out

    def block_forward(self, resid: Tensor, x: Tensor, norm_w: Tensor, eps: float) -> Tensor:
        """resid + block(rmsnorm(x) * norm_w): the decoder layer's form (norm in the router launch, residual in the combine)."""
        n = x.size // self.hidden
        out, xn = Tensor(x.shape, x.dtype), Tensor(x.shape, x.dtype)
        sh = [t.ptr for t in self.shared] if self.shared else [None] * 3
        check(lib.omx_moe_deepseek_block_forward(out.ptr, resid.ptr, x.ptr, norm_w.ptr, eps, xn.ptr, self.gate_w.ptr, self.w_gate.ptr,
                                                 self.w_up.ptr, self.w_down.ptr, self.n_shared, *sh, n, self.hidden, self.inter, self.E,
                                                 self.k, self.n_shared, self.norm, self.scale, None))
        return out
