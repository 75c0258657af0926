"""Host rule the DeepSeek-V2 family MoE tests hold the device to, written from the arithmetic and rounding points of
deepseek-ocr2-mlx/src/lib.rs: MLP::forward (:148-159), MoEGate::route (:178-200) and MoE::forward (:224-298).

`rnd=None` is the rule in float64 with no rounding at all.  `rnd=bf16` rounds where the reference's bf16 arrays round: every Linear's
output, fused_swiglu's output, the weighted sum's `as_dtype`, the add of the shared experts.  The router never rounds to bf16: its logits
are a float32 matmul of the widened operands, and softmax, the division by (sum + 1e-20) and the scale stay float32."""
import numpy as np

from oracle import ref_core as rc


def bf16(a):
    return rc.bf16_round(np.asarray(a, np.float32)).astype(np.float64)


def _id(a):
    return np.asarray(a, np.float64)


def silu(g):
    return g / (1.0 + np.exp(-g))


def mlp(x, w_gate, w_up, w_down, rnd=None):
    """down(fused_swiglu(up(x), gate(x))): the activation is computed from the rounded projections and rounded once"""
    r = rnd or _id
    g, u = r(_id(x) @ _id(w_gate).T), r(_id(x) @ _id(w_up).T)
    return r(r(silu(g) * u) @ _id(w_down).T)


def route(x, gate_w, k, norm_topk_prob, scale, f32=False):
    """-> inds [n, k] (descending score, ties to the lower index), weights [n, k].  f32: the reference's own float32 pipeline."""
    dt = np.float32 if f32 else np.float64
    logits = np.asarray(x, dt) @ np.asarray(gate_w, dt).T
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    scores = e / e.sum(axis=-1, keepdims=True)
    inds = np.argsort(-scores, axis=-1, kind="stable")[:, :k]
    sel = np.take_along_axis(scores, inds, -1)
    if norm_topk_prob and k > 1:
        sel = sel / (sel.sum(axis=-1, keepdims=True) + dt(1e-20))
    return inds.astype(np.uint32), (sel * dt(scale)).astype(np.float64)


def topk_gap(x, gate_w, k):
    """relative gap between the k-th and (k+1)-th softmax score of every row (inf where k == E)"""
    logits = _id(x) @ _id(gate_w).T
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    s = -np.sort(-(e / e.sum(axis=-1, keepdims=True)), axis=-1)
    if k >= s.shape[1]:
        return np.full(s.shape[0], np.inf)
    return (s[:, k - 1] - s[:, k]) / s[:, k - 1]


def block(x, gate_w, w_gate, w_up, w_down, k, shared=None, norm_topk_prob=False, scale=1.0, rnd=None):
    """MoE::forward on rows x [n, hidden]: w_gate / w_up [E, I, hidden], w_down [E, hidden, I]; shared = (gate, up, down) of the shared MLP
    or None.  -> (out [n, hidden], inds, weights)"""
    r = rnd or _id
    inds, weights = route(x, gate_w, k, norm_topk_prob, scale)
    n = len(x)
    moe = np.zeros((n, w_down.shape[1]))
    for t in range(n):
        for j in range(k):
            e = int(inds[t, j])
            moe[t] += mlp(x[t:t + 1], w_gate[e], w_up[e], w_down[e], rnd)[0] * weights[t, j]
    out = r(moe)
    if shared is not None:
        out = r(out + mlp(x, *shared, rnd))
    return out, inds, weights


def block_literal(x, gate_w, w_gate, w_up, w_down, k, shared=None, norm_topk_prob=False, scale=1.0):
    """The same block the reference's literal way (lib.rs:238-295), float64: the slots sorted by expert, each expert's MLP over its run of
    rows, the outputs concatenated and un-sorted through the inverse permutation, then weighted and summed over k."""
    inds, weights = route(x, gate_w, k, norm_topk_prob, scale)
    n, flat = len(x), inds.reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind="stable")
    sorted_idx, tokens = flat[order], _id(x)[order // k]
    outs, start = [], 0
    while start < len(sorted_idx):
        end = start + 1
        while end < len(sorted_idx) and sorted_idx[end] == sorted_idx[start]:
            end += 1
        e = int(sorted_idx[start])
        outs.append(mlp(tokens[start:end], w_gate[e], w_up[e], w_down[e]))
        start = end
    unsorted = np.concatenate(outs, 0)[np.argsort(order, kind="stable")]
    y = (unsorted.reshape(n, k, -1) * weights[:, :, None]).sum(axis=1)
    return y + mlp(x, *shared) if shared is not None else y


def route_mode1(x, gate_w, k, norm_topk_prob):
    """modes 0 / 1's arithmetic on the same router (the mistake a mode-2 model must not make): bf16 logits, bf16 scores"""
    logits = bf16(_id(x) @ _id(gate_w).T)
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    scores = bf16(e / e.sum(axis=-1, keepdims=True))
    inds = np.argsort(-scores, axis=-1, kind="stable")[:, :k]
    sel = np.take_along_axis(scores, inds, -1)
    if norm_topk_prob and k > 1:
        sel = bf16(sel / bf16(sel.sum(axis=-1, keepdims=True)))
    return inds.astype(np.uint32), sel


def weights_for(E, hidden, inter, n_shared, seed):
    """bf16-valued test weights: router, expert stacks, shared MLP (or None)"""
    g = np.random.default_rng(seed)
    u = lambda *s: g.uniform(-1.0, 1.0, s)
    gate_w = bf16(u(E, hidden) * 0.5)
    w_gate, w_up, w_down = bf16(u(E, inter, hidden) * 0.08), bf16(u(E, inter, hidden) * 0.08), bf16(u(E, hidden, inter) * 0.08)
    shared = None
    if n_shared:
        W = n_shared * inter
        shared = (bf16(u(W, hidden) * 0.08), bf16(u(W, hidden) * 0.08), bf16(u(hidden, W) * 0.08))
    return gate_w, w_gate, w_up, w_down, shared


def rows_for(n, hidden, seed):
    return bf16(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, hidden)))


def exact_router_inputs(n, E, hidden, seed):
    """Rows and a router whose float32 dot products are EXACT in any order: multiples of 2^-3 in [-1, 1] times multiples of 2^-5 in
    [-0.25, 0.25] -- every partial sum is a multiple of 2^-8 below 2^6, 14 bits.  The device's logits then equal the rule's, and what is
    left between them is the softmax, the division and the scale: the float32 operations the router's tolerance counts."""
    g = np.random.default_rng(seed)
    x = g.integers(-8, 9, (n, hidden)).astype(np.float64) / 8.0
    gw = g.integers(-8, 9, (E, hidden)).astype(np.float64) / 32.0
    return x, gw


# ---- the cases the device tests run (tests/test_gpu_deepseek_moe.py); tests/test_deepseek_moe_rule.py checks on the CPU that every one of
#      them has a selection no float32 logit error can flip ----
ROUTER_CASES = [(64, 6), (8, 8), (256, 1), (16, 6)]            # (experts, top_k); hidden 192; rows 1 and 5
ROUTER_HIDDEN = 192
BLOCK_E, BLOCK_K, BLOCK_HIDDEN = 16, 6, 192
BLOCK_WIDTHS, BLOCK_SHARED, BLOCK_ROWS = (64, 192), (0, 1, 2), (1, 4, 5, 70)
# a float32 dot product over 192 terms of magnitude <= 0.5 carries an error below 192 * 2^-24 * (sum of |terms|) < 1e-4: a relative gap
# of 1e-3 between the k-th and the (k + 1)-th score is out of its reach
MIN_GAP = 1e-3


def router_seed(E, k, rows):
    return 1000 + E * 10 + k + rows


def block_seed(width, n_shared, rows):
    return 2000 + width * 7 + n_shared * 131 + rows


def block_inputs(width, n_shared, rows):
    seed = block_seed(width, n_shared, rows)
    return rows_for(rows, BLOCK_HIDDEN, seed + 1), weights_for(BLOCK_E, BLOCK_HIDDEN, width, n_shared, seed)


# ---- modes 0 / 1 on the block inputs: what tests/golden/deepseek_moe_modes01.npz records from the commit before mode 2 existed ----
MODES01 = [(mode, rows) for mode in ("mixtral", "qwen3_moe") for rows in (1, 5, 70)]     # GEMV route (6 and 30 slots), grouped route


def bf16_bits(a):
    """float32 array holding bf16 values -> the 16-bit patterns"""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def run_modes01(omx):
    """{name: bits} of omx_moe_forward's output, selection and scores for every MODES01 case"""
    from ominix_mlx_amd import moe
    T = omx.ops.Tensor
    got = {}
    for mode, rows in MODES01:
        x, (gw, wg, wu, wd, _) = block_inputs(BLOCK_WIDTHS[0], 0, rows)
        blk = moe.SparseMoeBlock(T.from_numpy(gw), T.from_numpy(wg), T.from_numpy(wu), T.from_numpy(wd), BLOCK_K, mode, True)
        out, inds, scores = blk.forward(T.from_numpy(x), return_routing=True)
        got[f"{mode}_{rows}_out"], got[f"{mode}_{rows}_inds"] = bf16_bits(out.numpy()), inds.numpy().astype(np.uint32)
        got[f"{mode}_{rows}_scores"] = bf16_bits(scores.numpy())
    return got


# ---- the decoder: Qwen3Oracle's attention / norms / head (no q/k norm, non-traditional RoPE) with the DeepSeek layer plan ----
def tiny_decoder_config(norm_topk_prob=True):
    """the model of tests/test_gpu_deepseek_engine.py: 3 layers, hidden 256, 2 / 2 heads of 128, dense width 448 (an odd multiple of 64,
    like 6848), 16 experts of 192, top-6, vocabulary 1024"""
    from oracle import ref_qwen3 as rq
    return rq.Qwen3Config(256, 3, 448, 2, 2, 128, 1024, 1e-6, 10000.0, False, None, 8192, 16, 6, 192, "qwen3_moe", norm_topk_prob, False)


def decoder_weight_shapes(cfg, first_k_dense_replace, n_shared):
    from oracle import ref_qwen3 as rq
    import dataclasses
    s = rq.weight_shapes(dataclasses.replace(cfg, num_experts=0))
    h, Im, E = cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_experts
    for i in range(first_k_dense_replace, cfg.num_hidden_layers):
        p = f"model.layers.{i}.mlp."
        for n in ("gate_proj", "up_proj", "down_proj"):
            del s[p + n + ".weight"]
        s[p + "gate.weight"] = (E, h)
        s[p + "switch_mlp.gate_proj.weight"], s[p + "switch_mlp.up_proj.weight"] = (E, Im, h), (E, Im, h)
        s[p + "switch_mlp.down_proj.weight"] = (E, h, Im)
        if n_shared:
            s[p + "shared_experts.gate_proj.weight"], s[p + "shared_experts.up_proj.weight"] = (n_shared * Im, h), (n_shared * Im, h)
            s[p + "shared_experts.down_proj.weight"] = (h, n_shared * Im)
    return s


def decoder_weights(cfg, first_k_dense_replace, n_shared, base_seed):
    """the tensors omx_qwen3_synth_weights(base_seed) makes on the device (oracle/synth.py is its twin)"""
    from oracle import ref_qwen3 as rq, synth
    return {name: synth.tensor(name, shape, *rq.weight_spec(name), "bf16", base_seed)
            for name, shape in decoder_weight_shapes(cfg, first_k_dense_replace, n_shared).items()}


def make_oracle(cfg, weights, first_k_dense_replace, n_shared, scale, dt="bf16"):
    from oracle import ref_qwen3 as rq

    class DeepseekOracle(rq.Qwen3Oracle):
        """dt "bf16": the reference's rounding points; "f32": no 16-bit rounding anywhere (the float64 rule of the feed-forward)"""
        selected = None

        def mlp(self, i, x):
            B, L, h = x.shape
            x2, p, rnd = np.asarray(x, np.float64).reshape(B * L, h), f"model.layers.{i}.mlp.", (bf16 if self.dt == "bf16" else None)
            w = lambda n: self.w[p + n + ".weight"]
            if i < first_k_dense_replace:
                y = mlp(x2, w("gate_proj"), w("up_proj"), w("down_proj"), rnd)
            else:
                sh = tuple(w("shared_experts." + n) for n in ("gate_proj", "up_proj", "down_proj")) if n_shared else None
                y, inds, _ = block(x2, w("gate"), w("switch_mlp.gate_proj"), w("switch_mlp.up_proj"), w("switch_mlp.down_proj"),
                                   self.cfg.num_experts_per_tok, sh, self.cfg.norm_topk_prob, scale, rnd)
                if self.selected is not None:
                    self.selected.append((i, inds, topk_gap(x2, w("gate"), self.cfg.num_experts_per_tok)))
            return y.astype(np.float32).reshape(B, L, h)

    import dataclasses
    return DeepseekOracle(dataclasses.replace(cfg, num_experts=0), weights, dt)


# the engine test's runs: (routed_scaling_factor, base seed of the synthetic weights); 40 prompt tokens + 8 decoded.  The seeds were searched
# on the CPU (tests/test_deepseek_moe_rule.py re-checks them): at every row and layer the float32-everywhere rule and the rule at the bf16
# rounding points choose the same experts
ENGINE_RUNS = [(1.0, 0x0C0FFEE5), (2.5, 0x0C0FFEE7)]
ENGINE_PROMPT, ENGINE_NEW = 40, 8


def engine_selections(scale, base_seed, dt, n_shared=2, first_k=1):
    from oracle import synth
    cfg = tiny_decoder_config()
    o = make_oracle(cfg, decoder_weights(cfg, first_k, n_shared, base_seed), first_k, n_shared, scale, dt)
    o.selected = []
    tokens, logits = o.generate(synth.prompt_ids(ENGINE_PROMPT, cfg.vocab_size), ENGINE_NEW, return_logits=True)
    return o.selected, tokens, logits
