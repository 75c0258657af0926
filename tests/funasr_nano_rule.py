"""The Fun-ASR-Nano audio tower restated in numpy float64, written from funasr-nano-mlx/src/sensevoice_encoder.rs and adaptor.rs:
position add (:257-304), FSMN (:127-154), SAN-M attention (:205-244), encoder layer in both forms (:368-384), the tower over stacked
utterances (:453-478) and the adaptor with separate q, k, v (adaptor.rs:87-117, :176-187, :247-261).

An utterance in a joint pass is DEFINED as that utterance passed alone; `tower_segments` is the restatement of the device's pass (everything
over all rows, attention and FSMN cut at the boundaries) and tests/test_funasr_nano_rule.py holds the two equal."""
from __future__ import annotations

import numpy as np

ADAPTOR_HEADS, ADAPTOR_FFN = 8, 256          # adaptor.rs:226-227


def linear(x, w, b=None):
    """x w^T + b.  einsum's own loops, not BLAS: a row's result then does not depend on how many rows share the call (a BLAS product
    blocks by shape and moves the last bit), which is what lets the joint pass be compared with the utterances alone EXACTLY."""
    y = np.einsum("tk,nk->tn", np.ascontiguousarray(x), np.ascontiguousarray(w))
    return y if b is None else y + b


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def position_encoding(T: int, depth: int) -> np.ndarray:
    """SinusoidalPositionEncoder::encode (:257-284) for positions 1..T: [sin | cos] halves, timescale exp(-i ln(1e4) / (depth/2 - 1)).
    The angle is the reference's float32 product (positions and timescales are float32 arrays there); sin / cos of it in float64."""
    half = depth // 2
    inc = np.float32(np.log(np.float32(10000.0))) / (np.float32(half) - np.float32(1.0))
    inv = np.exp((np.arange(half, dtype=np.float32) * -inc).astype(np.float32)).astype(np.float32)
    st = (np.arange(1, T + 1, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32).astype(np.float64)
    return np.concatenate([np.sin(st), np.cos(st)], axis=1)


def position_add(x):
    """SinusoidalPositionEncoder::forward (:288-304): x + PE, NO scale."""
    x = np.asarray(x, np.float64)
    return x + position_encoding(*x.shape)


def segments(lengths):
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])
    return [(int(off[i]), int(off[i + 1])) for i in range(len(lengths))]


def fsmn(v, w, lengths=None):
    """FSMNBlock::forward (:127-154) without its residual: depthwise conv over time, taps w [C, k] (the checkpoint's [C, 1, k]), zero
    padding (k - 1) / 2 on both sides OF EACH UTTERANCE."""
    v = np.asarray(v, np.float64)
    w = np.asarray(w, np.float64).reshape(v.shape[1], -1)
    k = w.shape[1]
    left = (k - 1) // 2
    out = np.zeros_like(v)
    for lo, hi in segments([v.shape[0]] if lengths is None else lengths):
        T = hi - lo
        vp = np.pad(v[lo:hi], ((left, k - 1 - left), (0, 0)))
        for j in range(k):
            out[lo:hi] += vp[j:j + T] * w[:, j][None, :]
    return out


def attention(q, k, v, heads, lengths=None, mask=None):
    """softmax(q k^T / sqrt(D)) v per head and per utterance; mask: an additive [T, T] over ALL rows instead of the per-utterance loop."""
    T, dim = q.shape
    D = dim // heads
    out = np.zeros((T, dim))
    spans = [(0, T)] if mask is not None else segments([T] if lengths is None else lengths)
    for lo, hi in spans:
        qh, kh, vh = (t[lo:hi].reshape(-1, heads, D).transpose(1, 0, 2) for t in (q, k, v))
        s = qh @ kh.transpose(0, 2, 1) * (float(D) ** -0.5)
        if mask is not None:
            s = s + mask[None]
        s = s - s.max(-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(-1, keepdims=True)
        out[lo:hi] = (p @ vh).transpose(1, 0, 2).reshape(-1, dim)
    return out


def block_mask(lengths, value=-1e9):
    """0 inside an utterance, `value` across utterances"""
    T = int(np.sum(lengths))
    m = np.full((T, T), value)
    for lo, hi in segments(lengths):
        m[lo:hi, lo:hi] = 0.0
    return m


def sanm_attention(x, p, heads, lengths=None):
    """SANMAttention::forward (:205-244): linear_out(attention) + (conv(v) + v)"""
    qkv = linear(x, p["qkv_w"], p["qkv_b"])
    dim = qkv.shape[1] // 3
    q, k, v = qkv[:, :dim], qkv[:, dim:2 * dim], qkv[:, 2 * dim:]
    att = attention(q, k, v, heads, lengths)
    return linear(att, p["out_w"], p["out_b"]) + (fsmn(v, p["fsmn_w"], lengths) + v)


def encoder_layer(x, p, heads, lengths=None):
    """SenseVoiceEncoderLayer::forward (:368-384); the layer that changes the width (lfr_dim -> dim) has no attention residual"""
    x = np.asarray(x, np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    h = sanm_attention(layer_norm(x, p["norm1_w"], p["norm1_b"]), p, heads, lengths)
    if x.shape[1] == p["out_w"].shape[0]:
        h = x + h
    f = layer_norm(h, p["norm2_w"], p["norm2_b"])
    f = linear(np.maximum(linear(f, p["ffn_up_w"], p["ffn_up_b"]), 0.0), p["ffn_down_w"], p["ffn_down_b"])
    return h + f


_LAYER = {"norm1_w": "norm1.weight", "norm1_b": "norm1.bias", "qkv_w": "self_attn.linear_q_k_v.weight", "qkv_b": "self_attn.linear_q_k_v.bias",
          "out_w": "self_attn.linear_out.weight", "out_b": "self_attn.linear_out.bias", "fsmn_w": "self_attn.fsmn.weight",
          "norm2_w": "norm2.weight", "norm2_b": "norm2.bias", "ffn_up_w": "feed_forward.w_1.weight", "ffn_up_b": "feed_forward.w_1.bias",
          "ffn_down_w": "feed_forward.w_2.weight", "ffn_down_b": "feed_forward.w_2.bias"}


def layer_params(w, prefix):
    p = {k: np.asarray(w[f"{prefix}.{name}"], np.float64) for k, name in _LAYER.items()}
    p["fsmn_w"] = p["fsmn_w"].reshape(p["fsmn_w"].shape[0], -1)
    return p


def layer_prefixes(cfg):
    return (["encoder.encoders0.0"] + [f"encoder.encoders.{i}" for i in range(cfg["num_blocks"] - 1)],
            [f"encoder.tp_encoders.{i}" for i in range(cfg["tp_blocks"])])


def adaptor_block(x, w, p, lengths=None):
    """AdaptorBlock::forward (adaptor.rs:176-187) with AdaptorAttention's separate q, k, v (:87-117)"""
    g = lambda name: np.asarray(w[f"{p}.{name}"], np.float64)
    h = layer_norm(x, g("norm1.weight"), g("norm1.bias"))
    q = linear(h, g("self_attn.linear_q.weight"), g("self_attn.linear_q.bias"))
    k = linear(h, g("self_attn.linear_k.weight"), g("self_attn.linear_k.bias"))
    v = linear(h, g("self_attn.linear_v.weight"), g("self_attn.linear_v.bias"))
    a = attention(q, k, v, ADAPTOR_HEADS, lengths)
    x = x + linear(a, g("self_attn.linear_out.weight"), g("self_attn.linear_out.bias"))
    h = layer_norm(x, g("norm2.weight"), g("norm2.bias"))
    h = np.maximum(linear(h, g("feed_forward.w_1.weight"), g("feed_forward.w_1.bias")), 0.0)
    return x + linear(h, g("feed_forward.w_2.weight"), g("feed_forward.w_2.bias"))


def tower_segments(x, lengths, w, cfg):
    """SenseVoiceEncoder::forward (:453-478) + AudioAdaptor::forward (adaptor.rs:247-261) over utterances of `lengths` rows stacked in
    x [sum T, lfr_dim].  -> dict of the stages the device can show: pos, after_norm, tp_norm, linear2, out."""
    x = np.asarray(x, np.float64)
    g = lambda name: np.asarray(w[name], np.float64)
    st = {}
    h = np.concatenate([position_add(x[lo:hi]) for lo, hi in segments(lengths)])
    st["pos"] = h
    main, tp = layer_prefixes(cfg)
    heads = cfg["attention_heads"]
    for p in main:
        h = encoder_layer(h, layer_params(w, p), heads, lengths)
    h = layer_norm(h, g("encoder.after_norm.weight"), g("encoder.after_norm.bias"))
    st["after_norm"] = h
    for p in tp:
        h = encoder_layer(h, layer_params(w, p), heads, lengths)
    h = layer_norm(h, g("encoder.tp_norm.weight"), g("encoder.tp_norm.bias"))
    st["tp_norm"] = h
    h = np.maximum(linear(h, g("adaptor.linear1.weight"), g("adaptor.linear1.bias")), 0.0)
    h = linear(h, g("adaptor.linear2.weight"), g("adaptor.linear2.bias"))
    st["linear2"] = h
    for i in range(cfg["n_layer"]):
        h = adaptor_block(h, w, f"adaptor.blocks.{i}", lengths)
    st["out"] = h
    return st


def tower(x, w, cfg):
    """one utterance alone: the definition"""
    return tower_segments(x, [np.asarray(x).shape[0]], w, cfg)


DEFAULT_CFG = dict(lfr_dim=560, output_size=512, attention_heads=4, linear_units=2048, num_blocks=50, tp_blocks=20, kernel_size=11,
                   encoder_dim=512, ffn_dim=2048, llm_dim=1024, n_layer=2)
TINY_CFG = dict(lfr_dim=40, output_size=256, attention_heads=2, linear_units=512, num_blocks=3, tp_blocks=2, kernel_size=11,
                encoder_dim=256, ffn_dim=512, llm_dim=1024, n_layer=2)


def weight_shapes(cfg) -> dict:
    dim, ffn, llm, k = cfg["output_size"], cfg["linear_units"], cfg["llm_dim"], cfg["kernel_size"]
    s = {}
    main, tp = layer_prefixes(cfg)
    for i, p in enumerate(main + tp):
        d_in = cfg["lfr_dim"] if i == 0 else dim
        s.update({f"{p}.norm1.weight": (d_in,), f"{p}.norm1.bias": (d_in,), f"{p}.self_attn.linear_q_k_v.weight": (3 * dim, d_in),
                  f"{p}.self_attn.linear_q_k_v.bias": (3 * dim,), f"{p}.self_attn.linear_out.weight": (dim, dim),
                  f"{p}.self_attn.linear_out.bias": (dim,), f"{p}.self_attn.fsmn.weight": (dim, 1, k), f"{p}.norm2.weight": (dim,),
                  f"{p}.norm2.bias": (dim,), f"{p}.feed_forward.w_1.weight": (ffn, dim), f"{p}.feed_forward.w_1.bias": (ffn,),
                  f"{p}.feed_forward.w_2.weight": (dim, ffn), f"{p}.feed_forward.w_2.bias": (dim,)})
    for n in ("after_norm", "tp_norm"):
        s[f"encoder.{n}.weight"] = s[f"encoder.{n}.bias"] = (dim,)
    s["adaptor.linear1.weight"], s["adaptor.linear1.bias"] = (cfg["ffn_dim"], cfg["encoder_dim"]), (cfg["ffn_dim"],)
    s["adaptor.linear2.weight"], s["adaptor.linear2.bias"] = (llm, cfg["ffn_dim"]), (llm,)
    for i in range(cfg["n_layer"]):
        p = f"adaptor.blocks.{i}"
        for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
            s[f"{p}.self_attn.{n}.weight"], s[f"{p}.self_attn.{n}.bias"] = (llm, llm), (llm,)
        for n in ("norm1", "norm2"):
            s[f"{p}.{n}.weight"] = s[f"{p}.{n}.bias"] = (llm,)
        s[f"{p}.feed_forward.w_1.weight"], s[f"{p}.feed_forward.w_1.bias"] = (ADAPTOR_FFN, llm), (ADAPTOR_FFN,)
        s[f"{p}.feed_forward.w_2.weight"], s[f"{p}.feed_forward.w_2.bias"] = (llm, ADAPTOR_FFN), (llm,)
    return s


def synth_weights(cfg, seed: int = 3) -> dict:
    """float32 weights of the config's shapes: Linear ~ N(0, 1/fan_in), norm scales near 1, biases small -- and FSMN taps ~ N(0, 0.3), so a
    tap that reaches into a neighbouring utterance changes a row by O(1)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in weight_shapes(cfg).items():
        if name.endswith("fsmn.weight"):
            a = rng.normal(0.0, 0.3, shape)
        elif ".norm" in name or "_norm." in name:
            a = 1.0 + 0.1 * rng.normal(size=shape) if name.endswith("weight") else 0.05 * rng.normal(size=shape)
        elif name.endswith(".bias"):
            a = 0.02 * rng.normal(size=shape)
        else:
            a = rng.normal(0.0, 1.0 / np.sqrt(shape[-1]), shape)
        out[name] = a.astype(np.float32)
    return out
