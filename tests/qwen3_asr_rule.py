"""Host rules the Qwen3-ASR tests hold the device to.

forward_from_rows: the reference's forward_embeddings(inputs_embeds, cache) (qwen3-asr-mlx/src/qwen.rs, model.rs:720-769, 782) on the
frozen decoder oracle -- Qwen3Oracle.forward from the point where the embedding rows exist, so a prompt pass over caller-supplied
rows (omx_qwen3_prefill_embeds) has a reference that owes nothing to the device's gather."""
import numpy as np

from oracle import ref_core as rc


def embed_rows(oracle, ids):
    """Qwen3Oracle.forward's embedding rows of `ids` [T] -> [T, hidden] (values of the activation dtype, as float32)."""
    ids = np.asarray(ids)
    w = oracle.w
    if oracle.quant is None:
        return w["model.embed_tokens.weight"][ids]
    bits, group = oracle.quant
    return rc.dequantize(w["model.embed_tokens.weight"][ids], w["model.embed_tokens.scales"][ids], w["model.embed_tokens.biases"][ids],
                         group, bits, oracle.dt)


def forward_from_rows(oracle, h, caches):
    """Qwen3Oracle.forward (model.rs:394-424 + 480-490) with the embedding gather replaced by the rows h [T, hidden] or [1, T, hidden]:
    the rows are cast to the activation dtype (as_dtype, model.rs:759: one round-to-nearest-even), then every block, the final norm
    and the head over ALL positions -> logits [1, T, V].  caches: [] for an empty cache, or the list an earlier call filled."""
    cfg = oracle.cfg
    h = rc.rnd(np.asarray(h, dtype=np.float32), oracle.dt)
    if h.ndim == 2:
        h = h[None]
    T = h.shape[1]
    off = caches[0].offset() if caches else None
    m = rc.create_attention_mask(T, off, None, True)
    mask = m if isinstance(m, np.ndarray) else None
    if not caches:
        caches.extend(rc.KVCache() for _ in range(cfg.num_hidden_layers))
    for i in range(cfg.num_hidden_layers):
        h = oracle.block(i, h, mask, caches[i])
    h = rc.rms_norm(h, oracle.w["model.norm.weight"], cfg.rms_norm_eps, oracle.dt)
    return oracle.lin(h, "model.embed_tokens" if cfg.tie_word_embeddings else "lm_head")


def generate_from_rows(oracle, h, n_new):
    """Qwen3Oracle.generate(..., return_logits=True) at temperature 0 with the prompt given as rows: (tokens uint32 [n_new],
    logits [n_new, V] -- the prompt's last position, then each decode step's)."""
    caches = []
    last = forward_from_rows(oracle, h, caches)[:, -1, :]
    y = rc.sample_greedy(last)
    toks, rows = [int(y[0])], [last[0]]
    for _ in range(n_new - 1):
        last = oracle.forward(y[:, None].astype(np.int64), caches)[:, -1, :]
        y = rc.sample_greedy(last)
        toks.append(int(y[0]))
        rows.append(last[0])
    return np.array(toks, dtype=np.uint32), np.stack(rows)


# ---- the audio tower (qwen3-asr-mlx/src/encoder.rs:76-105, 254-458) in numpy float64 ----

import math

try:
    from scipy.special import erf as _erf          # the same function, vectorised in C
except ImportError:                                # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    """nn::gelu (mlx-rs/src/nn/activation.rs:164): x * (1 + erf(x / sqrt 2)) / 2, the exact form"""
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def conv_len(n):
    """output length of a kernel-3 stride-2 padding-1 convolution"""
    return (n + 2 - 3) // 2 + 1


def feat_extract_output_lengths(n, chunk=100):
    """get_feat_extract_output_lengths (encoder.rs:76-80) with the floor division of the model's own definition (Python's //): a
    remainder of 0 frames makes 0 rows.  (The reference's i32 `/` truncates: (0 - 1) / 2 = 0, one row too many at every multiple of
    the chunk -- 14 "valid" rows of the 13 a full chunk has.)"""
    per_chunk = conv_len(conv_len(conv_len(chunk)))
    leave = n % chunk
    f = (leave - 1) // 2 + 1
    return ((f - 1) // 2 + 1 - 1) // 2 + 1 + (n // chunk) * per_chunk


def sinusoid_table(length, channels):
    """SinusoidalPositionEmbedding::new (encoder.rs:89-105)"""
    half = channels // 2
    log_timescale = math.log(10000.0) / (half - 1)
    scaled = np.arange(length, dtype=np.float64)[:, None] * np.exp(-log_timescale * np.arange(half, dtype=np.float64))[None, :]
    return np.concatenate([np.sin(scaled), np.cos(scaled)], axis=1)


def conv3x3_s2(x, w, b):
    """nn::Conv2d, kernel 3, stride 2, padding 1, NHWC: x [B, H, W, Ci], w [Co, 3, 3, Ci], b [Co] -> [B, OH, OW, Co]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, Ci = x.shape
    OH, OW = conv_len(H), conv_len(W)
    xp = np.zeros((B, H + 2, W + 2, Ci))
    xp[:, 1:H + 1, 1:W + 1] = x
    cols = np.empty((B, OH, OW, 9 * Ci))
    for kh in range(3):
        for kw in range(3):
            cols[..., (kh * 3 + kw) * Ci:(kh * 3 + kw + 1) * Ci] = xp[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2]
    y = cols.reshape(-1, 9 * Ci) @ w.reshape(w.shape[0], -1).T + np.asarray(b, np.float64)
    return y.reshape(B, OH, OW, -1)


def chunk_mel(mel, chunk):
    """encoder.rs:307-351: [n_mels, F] -> ([chunks, n_mels, longest], chunk lengths), zero-padded on the right"""
    mel = np.asarray(mel, np.float64)
    F = mel.shape[1]
    lens = [min(chunk, F - s) for s in range(0, F, chunk)]
    out = np.zeros((len(lens), mel.shape[0], max(lens)))
    for i, n in enumerate(lens):
        out[i, :, :n] = mel[:, i * chunk:i * chunk + n]
    return out, lens


def window_boundaries(total, window):
    """encoder.rs:401-410"""
    b = [0] + [w * window for w in range(1, total // window + 1)]
    if total % window:
        b.append(total)
    return b


def block_mask(n, boundaries):
    """create_block_attention_mask (encoder.rs:439-458): additive, -1e9 outside the diagonal blocks"""
    m = np.full((n, n), -1e9)
    for s, e in zip(boundaries[:-1], boundaries[1:]):
        m[s:min(e, n), s:min(e, n)] = 0.0
    return m


def _softmax(s):
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    return p / p.sum(axis=-1, keepdims=True)


def masked_attention(q, k, v, heads, mask):
    """the reference's form: full attention under the additive mask, scale 1 (q arrives scaled); q / k / v [N, heads * hd]"""
    N = q.shape[0]
    qh, kh, vh = (np.asarray(a, np.float64).reshape(N, heads, -1).transpose(1, 0, 2) for a in (q, k, v))
    p = _softmax(qh @ kh.transpose(0, 2, 1) + mask[None])
    return (p @ vh).transpose(1, 0, 2).reshape(N, -1)


def window_attention(q, k, v, heads, window):
    """the same, restricted per window: unmasked and bidirectional inside [w * window, (w + 1) * window)"""
    N = q.shape[0]
    out = np.empty((N, q.shape[1]))
    for s in range(0, N, window):
        e = min(s + window, N)
        out[s:e] = masked_attention(q[s:e], k[s:e], v[s:e], heads, np.zeros((e - s, e - s)))
    return out


def layer_norm(x, w, b, eps=1e-5):
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def _lin(x, w, b=None):
    y = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    return y if b is None else y + np.asarray(b, np.float64)


def encoder_layer(x, w, p, heads, window):
    """AudioEncoderLayer::forward_layer (encoder.rs:212-227) with AudioAttention::forward_attn (:146-182)"""
    hd = x.shape[1] // heads
    h = layer_norm(x, w[p + "self_attn_layer_norm.weight"], w[p + "self_attn_layer_norm.bias"])
    q = _lin(h, w[p + "self_attn.q_proj.weight"], w[p + "self_attn.q_proj.bias"]) * hd ** -0.5
    k = _lin(h, w[p + "self_attn.k_proj.weight"], w[p + "self_attn.k_proj.bias"])
    v = _lin(h, w[p + "self_attn.v_proj.weight"], w[p + "self_attn.v_proj.bias"])
    a = window_attention(q, k, v, heads, window)
    x = x + _lin(a, w[p + "self_attn.out_proj.weight"], w[p + "self_attn.out_proj.bias"])
    h = layer_norm(x, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"])
    h = gelu(_lin(h, w[p + "fc1.weight"], w[p + "fc1.bias"]))
    return x + _lin(h, w[p + "fc2.weight"], w[p + "fc2.bias"])


def tower(mel, w, cfg):
    """AudioEncoder::forward_encoder (encoder.rs:303-436).  cfg: dict with config.json's audio_config keys.  Returns a dict of every
    stage: x1 / x2 / x3 [chunks, f, t, ds], rows [N, d_model] (assembled, positions added, compacted), out [N, output_dim]."""
    chunk = 2 * cfg["n_window"]
    x, lens = chunk_mel(mel, chunk)
    valid = [feat_extract_output_lengths(n, chunk) for n in lens]
    st = {}
    st["x1"] = gelu(conv3x3_s2(x[..., None], w["conv2d1.weight"], w["conv2d1.bias"]))
    st["x2"] = gelu(conv3x3_s2(st["x1"], w["conv2d2.weight"], w["conv2d2.bias"]))
    st["x3"] = gelu(conv3x3_s2(st["x2"], w["conv2d3.weight"], w["conv2d3.bias"]))
    B, f, t, c = st["x3"].shape
    y = _lin(st["x3"].transpose(0, 2, 3, 1).reshape(B, t, c * f), w["conv_out.weight"])
    y = y + sinusoid_table(cfg["max_source_positions"], cfg["d_model"])[:t][None]
    h = np.concatenate([y[i, :valid[i]] for i in range(B)], axis=0)
    st["rows"] = h
    total = feat_extract_output_lengths(np.asarray(mel).shape[1], chunk)
    assert total == h.shape[0]
    window = max(valid) * (cfg["n_window_infer"] // chunk)
    for l in range(cfg["encoder_layers"]):
        h = encoder_layer(h, w, f"layers.{l}.", cfg["encoder_attention_heads"], window)
    h = layer_norm(h, w["ln_post.weight"], w["ln_post.bias"])
    h = gelu(_lin(h, w["proj1.weight"], w["proj1.bias"]))
    st["out"] = _lin(h, w["proj2.weight"], w["proj2.bias"])
    return st


def tower_weight_shapes(cfg):
    """the keys behind "audio_tower." and their shapes (encoder.rs:255-297)"""
    ds, d, ffn = cfg["downsample_hidden_size"], cfg["d_model"], cfg["encoder_ffn_dim"]
    f3 = conv_len(conv_len(conv_len(cfg["num_mel_bins"])))
    s = {"conv2d1.weight": (ds, 3, 3, 1), "conv2d1.bias": (ds,), "conv2d2.weight": (ds, 3, 3, ds), "conv2d2.bias": (ds,),
         "conv2d3.weight": (ds, 3, 3, ds), "conv2d3.bias": (ds,), "conv_out.weight": (d, ds * f3),
         "ln_post.weight": (d,), "ln_post.bias": (d,), "proj1.weight": (d, d), "proj1.bias": (d,),
         "proj2.weight": (cfg["output_dim"], d), "proj2.bias": (cfg["output_dim"],)}
    for l in range(cfg["encoder_layers"]):
        p = f"layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"], s[p + f"self_attn.{n}.bias"] = (d, d), (d,)
        s[p + "self_attn_layer_norm.weight"] = s[p + "self_attn_layer_norm.bias"] = (d,)
        s[p + "final_layer_norm.weight"] = s[p + "final_layer_norm.bias"] = (d,)
        s[p + "fc1.weight"], s[p + "fc1.bias"], s[p + "fc2.weight"], s[p + "fc2.bias"] = (ffn, d), (ffn,), (d, ffn), (d,)
    return s


def tower_synth_weights(cfg, seed=0):
    """seeded float32 weights on the bf16 grid (a bf16 checkpoint widened): matrices ~ N(0, 1 / fan_in), norm weights 1 + noise"""
    g = np.random.default_rng(seed)
    out = {}
    for name, shape in tower_weight_shapes(cfg).items():
        if name.endswith("norm.weight") or name == "ln_post.weight":
            a = 1.0 + 0.05 * g.standard_normal(shape)
        elif name.endswith(".bias"):
            a = 0.05 * g.standard_normal(shape)
        else:
            a = g.standard_normal(shape) / math.sqrt(int(np.prod(shape[1:])))
        out[name] = rc.bf16_round(a.astype(np.float32))
    return out
