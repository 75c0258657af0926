"""Host rule the DeepSeek-OCR-2 vision tests hold the device to: the SAM ViT-B tower, the visual-causal-flow encoder, the projector and
`encode_image` in numpy float64, written from deepseek-ocr2-mlx/src/vision.rs (ImageEncoderViT::forward :385-431, SamBlock :243-267,
SamAttention :94-217, window_partition / window_unpartition :271-326, nearest_interpolate_2d :435-454), qwen2_encoder.rs
(forward_vision :198-244, Qwen2Attention :51-112, build_visual_causal_mask :249-288) and lib.rs (encode_image :467-497).  The bias is
built the reference's literal way -- gathered [q, k, 64] tables, then a full [N, N] array per head -- which only a rule can afford."""
import math

import numpy as np

from oracle import ref_core as rc
from qwen3_asr_rule import _lin, _softmax
from vit_rule import layer_norm, patch_embed

SAM = dict(embed_dim=768, depth=12, num_heads=12, mlp_dim=3072, window=14, global_attn_indexes=(2, 5, 8, 11), patch_size=16)
VCF = dict(hidden=896, layers=24, heads=14, kv_heads=2, intermediate=4864, rope_theta=1e6, eps=1e-6)
NECK = (256, 512, 896)                      # neck, net_2, net_3 widths of the checkpoint
# the tiny set the device tests run end to end at the real image sizes
TINY_SAM = dict(SAM, embed_dim=128, num_heads=2, mlp_dim=308, depth=4, global_attn_indexes=(1, 3))
TINY_NECK = (32, 64, 256)
TINY_VCF = dict(VCF, hidden=256, heads=4, kv_heads=2, intermediate=308, layers=3)
TINY_OUT = 160
SAM_PREFIX, VCF_PREFIX = "model.sam_model", "model.qwen2_model"


def behind(weights, prefix):
    return {k[len(prefix) + 1:]: v for k, v in weights.items() if k.startswith(prefix + ".")}


def gelu_tanh(x):
    """nn::gelu_approximate (mlx-rs/src/nn/activation.rs:168-177)"""
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def resample_indices(src, dst):
    """row i of dst <- min(int(float32(i) * (float32(src) / float32(dst))), src - 1): get_rel_pos_1d (vision.rs:186-196) and
    nearest_interpolate_2d (:435-454) alike"""
    scale = np.float32(src) / np.float32(dst)
    return [min(int(np.float32(i) * scale), src - 1) for i in range(dst)]


def rel_pos_gathered(table, g):
    """get_rel_pos_1d(g, g, table) (vision.rs:182-217) -> [g, g, hd]: entry [q, k] is row q - k + g - 1 of the table, the table first
    resampled to 2 g - 1 rows when its length differs"""
    t = np.asarray(table, np.float64)
    if t.shape[0] != 2 * g - 1:
        t = t[resample_indices(t.shape[0], 2 * g - 1)]
    idx = np.arange(g)[:, None] - np.arange(g)[None, :] + (g - 1)
    return t[idx]


def rel_pos_bias(q, gh, gw, th, tw):
    """compute_rel_pos_bias (vision.rs:138-178) for one head: q [gh * gw, hd] (unscaled) -> [N, N]"""
    rh, rw = rel_pos_gathered(th, gh), rel_pos_gathered(tw, gw)
    rq = np.asarray(q, np.float64).reshape(gh, gw, -1)
    rel_h = np.einsum("hwc,hkc->hwk", rq, rh)                      # [gh, gw, kh]
    rel_w = np.einsum("hwc,wkc->hwk", rq, rw)                      # [gh, gw, kw]
    return (rel_h[:, :, :, None] + rel_w[:, :, None, :]).reshape(gh * gw, gh * gw)


def grid_attention(qkv, heads, gh, gw, th, tw, bias=True, swap=False, key_mask=None):
    """SamAttention::forward_spatial without its Linears (vision.rs:104-132) on one grid: qkv [gh * gw, 3 * heads * hd] -> [N, heads * hd].
    bias / swap / key_mask are the deliberate mistakes of test_deepencoder_rule.py: no bias, h and w tables exchanged, keys left out."""
    N, d = gh * gw, qkv.shape[1] // 3
    hd = d // heads
    x = np.asarray(qkv, np.float64)
    out = np.empty((N, d))
    for h in range(heads):
        q, k, v = (x[:, i * d + h * hd:i * d + (h + 1) * hd] for i in range(3))
        s = q @ k.T * hd ** -0.5
        if bias:
            s = s + (rel_pos_bias(q, gh, gw, tw, th) if swap else rel_pos_bias(q, gh, gw, th, tw))
        if key_mask is not None:
            s = np.where(key_mask[None, :], s, -np.inf)
        out[:, h * hd:(h + 1) * hd] = _softmax(s) @ v
    return out


def window_partition(x, ws):
    """vision.rs:271-299 for one image: x [H, W, C] -> ([windows, ws, ws, C], (hp, wp)), zero padding on the bottom and right"""
    x = np.asarray(x, np.float64)
    H, W, C = x.shape
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    xp = np.zeros((H + ph, W + pw, C))
    xp[:H, :W] = x
    nh, nw = (H + ph) // ws, (W + pw) // ws
    return xp.reshape(nh, ws, nw, ws, C).transpose(0, 2, 1, 3, 4).reshape(nh * nw, ws, ws, C), (H + ph, W + pw)


def window_unpartition(windows, ws, pad_hw, hw):
    """vision.rs:302-326 for one image"""
    (hp, wp), (H, W) = pad_hw, hw
    nh, nw, C = hp // ws, wp // ws, windows.shape[-1]
    return windows.reshape(nh, nw, ws, ws, C).transpose(0, 2, 1, 3, 4).reshape(hp, wp, C)[:H, :W]


def sam_attention(qkv, heads, grid, window, th, tw, pad_qkv=None, **mistake):
    """the attention of one image as omx_sam_attention_f32 defines it: qkv [gh * gw, 3 d] in image order; window 0 global, else the
    grid zero-padded and cut into windows, a padded token's q | k | v being pad_qkv (the qkv Linear's bias: the padding is applied after
    norm1).  mistake: bias=False, swap=True, mask_padded=True."""
    gh, gw = grid
    d3 = qkv.shape[1]
    mask_padded = mistake.pop("mask_padded", False)
    if not window:
        return grid_attention(qkv, heads, gh, gw, th, tw, **mistake)
    real, _ = window_partition(np.ones((gh, gw, 1)), window)
    wins, pad_hw = window_partition(np.asarray(qkv, np.float64).reshape(gh, gw, d3), window)
    if (real == 0).any():
        assert pad_qkv is not None, "a padded grid needs the padded token's row"
        wins = np.where(real > 0, wins, np.asarray(pad_qkv, np.float64))
    out = np.stack([grid_attention(w.reshape(window * window, d3), heads, window, window, th, tw,
                                   key_mask=(r.reshape(-1) > 0) if mask_padded else None, **mistake).reshape(window, window, -1)
                    for w, r in zip(wins, real)])
    return window_unpartition(out, window, pad_hw, (gh, gw)).reshape(gh * gw, -1)


def conv3x3(x, w, stride):
    """nn::Conv2d, kernel 3, padding 1, no bias, NHWC x [B, H, W, Ci]; w is the CHECKPOINT's [Co, Ci, 3, 3], read as [Co, 3, 3, Ci]
    (vision.rs:472-475) -> [B, OH, OW, Co]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64).transpose(0, 2, 3, 1)
    B, H, W, Ci = x.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = np.zeros((B, H + 2, W + 2, Ci))
    xp[:, 1:H + 1, 1:W + 1] = x
    cols = np.empty((B, OH, OW, 9 * Ci))
    for kh in range(3):
        for kw in range(3):
            cols[..., (kh * 3 + kw) * Ci:(kh * 3 + kw + 1) * Ci] = xp[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride]
    return (cols.reshape(-1, 9 * Ci) @ w.reshape(w.shape[0], -1).T).reshape(B, OH, OW, -1)


def pos_embed_for(pos, G):
    """vision.rs:389-398: pos_embed [1, P, P, C] as is when P == G, else gathered nearest-neighbour per axis"""
    pos = np.asarray(pos, np.float64)[0]
    P = pos.shape[0]
    if P == G:
        return pos
    idx = resample_indices(P, G)
    return pos[idx][:, idx]


def sam_block(x, w, p, cfg, window):
    """SamBlock::forward (vision.rs:243-267) on one image x [G, G, C], the literal way: the padding is applied to norm1's output, the qkv
    and proj Linears run on the windows"""
    G, d, heads = x.shape[0], x.shape[2], cfg["num_heads"]
    h = layer_norm(x, w[p + "norm1.weight"], w[p + "norm1.bias"])
    wins, pad_hw = window_partition(h, window) if window else (h[None], (G, G))
    g = window if window else G
    outs = []
    for win in wins:
        qkv = _lin(win.reshape(g * g, d), w[p + "attn.qkv.weight"], w[p + "attn.qkv.bias"])
        a = grid_attention(qkv, heads, g, g, w[p + "attn.rel_pos_h"], w[p + "attn.rel_pos_w"])
        outs.append(_lin(a, w[p + "attn.proj.weight"], w[p + "attn.proj.bias"]).reshape(g, g, d))
    a = window_unpartition(np.stack(outs), window, pad_hw, (G, G)) if window else outs[0]
    x = x + a
    m = gelu_tanh(_lin(layer_norm(x, w[p + "norm2.weight"], w[p + "norm2.bias"]), w[p + "mlp.lin1.weight"], w[p + "mlp.lin1.bias"]))
    return x + _lin(m, w[p + "mlp.lin2.weight"], w[p + "mlp.lin2.bias"])


def sam_tower(images, w, cfg):
    """ImageEncoderViT::forward (vision.rs:385-431) on images [B, S, S, 3] in [-1, 1].  Returns every stage as rows over the stacked
    images: patches, h0, block<N>, neck (after the second LayerNorm2d) and out [B * (G / 4)^2, 896]."""
    images = np.asarray(images, np.float64)
    B, P, d = images.shape[0], cfg["patch_size"], cfg["embed_dim"]
    G = images.shape[1] // P
    st = {"patches": np.concatenate([patch_embed(im, w["patch_embed.proj.weight"], w.get("patch_embed.proj.bias"), P) for im in images])}
    h = st["patches"].reshape(B, G, G, d) + pos_embed_for(w["pos_embed"], G)
    st["h0"] = h.reshape(-1, d)
    for l in range(cfg["depth"]):
        window = 0 if l in cfg["global_attn_indexes"] else cfg["window"]
        h = np.stack([sam_block(x, w, f"blocks.{l}.", cfg, window) for x in h])
        st[f"block{l}"] = h.reshape(-1, d)
    c1 = w["neck.0.weight"].shape[0]
    n = _lin(h.reshape(-1, d), np.asarray(w["neck.0.weight"]).reshape(c1, d))
    n = layer_norm(n, w["neck.1.weight"], w["neck.1.bias"])                       # LayerNorm2d: over the channels of a pixel
    n = conv3x3(n.reshape(B, G, G, c1), w["neck.2.weight"], 1)
    n = layer_norm(n, w["neck.3.weight"], w["neck.3.bias"])
    st["neck"] = n.reshape(-1, c1)
    n = conv3x3(conv3x3(n, w["net_2.weight"], 2), w["net_3.weight"], 2)
    st["out"] = n.reshape(-1, n.shape[-1])
    st["rows_per_image"] = n.shape[1] * n.shape[2]
    return st


def rms_norm(x, w, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * np.asarray(w, np.float64)


def rope(x, base):
    """nn::Rope, traditional = false, offset 0: x [L, heads, 64], pairs (i, i + 32), theta_i = base^(-2 i / 64)"""
    x = np.asarray(x, np.float64)
    L, half = x.shape[0], x.shape[-1] // 2
    ang = np.arange(L)[:, None] * (float(base) ** (-np.arange(half) / half))[None, :]
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    return np.concatenate([x1 * c - x2 * s, x1 * s + x2 * c], axis=-1)


def visual_causal_mask(n_image, n_query):
    """build_visual_causal_mask (qwen2_encoder.rs:249-288) as a boolean "may attend" matrix: image rows see the image rows, query row i
    sees every image row and the query rows up to itself"""
    total = n_image + n_query
    i, j = np.arange(total)[:, None], np.arange(total)[None, :]
    return np.where(i < n_image, j < n_image, j <= i)


def prefix_causal_attention(qkv, heads, kv_heads, n_prefix):
    """one sequence of the attention omx_prefix_causal_attention_f32 defines: qkv [L, (heads + 2 kv_heads) * 64], row i sees keys
    j < max(n_prefix, i + 1); query head h reads key/value head h // (heads // kv_heads)"""
    x = np.asarray(qkv, np.float64)
    L = x.shape[0]
    q, k, v = x[:, :heads * 64].reshape(L, heads, 64), x[:, heads * 64:(heads + kv_heads) * 64].reshape(L, kv_heads, 64), \
        x[:, (heads + kv_heads) * 64:(heads + 2 * kv_heads) * 64].reshape(L, kv_heads, 64)
    see = np.arange(L)[None, :] < np.maximum(n_prefix, np.arange(L) + 1)[:, None]
    out = np.empty((L, heads * 64))
    for h in range(heads):
        g = h // (heads // kv_heads)
        s = np.where(see, q[:, h] @ k[:, g].T * 0.125, -np.inf)
        out[:, h * 64:(h + 1) * 64] = _softmax(s) @ v[:, g]
    return out


def vcf_layer(x, w, p, cfg, n_image):
    """Qwen2Layer::forward_with_mask (qwen2_encoder.rs:162-174) on one sequence x [L, hidden]"""
    H, KV, L = cfg["heads"], cfg["kv_heads"], x.shape[0]
    n = rms_norm(x, w[p + "input_layernorm.weight"], cfg["eps"])
    q = rope(_lin(n, w[p + "self_attn.q_proj.weight"], w[p + "self_attn.q_proj.bias"]).reshape(L, H, 64), cfg["rope_theta"])
    k = rope(_lin(n, w[p + "self_attn.k_proj.weight"], w[p + "self_attn.k_proj.bias"]).reshape(L, KV, 64), cfg["rope_theta"])
    v = _lin(n, w[p + "self_attn.v_proj.weight"], w[p + "self_attn.v_proj.bias"]).reshape(L, KV, 64)
    see = visual_causal_mask(n_image, L - n_image)
    a = np.empty((L, H * 64))
    for h in range(H):
        g = h // (H // KV)
        a[:, h * 64:(h + 1) * 64] = _softmax(np.where(see, q[:, h] @ k[:, g].T * 0.125, -np.inf)) @ v[:, g]
    x = x + _lin(a, w[p + "self_attn.o_proj.weight"])
    n = rms_norm(x, w[p + "post_attention_layernorm.weight"], cfg["eps"])
    gate, up = _lin(n, w[p + "mlp.gate_proj.weight"]), _lin(n, w[p + "mlp.up_proj.weight"])
    return x + _lin(gate / (1.0 + np.exp(-gate)) * up, w[p + "mlp.down_proj.weight"])


def vcf_encoder(x, w, cfg, images=1):
    """Qwen2Encoder::forward_vision (qwen2_encoder.rs:198-244) over `images` stacked images' rows x [images * n_img, hidden].  Returns
    the stages layer<N> [images * L, hidden] and out [images * n_query, hidden]."""
    x = np.asarray(x, np.float64)
    n_img = x.shape[0] // images
    query = np.asarray(w["query_768.weight" if n_img == 144 else "query_1024.weight"], np.float64)
    hs = [np.concatenate([x[b * n_img:(b + 1) * n_img], query]) for b in range(images)]
    st = {}
    for l in range(cfg["layers"]):
        hs = [vcf_layer(h, w, f"model.model.layers.{l}.", cfg, n_img) for h in hs]
        st[f"layer{l}"] = np.concatenate(hs)
    st["out"] = np.concatenate([rms_norm(h, w["model.model.norm.weight"], cfg["eps"])[n_img:] for h in hs])
    return st


def encode_view(images, weights, sam_cfg, vcf_cfg):
    """SAM -> encoder -> projector over stacked images of one size (lib.rs:473-478 / :482-485) -> [B * n_query, out_dim]"""
    sam = sam_tower(images, behind(weights, SAM_PREFIX), sam_cfg)
    rows = vcf_encoder(sam["out"], behind(weights, VCF_PREFIX), vcf_cfg, images=len(images))["out"]
    return _lin(rows, weights["model.projector.layers.weight"], weights["model.projector.layers.bias"])


def encode_image(global_image, crops, weights, sam_cfg, vcf_cfg):
    """DeepseekOCR2::encode_image (lib.rs:467-497): the crops' rows in the order given, the global view's rows, the separator"""
    parts = [] if crops is None or len(crops) == 0 else [encode_view(np.asarray(crops), weights, sam_cfg, vcf_cfg)]
    parts.append(encode_view(np.asarray(global_image)[None], weights, sam_cfg, vcf_cfg))
    parts.append(np.asarray(weights["model.view_seperator"], np.float64).reshape(1, -1))
    return np.concatenate(parts)


def weight_shapes(sam_cfg, vcf_cfg, neck=NECK, out_dim=1280, pos_grid=64):
    """every key of the vision side and its checkpoint shape (vision.rs:460-611, qwen2_encoder.rs:294-397, lib.rs:959-974)"""
    d, ffn, P = sam_cfg["embed_dim"], sam_cfg["mlp_dim"], sam_cfg["patch_size"]
    hd = d // sam_cfg["num_heads"]
    c1, c2, c3 = neck
    s = {"patch_embed.proj.weight": (d, 3, P, P), "patch_embed.proj.bias": (d,), "pos_embed": (1, pos_grid, pos_grid, d),
         "neck.0.weight": (c1, d, 1, 1), "neck.1.weight": (c1,), "neck.1.bias": (c1,), "neck.2.weight": (c1, c1, 3, 3), "neck.3.weight": (c1,),
         "neck.3.bias": (c1,), "net_2.weight": (c2, c1, 3, 3), "net_3.weight": (c3, c2, 3, 3)}
    for l in range(sam_cfg["depth"]):
        p = f"blocks.{l}."
        rel = 2 * pos_grid - 1 if l in sam_cfg["global_attn_indexes"] else 2 * sam_cfg["window"] - 1
        s[p + "norm1.weight"] = s[p + "norm1.bias"] = s[p + "norm2.weight"] = s[p + "norm2.bias"] = (d,)
        s[p + "attn.qkv.weight"], s[p + "attn.qkv.bias"] = (3 * d, d), (3 * d,)
        s[p + "attn.rel_pos_h"] = s[p + "attn.rel_pos_w"] = (rel, hd)
        s[p + "attn.proj.weight"], s[p + "attn.proj.bias"] = (d, d), (d,)
        s[p + "mlp.lin1.weight"], s[p + "mlp.lin1.bias"], s[p + "mlp.lin2.weight"], s[p + "mlp.lin2.bias"] = (ffn, d), (ffn,), (d, ffn), (d,)
    out = {SAM_PREFIX + "." + k: v for k, v in s.items()}
    h, I, H, KV = vcf_cfg["hidden"], vcf_cfg["intermediate"], vcf_cfg["heads"], vcf_cfg["kv_heads"]
    assert c3 == h, "net_3 feeds the encoder"
    q = {"model.model.norm.weight": (h,), "query_768.weight": (144, h), "query_1024.weight": (256, h)}
    for l in range(vcf_cfg["layers"]):
        p = f"model.model.layers.{l}."
        q[p + "input_layernorm.weight"] = q[p + "post_attention_layernorm.weight"] = (h,)
        q[p + "self_attn.q_proj.weight"], q[p + "self_attn.q_proj.bias"] = (H * 64, h), (H * 64,)
        for n in ("k_proj", "v_proj"):
            q[p + f"self_attn.{n}.weight"], q[p + f"self_attn.{n}.bias"] = (KV * 64, h), (KV * 64,)
        q[p + "self_attn.o_proj.weight"] = (h, H * 64)
        q[p + "mlp.gate_proj.weight"] = q[p + "mlp.up_proj.weight"] = (I, h)
        q[p + "mlp.down_proj.weight"] = (h, I)
    out.update({VCF_PREFIX + "." + k: v for k, v in q.items()})
    out["model.projector.layers.weight"], out["model.projector.layers.bias"], out["model.view_seperator"] = (out_dim, h), (out_dim,), (out_dim,)
    return out


def synth_tensor(g, name, shape):
    """scaled as vit_rule.synth_weights scales, so that activations stay O(1): matrices and convolutions ~ N(0, 1 / fan_in), norm weights
    1 + noise, biases small, positions / queries / separator ~ N(0, 0.5^2); the relative-position tables ~ N(0, 0.1^2): q . T then has
    about the spread of the scaled scores (8 x 0.1 per table against 1)"""
    if name.endswith(("norm1.weight", "norm2.weight", "norm.weight", "layernorm.weight", "neck.1.weight", "neck.3.weight")):
        a = 1.0 + 0.05 * g.standard_normal(shape)
    elif name.endswith(".bias"):
        a = 0.05 * g.standard_normal(shape)
    elif name.endswith(("rel_pos_h", "rel_pos_w")):
        a = 0.1 * g.standard_normal(shape)
    elif name.endswith(("pos_embed", "query_768.weight", "query_1024.weight", "view_seperator")):
        a = 0.5 * g.standard_normal(shape)
    else:
        a = g.standard_normal(shape) / math.sqrt(int(np.prod(shape[1:])))
    return rc.bf16_round(a.astype(np.float32))


def synth_weights(sam_cfg, vcf_cfg, seed=0, **kw):
    """seeded float32 weights on the bf16 grid (a bf16 checkpoint widened), under the checkpoint's full names"""
    g = np.random.default_rng(seed)
    return {name: synth_tensor(g, name, shape) for name, shape in weight_shapes(sam_cfg, vcf_cfg, **kw).items()}


def synth_attention_inputs(seed, grid, heads, table_rows=None, images=1, extra=8, q_gain=1.0):
    """what the attention tests feed the kernel: qkv [images * gh * gw, 3 * heads * 64 + extra] ~ N(0, 1) (q times q_gain), the two
    tables scaled as synth_tensor scales them (table_rows rows each; default the exact 2 g - 1), and a padded token's row ~ N(0, 1)"""
    gh, gw = grid
    g = np.random.default_rng(seed)
    d = heads * 64
    qkv = g.standard_normal((images * gh * gw, 3 * d + extra)).astype(np.float32)
    qkv[:, :d] *= np.float32(q_gain)
    th = synth_tensor(g, "attn.rel_pos_h", (table_rows or 2 * gh - 1, 64))
    tw = synth_tensor(g, "attn.rel_pos_w", (table_rows or 2 * gw - 1, 64))
    pad = g.standard_normal(3 * d).astype(np.float32)
    return qkv, th, tw, pad


def synth_images(n, size, seed):
    """float32 images in [-1, 1]"""
    return (np.random.default_rng(seed).random((n, size, size, 3), dtype=np.float32) * np.float32(2) - np.float32(1))
