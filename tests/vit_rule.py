"""Host rule the Moxin-VLM vision tests hold the device to: the two towers and the projector in numpy float64, written from
moxin-vlm-mlx/src/vision.rs (ViTEncoder::forward :259-310, ViTBlock :216-230, ViTAttention :97-130), projector.rs:34-40 and
lib.rs:299-328 / 427-440.  The prompt-pass reference is qwen3_asr_rule.forward_from_rows / generate_from_rows."""
import math

import numpy as np

from oracle import ref_core as rc
from qwen3_asr_rule import gelu, _lin, _softmax

DINO = dict(embed_dim=1024, depth=24, num_heads=16, head_dim=64, intermediate_dim=4096, has_cls_token=True, num_registers=4,
            has_layer_scale=True, patch_size=14, image_size=224, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
SIGLIP = dict(embed_dim=1152, depth=27, num_heads=16, head_dim=72, intermediate_dim=4304, has_cls_token=False, num_registers=0,
              has_layer_scale=False, patch_size=14, image_size=224, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
# the tiny pair the device tests run end to end: image 56 (16 patches), 128 = 2 x 64 with CLS + 4 registers + LayerScale, 144 = 2 x 72 plain
TINY_DINO = dict(DINO, embed_dim=128, num_heads=2, head_dim=64, intermediate_dim=308, depth=4, image_size=56)
TINY_SIGLIP = dict(SIGLIP, embed_dim=144, num_heads=2, head_dim=72, intermediate_dim=308, depth=4, image_size=56)


def num_patches(cfg):
    return (cfg["image_size"] // cfg["patch_size"]) ** 2


def num_tokens(cfg):
    return (1 if cfg["has_cls_token"] else 0) + cfg["num_registers"] + num_patches(cfg)


def normalize(image, cfg):
    """normalize_dino / normalize_siglip (lib.rs:427-440): image [S, S, 3] in [0, 1]"""
    return (np.asarray(image, np.float64) - np.asarray(cfg["mean"], np.float64)) / np.asarray(cfg["std"], np.float64)


def patch_embed(x, w, b, patch):
    """nn::Conv2d, kernel = stride = patch, no padding, NHWC x [S, S, 3]; w is the CHECKPOINT's [O, I, P, P], read as [O, P, P, I]
    (vision.rs:386-387); -> [num_patches, O], patches in row-major order of the grid"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64).transpose(0, 2, 3, 1)
    S, G, O = x.shape[0], x.shape[0] // patch, w.shape[0]
    cols = x[:G * patch, :G * patch].reshape(G, patch, G, patch, 3).transpose(0, 2, 1, 3, 4).reshape(G * G, patch * patch * 3)
    y = cols @ w.reshape(O, -1).T
    return y if b is None else y + np.asarray(b, np.float64)


def assemble(patches, w, cfg):
    """vision.rs:268-295: pos_embed of num_patches rows is added BEFORE the CLS row is prepended, of num_patches + 1 rows AFTER;
    register rows go between CLS and the patches and get no position"""
    np_, d = patches.shape
    pos = np.asarray(w["pos_embed"], np.float64).reshape(-1, d)
    h = patches
    before = pos.shape[0] == np_
    if before:
        h = h + pos
    if cfg["has_cls_token"]:
        h = np.concatenate([np.asarray(w["cls_token"], np.float64).reshape(1, d), h], axis=0)
    if not before:
        assert pos.shape[0] == h.shape[0], "pos_embed rows are neither form"
        h = h + pos
    if cfg["num_registers"]:
        reg = np.asarray(w["reg_token"] if "reg_token" in w else w["register_tokens"], np.float64).reshape(cfg["num_registers"], d)
        h = np.concatenate([h[:1], reg, h[1:]], axis=0)
    return h


def layer_norm(x, w, b, eps=1e-6):
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)          # biased
    y = (x - mu) / np.sqrt(var + eps) * np.asarray(w, np.float64)
    return y if b is None else y + np.asarray(b, np.float64)


def attention(q, k, v, heads):
    """unmasked softmax(q k^T hd^-0.5) v per head; q / k / v [N, heads * hd] -> [N, heads * hd] token-major"""
    N = q.shape[0]
    qh, kh, vh = (np.asarray(a, np.float64).reshape(N, heads, -1).transpose(1, 0, 2) for a in (q, k, v))
    p = _softmax(qh @ kh.transpose(0, 2, 1) * qh.shape[-1] ** -0.5)
    return (p @ vh).transpose(1, 0, 2).reshape(N, -1)


def _gamma(w, p):
    return np.asarray(w[p + "gamma"] if p + "gamma" in w else w[p + "scale_factor"], np.float64)


def block(x, w, p, cfg, stages=None):
    """ViTBlock::forward (vision.rs:216-230): h = x + ls1 * attn(LN1(x)); out = h + ls2 * fc2(gelu(fc1(LN2(h))))"""
    d = x.shape[1]
    st = {} if stages is None else stages
    st["ln1"] = layer_norm(x, w[p + "norm1.weight"], w.get(p + "norm1.bias"))
    st["qkv"] = _lin(st["ln1"], w[p + "attn.qkv.weight"], w.get(p + "attn.qkv.bias"))
    st["attn"] = attention(st["qkv"][:, :d], st["qkv"][:, d:2 * d], st["qkv"][:, 2 * d:], cfg["num_heads"])
    a = _lin(st["attn"], w[p + "attn.proj.weight"], w.get(p + "attn.proj.bias"))
    if cfg["has_layer_scale"]:
        a = a * _gamma(w, p + "ls1.")
    st["h"] = x + a
    st["ln2"] = layer_norm(st["h"], w[p + "norm2.weight"], w.get(p + "norm2.bias"))
    st["mlp"] = gelu(_lin(st["ln2"], w[p + "mlp.fc1.weight"], w.get(p + "mlp.fc1.bias")))
    m = _lin(st["mlp"], w[p + "mlp.fc2.weight"], w.get(p + "mlp.fc2.bias"))
    if cfg["has_layer_scale"]:
        m = m * _gamma(w, p + "ls2.")
    return st["h"] + m


def tower(image, w, cfg):
    """ViTEncoder::forward (vision.rs:259-310) on image [S, S, 3] in [0, 1].  Blocks 0 .. depth - 2 run; the final norm is not applied;
    CLS and register rows are dropped.  Returns every stage: col (normalised patches as rows), patches, tokens (assembled), the last
    block's ln1 / qkv / attn / h (after the attention residual) / ln2 / mlp, and out [num_patches, embed_dim]."""
    P = cfg["patch_size"]
    x = normalize(image, cfg)
    G = x.shape[0] // P
    st = {"col": x.reshape(G, P, G, P, 3).transpose(0, 2, 1, 3, 4).reshape(G * G, P * P * 3)}
    st["patches"] = patch_embed(x, w["patch_embed.proj.weight"], w.get("patch_embed.proj.bias"), P)
    st["tokens"] = h = assemble(st["patches"], w, cfg)
    for l in range(cfg["depth"] - 1):
        h = block(h, w, f"blocks.{l}.", cfg, st)
    skip = (1 + cfg["num_registers"]) if cfg["has_cls_token"] else 0
    st["out"] = h[skip:]
    return st


def projector(x, w):
    """FusedMLPProjector::forward (projector.rs:34-40)"""
    h = gelu(_lin(x, w["fc1.weight"], w.get("fc1.bias")))
    h = gelu(_lin(h, w["fc2.weight"], w.get("fc2.bias")))
    return _lin(h, w["fc3.weight"], w.get("fc3.bias"))


def visual_rows(image, dino_w, dino_cfg, sig_w, sig_cfg, proj_w):
    """lib.rs:306-313: the two towers' rows side by side, through the projector"""
    fused = np.concatenate([tower(image, dino_w, dino_cfg)["out"], tower(image, sig_w, sig_cfg)["out"]], axis=1)
    return projector(fused, proj_w)


def weight_shapes(cfg, pos_with_cls=None, conv_bias=True, blocks=None):
    """the keys behind a tower's prefix and their checkpoint shapes (vision.rs:380-557).  pos_with_cls: pos_embed has num_patches + 1 rows
    (default: when the tower has a CLS row); blocks: how many blocks get weights (default depth - 1, the ones that run)."""
    d, ffn, P = cfg["embed_dim"], cfg["intermediate_dim"], cfg["patch_size"]
    if pos_with_cls is None:
        pos_with_cls = bool(cfg["has_cls_token"])
    s = {"patch_embed.proj.weight": (d, 3, P, P), "pos_embed": (1, num_patches(cfg) + (1 if pos_with_cls else 0), d),
         "norm.weight": (d,), "norm.bias": (d,)}
    if conv_bias:
        s["patch_embed.proj.bias"] = (d,)
    if cfg["has_cls_token"]:
        s["cls_token"] = (1, 1, d)
    if cfg["num_registers"]:
        s["reg_token"] = (1, cfg["num_registers"], d)
    for l in range(cfg["depth"] - 1 if blocks is None else blocks):
        p = f"blocks.{l}."
        s[p + "norm1.weight"] = s[p + "norm1.bias"] = s[p + "norm2.weight"] = s[p + "norm2.bias"] = (d,)
        s[p + "attn.qkv.weight"], s[p + "attn.qkv.bias"] = (3 * d, d), (3 * d,)
        s[p + "attn.proj.weight"], s[p + "attn.proj.bias"] = (d, d), (d,)
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"], s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (ffn, d), (ffn,), (d, ffn), (d,)
        if cfg["has_layer_scale"]:
            s[p + "ls1.gamma"] = s[p + "ls2.gamma"] = (d,)
    return s


def synth_weights(cfg, seed=0, **kw):
    """seeded float32 weights on the bf16 grid (a bf16 checkpoint widened): matrices ~ N(0, 1 / fan_in), norm weights 1 + noise, LayerScale
    factors around 0.5, tokens and positions ~ N(0, 0.5^2)"""
    g = np.random.default_rng(seed)
    out = {}
    for name, shape in weight_shapes(cfg, **kw).items():
        if name.endswith(("norm1.weight", "norm2.weight", "norm.weight")):
            a = 1.0 + 0.05 * g.standard_normal(shape)
        elif name.endswith(".gamma"):
            a = 0.5 + 0.1 * g.standard_normal(shape)
        elif name.endswith(".bias"):
            a = 0.05 * g.standard_normal(shape)
        elif name in ("pos_embed", "cls_token", "reg_token"):
            a = 0.5 * g.standard_normal(shape)
        else:
            a = g.standard_normal(shape) / math.sqrt(int(np.prod(shape[1:])))
        out[name] = rc.bf16_round(a.astype(np.float32))
    return out


def projector_synth_weights(widths, seed=0):
    """widths (in, h1, h2, out) -> fc1 / fc2 / fc3 weights and biases"""
    g = np.random.default_rng(seed)
    out = {}
    for i in range(3):
        out[f"fc{i + 1}.weight"] = rc.bf16_round((g.standard_normal((widths[i + 1], widths[i])) / math.sqrt(widths[i])).astype(np.float32))
        out[f"fc{i + 1}.bias"] = rc.bf16_round((0.05 * g.standard_normal(widths[i + 1])).astype(np.float32))
    return out


def synth_image(size, seed):
    """a float32 image in [0, 1]"""
    return np.random.default_rng(seed).random((size, size, 3), dtype=np.float32)
