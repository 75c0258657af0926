"""Mixed-precision MLX checkpoints for the tests: per-matrix (bits, group_size) tables, the checkpoint they describe and its exact
reference.  The frozen oracle runs ONE format per model, so a mixed table is held to its 8-bit re-pack at the table's smallest group:
every matrix keeps its codes (they fit in 8 bits) and its bf16 scales / biases, the codes are packed at 8 bits and each scale / bias
is repeated group / g_min times -- the same dequantised values element for element, so Qwen3Oracle(cfg, w8, quant=(8, g_min)) is
exact for the mixed model."""
import numpy as np

from oracle import ref_qwen3 as rq
from test_gpu_quant_widths import _triplet, pack_bits

KINDS = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
         "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}


def table_a(cfg):
    """base (4, 64); v_proj and down_proj of the first and the last layer, and an untied lm_head, at (6, 64)"""
    t = {}
    for i in (0, cfg.num_hidden_layers - 1):
        t[f"model.layers.{i}.self_attn.v_proj"] = (6, 64)
        t[f"model.layers.{i}.mlp.down_proj"] = (6, 64)
    if not cfg.tie_word_embeddings:
        t["lm_head"] = (6, 64)
    return (4, 64), t


def table_b(cfg):
    """every kind different: base (3, 64), q (4, 64), k (8, 32), v (6, 128), o (5, 64), gate / up (2, 64), down (8, 64), embed (8, 64)"""
    per_kind = {"q": (4, 64), "k": (8, 32), "v": (6, 128), "o": (5, 64), "gate": (2, 64), "up": (2, 64), "down": (8, 64)}
    t = {f"model.layers.{i}.{KINDS[k]}": f for i in range(cfg.num_hidden_layers) for k, f in per_kind.items()}
    t["model.embed_tokens"] = (8, 64)
    return (3, 64), t


def quantization(base, table):
    """the config.json "quantization" block of a table"""
    q = {"bits": base[0], "group_size": base[1]}
    q.update({p: {"bits": b, "group_size": g} for p, (b, g) in table.items()})
    return q


def checkpoints(cfg, base, table):
    """(the mixed checkpoint, its 8-bit re-pack at g_min, g_min)"""
    g_min = min([base[1]] + [g for _, g in table.values()])
    wm, w8 = {}, {}
    for name, w in rq.synth_weights(cfg).items():
        prefix = name[:-len(".weight")]
        if prefix.endswith(rq.QUANTIZED) or prefix in ("model.embed_tokens", "lm_head"):
            bits, group = table.get(prefix, base)
            q, s, b = _triplet(w, group, bits)
            wm[prefix + ".weight"], wm[prefix + ".scales"], wm[prefix + ".biases"] = pack_bits(q, bits), s, b
            rep = group // g_min
            w8[prefix + ".weight"] = pack_bits(q, 8)
            w8[prefix + ".scales"], w8[prefix + ".biases"] = np.repeat(s, rep, axis=-1), np.repeat(b, rep, axis=-1)
        else:
            wm[name] = w8[name] = w
    return wm, w8, g_min


def oracle_of(cfg, w8, g_min):
    return rq.Qwen3Oracle(cfg, w8, quant=(8, g_min))
