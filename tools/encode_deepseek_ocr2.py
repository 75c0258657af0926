#!/usr/bin/env python3
"""Encode views with a DeepSeek-OCR-2 checkpoint's vision side, or (--synthetic) time the device stages at the real shapes.

    python tools/encode_deepseek_ocr2.py <model_dir> global.npy [--crops crops.npy] [--out rows.npy]
    python tools/encode_deepseek_ocr2.py --synthetic

global.npy is the [1024, 1024, 3] global view, crops.npy the [n, 768, 768, 3] crops (n <= 6): float in [-1, 1], or uint8 (mapped by
v / 127.5 - 1).  Resizing and cropping are the caller's (deepseek_ocr2.find_best_crop_ratio gives the crop grid).  The rows written are
`encode_image`'s: the crops' rows in the order given, the global view's, the separator -- [n, 1280] float32.

--synthetic:

The SAM ViT-B tower (12 blocks, 768 / 12 x 64 / 3072, window 14, blocks 2 / 5 / 8 / 11 global, neck 256 / 512 / 896), the
visual-causal-flow encoder (24 layers, 896 / 14 / 2 / 4864) and the projector 896 -> 1280 with synthetic weights: the rows mean nothing
and the times are real.  Device events on the stream the towers run on, median of three timed windows after a warm-up (the protocol of
tools/describe_moxin_vlm.py --synthetic); the attention kernels alone: ten calls per window.  Prints launch counts (split-K reduce
launches not counted), scratch bytes and achieved TFLOP/s computed from the shapes.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import  # noqa: E402

omx = omx_import.load_package()
from ominix_mlx_amd import deepseek_ocr2 as ds, vision  # noqa: E402

SAM, VCF = ds.SAM_DEFAULTS, ds.VCF_DEFAULTS


def event_ms(fn, reps=3, inner=1):
    """median device time of one call of fn over `reps` windows of `inner` calls after one warm-up: events on the null stream"""
    import torch
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return r, float(np.median(ts))


def synthetic_weights(seed=0):
    """real shapes; one random tensor per distinct shape, shared by the blocks (the times do not depend on the values)"""
    g = np.random.default_rng(seed)
    cache = {}

    def rnd(shape, fan):
        if (shape, fan) not in cache:
            cache[(shape, fan)] = g.standard_normal(shape, dtype=np.float32) / np.float32(np.sqrt(fan))
        return cache[(shape, fan)]

    d, ffn, h, I = SAM["embed_dim"], SAM["mlp_dim"], VCF["hidden"], VCF["intermediate"]
    s = {"patch_embed.proj.weight": rnd((d, 3, 16, 16), 768), "patch_embed.proj.bias": np.zeros(d, np.float32), "pos_embed": rnd((1, 64, 64, d), 4.0),
         "neck.0.weight": rnd((256, d, 1, 1), d), "neck.1.weight": np.ones(256, np.float32), "neck.1.bias": np.zeros(256, np.float32),
         "neck.2.weight": rnd((256, 256, 3, 3), 2304), "neck.3.weight": np.ones(256, np.float32), "neck.3.bias": np.zeros(256, np.float32),
         "net_2.weight": rnd((512, 256, 3, 3), 2304), "net_3.weight": rnd((896, 512, 3, 3), 4608)}
    for l in range(SAM["depth"]):
        p = f"blocks.{l}."
        rel = 127 if l in SAM["global_attn_indexes"] else 27
        for n in ("norm1", "norm2"):
            s[p + n + ".weight"], s[p + n + ".bias"] = np.ones(d, np.float32), np.zeros(d, np.float32)
        s[p + "attn.qkv.weight"], s[p + "attn.qkv.bias"] = rnd((3 * d, d), d), rnd((3 * d,), 400.0)
        s[p + "attn.rel_pos_h"], s[p + "attn.rel_pos_w"] = rnd((rel, 64), 100.0), rnd((rel, 64), 100.0)
        s[p + "attn.proj.weight"], s[p + "attn.proj.bias"] = rnd((d, d), d), np.zeros(d, np.float32)
        s[p + "mlp.lin1.weight"], s[p + "mlp.lin1.bias"] = rnd((ffn, d), d), np.zeros(ffn, np.float32)
        s[p + "mlp.lin2.weight"], s[p + "mlp.lin2.bias"] = rnd((d, ffn), ffn), np.zeros(d, np.float32)
    w = {ds.SAM_PREFIX + "." + k: v for k, v in s.items()}
    q = {"model.model.norm.weight": np.ones(h, np.float32), "query_768.weight": rnd((144, h), 4.0), "query_1024.weight": rnd((256, h), 4.0)}
    for l in range(VCF["layers"]):
        p = f"model.model.layers.{l}."
        q[p + "input_layernorm.weight"] = q[p + "post_attention_layernorm.weight"] = np.ones(h, np.float32)
        q[p + "self_attn.q_proj.weight"], q[p + "self_attn.q_proj.bias"] = rnd((h, h), h), np.zeros(h, np.float32)
        for n in ("k_proj", "v_proj"):
            q[p + f"self_attn.{n}.weight"], q[p + f"self_attn.{n}.bias"] = rnd((128, h), h), np.zeros(128, np.float32)
        q[p + "self_attn.o_proj.weight"] = rnd((h, h), h)
        q[p + "mlp.gate_proj.weight"] = q[p + "mlp.up_proj.weight"] = rnd((I, h), h)
        q[p + "mlp.down_proj.weight"] = rnd((h, I), I)
    w.update({ds.VCF_PREFIX + "." + k: v for k, v in q.items()})
    w[ds.PROJECTOR_WEIGHT], w[ds.PROJECTOR_BIAS], w[ds.SEPARATOR] = rnd((1280, h), h), np.zeros(1280, np.float32), rnd((1280,), 4.0)
    return w


def sam_flop(G, images):
    """floating-point operations of the SAM tower on `images` images of a G x G grid, from the shapes"""
    d, ffn, N, win = SAM["embed_dim"], SAM["mlp_dim"], G * G, SAM["window"]
    nwin = ((G + win - 1) // win) ** 2
    f = 2.0 * N * 768 * d
    for l in range(SAM["depth"]):
        f += 2.0 * N * d * (4 * d + 2 * ffn)
        f += 4.0 * N * N * d if l in SAM["global_attn_indexes"] else 4.0 * nwin * (win * win) ** 2 * d
    f += 2.0 * N * d * 256 + 2.0 * N * 2304 * 256 + 2.0 * (N / 4) * 2304 * 512 + 2.0 * (N / 16) * 4608 * 896
    return images * f


def vcf_flop(n_img, n_query, images):
    d, I, NQ, L = VCF["hidden"], VCF["intermediate"], (VCF["heads"] + 2 * VCF["kv_heads"]) * 64, n_img + n_query
    seen = n_img * n_img + sum(n_img + i + 1 for i in range(n_query))
    return images * VCF["layers"] * (2.0 * L * d * (NQ + d + 3 * I) + 4.0 * seen * d)


def synthetic():
    from ominix_mlx_amd import ops
    g = np.random.default_rng(1)
    enc = ds.DeepEncoder.from_weights(synthetic_weights())
    T = lambda a: ops.Tensor.from_numpy(a, "f32")
    view = T(g.random((1, 1024, 1024, 3), dtype=np.float32) * 2 - 1)
    crops = T(g.random((6, 768, 768, 3), dtype=np.float32) * 2 - 1)
    one = [T(g.random((1, 768, 768, 3), dtype=np.float32) * 2 - 1) for _ in range(6)]
    print("DeepSeek-OCR-2 vision side, real shapes, synthetic weights; device events, median of 3 windows after a warm-up")
    feat_v, ms = event_ms(lambda: enc.sam.forward(view))
    print(f"  SAM, one 1024 px view      median {ms:8.3f} ms   {enc.sam.launches()} launches   scratch {enc.sam.scratch_bytes() / 2 ** 20:7.1f} MiB   "
          f"{sam_flop(64, 1) / 1e9 / ms:6.1f} TFLOP/s of {sam_flop(64, 1) / 1e12:.3f} TFLOP")
    _, ms1 = event_ms(lambda: [enc.sam.forward(t) for t in one])
    feat_c, ms6 = event_ms(lambda: enc.sam.forward(crops))
    print(f"  SAM, six 768 px crops      stacked median {ms6:8.3f} ms ({enc.sam.launches()} launches, scratch {enc.sam.scratch_bytes() / 2 ** 20:7.1f} MiB, "
          f"{sam_flop(48, 6) / 1e9 / ms6:6.1f} TFLOP/s of {sam_flop(48, 6) / 1e12:.3f} TFLOP)   one at a time median {ms1:8.3f} ms")
    rows_v, ms = event_ms(lambda: enc.vcf.forward(feat_v, images=1))
    print(f"  encoder, the view (256 + 256 rows)    median {ms:8.3f} ms   {enc.vcf.launches()} launches   scratch {enc.vcf.scratch_bytes() / 2 ** 20:7.1f} MiB   "
          f"{vcf_flop(256, 256, 1) / 1e9 / ms:6.1f} TFLOP/s")
    rows_c, ms = event_ms(lambda: enc.vcf.forward(feat_c, images=6))
    print(f"  encoder, six crops (6 x (144 + 144))  median {ms:8.3f} ms   {enc.vcf.launches()} launches   scratch {enc.vcf.scratch_bytes() / 2 ** 20:7.1f} MiB   "
          f"{vcf_flop(144, 144, 6) / 1e9 / ms:6.1f} TFLOP/s")
    rows = T(np.zeros((6 * 144 + 256, 896), np.float32))
    _, ms = event_ms(lambda: vision.gemm_f32(rows, enc.proj_w, enc.proj_b), inner=10)
    print(f"  projector, 1120 rows                  median {ms:8.3f} ms   1 launch   {2.0 * 1120 * 896 * 1280 / 1e9 / ms:6.1f} TFLOP/s")
    _, ms = event_ms(lambda: enc.encode_image(view.numpy()[0], crops.numpy()))
    print(f"  encode_image, view + six crops, host arrays in, rows on the device: median {ms:8.3f} ms")
    # ---- the global-attention kernel alone ----
    for G in (48, 64):
        N = G * G
        qkv = T(g.standard_normal((N, 3 * 768), dtype=np.float32))
        th, tw = T(0.1 * g.standard_normal((127, 64), dtype=np.float32)), T(0.1 * g.standard_normal((127, 64), dtype=np.float32))
        _, ms = event_ms(lambda: vision.sam_attention_f32(qkv, 12, (G, G), 0, th, tw), inner=10)
        print(f"  global attention alone, {N} keys x 12 heads: median {ms:8.3f} ms   {4.0 * N * N * 768 / 1e9 / ms:6.1f} TFLOP/s")
    qkv = T(g.standard_normal((1024, 3 * 768), dtype=np.float32))
    zero = T(np.zeros((63, 64), np.float32))
    _, ms_new = event_ms(lambda: vision.sam_attention_f32(qkv, 12, (32, 32), 0, zero, zero), inner=10)
    _, ms_old = event_ms(lambda: vision.attention_f32(qkv, 12, 64), inner=10)
    print(f"  1024 keys x 12 heads of 64: the streaming kernel (zero tables) median {ms_new:8.3f} ms, the score-in-LDS kernel "
          f"(omx_vit_attention_f32) median {ms_old:8.3f} ms")
    enc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model_dir", nargs="?")
    ap.add_argument("global_view", nargs="?")
    ap.add_argument("--crops")
    ap.add_argument("--out", default="deepseek_ocr2_rows.npy")
    ap.add_argument("--synthetic", action="store_true")
    a = ap.parse_args()
    if a.synthetic:
        return synthetic()
    if not (a.model_dir and a.global_view):
        ap.error("give <model_dir> global.npy [--crops crops.npy], or --synthetic")
    enc = ds.DeepEncoder.load(a.model_dir)
    rows = enc.encode_image(np.load(a.global_view), np.load(a.crops) if a.crops else None).numpy()
    np.save(a.out, rows)
    print(f"{rows.shape[0]} rows of {rows.shape[1]} -> {a.out}   ({enc.launches()} launches for the last view)")
    enc.close()


if __name__ == "__main__":
    main()
