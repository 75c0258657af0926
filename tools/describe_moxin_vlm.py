#!/usr/bin/env python3
"""Describe an image with a Moxin-VLM checkpoint, or (--synthetic) time the device stages at the real shapes with synthetic weights.

    python tools/describe_moxin_vlm.py <model_dir> image.npy|image.ppm "prompt" [--quantize 4|8] [--max-tokens 256] [--temp 0]
    python tools/describe_moxin_vlm.py --synthetic [--tokens 64]

The image is a [224, 224, 3] array: an .npy file (uint8, or float in [0, 1]) or a binary .ppm (P6) of exactly that size.  Any other
format is opened with PIL when PIL can be imported and resized to 224 x 224 with PIL's BICUBIC filter -- which is NOT the `image`
crate's CatmullRom filter the reference's example resizes with (examples/generate.rs:48): the pixels, and with them the rows, differ
slightly from the reference's for such files.  Hand over a 224 x 224 array to compare like with like.

--synthetic:

DINOv2 ViT-L/14 (23 of 24 blocks, 1024 / 16 x 64 / 4096, 261 rows) and SigLIP SO400M/14 (26 of 27 blocks, 1152 / 16 x 72 / 4304, 256 rows),
the projector 2176 -> 8704 -> 4096 -> 4096, and a Mistral-7B-shaped decoder (36 layers, hidden 4096, 32 / 8 heads of 128, intermediate
14336, vocabulary 32064) in bf16 and in 4-bit group 64, all with synthetic weights: the tokens mean nothing and the times are real.
Towers and projector: device events on the stream they run on, median of three runs after a warm-up; prompt pass and decode steps: the
engine's own device events.  Prints the launch count of the towers and the projector (split-K reduce launches not counted).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import omx_import  # noqa: E402

omx = omx_import.load_package()
from ominix_mlx_amd import engine, moxin_vlm, vision  # noqa: E402

DINO = dict(embed_dim=1024, depth=24, num_heads=16, head_dim=64, intermediate_dim=4096, has_cls_token=True, num_registers=4, has_layer_scale=True)
SIGLIP = dict(embed_dim=1152, depth=27, num_heads=16, head_dim=72, intermediate_dim=4304, has_cls_token=False, num_registers=0, has_layer_scale=False)


def read_image(path):
    if path.endswith(".npy"):
        return np.load(path)
    if path.endswith(".ppm"):
        with open(path, "rb") as f:
            data = f.read()
        fields, pos = [], 0
        while len(fields) < 4:                          # magic, width, height, maxval; '#' comments run to the end of the line
            while data[pos:pos + 1].isspace():
                pos += 1
            if data[pos:pos + 1] == b"#":
                pos = data.index(b"\n", pos) + 1
                continue
            end = pos
            while not data[end:end + 1].isspace():
                end += 1
            fields.append(data[pos:end])
            pos = end
        if fields[0] != b"P6" or int(fields[3]) != 255:
            raise SystemExit(f"{path}: a binary PPM (P6) with maxval 255 is expected")
        w, h = int(fields[1]), int(fields[2])
        return np.frombuffer(data, np.uint8, w * h * 3, pos + 1).reshape(h, w, 3)
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit(f"{path}: only .npy and .ppm are read without PIL")
    return np.asarray(Image.open(path).convert("RGB").resize((224, 224), Image.BICUBIC))


def tower_weights(cfg, seed):
    g = np.random.default_rng(seed)
    d, ffn, np_ = cfg["embed_dim"], cfg["intermediate_dim"], 256
    rnd = lambda shape, fan: (g.standard_normal(shape, dtype=np.float32) / np.float32(np.sqrt(fan)))
    w = {"patch_embed.proj.weight": rnd((d, 3, 14, 14), 588), "patch_embed.proj.bias": np.zeros(d, np.float32),
         "pos_embed": rnd((1, np_ + (1 if cfg["has_cls_token"] else 0), d), 4.0)}
    if cfg["has_cls_token"]:
        w["cls_token"] = rnd((1, 1, d), 4.0)
    if cfg["num_registers"]:
        w["reg_token"] = rnd((1, cfg["num_registers"], d), 4.0)
    for l in range(cfg["depth"] - 1):
        p = f"blocks.{l}."
        for n in ("norm1", "norm2"):
            w[p + n + ".weight"], w[p + n + ".bias"] = np.ones(d, np.float32), np.zeros(d, np.float32)
        w[p + "attn.qkv.weight"], w[p + "attn.qkv.bias"] = rnd((3 * d, d), d), np.zeros(3 * d, np.float32)
        w[p + "attn.proj.weight"], w[p + "attn.proj.bias"] = rnd((d, d), d), np.zeros(d, np.float32)
        w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"] = rnd((ffn, d), d), np.zeros(ffn, np.float32)
        w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"] = rnd((d, ffn), ffn), np.zeros(d, np.float32)
        if cfg["has_layer_scale"]:
            w[p + "ls1.gamma"] = w[p + "ls2.gamma"] = np.full(d, 0.5, np.float32)
    return w


def event_ms(fn, reps=3):
    """median device time of fn over `reps` runs after one warm-up: events on the null stream, the one the towers run on"""
    import torch
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return r, float(np.median(ts))


def synthetic(tokens):
    g = np.random.default_rng(0)
    dino, siglip, proj = vision.ViTEncoder.dinov2_large(), vision.ViTEncoder.siglip_so400m(), vision.Projector()
    dino.load_weights(tower_weights(DINO, 1))
    siglip.load_weights(tower_weights(SIGLIP, 2))
    widths = (2176, 8704, 4096, 4096)
    proj.load_weights({f"fc{i + 1}.weight": (g.standard_normal((widths[i + 1], widths[i]), dtype=np.float32) / np.float32(np.sqrt(widths[i])))
                       for i in range(3)})
    img = omx.ops.Tensor.from_numpy(g.random((224, 224, 3), dtype=np.float32), "f32")
    fused = omx.ops.Tensor((256, 2176), "f32")
    _, dino_ms = event_ms(lambda: dino.forward(img, out=fused, column=0))
    _, sig_ms = event_ms(lambda: siglip.forward(img, out=fused, column=1024))
    rows, proj_ms = event_ms(lambda: proj.forward(fused))
    flop = 0.0
    for c, T in ((DINO, 261), (SIGLIP, 256)):
        d, ffn = c["embed_dim"], c["intermediate_dim"]
        flop += 2.0 * 256 * 588 * d + (c["depth"] - 1) * (2.0 * T * d * (4 * d + 2 * ffn) + 4.0 * T * T * d)
    pflop = 2.0 * 256 * (2176 * 8704 + 8704 * 4096 + 4096 * 4096)
    print(f"towers + projector: {(flop + pflop) / 1e12:.3f} TFLOP float32 (computed from the shapes)")
    print(f"  DINOv2 ViT-L/14    median {dino_ms:8.3f} ms   {dino.launches()} launches   device events, 3 runs after a warm-up")
    print(f"  SigLIP SO400M/14   median {sig_ms:8.3f} ms   {siglip.launches()} launches")
    print(f"  projector          median {proj_ms:8.3f} ms   3 launches")
    print(f"  towers + projector {dino_ms + sig_ms + proj_ms:8.3f} ms   {dino.launches() + siglip.launches() + 3} launches "
          f"= {(flop + pflop) / 1e9 / (dino_ms + sig_ms + proj_ms):.1f} TFLOP/s")
    V = 32064
    ids = np.concatenate([[1], np.full(256, 32000), (np.arange(12) * 7919 + 13) % 32000]).astype(np.uint32)
    for quant in (None, {"bits": 4, "group_size": 64}):
        m = engine.Model(**dict(moxin_vlm.text_model_args({}), max_context=1024, quantization=quant))
        m.synth_weights()
        pf, dec = [], []
        for i in range(4):
            m.reset()
            m.prefill(ids, embeds=rows, embeds_at=1)
            m.decode(tokens)
            if i >= 1:
                pf.append(m.last_prefill_ms())
                dec.append(m.last_decode_ms() / tokens)
        print(f"  decoder {'4-bit' if quant else 'bf16 '}: prompt pass over {ids.size} rows median {np.median(pf):8.3f} ms, per token median {np.median(dec):7.4f} ms "
              f"over {tokens} steps   device events, 3 runs after a warm-up")
        m.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_dir", nargs="?")
    ap.add_argument("image", nargs="?")
    ap.add_argument("prompt", nargs="?", default="Describe this image.")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--quantize", type=int, default=0, choices=(0, 4, 8))
    ap.add_argument("--max-tokens", type=int, default=256)
    ap.add_argument("--temp", type=float, default=0.0)
    ap.add_argument("--tokens", type=int, default=64, help="--synthetic: decode steps per timed run")
    a = ap.parse_args()
    if a.synthetic:
        return synthetic(a.tokens)
    if not (a.model_dir and a.image):
        ap.error('give <model_dir> <image> "prompt", or --synthetic')
    vlm = moxin_vlm.MoxinVLM.load(a.model_dir, quantize=a.quantize)
    print(vlm.describe(read_image(a.image), a.prompt, a.max_tokens, a.temp))
    t = vlm.last_times
    print(f"towers {t['towers_ms']:.1f} ms, projector {t['projector_ms']:.1f} ms ({t['launches']} launches), prompt pass over {t['prompt_rows']} rows "
          f"{t['prompt_pass_ms']:.2f} ms, {t['tokens']} tokens at {t['per_token_ms']:.2f} ms", file=sys.stderr)


if __name__ == "__main__":
    main()
