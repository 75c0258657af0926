"""The Moxin-VLM vision towers and projector on the device (csrc/vit_encoder.hip; vision.ViTEncoder, vision.Projector,
vision.attention_f32, vision.gemm_f32) against their numpy float64 restatement (tests/vit_rule.py, written from
moxin-vlm-mlx/src/vision.rs and projector.rs).

Tolerance: the project's float32 rule -- error <= 1e-4 x the largest magnitude of the float64 result (TOL["f32"] of
tests/test_gpu_paraformer.py, TOL of tests/test_gpu_qwen3_asr.py) -- at every stage read.  Each test prints its measured worst ratio."""
import functools

import numpy as np
import pytest

import vit_rule as rule

pytestmark = pytest.mark.gpu

TOL = 1e-4

TINY_DINO, TINY_SIGLIP = rule.TINY_DINO, rule.TINY_SIGLIP
PROJ = (272, 544, 256, 256)


def _ratio(got, ref, what):
    r = np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max()
    print(f"{what}: worst error / largest magnitude = {r:.3e}")
    return r


def _tower(cfg, w, **kw):
    from ominix_mlx_amd import vision
    e = vision.ViTEncoder(**dict(cfg, **kw))
    e.load_weights(w)
    return e


@pytest.mark.parametrize("width", [64, 72])
@pytest.mark.parametrize("heads", [2, 16])
def test_attention_against_the_rule(omx, heads, width):
    """The attention kernel alone: one row, a tile short of / exactly / one past 16 and 64 rows, more than one block, the towers' own 256
    and 261, and 257; q | k | v read in place from a stacked projection whose rows are 8 floats longer than 3 * dim."""
    from ominix_mlx_amd import ops, vision
    d = heads * width
    ld = 3 * d + 8
    for n in (1, 15, 16, 17, 63, 64, 65, 256, 257, 261):
        g = np.random.default_rng(1000 * heads + 10 * width + n)
        qkv = g.standard_normal((n, ld)).astype(np.float32)
        q, k, v = (qkv[:, i * d:(i + 1) * d].astype(np.float64) for i in range(3))
        got = vision.attention_f32(ops.Tensor.from_numpy(qkv, "f32"), heads, width).numpy()
        assert got.shape == (n, d)
        assert _ratio(got, rule.attention(q, k, v, heads), f"attention width {width} heads {heads} N {n}") <= TOL


def test_attention_gives_the_same_bits_twice_and_takes_its_largest_size(omx):
    from ominix_mlx_amd import ops, vision
    qkv = np.random.default_rng(3).standard_normal((1024, 3 * 72)).astype(np.float32)
    t = ops.Tensor.from_numpy(qkv, "f32")
    a, b = vision.attention_f32(t, 1, 72).numpy(), vision.attention_f32(t, 1, 72).numpy()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    q, k, v = (qkv[:, i * 72:(i + 1) * 72].astype(np.float64) for i in range(3))
    assert _ratio(a, rule.attention(q, k, v, 1), "attention width 72 N 1024") <= TOL


@pytest.mark.parametrize("base,cls,reg,pos_with_cls,conv_bias", [
    ("dino", True, 4, True, True), ("dino", True, 4, False, False), ("dino", True, 0, True, False), ("dino", False, 0, False, True),
    ("siglip", False, 0, False, True), ("siglip", True, 0, False, False), ("siglip", True, 2, True, True)])
def test_patch_embedding_and_assembly_at_the_real_widths(omx, base, cls, reg, pos_with_cls, conv_bias):
    """depth 1: no block runs.  Both pos_embed forms, with and without CLS / registers, with and without a convolution bias, at both towers'
    widths and image statistics: the normalised patches, the convolution, the assembled rows and what comes out."""
    cfg = dict(rule.DINO if base == "dino" else rule.SIGLIP, depth=1, has_cls_token=cls, num_registers=reg)
    w = rule.synth_weights(cfg, seed=11 + reg, pos_with_cls=pos_with_cls, conv_bias=conv_bias)
    img = rule.synth_image(224, 7)
    st = rule.tower(img, w, cfg)
    e = _tower(cfg, w)
    out = e.forward(img).numpy()
    what = f"{base} cls {cls} reg {reg} pos+cls {pos_with_cls} bias {conv_bias}"
    assert e.tokens() == st["tokens"].shape[0] == rule.num_tokens(cfg) and e.rows() == 256 and out.shape == st["out"].shape
    assert _ratio(e.debug_read("col", st["col"].shape), st["col"], what + " normalised patches") <= TOL
    assert _ratio(e.debug_read("patches", st["patches"].shape), st["patches"], what + " convolution") <= TOL
    assert _ratio(e.debug_read("h", st["tokens"].shape), st["tokens"], what + " assembled rows") <= TOL
    assert _ratio(out, st["out"], what + " rows out") <= TOL
    e.close()


@pytest.mark.parametrize("base", ["dino", "siglip"])
def test_one_block_at_the_real_width(omx, base):
    """depth 2 on the real 224 x 224 image: one block at 1024 / 16 x 64 / 4096 with LayerScale over 261 rows, and at 1152 / 16 x 72 / 4304
    without over 256 (4304 is no multiple of 64, as N of fc1 and as K of fc2).  Every stage of the block."""
    cfg = dict(rule.DINO if base == "dino" else rule.SIGLIP, depth=2)
    w = rule.synth_weights(cfg, seed=21)
    img = rule.synth_image(224, 8)
    st = rule.tower(img, w, cfg)
    e = _tower(cfg, w)
    out = e.forward(img).numpy()
    assert e.tokens() == (261 if base == "dino" else 256)
    for name in ("ln1", "qkv", "attn", "h", "ln2", "mlp"):
        assert _ratio(e.debug_read(name, st[name].shape), st[name], f"one {base} block, {name}") <= TOL
    assert _ratio(out, st["out"], f"one {base} block, rows out") <= TOL
    e.close()


@functools.lru_cache(maxsize=None)
def _tiny_pair():
    return rule.synth_weights(TINY_DINO, seed=1), rule.synth_weights(TINY_SIGLIP, seed=2), rule.projector_synth_weights(PROJ, seed=3)


def _pair_rows(image, dino, siglip, proj):
    from ominix_mlx_amd import ops
    fused = ops.Tensor((dino.rows(), 272), "f32")
    dino.forward(image, out=fused, column=0)
    siglip.forward(image, out=fused, column=128)
    return fused, proj.forward(fused)


def _tiny_handles():
    from ominix_mlx_amd import vision
    dw, sw, pw = _tiny_pair()
    proj = vision.Projector()
    proj.load_weights(pw)
    return _tower(TINY_DINO, dw), _tower(TINY_SIGLIP, sw), proj


def test_tiny_tower_pair_end_to_end(omx):
    """image 56, patch 14 (16 patches): 128 = 2 x 64 with CLS + 4 registers + LayerScale and 144 = 2 x 72 plain, MLP 308, depth 4, both
    towers writing into the two column ranges of one [16, 272] buffer, then the projector 272 -> 544 -> 256 -> 256."""
    dw, sw, pw = _tiny_pair()
    dino, siglip, proj = _tiny_handles()
    img = rule.synth_image(56, 9)
    fused, rows = _pair_rows(img, dino, siglip, proj)
    d_ref, s_ref = rule.tower(img, dw, TINY_DINO)["out"], rule.tower(img, sw, TINY_SIGLIP)["out"]
    f = fused.numpy()
    assert dino.tokens() == 21 and siglip.tokens() == 16 and proj.dims() == (272, 256)
    assert _ratio(f[:, :128], d_ref, "tiny DINOv2-shaped tower") <= TOL
    assert _ratio(f[:, 128:], s_ref, "tiny SigLIP-shaped tower") <= TOL
    ref = rule.visual_rows(img, dw, TINY_DINO, sw, TINY_SIGLIP, pw)
    assert rows.shape == (16, 256)
    assert _ratio(rows.numpy(), ref, "tiny pair through the projector") <= TOL
    # a uint8 image is the same image / 255
    u8 = (img * 255).astype(np.uint8)
    assert _ratio(dino.forward(u8).numpy(), rule.tower(u8.astype(np.float32) / np.float32(255), dw, TINY_DINO)["out"], "uint8 image") <= TOL
    for h in (dino, siglip, proj):
        h.close()


def test_one_handle_reused(omx):
    """different images through one set of handles, and the same image twice: each result is a fresh set's, bit for bit"""
    one = _tiny_handles()
    for seed in (1, 2, 1, 1):
        img = rule.synth_image(56, seed)
        fresh = _tiny_handles()
        a, b = _pair_rows(img, *one), _pair_rows(img, *fresh)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
        for h in fresh:
            h.close()
    for h in one:
        h.close()


@pytest.mark.parametrize("M,N,K", [(1, 128, 256), (70, 100, 308), (33, 50, 37), (64, 64, 2048)])
def test_gemm_epilogues_against_the_unfused_product(omx, M, N, K):
    """GELU and scale-residual in launch_gemm_f32's epilogues: one row; N and K off the 64-tile grid (K = 308 on the pipelined kernel,
    K = 37 on the staged one); a product that splits K (one 64 x 64 tile of 32 K tiles).  The plain launch of the same product gives the
    numbers the epilogue starts from: resid + gamma * (product + bias) must be those float32 operations bit for bit, GELU is held to the
    float64 erf form of the plain launch's values, and all of it to float64."""
    from ominix_mlx_amd import ops, vision
    g = np.random.default_rng(M * 1000 + K)
    a, w = g.standard_normal((M, K)).astype(np.float32), (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias, resid, gamma = (g.standard_normal(s).astype(np.float32) for s in ((N,), (M, N), (N,)))
    T = lambda x: ops.Tensor.from_numpy(x, "f32")
    ta, tw, tb, tr, tg = T(a), T(w), T(bias), T(resid), T(gamma)
    plain = vision.gemm_f32(ta, tw, tb).numpy()
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    what = f"M {M} N {N} K {K}"
    assert _ratio(plain, ref, what + " plain") <= TOL
    scaled = vision.gemm_f32(ta, tw, tb, resid=tr, col_scale=tg).numpy()
    np.testing.assert_array_equal(scaled.view(np.uint32), (plain * gamma + resid).view(np.uint32))
    assert _ratio(scaled, resid + gamma * ref, what + " scale-residual") <= TOL
    act = vision.gemm_f32(ta, tw, tb, gelu=True).numpy()
    # (the epilogue's own arithmetic on the plain launch's float32 values: erff to a few ulp and three roundings, 8 ulp = 4.8e-7 < 1e-6)
    assert _ratio(act, rule.gelu(plain), what + " GELU of the plain launch's values") <= 1e-6
    assert _ratio(act, rule.gelu(ref), what + " GELU") <= TOL
    both = vision.gemm_f32(ta, tw, tb, resid=tr, col_scale=tg, gelu=True).numpy()
    np.testing.assert_array_equal(both.view(np.uint32), (act * gamma + resid).view(np.uint32))
    # no epilogue field set: ops.linear's float32 route, bit for bit
    np.testing.assert_array_equal(plain.view(np.uint32), ops.linear(ta, tw, tb).numpy().view(np.uint32))


def test_refusals_are_named(omx):
    from ominix_mlx_amd import ops, vision
    with pytest.raises(omx.OmxError, match="InvalidConfig.*head width 32"):
        vision.ViTEncoder(**dict(TINY_DINO, head_dim=32, num_heads=4))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*embed_dim 128 is not heads \\* head width = 3 \\* 64"):
        vision.ViTEncoder(**dict(TINY_DINO, num_heads=3))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*image size 60 is not a multiple of the patch 14"):
        vision.ViTEncoder(**dict(TINY_DINO, image_size=60))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*exceed the attention kernel's 1024"):
        vision.ViTEncoder(**dict(TINY_DINO, image_size=14 * 32))
    qkv = ops.Tensor.from_numpy(np.zeros((4, 3 * 128), np.float32), "f32")
    with pytest.raises(omx.OmxError, match="InvalidConfig.*head width 128"):
        vision.attention_f32(qkv, 1, 128)
    with pytest.raises(omx.OmxError, match="InvalidConfig.*1025 rows"):
        vision.attention_f32(ops.Tensor((1025, 192), "f32"), 1, 64)
    dw, sw, pw = _tiny_pair()
    img = rule.synth_image(56, 1)
    e = _tower(TINY_DINO, dw, prefix="vision_backbone.featurizer")
    bad = img.copy()
    bad[3, 40, 1] = np.inf
    with pytest.raises(omx.OmxError, match="image holds a NaN or an infinity"):
        e.forward(bad)
    with pytest.raises(omx.OmxError, match="ShapeMismatch: image has shape"):
        e.forward(rule.synth_image(42, 1))
    e.load_weights({"pos_embed": np.zeros((1, 18, 128), np.float32)})
    with pytest.raises(omx.OmxError, match="ShapeMismatch: vision_backbone.featurizer.pos_embed.*neither 16 rows.*nor 17 rows"):
        e.forward(img)
    e.close()
    for missing, named in (("blocks.2.attn.qkv.weight", "blocks.2.attn.qkv.weight"), ("blocks.1.ls2.gamma", "blocks.1.ls2.gamma or .*ls2.scale_factor"),
                           ("reg_token", "reg_token or .*register_tokens"), ("cls_token", "cls_token"), ("pos_embed", "pos_embed")):
        e = _tower(TINY_DINO, {k: v for k, v in dw.items() if k != missing}, prefix="vision_backbone.featurizer")
        with pytest.raises(omx.OmxError, match="WeightNotFound: vision_backbone.featurizer." + named):
            e.forward(img)
        e.close()
    # a plain tower takes no pos_embed with a CLS row
    e = _tower(TINY_SIGLIP, dict(sw, pos_embed=np.zeros((1, 17, 144), np.float32)))
    with pytest.raises(omx.OmxError, match="ShapeMismatch: pos_embed"):
        e.forward(img)
    e.close()
    p = vision.Projector()
    p.load_weights({k: v for k, v in pw.items() if k != "fc2.weight"})
    with pytest.raises(omx.OmxError, match="WeightNotFound: projector.fc2.weight"):
        p.dims()
    p.close()
