"""The DeepSeek-OCR-2 vision side on the device (csrc/sam_encoder.hip, csrc/vcf_encoder.hip, csrc/attn_stream_f32.hpp; vision.SamEncoder,
vision.VisualCausalEncoder, vision.sam_attention_f32, vision.prefix_causal_attention_f32, deepseek_ocr2.DeepEncoder) against its numpy
float64 restatement (tests/deepencoder_rule.py, written from deepseek-ocr2-mlx/src/vision.rs, qwen2_encoder.rs and lib.rs).

Tolerance: the project's float32 rule -- error <= 1e-4 x the largest magnitude of the float64 result (tests/test_gpu_vit.py) -- at every
stage read.  Each test prints its measured worst ratio.  tests/test_deepencoder_rule.py shows that the inputs used here put a kernel that
drops the bias, exchanges its tables or masks the padded keys more than 100 x that tolerance away."""
import functools

import numpy as np
import pytest

import deepencoder_rule as rule

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _ratio(got, ref, what):
    r = np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max()
    print(f"{what}: worst error / largest magnitude = {r:.3e}")
    return r


def _T(a):
    from ominix_mlx_amd import ops
    return ops.Tensor.from_numpy(np.ascontiguousarray(a, np.float32), "f32")


def _sam_attention(qkv, heads, grid, window, th, tw, pad=None, images=1):
    from ominix_mlx_amd import vision
    return vision.sam_attention_f32(_T(qkv), heads, grid, window, _T(th), _T(tw), None if pad is None else _T(pad), images).numpy()


def _sam_rule(qkv, heads, grid, window, th, tw, pad=None, images=1):
    d3, n = 3 * heads * 64, grid[0] * grid[1]
    return np.concatenate([rule.sam_attention(qkv[i * n:(i + 1) * n, :d3], heads, grid, window, th, tw, pad) for i in range(images)])


# ---- global attention ----
GLOBAL = {"a": ((1, 1), None), "b": ((4, 4), None), "c": ((5, 3), None), "d": ((17, 17), None), "e": ((33, 31), None), "f": ((32, 33), None),
          "g": ((48, 48), 127)}


@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("case", sorted(GLOBAL))
def test_global_attention_against_the_rule(omx, case, heads):
    """one key; exactly one 16-key tile; a non-square grid with a partial tile; several tiles; 1023 keys; 1056 keys, just past what the
    score-in-LDS kernels take; 48 x 48 with the checkpoint's 127-row table resampled to 95 rows.  Rows 8 floats longer than 3 * dim."""
    grid, rows = GLOBAL[case]
    qkv, th, tw, _ = rule.synth_attention_inputs(100 * heads + ord(case), grid, heads, table_rows=rows)
    got = _sam_attention(qkv, heads, grid, 0, th, tw)
    assert got.shape == (grid[0] * grid[1], heads * 64)
    assert _ratio(got, _sam_rule(qkv, heads, grid, 0, th, tw), f"global attention {grid[0]} x {grid[1]}, {heads} heads") <= TOL


def test_global_attention_at_its_largest_size_gives_the_same_bits_twice(omx):
    qkv, th, tw, _ = rule.synth_attention_inputs(11, (64, 64), 2)
    a, b = _sam_attention(qkv, 2, (64, 64), 0, th, tw), _sam_attention(qkv, 2, (64, 64), 0, th, tw)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert _ratio(a, _sam_rule(qkv, 2, (64, 64), 0, th, tw), "global attention 64 x 64, 4096 keys") <= TOL


def test_global_attention_over_stacked_images(omx):
    qkv, th, tw, _ = rule.synth_attention_inputs(12, (17, 17), 2, images=3)
    got = _sam_attention(qkv, 2, (17, 17), 0, th, tw, images=3)
    assert _ratio(got, _sam_rule(qkv, 2, (17, 17), 0, th, tw, images=3), "global attention, three images") <= TOL


def test_global_attention_with_a_moving_maximum(omx):
    """q times 6: scores of spread 6, the running maximum rises again and again along the keys"""
    qkv, th, tw, _ = rule.synth_attention_inputs(13, (17, 17), 2, q_gain=6.0)
    assert _ratio(_sam_attention(qkv, 2, (17, 17), 0, th, tw), _sam_rule(qkv, 2, (17, 17), 0, th, tw), "global attention, q x 6") <= TOL


def test_global_attention_whose_largest_score_is_the_last_key(omx):
    """row 40's largest score is its last key, the only key of a partial tile in the last chunk: every earlier chunk is rescaled"""
    grid, heads = (33, 31), 2
    qkv, th, tw, _ = rule.synth_attention_inputs(14, grid, heads)
    n = grid[0] * grid[1]
    for h in range(heads):
        qkv[n - 1, 128 + 64 * h:128 + 64 * (h + 1)] = 2 * qkv[40, 64 * h:64 * (h + 1)]          # k[last] = 2 q[40]: score ~ 2 * 64 / 8
    q, k = qkv[40, :64].astype(np.float64), qkv[:, 128:192].astype(np.float64)
    s = k @ q * 0.125 + rule.rel_pos_bias(qkv[:, :64], grid[0], grid[1], th, tw)[40]
    assert s.argmax() == n - 1
    assert _ratio(_sam_attention(qkv, heads, grid, 0, th, tw), _sam_rule(qkv, heads, grid, 0, th, tw), "global attention, largest score last") <= TOL


# ---- window attention ----
@pytest.mark.parametrize("grid,heads", [((14, 14), 2), ((6, 6), 2), ((20, 17), 2), ((48, 48), 12), ((64, 64), 2)])
def test_window_attention_against_the_rule(omx, grid, heads):
    """no padding; a grid smaller than a window; padding on both axes over four windows; the two real grids (48 -> 56, 64 -> 70)"""
    qkv, th, tw, pad = rule.synth_attention_inputs(200 + grid[0] + grid[1], grid, heads, table_rows=27)
    got = _sam_attention(qkv, heads, grid, 14, th, tw, pad)
    assert _ratio(got, _sam_rule(qkv, heads, grid, 14, th, tw, pad), f"window attention {grid[0]} x {grid[1]}, {heads} heads") <= TOL


def test_window_attention_over_stacked_images_and_the_same_bits_twice(omx):
    qkv, th, tw, pad = rule.synth_attention_inputs(21, (20, 17), 2, table_rows=27, images=2)
    a, b = _sam_attention(qkv, 2, (20, 17), 14, th, tw, pad, images=2), _sam_attention(qkv, 2, (20, 17), 14, th, tw, pad, images=2)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert _ratio(a, _sam_rule(qkv, 2, (20, 17), 14, th, tw, pad, images=2), "window attention, two images") <= TOL


def test_attention_refusals_are_named(omx):
    from ominix_mlx_amd import ops, vision
    qkv, th, tw, pad = rule.synth_attention_inputs(22, (20, 17), 2, table_rows=27)
    with pytest.raises(omx.OmxError, match="20 x 17 grid is no multiple of the window 14: pad_qkv"):
        _sam_attention(qkv, 2, (20, 17), 14, th, tw)
    with pytest.raises(omx.OmxError, match="InvalidConfig.*head width 32"):
        vision.sam_attention_f32(ops.Tensor((16, 3 * 64), "f32"), 2, (4, 4), 0, ops.Tensor((7, 32), "f32"), ops.Tensor((7, 32), "f32"))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*head width 32"):
        vision.prefix_causal_attention_f32(ops.Tensor((16, 8 * 32), "f32"), 4, 2, 0, width=32)
    with pytest.raises(omx.OmxError, match="InvalidConfig.*heads=3 kv_heads=2"):
        vision.prefix_causal_attention_f32(ops.Tensor((16, 7 * 64), "f32"), 3, 2, 0)


# ---- prefix-causal attention ----
@pytest.mark.parametrize("heads,kv_heads", [(14, 2), (4, 2)])
@pytest.mark.parametrize("L,n_prefix", [(1, 0), (17, 0), (17, 17), (16, 8), (65, 16), (288, 144), (512, 256), (257, 1), (1024, 512)])
def test_prefix_causal_attention_against_the_rule(omx, L, n_prefix, heads, kv_heads):
    """plain causal (prefix 0), no mask (prefix L), a prefix inside the first query block, past it, the two real shapes, a one-row prefix,
    1024 rows; 7 and 2 query heads per key/value head; rows 8 floats longer than the heads"""
    from ominix_mlx_amd import vision
    ld = (heads + 2 * kv_heads) * 64 + 8
    qkv = np.random.default_rng(1000 * L + 10 * n_prefix + heads).standard_normal((L, ld)).astype(np.float32)
    got = vision.prefix_causal_attention_f32(_T(qkv), heads, kv_heads, n_prefix).numpy()
    assert got.shape == (L, heads * 64)
    assert _ratio(got, rule.prefix_causal_attention(qkv, heads, kv_heads, n_prefix), f"prefix-causal L {L} prefix {n_prefix} heads {heads} / {kv_heads}") <= TOL


def test_prefix_causal_attention_over_stacked_images_and_the_same_bits_twice(omx):
    from ominix_mlx_amd import vision
    L, n_prefix, heads, kv = 65, 16, 4, 2
    qkv = np.random.default_rng(31).standard_normal((3 * L, (heads + 2 * kv) * 64)).astype(np.float32)
    a = vision.prefix_causal_attention_f32(_T(qkv), heads, kv, n_prefix, images=3).numpy()
    b = vision.prefix_causal_attention_f32(_T(qkv), heads, kv, n_prefix, images=3).numpy()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    ref = np.concatenate([rule.prefix_causal_attention(qkv[i * L:(i + 1) * L], heads, kv, n_prefix) for i in range(3)])
    assert _ratio(a, ref, "prefix-causal, three images") <= TOL


# ---- the towers ----
def test_one_window_block_and_one_global_block_at_the_real_widths(omx):
    """depth 2, block 1 global, 768 / 12 x 64 / 3072 on a 768 px image: 2304 rows, 4 x 4 padded windows (48 -> 56), pos_embed gathered
    64 -> 48 and the 127-row table resampled to 95; every stage, the neck and the rows out"""
    from ominix_mlx_amd import vision
    cfg = dict(rule.SAM, depth=2, global_attn_indexes=(1,))
    w = rule.behind(rule.synth_weights(cfg, dict(rule.VCF, layers=0), seed=41), rule.SAM_PREFIX)
    img = rule.synth_images(1, 768, 42)
    st = rule.sam_tower(img, w, cfg)
    e = vision.SamEncoder(**cfg, prefix=rule.SAM_PREFIX, keep_stages=True)
    e.load_weights(w)
    out = e.forward(img).numpy()
    assert e.tokens(768) == (48, 144, 896) and out.shape == (144, 896)
    for name in ("patches", "h0", "block0", "block1", "neck"):
        assert _ratio(e.debug_read(name, st[name].shape), st[name], f"SAM at the real widths, {name}") <= TOL
    assert _ratio(e.debug_read("out", st["out"].shape), st["out"], "SAM at the real widths, out (debug_read)") <= TOL
    assert _ratio(out, st["out"], "SAM at the real widths, rows out") <= TOL
    assert e.launches() == 3 + 2 * 7 + 3 + 3 * 2
    e.close()


def test_one_encoder_layer_at_the_real_widths(omx):
    """896 / 14 / 2 / 4864 over 144 image rows + the 144 rows of query_768"""
    from ominix_mlx_amd import vision
    cfg = dict(rule.VCF, layers=1)
    w = rule.behind(rule.synth_weights(dict(rule.TINY_SAM, depth=0), cfg, seed=43, neck=(32, 64, 896)), rule.VCF_PREFIX)
    x = np.random.default_rng(44).standard_normal((144, 896)).astype(np.float32)
    st = rule.vcf_encoder(x, w, cfg)
    e = vision.VisualCausalEncoder(**cfg, prefix=rule.VCF_PREFIX, keep_stages=True)
    e.load_weights(w)
    out = e.forward(_T(x)).numpy()
    assert e.tokens(144) == (144, 288) and out.shape == (144, 896)
    assert _ratio(e.debug_read("layer0", st["layer0"].shape), st["layer0"], "one encoder layer at the real widths, layer0") <= TOL
    assert _ratio(out, st["out"], "one encoder layer at the real widths, out") <= TOL
    e.close()


@functools.lru_cache(maxsize=None)
def _tiny():
    """weights, views and the rule's rows of the whole encode_image at tiny widths and the real image sizes, computed once"""
    w = rule.synth_weights(rule.TINY_SAM, rule.TINY_VCF, seed=51, neck=rule.TINY_NECK, out_dim=rule.TINY_OUT)
    view, crops = rule.synth_images(1, 1024, 52)[0], rule.synth_images(2, 768, 53)
    return w, view, crops, rule.encode_image(view, crops, w, rule.TINY_SAM, rule.TINY_VCF)


def _tiny_encoder():
    from ominix_mlx_amd import deepseek_ocr2
    return deepseek_ocr2.DeepEncoder.from_weights(_tiny()[0], rule.TINY_SAM, rule.TINY_VCF)


def test_encode_image_end_to_end(omx):
    """SAM 128 / 2 x 64 / 308, depth 4, blocks 1 and 3 global, neck 32 / 64 / 256; encoder 256 / 4 / 2 / 308, 3 layers; projector
    256 -> 160; a 1024 px view (query_1024) and two 768 px crops (query_768) in one stacked pass; the separator last"""
    w, view, crops, ref = _tiny()
    enc = _tiny_encoder()
    a = enc.encode_image(view, crops).numpy()
    b = enc.encode_image(view, crops).numpy()
    assert a.shape == ref.shape == (2 * 144 + 256 + 1, rule.TINY_OUT)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    for name, lo, hi in (("crop 0", 0, 144), ("crop 1", 144, 288), ("global view", 288, 544)):
        assert _ratio(a[lo:hi], ref[lo:hi], f"encode_image, {name}") <= TOL
    np.testing.assert_array_equal(a[-1], w["model.view_seperator"])
    # a view alone: its rows and the separator
    alone = enc.encode_image(view).numpy()
    assert alone.shape == (257, rule.TINY_OUT)
    assert _ratio(alone[:256], ref[288:544], "encode_image, a view alone") <= TOL
    np.testing.assert_array_equal(alone[-1], w["model.view_seperator"])
    enc.close()


def test_sam_scratch_stays_far_below_the_reference_bias_array(omx):
    """real widths, one global block, one 1024 px image: 4096 keys x 12 heads.  The reference's bias array alone is heads * N^2 * 4 bytes."""
    from ominix_mlx_amd import vision
    cfg = dict(rule.SAM, depth=1, global_attn_indexes=(0,))
    w = rule.behind(rule.synth_weights(cfg, dict(rule.VCF, layers=0), seed=61), rule.SAM_PREFIX)
    e = vision.SamEncoder(**cfg, prefix=rule.SAM_PREFIX)
    e.load_weights(w)
    out = e.forward(rule.synth_images(1, 1024, 62)).numpy()
    assert out.shape == (256, 896) and np.isfinite(out).all()
    print(f"SAM scratch after one 1024 px image: {e.scratch_bytes()} bytes")
    assert 0 < e.scratch_bytes() < 12 * 4096 * 4096 * 4 == 805306368
    e.close()
