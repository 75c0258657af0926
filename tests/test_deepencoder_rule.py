"""CPU-only: the DeepSeek-OCR-2 vision rule (tests/deepencoder_rule.py) against forms too literal to be wrong, the data conditions the
device tests of tests/test_gpu_deepencoder.py rely on, and the host logic of ominix_mlx_amd/deepseek_ocr2.py."""
import numpy as np

import deepencoder_rule as rule

TOL = 1e-4          # the device tests' tolerance (tests/test_gpu_deepencoder.py)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_bias_against_five_loops():
    gh, gw, hd = 3, 2, 8
    g = np.random.default_rng(0)
    q, th, tw = g.standard_normal((gh * gw, hd)), g.standard_normal((2 * gh - 1, hd)), g.standard_normal((2 * gw - 1, hd))
    want = np.zeros((gh * gw, gh * gw))
    for qh in range(gh):
        for qw in range(gw):
            for kh in range(gh):
                for kw in range(gw):
                    for c in range(hd):
                        want[qh * gw + qw, kh * gw + kw] += q[qh * gw + qw, c] * (th[qh - kh + gh - 1, c] + tw[qw - kw + gw - 1, c])
    np.testing.assert_allclose(rule.rel_pos_bias(q, gh, gw, th, tw), want, rtol=0, atol=1e-12)


def test_partition_round_trip_with_padding_on_both_axes():
    H, W, C, ws = 20, 17, 3, 14
    x = np.random.default_rng(1).standard_normal((H, W, C))
    wins, pad_hw = rule.window_partition(x, ws)
    assert pad_hw == (28, 28) and wins.shape == (4, ws, ws, C)
    for n in range(4):
        for i in range(ws):
            for j in range(ws):
                y, xx = (n // 2) * ws + i, (n % 2) * ws + j
                want = x[y, xx] if (y < H and xx < W) else np.zeros(C)
                assert (wins[n, i, j] == want).all()
    np.testing.assert_array_equal(rule.window_unpartition(wins, ws, pad_hw, (H, W)), x)


def test_mask_against_the_two_loops():
    for n_image, n_query in ((4, 3), (1, 1), (5, 0), (3, 6)):
        total = n_image + n_query
        want = np.zeros((total, total), bool)
        for i in range(n_image):
            for j in range(n_image):
                want[i, j] = True
        for i in range(n_query):
            qi = n_image + i
            for j in range(n_image):
                want[qi, j] = True
            for j in range(i + 1):
                want[qi, n_image + j] = True
        got = rule.visual_causal_mask(n_image, n_query)
        np.testing.assert_array_equal(got, want)
        # the form the kernel takes: row i sees keys j < max(n_prefix, i + 1)
        np.testing.assert_array_equal(got, np.arange(total)[None, :] < np.maximum(n_image, np.arange(total) + 1)[:, None])


def test_resampling_indices_written_out():
    triple = lambda n: [4 * (i // 3) + i % 3 for i in range(n)]          # 0 1 2 | 4 5 6 | 8 9 10 | ...
    assert rule.resample_indices(127, 95)[:10] == [0, 1, 2, 4, 5, 6, 8, 9, 10, 12]
    assert rule.resample_indices(127, 95)[-5:] == [120, 121, 122, 124, 125]
    assert rule.resample_indices(127, 95) == triple(95)
    assert rule.resample_indices(64, 48)[:7] == [0, 1, 2, 4, 5, 6, 8] and rule.resample_indices(64, 48)[-3:] == [60, 61, 62]
    assert rule.resample_indices(64, 48) == triple(48)
    # the gathered table of a resampled length, and the position grid
    t = np.arange(127 * 2, dtype=np.float64).reshape(127, 2)
    got = rule.rel_pos_gathered(t, 48)
    assert got.shape == (48, 48, 2) and (got[0, 47] == t[0]).all() and (got[47, 0] == t[125]).all() and (got[5, 5] == t[triple(95)[47]]).all()
    pos = np.arange(64 * 64, dtype=np.float64).reshape(1, 64, 64, 1)
    pe = rule.pos_embed_for(pos, 48)
    assert pe.shape == (48, 48, 1) and pe[3, 47, 0] == 4 * 64 + 62 and (rule.pos_embed_for(pos, 64) == pos[0]).all()


def test_convolutions_against_loops_in_the_checkpoint_layout():
    g = np.random.default_rng(2)
    x, w = g.standard_normal((2, 5, 5, 3)), g.standard_normal((4, 3, 3, 3))          # w [O, I, kh, kw]
    for stride in (1, 2):
        OH = (5 - 1) // stride + 1
        want = np.zeros((2, OH, OH, 4))
        for b in range(2):
            for oh in range(OH):
                for ow in range(OH):
                    for o in range(4):
                        for kh in range(3):
                            for kw in range(3):
                                ih, iw = stride * oh - 1 + kh, stride * ow - 1 + kw
                                if 0 <= ih < 5 and 0 <= iw < 5:
                                    want[b, oh, ow, o] += (x[b, ih, iw, :] * w[o, :, kh, kw]).sum()
        np.testing.assert_allclose(rule.conv3x3(x, w, stride), want, rtol=0, atol=1e-12)


def test_the_bias_is_neither_negligible_nor_dominant():
    """with the synthetic tables the bias has about the spread of the scaled scores: a kernel that drops or mangles it is far off"""
    qkv, th, tw, _ = rule.synth_attention_inputs(5, (17, 17), 2)
    q, k = qkv[:, :64].astype(np.float64), qkv[:, 128:192].astype(np.float64)
    scores, bias = q @ k.T * 0.125, rule.rel_pos_bias(q, 17, 17, th, tw)
    print(f"std of the scaled scores {scores.std():.3f}, of the bias {bias.std():.3f}")
    assert 0.25 * scores.std() <= bias.std() <= 4 * scores.std()


def test_each_mistake_is_far_outside_the_tolerance():
    """no bias, h and w tables exchanged, padded keys masked out instead of kept: each is > 100 x the device tolerance away"""
    qkv, th, tw, pad = rule.synth_attention_inputs(6, (20, 17), 2, table_rows=27)
    x = qkv[:, :384]
    true = rule.sam_attention(x, 2, (20, 17), 14, th, tw, pad)
    for name, kw in (("bias left out", dict(bias=False)), ("tables swapped", dict(swap=True)), ("padded keys masked", dict(mask_padded=True))):
        r = _rel(rule.sam_attention(x, 2, (20, 17), 14, th, tw, pad, **kw), true)
        print(f"window attention, {name}: {r:.3e}")
        assert r > 100 * TOL
    qkv, th, tw, _ = rule.synth_attention_inputs(7, (5, 3), 2)
    x = qkv[:, :384]
    true = rule.sam_attention(x, 2, (5, 3), 0, th, tw)
    for name, kw in (("bias left out", dict(bias=False)), ("tables swapped", dict(swap=True))):
        r = _rel(rule.sam_attention(x, 2, (5, 3), 0, th, tw, **kw), true)
        print(f"global attention, {name}: {r:.3e}")
        assert r > 100 * TOL


def test_prefix_causal_attention_is_the_masked_form():
    """the kernel's statement (a key limit per row) and the reference's (a mask) agree, GQA mapping included"""
    g = np.random.default_rng(8)
    L, H, KV, n_image = 11, 4, 2, 5
    x = g.standard_normal((L, (H + 2 * KV) * 64))
    see = rule.visual_causal_mask(n_image, L - n_image)
    q, k, v = x[:, :H * 64].reshape(L, H, 64), x[:, H * 64:(H + KV) * 64].reshape(L, KV, 64), x[:, (H + KV) * 64:].reshape(L, KV, 64)
    want = np.empty((L, H * 64))
    for i in range(L):
        for h in range(H):
            s = np.array([q[i, h] @ k[j, h // 2] / 8.0 if see[i, j] else -np.inf for j in range(L)])
            p = np.exp(s - s.max())
            want[i, h * 64:(h + 1) * 64] = (p / p.sum()) @ v[:, h // 2]
    np.testing.assert_allclose(rule.prefix_causal_attention(x, H, KV, n_image), want, rtol=0, atol=1e-12)


def test_rope_pairs_and_angles():
    x = np.random.default_rng(9).standard_normal((3, 1, 64))
    got = rule.rope(x, 1e6)
    np.testing.assert_array_equal(got[0], x[0])                                  # position 0
    for i in (0, 5, 31):
        a = 2 * 1e6 ** (-2 * i / 64)                                             # position 2
        np.testing.assert_allclose(got[2, 0, i], x[2, 0, i] * np.cos(a) - x[2, 0, i + 32] * np.sin(a), atol=1e-12)
        np.testing.assert_allclose(got[2, 0, i + 32], x[2, 0, i] * np.sin(a) + x[2, 0, i + 32] * np.cos(a), atol=1e-12)


def test_crop_ratio_and_token_count(omx):
    from ominix_mlx_amd import deepseek_ocr2 as ds
    assert ds.find_best_crop_ratio(1536, 768, 2, 6) == (2, 1)
    assert ds.find_best_crop_ratio(1000, 1000, 2, 6) == (2, 2)
    assert ds.find_best_crop_ratio(800, 2400, 2, 6) == (1, 3)
    assert ds.image_token_count(1024, 768, (1, 1)) == 257
    assert ds.image_token_count(1024, 768, (2, 1)) == 545
    # uint8 views are v / 127.5 - 1 in float32 (examples/infer.rs:97-100); float views pass as they are; anything else is refused by name
    u8 = np.arange(4 * 4 * 3, dtype=np.uint8).reshape(4, 4, 3) * 5
    np.testing.assert_array_equal(ds.image_array(u8), u8.astype(np.float32) / np.float32(127.5) - np.float32(1))
    f = np.linspace(-1, 1, 48, dtype=np.float32).reshape(4, 4, 3)
    np.testing.assert_array_equal(ds.image_array(f), f)
    import pytest
    with pytest.raises(omx.OmxError, match="ShapeMismatch: image has shape"):
        ds.image_array(np.zeros((4, 5, 3), np.float32))
    with pytest.raises(omx.OmxError, match="image dtype int32"):
        ds.image_array(np.zeros((4, 4, 3), np.int32))


def test_row_order_and_count_agree_with_the_token_count(omx):
    from ominix_mlx_amd import deepseek_ocr2 as ds
    for ratio in ((1, 1), (2, 1), (1, 3), (2, 3)):
        n_crops = ratio[0] * ratio[1] if ratio != (1, 1) else 0
        plan = ds.row_plan(1024, 768, n_crops)
        assert [p[0] for p in plan] == [f"crop{i}" for i in range(n_crops)] + ["global", "separator"]
        at = 0
        for _, first, rows in plan:
            assert first == at
            at += rows
        assert at == ds.image_token_count(1024, 768, ratio)
        assert plan[-1][2] == 1 and plan[-2][2] == 256 and all(p[2] == 144 for p in plan[:-2])
    # the rule's encode_image lays its rows out the same way
    w = rule.synth_weights(dict(rule.TINY_SAM, depth=1, global_attn_indexes=()), dict(rule.TINY_VCF, layers=1), seed=3, neck=rule.TINY_NECK,
                           out_dim=rule.TINY_OUT, pos_grid=8)
    sam_cfg, vcf_cfg = dict(rule.TINY_SAM, depth=1, global_attn_indexes=()), dict(rule.TINY_VCF, layers=1)
    view, crops = rule.synth_images(1, 128, 1)[0], rule.synth_images(2, 64, 2)
    rows = rule.encode_image(view, crops, w, sam_cfg, vcf_cfg)
    per_crop, per_view = 256, 256                                               # neither view has 144 rows: query_1024 for both
    assert rows.shape == (2 * per_crop + per_view + 1, rule.TINY_OUT)
    np.testing.assert_array_equal(rows[-1], w["model.view_seperator"].astype(np.float64))
    np.testing.assert_allclose(rows[:2 * per_crop], rule.encode_view(crops, w, sam_cfg, vcf_cfg), rtol=0, atol=1e-12)
    np.testing.assert_allclose(rows[2 * per_crop:-1], rule.encode_view(view[None], w, sam_cfg, vcf_cfg), rtol=0, atol=1e-12)
