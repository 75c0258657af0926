"""CPU-only: the numpy rule of the Moxin-VLM vision towers (tests/vit_rule.py) against forms too literal to be wrong."""
import numpy as np
import pytest

import vit_rule as rule


def test_patch_embed_is_the_six_loop_convolution():
    """a 28 x 28 image, patch 14 (a 2 x 2 grid), 5 output channels: out[py, px, o] = b[o] + sum_{kh, kw, c} x[14 py + kh, 14 px + kw, c]
    w[o, c, kh, kw] with the CHECKPOINT's weight layout [O, I, P, P]"""
    g = np.random.default_rng(0)
    x, w, b = g.standard_normal((28, 28, 3)), g.standard_normal((5, 3, 14, 14)), g.standard_normal(5)
    want = np.zeros((2, 2, 5))
    for py in range(2):
        for px in range(2):
            for o in range(5):
                acc = b[o]
                for kh in range(14):
                    for kw in range(14):
                        for c in range(3):
                            acc += x[14 * py + kh, 14 * px + kw, c] * w[o, c, kh, kw]
                want[py, px, o] = acc
    np.testing.assert_allclose(rule.patch_embed(x, w, b, 14), want.reshape(4, 5), rtol=0, atol=1e-11)
    np.testing.assert_allclose(rule.patch_embed(x, w, None, 14), want.reshape(4, 5) - b, rtol=0, atol=1e-11)


@pytest.mark.parametrize("heads,width,n", [(2, 64, 5), (3, 72, 17)])
def test_attention_is_the_per_row_softmax(heads, width, n):
    g = np.random.default_rng(heads)
    q, k, v = (g.standard_normal((n, heads * width)) for _ in range(3))
    want = np.zeros((n, heads * width))
    for h in range(heads):
        c = slice(h * width, (h + 1) * width)
        for i in range(n):
            s = np.array([q[i, c] @ k[j, c] for j in range(n)]) / np.sqrt(width)
            p = np.exp(s - s.max())
            want[i, c] = (p / p.sum()) @ v[:, c]
    np.testing.assert_allclose(rule.attention(q, k, v, heads), want, rtol=0, atol=1e-12)


def test_assembly_orders_and_token_counts():
    """pos_embed of num_patches rows is added before the CLS row is prepended (CLS gets no position), of num_patches + 1 rows after
    (CLS gets row 0); registers sit between CLS and the patches with no position"""
    g = np.random.default_rng(1)
    cfg = dict(rule.DINO, embed_dim=8, image_size=28)
    assert rule.num_patches(cfg) == 4 and rule.num_tokens(cfg) == 9
    assert rule.num_tokens(rule.DINO) == 261 and rule.num_tokens(rule.SIGLIP) == 256 and rule.num_patches(rule.DINO) == 256
    patches, cls, reg = g.standard_normal((4, 8)), g.standard_normal((1, 1, 8)), g.standard_normal((1, 4, 8))
    for rows in (4, 5):
        pos = g.standard_normal((1, rows, 8))
        h = rule.assemble(patches, {"pos_embed": pos, "cls_token": cls, "register_tokens": reg}, cfg)
        assert h.shape == (9, 8)
        np.testing.assert_array_equal(h[0], cls[0, 0] + (pos[0, 0] if rows == 5 else 0))
        np.testing.assert_array_equal(h[1:5], reg[0])
        np.testing.assert_array_equal(h[5:], patches + pos[0, rows - 4:])
    plain = dict(rule.SIGLIP, embed_dim=8, image_size=28)
    pos = g.standard_normal((1, 4, 8))
    np.testing.assert_array_equal(rule.assemble(patches, {"pos_embed": pos}, plain), patches + pos[0])
    with pytest.raises(AssertionError):
        rule.assemble(patches, {"pos_embed": g.standard_normal((1, 5, 8))}, plain)


def test_tower_runs_depth_minus_one_blocks_and_drops_the_extra_rows():
    cfg = dict(rule.DINO, embed_dim=128, num_heads=2, intermediate_dim=96, depth=3, image_size=28)
    w = rule.synth_weights(cfg, seed=2)
    assert "blocks.1.norm1.weight" in w and "blocks.2.norm1.weight" not in w
    img = rule.synth_image(28, 3)
    st = rule.tower(img, w, cfg)
    assert st["tokens"].shape == (9, 128) and st["out"].shape == (4, 128) and st["col"].shape == (4, 588)
    by_hand = rule.block(rule.block(st["tokens"], w, "blocks.0.", cfg), w, "blocks.1.", cfg)[5:]
    np.testing.assert_array_equal(st["out"], by_hand)
    # the final norm's weights take no part
    w2 = dict(w, **{"norm.weight": w["norm.weight"] * 3})
    np.testing.assert_array_equal(rule.tower(img, w2, cfg)["out"], st["out"])
    # LayerScale under its other spelling
    w3 = {k.replace(".gamma", ".scale_factor"): v for k, v in w.items()}
    np.testing.assert_array_equal(rule.tower(img, w3, cfg)["out"], st["out"])


def test_projector_is_three_linears_and_two_gelus():
    w = rule.projector_synth_weights((12, 20, 8, 8), seed=4)
    x = np.random.default_rng(5).standard_normal((3, 12))
    h = rule.gelu(x @ w["fc1.weight"].astype(np.float64).T + w["fc1.bias"])
    h = rule.gelu(h @ w["fc2.weight"].astype(np.float64).T + w["fc2.bias"])
    np.testing.assert_allclose(rule.projector(x, w), h @ w["fc3.weight"].astype(np.float64).T + w["fc3.bias"], rtol=0, atol=1e-13)
