"""CPU: the DeepSeek-V2 family MoE rule (tests/deepseek_moe_rule.py) against a literal restatement of the reference's path, the mistakes
it must tell apart, and the condition under which the device tests may compare every row: at each of their seeds the selection has a gap
no float32 logit error can close."""
import numpy as np
import pytest

import deepseek_moe_rule as dr


@pytest.mark.parametrize("n_shared,k,norm,scale", [(0, 6, False, 1.0), (2, 6, True, 2.5), (1, 1, True, 2.5), (2, 3, False, 0.5)])
def test_block_equals_the_literal_path(n_shared, k, norm, scale):
    x = dr.rows_for(9, 64, 5)
    gw, wg, wu, wd, sh = dr.weights_for(16, 64, 64, n_shared, 6)
    got, inds, w = dr.block(x, gw, wg, wu, wd, k, sh, norm, scale)
    ref = dr.block_literal(x, gw, wg, wu, wd, k, sh, norm, scale)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert (np.diff(w, axis=1) <= 0).all()                        # descending
    if norm and k > 1:
        np.testing.assert_allclose(w.sum(axis=1), scale, rtol=1e-12)


def test_split_shared_mlp_equals_the_whole_one():
    """the pseudo-expert split the slot form rests on (gate / up row blocks, down column blocks)"""
    _, _, _, _, sh = dr.weights_for(4, 64, 64, 2, 11)
    x = dr.rows_for(5, 64, 12)
    g, u, d = sh
    whole = dr.mlp(x, g, u, d)
    parts = sum(dr.mlp(x, g[i * 64:(i + 1) * 64], u[i * 64:(i + 1) * 64], d[:, i * 64:(i + 1) * 64]) for i in range(2))
    assert np.abs(whole - parts).max() <= 1e-13 * np.abs(whole).max()


def _far(a, b):
    return np.abs(a - b).max() / np.abs(a).max()


def test_dropping_the_shared_experts_is_seen():
    x = dr.rows_for(4, 64, 21)
    gw, wg, wu, wd, sh = dr.weights_for(16, 64, 64, 2, 22)
    sh = tuple(s * 4 for s in sh)
    right = dr.block(x, gw, wg, wu, wd, 6, sh, True, 1.0)[0]
    assert _far(right, dr.block(x, gw, wg, wu, wd, 6, None, True, 1.0)[0]) > 0.5


def test_ignoring_the_scale_is_seen():
    x = dr.rows_for(4, 64, 23)
    gw, wg, wu, wd, _ = dr.weights_for(16, 64, 64, 0, 24)
    right = dr.block(x, gw, wg, wu, wd, 6, None, True, 2.5)[0]
    assert _far(right, dr.block(x, gw, wg, wu, wd, 6, None, True, 1.0)[0]) > 0.5


def test_normalising_at_top1_is_seen():
    """the reference leaves a single selected score as the softmax gave it (k > 1 guards the division) and still scales it"""
    x = dr.rows_for(4, 64, 25)
    gw, wg, wu, wd, _ = dr.weights_for(16, 64, 64, 0, 26)
    right, inds, w = dr.block(x, gw, wg, wu, wd, 1, None, True, 2.5)
    assert (w < 2.5 * 0.9).all()
    wrong = np.stack([dr.mlp(x[t:t + 1], wg[int(inds[t, 0])], wu[int(inds[t, 0])], wd[int(inds[t, 0])])[0] * 2.5 for t in range(4)])
    assert _far(right, wrong) > 0.5


def test_bf16_router_arithmetic_is_seen():
    """Expert 1's float32 logit is 1 + 2^-10, expert 0's is 1: the float32 router takes expert 1.  Rounded to bf16 (modes 0 / 1) both
    are 1.0 and the tie goes to expert 0, whose output is the opposite sign."""
    x = np.zeros((1, 64)); x[0, 0] = x[0, 1] = 1.0
    gw = np.full((4, 64), 0.0); gw[:, 0] = [1.0, 1.0, -2.0, -2.0]; gw[1, 1] = 2.0 ** -10
    _, wg, wu, wd, _ = dr.weights_for(4, 64, 64, 0, 27)
    wg[1], wu[1], wd[1] = wg[0], wu[0], -wd[0]
    right, inds, _ = dr.block(x, gw, wg, wu, wd, 1, None, False, 1.0)
    assert inds[0, 0] == 1
    i1, s1 = dr.route_mode1(x, gw, 1, False)
    assert i1[0, 0] == 0
    wrong = dr.mlp(x, wg[0], wu[0], wd[0]) * s1[0, 0]
    assert _far(right, wrong) > 0.5


@pytest.mark.parametrize("E,k", dr.ROUTER_CASES)
@pytest.mark.parametrize("rows", [1, 5])
def test_router_cases_have_exact_logits_and_a_gap(E, k, rows):
    x, gw = dr.exact_router_inputs(rows, E, dr.ROUTER_HIDDEN, dr.router_seed(E, k, rows))
    assert (dr.bf16(x) == x).all() and (dr.bf16(gw) == gw).all()
    f32 = (x.astype(np.float32) @ gw.astype(np.float32).T).astype(np.float64)
    assert (f32 == x @ gw.T).all()                                  # exact in float32
    gap = dr.topk_gap(x, gw, k)
    assert ((gap == 0) | (gap > dr.MIN_GAP)).all()                  # an exact tie is settled by the index on both sides
    for norm in (False, True):
        i64, _ = dr.route(x, gw, k, norm, 2.5)
        i32, _ = dr.route(x, gw, k, norm, 2.5, f32=True)
        np.testing.assert_array_equal(i64, i32)


@pytest.mark.parametrize("width", dr.BLOCK_WIDTHS)
@pytest.mark.parametrize("n_shared", dr.BLOCK_SHARED)
@pytest.mark.parametrize("rows", dr.BLOCK_ROWS)
def test_block_seeds_select_the_same_experts_in_float64_and_float32(width, n_shared, rows):
    """The block's router reads the block's own input, so the bf16 rounding points (all behind the router) cannot move its selection;
    what could is the float32 logit.  Every seed the device test uses keeps the k-th score MIN_GAP clear of the next."""
    x, (gw, *_rest) = dr.block_inputs(width, n_shared, rows)
    assert (dr.topk_gap(x, gw, dr.BLOCK_K) > dr.MIN_GAP).all()
    np.testing.assert_array_equal(dr.route(x, gw, dr.BLOCK_K, True, 1.0)[0], dr.route(x, gw, dr.BLOCK_K, True, 1.0, f32=True)[0])


def test_treating_layer_0_as_moe_is_seen():
    """layer 0 of the plan is a dense MLP of intermediate_size (first_k_dense_replace = 1): a model that runs an MoE block there
    computes something else altogether"""
    cfg = dr.tiny_decoder_config()
    w = dr.decoder_weights(cfg, 1, 2, 0x0C0FFEE5)
    w.update({k: v for k, v in dr.decoder_weights(cfg, 0, 2, 0x0C0FFEE5).items() if k.startswith("model.layers.0.mlp.")})
    x = dr.rows_for(6, cfg.hidden_size, 31).reshape(1, 6, -1).astype(np.float32)
    right = dr.make_oracle(cfg, w, 1, 2, 1.0).mlp(0, x)
    wrong = dr.make_oracle(cfg, w, 0, 2, 1.0).mlp(0, x)
    assert _far(right, wrong) > 0.5


@pytest.mark.parametrize("scale,seed", dr.ENGINE_RUNS)
def test_engine_seeds_select_the_same_experts_with_and_without_bf16_rounding(scale, seed):
    """40 prompt tokens + 8 decoded through the 3-layer decoder: the rule without any 16-bit rounding and the rule at the reference's
    bf16 rounding points send every row of every MoE layer to the same experts, and decode the same tokens -- so the device test compares
    every row."""
    a, ta, _ = dr.engine_selections(scale, seed, "bf16")
    b, tb, _ = dr.engine_selections(scale, seed, "f32")
    assert len(a) == len(b) and len(a) == 2 * (1 + dr.ENGINE_NEW - 1)
    for (la, ia, _g), (lb, ib, _h) in zip(a, b):
        assert la == lb
        np.testing.assert_array_equal(np.sort(ia, axis=1), np.sort(ib, axis=1))
    np.testing.assert_array_equal(ta, tb)
