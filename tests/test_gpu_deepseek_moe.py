"""GPU: the DeepSeek-V2 family MoE block (csrc/moe.hip: the mode-2 router, routed + shared experts) against tests/deepseek_moe_rule.py.

Router: the inputs make every float32 gate dot product exact (deepseek_moe_rule.exact_router_inputs), so the indices must equal the
rule's and the weights agree within (E + 8) * 2^-24 relative -- the E float32 additions of the softmax sum plus the divisions and the
scale.  Block: 2 bf16 ulps + 2^-7 * max|ref|, the bound of tests/test_gpu_moe.py, against the rule at the reference's bf16 rounding
points; every row is compared (tests/test_deepseek_moe_rule.py shows on the CPU that no seed here has a selection float32 can flip).
Modes 0 / 1 are held to tests/golden/deepseek_moe_modes01.npz, recorded by tests/golden/make_deepseek_moe_golden.py on the commit before
this router joined the kernel they share: the same bits."""
import functools
import os

import numpy as np
import pytest

import deepseek_moe_rule as dr
from test_gpu_primitives import assert_bf16_close

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepseek_moe_modes01.npz")


@pytest.mark.parametrize("E,k", dr.ROUTER_CASES)
@pytest.mark.parametrize("rows", [1, 5])
def test_router_mode2(omx, E, k, rows):
    from ominix_mlx_amd import moe
    T = omx.ops.Tensor
    x, gw = dr.exact_router_inputs(rows, E, dr.ROUTER_HIDDEN, dr.router_seed(E, k, rows))
    z = np.zeros((E, 64, dr.ROUTER_HIDDEN), np.float32)
    worst = 0.0
    for norm in (False, True):
        for scale in (1.0, 2.5):
            blk = moe.DeepseekMoeBlock(gw, z, z, z.transpose(0, 2, 1), k, norm_topk_prob=norm, routed_scaling_factor=scale)
            inds, w = blk.route(T.from_numpy(x))
            ref_i, ref_w = dr.route(x, gw, k, norm, scale)
            np.testing.assert_array_equal(inds.numpy(), ref_i)
            rel = np.abs(w.numpy().astype(np.float64) - ref_w) / ref_w
            worst = max(worst, rel.max())
            print(f"router E={E} k={k} rows={rows} norm={norm} scale={scale}: worst relative {rel.max():.3e} (bound {(E + 8) * 2.0 ** -24:.3e})")
            assert rel.max() <= (E + 8) * 2.0 ** -24


def test_router_mode2_with_the_block_norm_folded_in(omx):
    """the RMSNorm-in-the-router launch: the rows it leaves are ops.rms_norm's, and it routes those rows"""
    from ominix_mlx_amd import moe
    T = omx.ops.Tensor
    E, k, h = 16, 6, dr.ROUTER_HIDDEN
    x = dr.rows_for(5, h, 41)
    gw = dr.weights_for(E, h, 64, 0, 42)[0]
    nw = dr.bf16(1.0 + 0.1 * np.random.default_rng(43).standard_normal(h))
    xn_ref = omx.ops.rms_norm(T.from_numpy(x), T.from_numpy(nw), 1e-6).numpy()
    inds, w, xn = T((5, k), "u32"), T((5, k), "f32"), T((5, h), "bf16")
    dx, dgw, dnw = T.from_numpy(x), T.from_numpy(gw), T.from_numpy(nw)
    omx.check(omx.lib.omx_moe_route_deepseek(inds.ptr, w.ptr, dx.ptr, dgw.ptr, dnw.ptr, 1e-6, xn.ptr, 5, h, E, k, 1, 2.5, None))
    np.testing.assert_array_equal(xn.numpy(), xn_ref)
    assert (dr.topk_gap(xn_ref, gw, k) > dr.MIN_GAP).all()
    ref_i, ref_w = dr.route(xn_ref, gw, k, True, 2.5)
    np.testing.assert_array_equal(inds.numpy(), ref_i)
    # (ordinary inputs: the float32 logits carry their own error, 192 terms -- a looser sanity bound than the exact-logit cases)
    np.testing.assert_allclose(w.numpy(), ref_w, rtol=1e-4)


@functools.lru_cache(maxsize=None)
def _reference(width, n_shared, rows):
    x, (gw, wg, wu, wd, sh) = dr.block_inputs(width, n_shared, rows)
    return dr.block(x, gw, wg, wu, wd, dr.BLOCK_K, sh, True, 2.5, rnd=dr.bf16)


@pytest.mark.parametrize("slots_env", ["1", "0"])
@pytest.mark.parametrize("rows", dr.BLOCK_ROWS)
@pytest.mark.parametrize("n_shared", dr.BLOCK_SHARED)
@pytest.mark.parametrize("width", dr.BLOCK_WIDTHS)
def test_block(omx, monkeypatch, width, n_shared, rows, slots_env):
    from ominix_mlx_amd import moe
    monkeypatch.setenv("OMX_MOE_SHARED_SLOTS", slots_env)
    x, (gw, wg, wu, wd, sh) = dr.block_inputs(width, n_shared, rows)
    blk = moe.DeepseekMoeBlock(gw, wg, wu, wd, dr.BLOCK_K, sh, n_shared, norm_topk_prob=True, routed_scaling_factor=2.5)
    slot_form = slots_env == "1" and n_shared > 0 and rows * (dr.BLOCK_K + n_shared) <= 32
    assert blk.form(rows) == (0 if slot_form else 1 if rows * dr.BLOCK_K <= 32 else 2)
    out, inds, w = blk.forward(omx.ops.Tensor.from_numpy(x), return_routing=True)
    ref, ref_i, ref_w = _reference(width, n_shared, rows)
    np.testing.assert_array_equal(inds.numpy(), ref_i)
    np.testing.assert_allclose(w.numpy(), ref_w, rtol=1e-4)
    err = np.abs(out.numpy() - ref).max()
    print(f"block width={width} shared={n_shared} rows={rows} form={blk.form(rows)}: worst {err:.3e} of max|ref| {np.abs(ref).max():.3e}")
    assert_bf16_close(out.numpy(), ref, 2, atol=2.0 ** -7 * np.abs(ref).max())


@pytest.mark.parametrize("rows", [1, 5, 70])
def test_block_inside_a_decoder_layer(omx, rows):
    """resid + block(rmsnorm(x)): the norm in the router launch and the residual in the combine equal the three steps done apart"""
    from ominix_mlx_amd import moe
    T = omx.ops.Tensor
    x, (gw, wg, wu, wd, sh) = dr.block_inputs(64, 2, rows)
    nw = dr.bf16(1.0 + 0.1 * np.random.default_rng(44).standard_normal(dr.BLOCK_HIDDEN))
    blk = moe.DeepseekMoeBlock(gw, wg, wu, wd, dr.BLOCK_K, sh, 2, norm_topk_prob=True, routed_scaling_factor=1.0)
    xn = omx.ops.rms_norm(T.from_numpy(x), T.from_numpy(nw), 1e-6)
    apart = dr.bf16(x + blk.forward(xn).numpy())
    dx, dnw = T.from_numpy(x), T.from_numpy(nw)
    got = blk.block_forward(dx, dx, dnw, 1e-6).numpy()
    np.testing.assert_array_equal(got, apart)


def test_refusals(omx):
    from ominix_mlx_amd import moe
    z = lambda *s: np.zeros(s, np.float32)
    T = omx.ops.Tensor
    with pytest.raises(omx.OmxError, match="top_k"):
        moe.DeepseekMoeBlock(z(4, 192), z(4, 64, 192), z(4, 64, 192), z(4, 192, 64), 9).forward(T.from_numpy(z(1, 192)))
    blk = moe.DeepseekMoeBlock(z(4, 192), z(4, 64, 192), z(4, 64, 192), z(4, 192, 64), 2, (z(64, 192), z(64, 192), z(192, 64)), 1)
    blk.shared = None                                   # 70 rows do not fit the slots: the whole shared MLP is needed, by name
    with pytest.raises(omx.OmxError, match="shared"):
        blk.forward(T.from_numpy(z(70, 192)))


def test_modes_0_and_1_keep_their_bits(omx):
    want = np.load(GOLDEN)
    got = dr.run_modes01(omx)
    assert sorted(got) == sorted(want.files)
    for name in want.files:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
