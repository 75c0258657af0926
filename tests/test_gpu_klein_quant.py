"""GPU: the quantized FLUX.2-klein DiT (flux-klein-mlx/src/klein_quantized.rs) on the packed-weight matrix-core GEMM (csrc/qgemm.hip).

  * kernel: every output equals omx_dequantize followed by the bf16 16x16x32 kernel -- the eight-wave 256^2 kernel, pinned with
    OMX_GEMM_TILE=256 OMX_GEMM_MFMA=16 (the segmented SwiGLU launch: its 16x16x32 kernels) -- bit for bit; the gated form against float64;
  * the tiny model against oracle/ref_klein.py fed the dequantised triplets, with the bf16 test's bound;
  * real widths: the int8 model against the bf16 model holding the dequantised weights, and the same bits under the schedule switches;
  * weight_bytes() accounting and the error paths."""
import ctypes

import numpy as np
import pytest

from oracle import ref_core as rc, ref_klein as rk

pytestmark = pytest.mark.gpu

FORMATS = [(b, g) for b in (4, 8) for g in (32, 64, 128)]


def _pin_bf16_kernel(monkeypatch):
    monkeypatch.setenv("OMX_GEMM_TILE", "256")
    monkeypatch.setenv("OMX_GEMM_MFMA", "16")


def _operands(omx, M, N, K, group, bits, seed):
    x = omx.ops.fill_uniform((M, K), seed, 1.0)
    w = omx.ops.fill_uniform((N, K), seed + 1, 0.05)
    q, s, b = omx.ops.quantize(w, group, bits)
    return x, q, s, b


@pytest.mark.parametrize("bits,group", FORMATS)
@pytest.mark.parametrize("M,N,K", [(17, 128, 128), (40, 128, 3072), (300, 3072, 3072), (512, 9216, 3072), (4608, 3072, 12288),
                                   (4608, 128, 3072)])
def test_plain_is_bit_equal_to_dequantize_then_bf16_gemm(omx, monkeypatch, M, N, K, bits, group):
    x, q, s, b = _operands(omx, M, N, K, group, bits, 11 + M)
    got = omx.ops.quantized_linear(x, q, s, b, group, bits).numpy()
    _pin_bf16_kernel(monkeypatch)
    ref = omx.ops.linear(x, omx.ops.dequantize(q, s, b, group, bits)).numpy()
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("bits,group", FORMATS)
@pytest.mark.parametrize("M,n_plain,half,K", [(17, 0, 256, 128), (300, 768, 388, 512), (512, 0, 9216, 3072)])
def test_swiglu_is_bit_equal_to_dequantize_then_bf16_swiglu(omx, monkeypatch, M, n_plain, half, K, bits, group):
    x, q, s, b = _operands(omx, M, n_plain + 2 * half, K, group, bits, 23 + M)
    plain, act = omx.ops.quantized_linear_swiglu(x, q, s, b, n_plain, group, bits)
    _pin_bf16_kernel(monkeypatch)
    rplain, ract = omx.ops.linear_swiglu(x, omx.ops.dequantize(q, s, b, group, bits), n_plain)
    assert np.abs(ract.numpy()).max() > 0
    np.testing.assert_array_equal(act.numpy(), ract.numpy())
    if n_plain:
        np.testing.assert_array_equal(plain.numpy(), rplain.numpy())


@pytest.mark.parametrize("bits,group", [(8, 64), (4, 64)])
def test_swiglu_single_block_width(omx, monkeypatch, bits, group):
    """The single block's to_qkv_mlp at real width and the 1024^2 sequence: n_plain = 3 * 3072, half = 9216, 4 608 rows."""
    M, n_plain, half, K = 4608, 3 * 3072, 9216, 3072
    x, q, s, b = _operands(omx, M, n_plain + 2 * half, K, group, bits, 5)
    plain, act = omx.ops.quantized_linear_swiglu(x, q, s, b, n_plain, group, bits)
    _pin_bf16_kernel(monkeypatch)
    rplain, ract = omx.ops.linear_swiglu(x, omx.ops.dequantize(q, s, b, group, bits), n_plain)
    np.testing.assert_array_equal(act.numpy(), ract.numpy())
    np.testing.assert_array_equal(plain.numpy(), rplain.numpy())


@pytest.mark.parametrize("bits,group", [(8, 64), (4, 32), (4, 128)])
@pytest.mark.parametrize("M,N,K", [(40, 132, 128), (300, 3072, 3072)])
def test_gated_form_against_float64(omx, M, N, K, bits, group):
    T = omx.ops.Tensor
    x, q, s, b = _operands(omx, M, N, K, group, bits, 31 + N)
    g = np.random.default_rng(M)
    resid = rc.bf16_round(g.standard_normal((M, N)).astype(np.float32))
    gate = rc.bf16_round(g.standard_normal(N).astype(np.float32))
    got = omx.ops.quantized_linear(x, q, s, b, group, bits, resid=T.from_numpy(resid), gate=T.from_numpy(gate)).numpy()
    xs = x.numpy().astype(np.float64)
    wd = rc.dequantize(q.numpy(), s.numpy(), b.numpy(), group, bits, "bf16").astype(np.float64)
    acc = xs @ wd.T
    ref = resid.astype(np.float64) + acc * gate.astype(np.float64)
    ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 7)
    f32 = K * 2.0 ** -23 * (np.abs(xs) @ np.abs(wd).T) * np.abs(gate) + 2.0 ** -23 * (np.abs(resid) + np.abs(acc * gate))
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= ulp + f32).all(), f"max excess {(err - ulp - f32).max()}"


def _quantized_dict(omx, weights, group, bits):
    """bf16 weights -> (the triplets on device by the internal names, the dequantised weights for the oracle)."""
    from ominix_mlx_amd import klein
    T = omx.ops.Tensor
    dev, deq = {}, {}
    for name, a in weights.items():
        if not klein.is_linear_weight(name):
            dev[name], deq[name] = a, a
            continue
        q, s, b = omx.ops.quantize(T.from_numpy(a), group, bits)
        base = name[:-len(".weight")]
        dev[name], dev[base + ".scales"], dev[base + ".biases"] = q, s, b
        deq[name] = rc.dequantize(q.numpy(), s.numpy(), b.numpy(), group, bits, "bf16")
    return dev, deq


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("s_txt,grid", [(16, (4, 6)), (70, (9, 9))])
def test_tiny_quantized_model_matches_the_oracle(omx, s_txt, grid, bits):
    from ominix_mlx_amd import klein
    T = omx.ops.Tensor
    group = 64
    p = rk.KleinParams.tiny()
    weights = rk.synth_weights(p)
    dev, deq = _quantized_dict(omx, weights, group, bits)
    g = np.random.default_rng(7)
    s_img = grid[0] * grid[1]
    latent = rc.bf16_round(g.standard_normal((s_img, p.in_channels)).astype(np.float32))
    txt = rc.bf16_round(g.standard_normal((s_txt, p.txt_embed_dim)).astype(np.float32))
    cos, sin = rk.compute_rope(np.concatenate([rk.create_txt_ids(s_txt), rk.create_img_ids(*grid)], 0))
    ref = rk.KleinOracle(p, deq).forward_with_rope(latent, txt, 750.0, cos, sin)

    args = (p.in_channels, p.hidden_size, p.txt_embed_dim, p.num_heads, p.depth, p.depth_single, p.head_dim, p.mlp_hidden)
    rcos, rsin = klein.compute_rope(klein.create_txt_ids(s_txt), klein.create_img_ids(*grid))
    m = klein.FluxKlein(*args)
    m.load_quantized_weights(dev, group, bits)
    out = m.forward_with_rope(T.from_numpy(latent), T.from_numpy(txt), 750.0, rcos, rsin).numpy()
    bound = 2.0 ** -6 * np.abs(ref).max() * np.sqrt(p.depth + p.depth_single)
    assert np.abs(out - ref).max() <= bound, f"max err {np.abs(out - ref).max():.4f} > {bound:.4f}"
    # from_unquantized on the same bf16 weights: the same triplets, the same bits
    m2 = klein.FluxKlein(*args)
    m2.load_weights(weights)
    m2.quantize(group, bits)
    out2 = m2.forward_with_rope(T.from_numpy(latent), T.from_numpy(txt), 750.0, rcos, rsin).numpy()
    np.testing.assert_array_equal(out, out2)


def _real_width_weights(omx, p, group, bits):
    """Device weights of one double + one single block at the real widths: bf16 draws, their triplets, the dequantised copies."""
    from ominix_mlx_amd import klein
    packed, deq = {}, {}
    for i, (name, shape) in enumerate(sorted(rk.weight_shapes(p).items())):
        if not klein.is_linear_weight(name):
            t = omx.ops.fill_uniform(shape, 1000 + i, 0.01, 1.0)
            packed[name] = deq[name] = t
            continue
        q, s, b = omx.ops.quantize(omx.ops.fill_uniform(shape, 1000 + i, 0.02 * np.sqrt(3)), group, bits)
        base = name[:-len(".weight")]
        packed[name], packed[base + ".scales"], packed[base + ".biases"] = q, s, b
        deq[name] = omx.ops.dequantize(q, s, b, group, bits)
    return packed, deq


@pytest.mark.parametrize("s_txt,grid", [(128, (16, 32)), (512, (64, 64))])
def test_real_widths_int8_against_bf16_and_schedules(omx, monkeypatch, s_txt, grid):
    from ominix_mlx_amd import klein
    group, bits = 64, 8
    p = rk.KleinParams(depth=1, depth_single=1)
    packed, deq = _real_width_weights(omx, p, group, bits)
    lat = omx.ops.fill_uniform((grid[0] * grid[1], 128), 1, 1.7)
    txt = omx.ops.fill_uniform((s_txt, 7680), 2, 1.7)
    rcos, rsin = klein.compute_rope(klein.create_txt_ids(s_txt), klein.create_img_ids(*grid))
    mb = klein.FluxKlein(depth=1, depth_single=1)
    mb.load_weights(deq)
    ref = mb.forward_with_rope(lat, txt, 500.0, rcos, rsin).numpy()
    mb.close()
    outs = {}
    for name, env in {"default": {}, "one_stream": {"OMX_KLEIN_DUAL_STREAM": "0"}, "swiglu_kernel": {"OMX_KLEIN_FUSE_SWIGLU": "0"}}.items():
        for k in ("OMX_KLEIN_DUAL_STREAM", "OMX_KLEIN_FUSE_SWIGLU"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = klein.FluxKlein(depth=1, depth_single=1)
        m.load_quantized_weights(packed, group, bits)
        outs[name] = m.forward_with_rope(lat, txt, 500.0, rcos, rsin).numpy()
        m.close()
    out = outs["default"]
    assert np.isfinite(out).all() and np.abs(out).max() > 0 and out.std() > 0
    bound = 2.0 ** -6 * np.abs(ref).max() * np.sqrt(2)
    assert np.abs(out - ref).max() <= bound, f"max err {np.abs(out - ref).max():.4f} > {bound:.4f}"
    np.testing.assert_array_equal(out, outs["one_stream"])
    np.testing.assert_array_equal(out, outs["swiglu_kernel"])


@pytest.mark.parametrize("bits,group", [(8, 64), (4, 32), (4, 128)])
def test_weight_bytes_accounting(omx, bits, group):
    from ominix_mlx_amd import klein
    p = rk.KleinParams.tiny()
    m = klein.FluxKlein(p.in_channels, p.hidden_size, p.txt_embed_dim, p.num_heads, p.depth, p.depth_single, p.head_dim, p.mlp_hidden)
    m.synth_weights()
    shapes = rk.weight_shapes(p)
    assert m.weight_bytes() == sum(int(np.prod(s)) * 2 for s in shapes.values())
    m.quantize(group, bits)
    want = 0
    for name, s in shapes.items():
        if klein.is_linear_weight(name):
            rows, cols = s
            want += rows * cols * bits // 8 + 2 * rows * (cols // group) * 2
        else:
            want += int(np.prod(s)) * 2
    assert m.weight_bytes() == want


def test_errors(omx):
    from ominix_mlx_amd import klein, lib
    T = omx.ops.Tensor
    x, q, s, b = _operands(omx, 20, 64, 256, 64, 8, 3)
    with pytest.raises(omx.OmxError):                                   # bits = 3
        omx.ops.quantized_linear(x, q, s, b, 64, 3)
    with pytest.raises(omx.OmxError, match="bits"):                     # ... at the C boundary too
        omx.check(lib.omx_quantized_linear_mfma(T((20, 64), "bf16").ptr, x.ptr, q.ptr, s.ptr, b.ptr, None, None, 20, 64, 256, 64, 3, None))
    with pytest.raises(omx.OmxError, match="group_size"):               # group = 48
        omx.ops.quantized_linear(x, q, s, b, 48, 8)
    x2, q2, s2, b2 = _operands(omx, 20, 64, 192, 64, 8, 4)
    with pytest.raises(omx.OmxError, match="multiple of group_size"):   # K % group != 0
        omx.ops.quantized_linear(x2, q2, s2, b2, 128, 8)
    p = rk.KleinParams.tiny()
    args = (p.in_channels, p.hidden_size, p.txt_embed_dim, p.num_heads, p.depth, p.depth_single, p.head_dim, p.mlp_hidden)
    m = klein.FluxKlein(*args)
    wq, ws, wb = omx.ops.quantize(omx.ops.fill_uniform((256, 128), 9, 0.05), 64, 8)
    with pytest.raises(omx.OmxError, match="do not form"):              # scales of another matrix
        m.load_quantized_weights({"x_embedder.weight": wq, "x_embedder.scales": s, "x_embedder.biases": wb}, 64, 8)
    with pytest.raises(omx.OmxError, match="bits"):
        omx.check(lib.omx_klein_set_quantized_weight(m._h, b"x_embedder.weight", wq.ptr, ws.ptr, wb.ptr, 256, 128, 64, 3))
    with pytest.raises(omx.OmxError, match="group_size"):
        omx.check(lib.omx_klein_set_quantized_weight(m._h, b"x_embedder.weight", wq.ptr, ws.ptr, wb.ptr, 256, 128, 48, 8))
    m.close()
    tp = klein.FluxKlein(*args, tp_rank=0, tp_size=2)
    tp.synth_weights()
    with pytest.raises(omx.OmxError, match="tensor parallelism"):
        tp.quantize(64, 8)
    tp.close()


def test_quantize_after_a_mixed_load_keeps_the_loaded_triplets(omx):
    """A model loaded with some Linears packed and the rest bf16, then quantize(): the packed triplets this object uploaded are still
    read by the forward, so they must stay referenced; the result equals the model loaded fully packed."""
    import gc
    from ominix_mlx_amd import klein
    T = omx.ops.Tensor
    group, bits = 64, 8
    p = rk.KleinParams.tiny()
    weights = rk.synth_weights(p)
    dev, _ = _quantized_dict(omx, weights, group, bits)
    host = {n: t.numpy() if isinstance(t, T) else t for n, t in dev.items()}   # numpy: the model uploads (and owns) every tensor
    packed_names = [n for n in weights if klein.is_linear_weight(n) and not n.startswith("double_blocks.")]
    mixed = {}
    for n, a in weights.items():
        if n in packed_names:
            base = n[:-len(".weight")]
            mixed[n], mixed[base + ".scales"], mixed[base + ".biases"] = host[n], host[base + ".scales"], host[base + ".biases"]
        else:
            mixed[n] = a
    args = (p.in_channels, p.hidden_size, p.txt_embed_dim, p.num_heads, p.depth, p.depth_single, p.head_dim, p.mlp_hidden)
    m = klein.FluxKlein(*args)
    m.load_quantized_weights(mixed, group, bits)
    m.quantize(group, bits)
    gc.collect()
    for n in packed_names:
        kind, tensors = m._keep_of[n]
        assert kind == "packed" and all(any(t is k for k in m._keep) for t in tensors), n
    assert not any(kind == "bf16" and klein.is_linear_weight(n) for n, (kind, _) in m._keep_of.items())
    ref = klein.FluxKlein(*args)
    ref.load_quantized_weights(host, group, bits)
    assert m.weight_bytes() == ref.weight_bytes()
    g = np.random.default_rng(3)
    s_txt, grid = 16, (4, 6)
    latent = T.from_numpy(rc.bf16_round(g.standard_normal((grid[0] * grid[1], p.in_channels)).astype(np.float32)))
    txt = T.from_numpy(rc.bf16_round(g.standard_normal((s_txt, p.txt_embed_dim)).astype(np.float32)))
    rcos, rsin = klein.compute_rope(klein.create_txt_ids(s_txt), klein.create_img_ids(*grid))
    out = m.forward_with_rope(latent, txt, 750.0, rcos, rsin).numpy()
    want = ref.forward_with_rope(latent, txt, 750.0, rcos, rsin).numpy()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    np.testing.assert_array_equal(out, want)


def test_load_quantized_weights_rejects_malformed_input(omx):
    from ominix_mlx_amd import klein
    p = rk.KleinParams.tiny()
    m = klein.FluxKlein(p.in_channels, p.hidden_size, p.txt_embed_dim, p.num_heads, p.depth, p.depth_single, p.head_dim, p.mlp_hidden)
    wq, ws, wb = omx.ops.quantize(omx.ops.fill_uniform((256, 128), 9, 0.05), 64, 8)
    with pytest.raises(omx.OmxError, match="expected a `.weight`"):
        m.load_quantized_weights({"x_embedder.w": wq}, 64, 8)
    with pytest.raises(omx.OmxError, match="no `.weight` beside it"):
        m.load_quantized_weights({"x_embedder.scales": ws, "x_embedder.biases": wb}, 64, 8)
    with pytest.raises(omx.OmxError, match="uint32"):                   # float values where packed words belong
        m.load_quantized_weights({"x_embedder.weight": wq.numpy().astype(np.float32), "x_embedder.scales": ws, "x_embedder.biases": wb}, 64, 8)
    with pytest.raises(omx.OmxError, match="device tensor of dtype"):   # a bf16 device tensor where packed words belong
        m.load_quantized_weights({"x_embedder.weight": omx.ops.fill_uniform((256, 32), 1, 1.0), "x_embedder.scales": ws,
                                  "x_embedder.biases": wb}, 64, 8)
    m.close()
