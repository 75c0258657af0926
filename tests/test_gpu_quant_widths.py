"""MLX's 2 / 3 / 5 / 6-bit affine checkpoints on the device: quantize, dequantize, the packed decode GEMV in every fused form, gather_qmm,
the mlx-c handle layer, the Qwen3 engine (prompt pass, hipGraph decode step, loader, float16 triplets) and the drop-in route.

The oracle packs only widths that divide 32, so the reference of a b-bit model is its 8-bit RE-PACK: the same q (it fits in b bits), the
same bf16 scales and biases, packed at 8 bits, dequantise to the same values -- Qwen3Oracle(cfg, w8, quant=(8, group)) is then exact for
the b-bit model, and every dequantising path must give the b-bit and the 8-bit form bit for bit the same result."""
import numpy as np
import pytest

from oracle import ref_core as rc, ref_qwen3 as rq, synth
from test_gpu_primitives import assert_bf16_close, rand
from test_quant_widths import dequantize_any, pack_bits, quantize_any, unpack_bits

pytestmark = pytest.mark.gpu

NEW = [2, 3, 5, 6]


def _triplet(w, group, bits, sdt="bf16"):
    """(q, scales, biases) at `bits` with the scales / biases rounded to `sdt` -- the form an MLX checkpoint stores."""
    q, s, b = quantize_any(w, group, bits)
    return q, rc.rnd(s, sdt).astype(np.float32), rc.rnd(b, sdt).astype(np.float32)


def _dev(T, a, dt):
    return T.from_numpy(np.ascontiguousarray(a), dt)


# ---- 1. quantize / dequantize ----

@pytest.mark.parametrize("bits", [3, 5, 6])
@pytest.mark.parametrize("group", [32, 64, 128])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_quantize_matches_numpy(omx, bits, group, dtype):
    T = omx.ops.Tensor
    w = rc.rnd(rand((64, 512), 1000 + bits * 7 + group) * 0.3, dtype).astype(np.float32) if dtype != "f32" else rand((64, 512), 1000 + bits + group)
    pq, s, b = omx.ops.quantize(T.from_numpy(w, dtype), group, bits)
    assert pq.shape == (64, 512 * bits // 32) and s.shape == (64, 512 // group)
    q, rs, rb = quantize_any(w, group, bits)
    want_s, want_b = (rs, rb) if dtype == "f32" else (rc.rnd(rs, dtype), rc.rnd(rb, dtype))
    np.testing.assert_array_equal(s.numpy(), want_s)
    np.testing.assert_array_equal(b.numpy(), want_b)
    got = unpack_bits(pq.numpy(), bits).astype(np.int64)
    diff = got != q.astype(np.int64)
    assert diff.mean() <= 1e-3 and (np.abs(got - q.astype(np.int64))[diff] == 1).all()


@pytest.mark.parametrize("bits", [3, 5, 6])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_reference_bound_kat_at_the_new_widths(omx, bits, dtype):
    """mlx-rs ops/quantization.rs:289-305 at 3 / 5 / 6 bits: ones[128, 1] * arange(512), group 128, max |x - x_hat| <= 127 / 2^bits."""
    T = omx.ops.Tensor
    x = np.tile(np.arange(512, dtype=np.float32), (128, 1))
    if dtype != "f32":
        x = rc.rnd(x, dtype).astype(np.float32)
    pq, s, b = omx.ops.quantize(T.from_numpy(x, dtype), 128, bits)
    assert pq.shape == (128, 512 * bits // 32) and s.shape == (128, 4)
    x_hat = omx.ops.dequantize(pq, s, b, 128, bits).numpy()
    slack = 0.0 if dtype == "f32" else 512 * (2.0 ** -8 if dtype == "bf16" else 2.0 ** -11)
    assert np.abs(x - x_hat).max() <= 127.0 / (1 << bits) + slack


@pytest.mark.parametrize("bits", NEW)
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_dequantize_is_exact_and_equals_the_8bit_repack(omx, bits, dtype):
    T = omx.ops.Tensor
    group = 64
    q, s, b = _triplet(rand((40, 1536), 1100 + bits) * 0.2, group, bits, dtype)
    got = omx.ops.dequantize(_dev(T, pack_bits(q, bits), "u32"), _dev(T, s, dtype), _dev(T, b, dtype), group, bits).numpy()
    np.testing.assert_array_equal(got, dequantize_any(q, s, b, group, dtype))
    # 1a: the same q packed at 8 bits -> the same bits
    got8 = omx.ops.dequantize(_dev(T, pack_bits(q, 8), "u32"), _dev(T, s, dtype), _dev(T, b, dtype), group, 8).numpy()
    np.testing.assert_array_equal(got, got8)


@pytest.mark.parametrize("bits", NEW)
def test_prompt_sized_matmul_equals_the_8bit_repack(omx, bits):
    """M > 16: dequantise into the workspace + the bf16 GEMM -- the same W as the 8-bit re-pack, so the same result bit for bit."""
    T = omx.ops.Tensor
    q, s, b = _triplet(rand((384, 1536), 1200 + bits) * 0.05, 64, bits)
    x = _dev(T, rc.bf16_round(rand((40, 1536), 1201)), "bf16")
    got = omx.ops.quantized_matmul(x, _dev(T, pack_bits(q, bits), "u32"), _dev(T, s, "bf16"), _dev(T, b, "bf16"), 64, bits).numpy()
    want = omx.ops.quantized_matmul(x, _dev(T, pack_bits(q, 8), "u32"), _dev(T, s, "bf16"), _dev(T, b, "bf16"), 64, 8).numpy()
    np.testing.assert_array_equal(got, want)


# ---- 2. quantized_matmul against numpy ----

@pytest.mark.parametrize("bits", NEW)
@pytest.mark.parametrize("K", [512, 1536, 4096, 14336])
@pytest.mark.parametrize("M", [1, 5, 16, 40])
def test_quantized_matmul_matches_numpy(omx, M, K, bits):
    T = omx.ops.Tensor
    N, group = 192, 64 if K != 1536 else 32
    q, s, b = _triplet(rand((N, K), 1300 + K + bits) * 0.05, group, bits)
    x = rc.bf16_round(rand((M, K), 1301 + M))
    got = omx.ops.quantized_matmul(_dev(T, x, "bf16"), _dev(T, pack_bits(q, bits), "u32"), _dev(T, s, "bf16"), _dev(T, b, "bf16"),
                                   group, bits).numpy().astype(np.float64)
    w = dequantize_any(q, s, b, group, "f32").astype(np.float64)
    ref = x.astype(np.float64) @ w.T
    noise = 4 * 2.0 ** -9 * np.sqrt((x.astype(np.float64) ** 2) @ (w ** 2).T)
    assert got.shape == ref.shape
    assert (np.abs(got - ref) <= np.abs(ref) * 2.0 ** -7 + noise + 1e-6).all()


@pytest.mark.parametrize("M", [1, 40])
def test_quantized_matmul_with_float16_triplets(omx, M):
    T = omx.ops.Tensor
    N, K, group, bits = 256, 4096, 64, 6
    q, s, b = _triplet(rc.rnd(rand((N, K), 1400) * 0.1, "f16"), group, bits, "f16")
    x = rc.rnd(rand((M, K), 1401), "f16").astype(np.float32)
    got_t = omx.ops.quantized_matmul(_dev(T, x, "f16"), _dev(T, pack_bits(q, bits), "u32"), _dev(T, s.astype(np.float16), "f16"),
                                     _dev(T, b.astype(np.float16), "f16"), group, bits)
    assert got_t.dtype == omx.ops.dtype_code("f16")
    w = dequantize_any(q, s, b, group, "f16").astype(np.float64)
    ref = x.astype(np.float64) @ w.T
    noise = 4 * 2.0 ** -12 * np.sqrt((x.astype(np.float64) ** 2) @ (w ** 2).T)
    assert (np.abs(got_t.numpy().astype(np.float64) - ref) <= 2.0 ** -10 * np.abs(ref) + noise + 1e-6).all()


# ---- 3. the fused decode-step forms (omx_debug_qgemv: what engine.hip launches) ----

from test_gpu_quant import EPI_ARGMAX, EPI_F32, EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU, PRO_NONE, PRO_RMSNORM, _bind_debug   # noqa: E402


@pytest.mark.parametrize("bits", [3, 6])
@pytest.mark.parametrize("N,K,pro,epi,single,stack", [
    (1536, 1536, PRO_RMSNORM, EPI_STORE, 0, 1024),      # q | k+v stacked: two members, the 24-chunk row masks 40 lanes
    (1536, 4096, PRO_RMSNORM, EPI_STORE, 0, 1024),
    (1000, 1536, PRO_NONE, EPI_RESIDUAL, 0, 0),         # ragged N
    (1024, 4096, PRO_NONE, EPI_RESIDUAL, 0, 0),
    (768, 1536, PRO_RMSNORM, EPI_SWIGLU, 0, 0),         # gate / up, nn::silu(g) * u roundings
    (768, 4096, PRO_NONE, EPI_SWIGLU, 1, 0),            # ... fused_swiglu's single rounding
    (520, 4096, PRO_NONE, EPI_F32, 0, 0),               # unrounded f32 row sums
    (20000, 1536, PRO_RMSNORM, EPI_ARGMAX, 0, 0),       # logits + argmax partials
    (20000, 4096, PRO_RMSNORM, EPI_ARGMAX, 0, 0),
])
def test_fused_packed_gemv_forms_match_numpy(omx, bits, N, K, pro, epi, single, stack):
    lib = _bind_debug(omx)
    T = omx.ops.Tensor
    group = 64
    seed = 1500 + N % 97 + epi + bits
    x = rc.bf16_round(rand((1, K), seed))
    nw = rc.bf16_round(1.0 + 0.1 * rand((K,), seed + 1))
    resid = rc.bf16_round(rand((N,), seed + 2))
    mats = [_triplet(rand((N, K), seed + 3 + j) * 0.05, group, bits) for j in range(2 if epi == EPI_SWIGLU else 1)]
    xin = rc.rms_norm(x, nw, 1e-6, "bf16") if pro == PRO_RMSNORM else x
    wd = [dequantize_any(m[0], m[1], m[2], group, "f32").astype(np.float64) for m in mats]
    ys = [(xin.astype(np.float64) @ w_.T)[0] for w_ in wd]
    noise = [4 * 2.0 ** -9 * np.sqrt((xin.astype(np.float64) ** 2) @ (w_ ** 2).T)[0] for w_ in wd]

    def up(q, s, b):
        return _dev(T, pack_bits(q, bits), "u32"), _dev(T, s, "bf16"), _dev(T, b, "bf16")
    if stack:
        q_, s_, b_ = mats[0]
        dev = [up(q_[:stack], s_[:stack], b_[:stack]), up(q_[stack:], s_[stack:], b_[stack:])]
    else:
        dev = [up(*m) for m in mats]
    xd, nwd, rd = T.from_numpy(x), T.from_numpy(nw), T.from_numpy(resid)
    out = T.from_numpy(np.zeros((N,), np.float32))
    out32 = T.from_numpy(np.zeros((N,), np.float32), "f32")
    nslot = lib.omx_debug_qgemv_grid(N)
    slots = T.from_numpy(np.zeros((2 * nslot,), np.uint32), "u32")
    second = dev[1] if len(dev) > 1 else (None, None, None)
    omx.check(lib.omx_debug_qgemv(out.ptr, out32.ptr, slots.ptr, xd.ptr, nwd.ptr, rd.ptr, dev[0][0].ptr, dev[0][1].ptr, dev[0][2].ptr,
                                  second[0].ptr if second[0] else None, second[1].ptr if second[1] else None,
                                  second[2].ptr if second[2] else None, stack, N, K, group, bits, pro, epi, 1e-6, single, None))
    omx.check(omx.lib.omx_synchronize(None))
    got16 = out.numpy().astype(np.float64)
    ulp = 2.0 ** -7
    if epi == EPI_F32:
        assert (np.abs(out32.numpy().astype(np.float64) - ys[0]) <= noise[0] + 1e-6).all()
    elif epi == EPI_STORE:
        assert (np.abs(got16 - ys[0]) <= np.abs(ys[0]) * ulp + noise[0] + 1e-6).all()
    elif epi == EPI_RESIDUAL:
        ref = resid.astype(np.float64) + ys[0]
        assert (np.abs(got16 - ref) <= (np.abs(ref) + np.abs(ys[0])) * ulp + noise[0] + 1e-6).all()
    elif epi == EPI_SWIGLU:
        g, u = ys
        sg = 1.0 / (1.0 + np.exp(-g))
        ref = g * sg * u
        tol = np.abs(ref) * 4 * ulp + 1.1 * (noise[0] + np.abs(g) * ulp) * np.abs(u) + (noise[1] + np.abs(u) * ulp) * np.abs(g * sg) + 1e-6
        assert (np.abs(got16 - ref) <= tol).all()
    else:
        assert (np.abs(got16 - ys[0]) <= np.abs(ys[0]) * ulp + noise[0] + 1e-6).all()
        best = int(slots.numpy().view(np.uint64)[:nslot].max())
        idx = (~best) & 0xFFFFFFFF
        assert idx == int(np.argmax(got16))


# ---- 4. gather_qmm, 5. the mlx-c handle layer ----

def test_gather_qmm_selects_the_expert_per_row_at_6_bits(omx):
    T = omx.ops.Tensor
    E, N, K, n, k, group, bits = 4, 256, 1536, 3, 2, 64, 6
    ts = [_triplet(rand((N, K), 1600 + e) * 0.05, group, bits) for e in range(E)]
    pq = np.stack([pack_bits(t[0], bits) for t in ts])
    s, b = np.stack([t[1] for t in ts]), np.stack([t[2] for t in ts])
    x = rc.bf16_round(rand((n, K), 1610))
    inds = np.array([[0, 3], [2, 2], [1, 0]], np.uint32)
    got = omx.ops.gather_qmm(_dev(T, x, "bf16"), _dev(T, pq, "u32"), _dev(T, s, "bf16"), _dev(T, b, "bf16"),
                             T.from_numpy(inds.reshape(-1), "u32"), x_div=k, group_size=group, bits=bits).numpy().reshape(n, k, N)
    for t in range(n):
        for j in range(k):
            e = int(inds[t, j])
            ref = (x[t].astype(np.float64) @ dequantize_any(ts[e][0], ts[e][1], ts[e][2], group, "f32").astype(np.float64).T)
            assert_bf16_close(got[t, j], ref, 1, atol=2.0 ** -8 * np.abs(ref).max())


@pytest.mark.parametrize("bits", [3, 6])
def test_mlx_c_entry_points_at_the_new_widths(omx, bits):
    from ominix_mlx_amd import mlx_c as mx
    w = rc.bf16_round(rand((128, 1024), 1700 + bits) * 0.1)
    x = rc.bf16_round(rand((1, 1024), 1701))
    wq, s, b = mx.quantize(mx.Array.from_numpy(w), group_size=64, bits=bits)
    assert wq.shape == (128, 1024 * bits // 32) and s.shape == (128, 16) and wq.dtype == mx.UINT32
    q = unpack_bits(wq.numpy(), bits)
    w_hat = mx.dequantize(wq, s, b, group_size=64, bits=bits).numpy()
    np.testing.assert_array_equal(w_hat, dequantize_any(q, s.numpy(), b.numpy(), 64, "bf16"))
    g = w.reshape(128, -1, 64)   # the reference's bound (quantization.rs:289-305): max |x - x_hat| <= range / 2^bits per group
    assert (np.abs(w_hat - w) <= np.repeat(g.max(-1) - g.min(-1), 64, axis=-1) / (1 << bits) + np.abs(w) * 2.0 ** -7 + 1e-6).all()
    y = mx.quantized_matmul(mx.Array.from_numpy(x), wq, s, b, group_size=64, bits=bits).numpy()
    ref = x.astype(np.float64) @ dequantize_any(q, s.numpy(), b.numpy(), 64, "f32").astype(np.float64).T
    assert_bf16_close(y, ref, 1, atol=2.0 ** -8 * np.abs(ref).max())


# ---- 6. / 7. the engine ----

CONFIGS = {
    "gqa2_d64": rq.Qwen3Config(512, 2, 1536, 8, 4, 64, 2048, 1e-6, 1e6, False),
    "gqa4_d128": rq.Qwen3Config(1024, 3, 3072, 8, 2, 128, 4096, 1e-6, 1e6, True),
}


def _checkpoints(cfg, bits, group, sdt="bf16"):
    """(b-bit checkpoint, its 8-bit re-pack): the same q, scales and biases."""
    wb, w8 = {}, {}
    for name, w in rq.synth_weights(cfg).items():
        prefix = name[:-len(".weight")]
        if prefix.endswith(rq.QUANTIZED) or prefix in ("model.embed_tokens", "lm_head"):
            q, s, b = _triplet(w, group, bits, sdt)
            for d, pb in ((wb, bits), (w8, 8)):
                d[prefix + ".weight"] = pack_bits(q, pb)
                d[prefix + ".scales"], d[prefix + ".biases"] = (s, b) if sdt == "bf16" else (s.astype(np.float16), b.astype(np.float16))
        else:
            wb[name] = w8[name] = w
    return wb, w8


def _model(cfg, quant, max_context=256):
    from ominix_mlx_amd import engine
    return engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                        num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                        vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                        tie_word_embeddings=cfg.tie_word_embeddings, max_context=max_context, quantization=quant)


def _hold_to_oracle(got, logits0, ref_tokens, ref_logits, layers):
    """test_quantized_checkpoint_decode_matches_oracle's rule: first logits within the bound, tokens equal up to a near-tie."""
    bound = 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(2 * layers)
    assert np.abs(logits0 - ref_logits[0]).max() <= bound
    margins = rc.argmax_margin(ref_logits)
    for i in range(len(got)):
        if got[i] != ref_tokens[i]:
            assert margins[i] <= 2 * bound, f"token {i}: got {got[i]} want {ref_tokens[i]} with margin {margins[i]:.4f} > {2*bound:.4f}"
            break


@pytest.mark.parametrize("name", ["gqa4_d128", "gqa2_d64"])
@pytest.mark.parametrize("bits,group", [(2, 64), (3, 32), (3, 64), (5, 64), (6, 64), (6, 128)])
def test_engine_decode_matches_the_8bit_repack_oracle(omx, name, bits, group):
    cfg = CONFIGS[name]
    wb, w8 = _checkpoints(cfg, bits, group)
    oracle = rq.Qwen3Oracle(cfg, w8, quant=(8, group))
    n_prompt, n_new = 48, 10
    prompt = synth.prompt_ids(n_prompt, cfg.vocab_size)
    ref_tokens, ref_logits = oracle.generate(prompt, n_new, return_logits=True)
    outs = []
    for upload in (True, False):
        m = _model(cfg, {"bits": bits, "group_size": group})
        m.load_weights(wb) if upload else m.synth_weights()
        first = m.prefill(prompt)
        logits0 = m.last_logits()
        got = np.concatenate([[first], m.decode(n_new - 1)]).astype(np.uint32)
        assert m.decode_path() == "graph"
        outs.append((got, logits0))
        m.close()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    _hold_to_oracle(outs[0][0], outs[0][1], ref_tokens, ref_logits, cfg.num_hidden_layers)


def test_engine_with_float16_triplets_at_6_bits(omx):
    """A float16 checkpoint (scales / biases float16: the model runs in float16) at 6 bits against the same q re-packed at 8 bits on the
    engine: the 8-bit engine is pinned to the oracle by test_gpu_qwen3.py; the two differ only in the packed GEMV's unpacking."""
    cfg = CONFIGS["gqa4_d128"]
    wb, w8 = _checkpoints(cfg, 6, 64, "f16")
    prompt = synth.prompt_ids(40, cfg.vocab_size)
    res = []
    for w, bits in ((wb, 6), (w8, 8)):
        m = _model(cfg, {"bits": bits, "group_size": 64, "scales_dtype": "float16"})
        m.load_weights(w)
        first = m.prefill(prompt)
        logits0 = m.last_logits()
        res.append((np.concatenate([[first], m.decode(7)]).astype(np.uint32), logits0, m.decode_path()))
        m.close()
    (tb, lb, pb), (t8, l8, _) = res
    assert pb == "graph"
    assert np.isfinite(lb).all()
    assert np.abs(lb - l8).max() <= 2.0 ** -10 * np.abs(l8).max() * np.sqrt(2 * cfg.num_hidden_layers)
    n = 0
    while n < len(tb) and tb[n] == t8[n]:
        n += 1
    assert n >= 4, (tb, t8)


@pytest.mark.parametrize("sdt", ["bfloat16", "float16"])
def test_load_model_from_a_6bit_checkpoint_directory(omx, tmp_path, sdt):
    import json
    from ominix_mlx_amd import loader
    cfg = CONFIGS["gqa4_d128"]
    w, _ = _checkpoints(cfg, 6, 64, "bf16" if sdt == "bfloat16" else "f16")
    d = str(tmp_path)
    json.dump({"hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_hidden_layers, "intermediate_size": cfg.intermediate_size,
               "num_attention_heads": cfg.num_attention_heads, "num_key_value_heads": cfg.num_key_value_heads, "head_dim": cfg.head_dim,
               "vocab_size": cfg.vocab_size, "rms_norm_eps": cfg.rms_norm_eps, "rope_theta": cfg.rope_theta,
               "tie_word_embeddings": cfg.tie_word_embeddings, "quantization": {"bits": 6, "group_size": 64}},
              open(f"{d}/config.json", "w"))
    names = sorted(w)
    shards = {"model-00001-of-00002.safetensors": names[: len(names) // 2], "model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for fn, keys in shards.items():
        raw = lambda k: w[k].dtype in (np.uint32, np.float16)
        tensors = {k: (w[k] if raw(k) else rc.to_bf16_bits(w[k])) for k in keys}
        loader.write_safetensors(f"{d}/{fn}", tensors, bf16_names=tuple(k for k in keys if not raw(k)))
    json.dump({"metadata": {}, "weight_map": {k: fn for fn, keys in shards.items() for k in keys}}, open(f"{d}/model.safetensors.index.json", "w"))
    prompt = synth.prompt_ids(20, cfg.vocab_size)
    m = loader.load_model(d, max_context=256)
    got = np.concatenate([[m.prefill(prompt)], m.decode(6)])
    logits = m.last_logits()
    m.close()
    ref = _model(cfg, {"bits": 6, "group_size": 64, "scales_dtype": sdt})
    ref.load_weights(w)
    want = np.concatenate([[ref.prefill(prompt)], ref.decode(6)])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(logits, ref.last_logits())
    ref.close()


# ---- 8. the drop-in route ----

def test_drop_in_route_on_a_6bit_checkpoint(omx):
    """test_gpu_mlx_lazy.py::test_drop_in_route_on_a_quantized_checkpoint's 8-bit check at 6 bits: the VALU kernel in every mode."""
    from ominix_mlx_amd import engine, mlx_c as mx
    cfg = dict(hidden_size=1024, num_hidden_layers=2, intermediate_size=2048, num_attention_heads=8, num_key_value_heads=4, head_dim=128,
               vocab_size=2048, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False)
    m = engine.Model(max_context=512, quantization={"bits": 6, "group_size": 64}, **cfg)
    m.synth_weights()
    prompt = synth.prompt_ids(100, cfg["vocab_size"])
    want = [int(m.prefill(prompt))] + [int(t) for t in m.decode(60)]
    runs = {}
    try:
        for name, (lazy, fuse) in {"eager": (False, False), "recorded": (True, False), "fused": (True, True)}.items():
            mx.lazy_mode(lazy, fuse)
            s0 = mx.lazy_stats()
            runs[name] = ([int(t) for t in m.per_op_route(prompt, 60)["tokens"]], s0, mx.lazy_stats())
    finally:
        mx.lazy_mode(True, True)
    assert runs["eager"][0] == runs["recorded"][0]
    assert runs["fused"][0] == runs["eager"][0]
    assert runs["fused"][0][:24] == want[:24]
    _, s0, s1 = runs["fused"]
    assert s1["fused_launches"] - s0["fused_launches"] >= 5 * cfg["num_hidden_layers"] * 60
    m.close()


# ---- 9. refusals ----

def test_widths_outside_the_set_are_refused(omx):
    from ominix_mlx_amd import mlx_c as mx
    T = omx.ops.Tensor
    w = T.from_numpy(rc.bf16_round(rand((16, 512), 1800)))
    with pytest.raises(omx.OmxError, match="bits"):
        omx.ops.quantize(w, 64, 7)
    pq = T.from_numpy(np.zeros((16, 112), np.uint32), "u32")   # 512 * 7 / 32 words
    sb = T.from_numpy(np.zeros((16, 8), np.float32))
    with pytest.raises(omx.OmxError, match="bits"):
        omx.ops.dequantize(pq, sb, sb, 64, 7)
    x = T.from_numpy(rc.bf16_round(rand((1, 512), 1801)))
    with pytest.raises(omx.OmxError, match="bits"):
        omx.ops.quantized_matmul(x, pq, sb, sb, 64, 7)
    pq3 = T.from_numpy(np.zeros((2, 16, 112), np.uint32), "u32")
    sb3 = T.from_numpy(np.zeros((2, 16, 8), np.float32))
    with pytest.raises(omx.OmxError, match="bits"):
        omx.ops.gather_qmm(x, pq3, sb3, sb3, T.from_numpy(np.zeros((1,), np.uint32), "u32"), group_size=64, bits=7)
    with pytest.raises(omx.OmxError, match="bits"):
        mx.quantize(mx.Array.from_numpy(rc.bf16_round(rand((16, 512), 1802))), group_size=64, bits=7)
    cfg = CONFIGS["gqa2_d64"]
    with pytest.raises(omx.OmxError, match="InvalidConfig.*bits"):
        _model(cfg, {"bits": 7, "group_size": 64})


@pytest.mark.parametrize("bits", NEW)
def test_new_widths_refuse_experts_and_tensor_parallelism(omx, bits):
    from ominix_mlx_amd import engine
    base = dict(hidden_size=512, num_hidden_layers=2, intermediate_size=1536, num_attention_heads=8, num_key_value_heads=4, head_dim=64,
                vocab_size=2048, max_context=256, quantization={"bits": bits, "group_size": 64})
    with pytest.raises(omx.OmxError, match=f"InvalidConfig: {bits}-bit"):
        engine.Model(**base, num_experts=4, num_experts_per_tok=2, moe_intermediate_size=512)
    with pytest.raises(omx.OmxError, match=f"InvalidConfig: {bits}-bit"):
        engine.Model(**base, tp_size=2)
