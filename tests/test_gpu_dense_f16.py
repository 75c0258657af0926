"""GPU: dense float16 checkpoints -- the decode GEMV's float16 form (csrc/gemv.hip, omx_debug_gemv), omx_linear / mlx_matmul /
mlx_addmm in float16 at decode sizes, and the Qwen3 engine with float16_weights against the float16 oracle."""
import ctypes
import json
import zlib

import numpy as np
import pytest

from oracle import ref_core as rc
from oracle import ref_decode as rd
from oracle import ref_qwen3 as rq
from oracle import synth

pytestmark = pytest.mark.gpu

PRO_NONE, PRO_RMSNORM = 0, 1
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU, EPI_ARGMAX = 0, 1, 2, 3
EPS = 1e-6
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib(omx):
    from ominix_mlx_amd import engine   # (its binding table declares omx_debug_gemv)
    assert "omx_debug_gemv" in engine.ENGINE_SIGNATURES
    return omx.lib


def ulp16(v):
    """float16 ulp at |v| (subnormal spacing 2^-24 below 2^-14)."""
    return rd.ulp16(v, "f16")


def f16(v):
    return rd.rnd(v, "f16")


def rand_f16(rng, shape, lo_exp=8, hi_exp=14):
    """float16 values with random sign / mantissa and exponent field in [lo_exp, hi_exp] (|v| in [2^(lo-15), 2^(hi-14)))."""
    u = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    e = (lo_exp + (u >> np.uint16(10)) % np.uint16(hi_exp - lo_exp + 1)).astype(np.uint16)
    bits = (u & np.uint16(0x83FF)) | (e << np.uint16(10))
    return bits.view(np.float16)


rows_dot = rd.rows_dot   # exact W @ x and sum |W| |x| per row (oracle/ref_decode.py, shared with the bf16 GEMV tests)


def rmsnorm_f16(x, nw):
    """the kernel's prologue: f32 sum of squares, rstd = 1/sqrt(ss/K + eps), xn = f16((x * rstd) * w) in f32 arithmetic"""
    return rd.rmsnorm16(x, nw, EPS, "f16").astype(np.float16)


def run_gemv(omx, lib, mats, x, pro, epi, nw=None, resid=None, bias=None, single_round=0):
    from ominix_mlx_amd.ops import Tensor
    N = mats[0].shape[0] if epi == EPI_SWIGLU else sum(m.shape[0] for m in mats)
    K = x.size
    dw = [Tensor.from_numpy(m, "f16") for m in mats]
    dx = Tensor.from_numpy(x, "f16")
    dn = Tensor.from_numpy(nw, "f16") if nw is not None else None
    dr = Tensor.from_numpy(resid, "f16") if resid is not None else None
    db = Tensor.from_numpy(bias, "f16") if bias is not None else None
    out = Tensor((N,), "f16")
    nslot = lib.omx_debug_gemv_grid(N, K)
    slots = Tensor((nslot * 2,), "u32")
    p = lambda t: t.ptr if t is not None else None
    n0 = mats[0].shape[0]
    n1 = mats[1].shape[0] if len(mats) > 2 else 0
    omx.check(lib.omx_debug_gemv(out.ptr, slots.ptr, dx.ptr, p(dn), p(dr), p(db), dw[0].ptr, dw[1].ptr if len(dw) > 1 else None,
                                 dw[2].ptr if len(dw) > 2 else None, n0, n1, N, K, pro, epi, 1, EPS, single_round, None))
    got = out.numpy().astype(np.float64)
    keys = slots.numpy().view(np.uint64)
    return got, keys


def check_plain(got, exact, mag, K, extra=0.0):
    """|got - f16(exact)| <= 1/2 ulp_f16 + the f32 accumulation bound K 2^-24 sum|x w| (+ the prologue's rounding flips)"""
    rd.check_plain(got, exact, mag, K, extra, "f16")


def flip_slack(W, xn):
    """RMSNorm output rounding may flip a few float16 roundings of xn against the host's f32 rstd: 4 flips of the widest ulp"""
    return rd.flip_slack(W, xn, "f16")


SHAPES = {   # Qwen3-8B decode widths, plus shapes that take the generic kernel (K not a multiple of 512 with a prologue) or a tail
    # name: (prologue, epilogue, member rows, K, swiglu_single_round)
    "qkv": (PRO_RMSNORM, EPI_STORE, (4096, 1024, 1024), 4096, 0),
    "o": (PRO_NONE, EPI_RESIDUAL, (4096,), 4096, 0),
    "gate_up": (PRO_RMSNORM, EPI_SWIGLU, (12288, 12288), 4096, 0),
    "gate_up_fused": (PRO_RMSNORM, EPI_SWIGLU, (12288, 12288), 4096, 1),
    "down": (PRO_NONE, EPI_RESIDUAL, (4096,), 12288, 0),
    "lm_head": (PRO_RMSNORM, EPI_ARGMAX, (151936,), 4096, 0),
    "generic_store": (PRO_RMSNORM, EPI_STORE, (300,), 1000, 0),
    "tail_k1000": (PRO_NONE, EPI_STORE, (300,), 1000, 0),
    "generic_residual": (PRO_NONE, EPI_RESIDUAL, (300,), 1000, 0),
    "generic_swiglu": (PRO_RMSNORM, EPI_SWIGLU, (300, 300), 1000, 0),
    "generic_swiglu_fused": (PRO_RMSNORM, EPI_SWIGLU, (300, 300), 1000, 1),
    "generic_argmax": (PRO_RMSNORM, EPI_ARGMAX, (301,), 1000, 0),
    "tail_plain": (PRO_NONE, EPI_STORE, (515,), 1536 + 64, 0),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_f16_gemv_forms(omx, lib, name):
    pro, epi, ns, K, single_round = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    mats = [rand_f16(rng, (n, K), 7, 12) for n in ns]
    x = rand_f16(rng, (K,), 10, 15)
    nw = rand_f16(rng, (K,), 13, 15) if pro == PRO_RMSNORM else None
    N = ns[0] if epi == EPI_SWIGLU else sum(ns)
    resid = rand_f16(rng, (N,), 12, 16) if epi == EPI_RESIDUAL else None
    got, keys = run_gemv(omx, lib, mats, x, pro, epi, nw, resid, single_round=single_round)
    xin = rmsnorm_f16(x, nw) if pro == PRO_RMSNORM else x
    W = mats[0] if len(mats) == 1 or epi == EPI_SWIGLU else np.concatenate(mats)
    exact, mag = rows_dot(W, xin)
    slack = flip_slack(W, xin) if pro == PRO_RMSNORM else 0.0
    if epi == EPI_STORE:
        check_plain(got, exact, mag, K, slack)
    elif epi == EPI_ARGMAX:
        check_plain(got, exact, mag, K, slack)
        best = int(keys.max())
        assert (~best) & 0xFFFFFFFF == int(np.argmax(got)), "argmax must be the lowest index of the float16 logits' maximum"
    elif epi == EPI_RESIDUAL:
        # out = f16(r + f16(acc)): f16(acc) may sit one float16 rounding away from f16(exact)
        ref = f16(resid.astype(np.float64) + f16(exact))
        acc = K * U24 * mag
        tol = 0.5 * ulp16(ref) + ulp16(exact) + acc
        assert np.all(np.abs(got - ref) <= tol)
        assert np.array_equal(got, f16(got))
    else:
        exact_u, mag_u = rows_dot(mats[1], xin)
        g, u = f16(exact), f16(exact_u)
        if single_round:
            ref = f16(g / (1.0 + np.exp(-g)) * u)
        else:
            ref = f16(f16(g * f16(1.0 / (1.0 + np.exp(-g)))) * u)
        eg = ulp16(exact) + K * U24 * mag + slack
        eu = ulp16(exact_u) + K * U24 * mag_u + slack
        tol = 2.0 * ulp16(ref) + 1.2 * (np.abs(u) * eg + np.abs(g) * eu)
        bad = np.nonzero(np.abs(got - ref) > tol)[0]
        assert bad.size == 0, f"{bad.size} SwiGLU rows off, e.g. {bad[0]}: got {got[bad[0]]} want {ref[bad[0]]}"
        assert np.array_equal(got, f16(got))


def test_f16_gemv_bias_and_refusals(omx, lib):
    from ominix_mlx_amd.ops import Tensor
    rng = np.random.default_rng(5)
    K, N = 2048, 1000
    W, x, b = rand_f16(rng, (N, K), 7, 12), rand_f16(rng, (K,), 10, 15), rand_f16(rng, (N,), 10, 15)
    got, _ = run_gemv(omx, lib, [W], x, PRO_NONE, EPI_STORE, bias=b)
    exact, mag = rows_dot(W, x)
    check_plain(got, exact + b.astype(np.float64), mag, K)
    # every float16 combination outside the plain decode forms is refused by name
    dw, dx, out = Tensor.from_numpy(W, "f16"), Tensor.from_numpy(x, "f16"), Tensor((N,), "f32")
    with pytest.raises(omx.OmxError, match="float16 takes EPI_STORE"):
        omx.check(lib.omx_debug_gemv(out.ptr, None, dx.ptr, None, None, None, dw.ptr, None, None, N, 0, N, K, PRO_NONE, 4, 1, EPS, 0, None))
    with pytest.raises(omx.OmxError, match="float16 takes PRO_NONE or PRO_RMSNORM"):
        omx.check(lib.omx_debug_gemv(out.ptr, None, dx.ptr, None, None, None, dw.ptr, dw.ptr, None, N, 0, N, K, 2, EPI_SWIGLU, 1, EPS, 0, None))


# ---- omx_linear / mlx_matmul / mlx_addmm in float16 ----

@pytest.mark.parametrize("M", [1, 4, 8, 64])
@pytest.mark.parametrize("with_bias", [False, True])
def test_f16_linear_and_mlx_matmul(omx, M, with_bias):
    from ominix_mlx_amd import mlx_c as mx, ops
    from ominix_mlx_amd.ops import Tensor
    rng = np.random.default_rng(M * 2 + with_bias)
    N, K = 768, 1024
    x = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    b = (rng.standard_normal((N,)) * 0.5).astype(np.float16) if with_bias else None
    xf, wf, bf = x.astype(np.float32), w.astype(np.float32), (b.astype(np.float32) if with_bias else None)
    ref = rc.linear(xf, wf, bf, "f16")
    exact = xf.astype(np.float64) @ wf.astype(np.float64).T + (bf if with_bias else 0.0)
    mag = np.abs(xf.astype(np.float64)) @ np.abs(wf.astype(np.float64)).T
    tol = 0.5 * ulp16(np.abs(exact)) + K * U24 * mag + (ulp16(np.abs(exact)) if M > 8 else 0.0)
    got = ops.linear(Tensor.from_numpy(x, "f16"), Tensor.from_numpy(w, "f16"), Tensor.from_numpy(b, "f16") if with_bias else None).numpy()
    assert np.all(np.abs(got - exact) <= tol)
    assert np.abs(got - ref).max() <= np.max(ulp16(np.abs(ref)))
    # nn::Linear through the mlx-c ABI: matmul(x, w.t()) / addmm(bias, x, w.t())
    X, Wt = mx.Array.from_numpy(x, mx.FLOAT16), mx.transpose(mx.Array.from_numpy(w, mx.FLOAT16))
    res = mx.addmm(mx.Array.from_numpy(b, mx.FLOAT16), X, Wt) if with_bias else mx.matmul(X, Wt)
    assert res.dtype == mx.FLOAT16
    np.testing.assert_array_equal(res.numpy(), got)


def test_f16_linear_unsupported_shapes(omx):
    from ominix_mlx_amd import ops
    from ominix_mlx_amd.ops import Tensor
    x4, w4 = Tensor.from_numpy(np.ones((4, 1004), np.float16), "f16"), Tensor.from_numpy(np.ones((16, 1004), np.float16), "f16")
    with pytest.raises(omx.OmxError, match="at most 8 rows takes K % 8 == 0"):
        ops.linear(x4, w4)
    x16, w16 = Tensor.from_numpy(np.ones((16, 1000), np.float16), "f16"), Tensor.from_numpy(np.ones((16, 1000), np.float16), "f16")
    with pytest.raises(omx.OmxError, match="more than 8 rows takes K % 64 == 0"):
        ops.linear(x16, w16)


# ---- the Qwen3 engine on dense float16 weights ----

def _cfg(tied):
    """the gqa4_d128 test model (test_gpu_qwen3.py), tied or untied head"""
    return rq.Qwen3Config(1024, 3, 3072, 8, 2, 128, 4096, 1e-6, 1e6, tied)


def _kw(cfg, max_context=256):
    return dict(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                tie_word_embeddings=cfg.tie_word_embeddings, rope_scaling=cfg.rope_scaling, max_context=max_context)


def _bound(cfg, ref_logits):
    return 2.0 ** -10 * np.abs(ref_logits).max() * np.sqrt(2 * cfg.num_hidden_layers)


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("serial_prefill", ["0", "1"])
def test_dense_f16_engine_matches_f16_oracle(omx, monkeypatch, tied, serial_prefill):
    """Model(dtype="float16") on the synthetic model's float16 weights: the prompt through the float16 matrix-core pass (or the decode
    step token by token), 16 decode steps through the float16 GEMVs, against Qwen3Oracle(dt="f16") on the same float16 values."""
    from ominix_mlx_amd import engine
    cfg = _cfg(tied)
    w = rq.synth_weights(cfg, dt="f16")
    n_prompt, n_new = 40, 17
    monkeypatch.setenv("OMX_PREFILL_SERIAL", serial_prefill)
    prompt = synth.prompt_ids(n_prompt, cfg.vocab_size)
    m = engine.Model(dtype="float16", **_kw(cfg))
    assert m.cfg.float16_weights == 1 and m.f16
    m.load_weights({k: v.astype(np.float16) for k, v in w.items()})
    first = m.prefill(prompt)
    logits0 = m.last_logits()
    got = np.concatenate([[first], m.decode(n_new - 1)]).astype(np.uint32)
    assert m.decode_path() == "graph"
    logits_last = m.last_logits()
    m.close()
    ref_tokens, ref_logits = rq.Qwen3Oracle(cfg, w, dt="f16").generate(prompt, n_new, return_logits=True)
    bound = _bound(cfg, ref_logits)
    assert np.array_equal(logits0, f16(logits0)), "last_logits of a float16 model are float16 values"
    assert np.abs(logits0 - ref_logits[0]).max() <= bound
    # the bf16 computation of the same weights lies outside the float16 bound: this is a float16 model, not a rounded copy
    ref_bf16 = rq.Qwen3Oracle(cfg, w, dt="bf16").generate(prompt, 1, return_logits=True)[1]
    assert np.abs(ref_bf16[0] - ref_logits[0]).max() > bound
    margins = rc.argmax_margin(ref_logits)
    n_eq = n_new
    for i in range(n_new):
        if got[i] != ref_tokens[i]:
            assert margins[i] <= 2 * bound, f"token {i}: got {got[i]} want {ref_tokens[i]} with margin {margins[i]:.4f} > {2*bound:.4f}"
            n_eq = i
            break
    if n_eq == n_new:
        assert np.abs(logits_last - ref_logits[-1]).max() <= bound


def test_dense_f16_sampler_encode_and_synth(omx):
    from ominix_mlx_amd import engine
    cfg = _cfg(True)
    w = rq.synth_weights(cfg, dt="f16")
    prompt = synth.prompt_ids(24, cfg.vocab_size)
    m = engine.Model(dtype="float16", **_kw(cfg))
    m.synth_weights()
    # device-synthesised float16 weights == synth.tensor(dt="f16"), bit for bit
    for name in ("model.embed_tokens.weight", "model.layers.1.mlp.down_proj.weight", "model.layers.0.input_layernorm.weight"):
        ptr, nb = ctypes.c_void_p(), ctypes.c_size_t()
        omx.check(omx.lib.omx_qwen3_get_weight(m._h, name.encode(), ctypes.byref(ptr), ctypes.byref(nb)))
        host = np.empty(w[name].size, np.float16)
        omx.check(omx.lib.omx_memcpy_d2h(host.ctypes.data, ptr, host.nbytes, None))
        np.testing.assert_array_equal(host.reshape(w[name].shape).astype(np.float32), w[name])
    # temperature sampling on float16 logits: runs, and a fixed seed reproduces the draw
    runs = []
    for _ in range(2):
        m.reset()
        m.set_sampler(0.8, seed=7)
        runs.append(np.concatenate([[m.prefill(prompt)], m.decode(8)]))
    np.testing.assert_array_equal(runs[0], runs[1])
    m.set_sampler(0.0)
    # encode (no padding mask): the taps within the float16 bound of the oracle
    oracle = rq.Qwen3Oracle(cfg, w, dt="f16")
    for n in (77, 5):
        ids = synth.prompt_ids(n, cfg.vocab_size)
        m.reset()
        got = m.encode(ids, extract_layers=(0, 2)).numpy()
        ref = oracle.encode(ids, extract_layers=(0, 2))
        bound = 2.0 ** -10 * np.abs(ref).max() * np.sqrt(2 * cfg.num_hidden_layers)
        assert np.abs(got - ref).max() <= bound, f"encode({n}) off by {np.abs(got - ref).max()} (bound {bound})"
    m.close()


def _write_checkpoint(loader, d, cfg, w):
    json.dump({"hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_hidden_layers, "intermediate_size": cfg.intermediate_size,
               "num_attention_heads": cfg.num_attention_heads, "num_key_value_heads": cfg.num_key_value_heads, "head_dim": cfg.head_dim,
               "vocab_size": cfg.vocab_size, "rms_norm_eps": cfg.rms_norm_eps, "rope_theta": cfg.rope_theta,
               "tie_word_embeddings": cfg.tie_word_embeddings}, open(f"{d}/config.json", "w"))
    names = sorted(w)
    shards = {"model-00001-of-00002.safetensors": names[: len(names) // 2], "model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for fn, keys in shards.items():
        loader.write_safetensors(f"{d}/{fn}", {k: w[k].astype(np.float16) for k in keys})
    json.dump({"metadata": {}, "weight_map": {k: fn for fn, keys in shards.items() for k in keys}}, open(f"{d}/model.safetensors.index.json", "w"))


def test_load_model_f16_checkpoint_runs_in_float16(omx, tmp_path):
    """loader.load_model on a two-shard F16 checkpoint gives the model Model(dtype="float16") gives on the same arrays;
    dtype="bfloat16" reproduces the old conversion to bf16 bit for bit."""
    from ominix_mlx_amd import engine, loader
    cfg = _cfg(False)
    w = rq.synth_weights(cfg, dt="f16")
    d = str(tmp_path)
    _write_checkpoint(loader, d, cfg, w)
    prompt = synth.prompt_ids(20, cfg.vocab_size)

    def run(m):
        toks = np.concatenate([[m.prefill(prompt)], m.decode(6)])
        lg = m.last_logits()
        m.close()
        return toks, lg

    got = run(loader.load_model(d, max_context=256))
    ref_m = engine.Model(dtype="float16", **_kw(cfg))
    ref_m.load_weights({k: v.astype(np.float16) for k, v in w.items()})
    want = run(ref_m)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    old = run(loader.load_model(d, max_context=256, dtype="bfloat16"))
    bf = engine.Model(**_kw(cfg))
    bf.load_weights({k: v.astype(np.float16) for k, v in w.items()})   # float16 arrays uploaded as bf16, as load_model used to
    want_bf = run(bf)
    np.testing.assert_array_equal(old[0], want_bf[0])
    np.testing.assert_array_equal(old[1], want_bf[1])


def test_dense_f16_refusals(omx):
    from ominix_mlx_amd import engine
    cfg = _cfg(True)
    kw = _kw(cfg)
    with pytest.raises(omx.OmxError, match="float16_weights marks a dense checkpoint"):
        engine.Model(dtype="float16", quantization={"bits": 4, "group_size": 64}, **kw)
    with pytest.raises(omx.OmxError, match="float16_weights with experts"):
        engine.Model(dtype="float16", num_experts=4, num_experts_per_tok=2, moe_intermediate_size=512, **kw)
    with pytest.raises(omx.OmxError, match="float16_weights under tensor / expert parallelism"):
        engine.Model(dtype="float16", **dict(kw, tp_size=2, tp_rank=0))
    with pytest.raises(omx.OmxError, match="float16_weights with attention_bias"):
        engine.Model(dtype="float16", attention_bias=True, qk_norm=False, **kw)
    with pytest.raises(omx.OmxError, match="float16_weights needs head_dim 128"):
        engine.Model(dtype="float16", **dict(kw, head_dim=64))
    with pytest.raises(omx.OmxError, match="dtype 'float64'"):
        engine.Model(dtype="float64", **kw)
    m = engine.Model(dtype="float16", **kw)
    m.synth_weights()
    m.prefill(synth.prompt_ids(4, cfg.vocab_size))
    with pytest.raises(omx.OmxError, match="dense float16 models \\(float16_weights\\) are not supported"):
        m.verify([1, 2, 3])
    with pytest.raises(omx.OmxError, match="float16 encoder with an attention_mask"):
        m.encode([1, 2, 3, 4], attention_mask=[1, 1, 1, 0], extract_layers=(0,))
    m.close()
