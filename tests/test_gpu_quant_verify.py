"""Speculative decoding on MLX-quantized targets: the few-row packed GEMV (csrc/qgemv_rows.hip) and omx_qwen3_verify on packed dense
models.

1. omx_debug_qgemv_rows against launch_qgemv's VALU kernel on the same rows (n_batch = M, no matrix-core tiles): bit for bit, every
   width, row count, form, K (12288 stages the activation rows in chunks at M = 8), with and without the interleaved scale | bias words.
2. The engine's verify pass on packed checkpoints against the oracle; 3. SpeculativeGenerate on a 4-bit target and draft;
4. the verify pass dequantises no weight (omx_qwen3_dequant_bytes); 5. what verify still refuses."""
import ctypes
import dataclasses

import numpy as np
import pytest

from oracle import ref_core as rc, ref_qwen3 as rq, synth
from test_gpu_primitives import rand
from test_gpu_quant import EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU, PRO_NONE, PRO_RMSNORM
from test_gpu_quant_widths import CONFIGS, _checkpoints, _triplet
from test_quant_widths import dequantize_any, pack_bits

pytestmark = pytest.mark.gpu

TARGET = rq.Qwen3Config(512, 3, 1536, 8, 2, 64, 2048, 1e-6, 1e6, False)   # test_gpu_speculative.py's target


def _bind(omx):
    lib = omx.lib
    vp = ctypes.c_void_p
    lib.omx_debug_qgemv_rows.restype = ctypes.c_int
    lib.omx_debug_qgemv_rows.argtypes = [vp] * 4 + [ctypes.POINTER(vp)] * 3 + [ctypes.POINTER(ctypes.c_int)] + [ctypes.c_int] * 8 + \
        [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    return lib


# (pro, epi, swiglu_single_round, members): members = row counts of a q | k | v stack, or None for gate / up (SwiGLU)
FORMS = {
    "store": (PRO_NONE, EPI_STORE, 0, [300]),
    "norm_store_qkv": (PRO_RMSNORM, EPI_STORE, 0, [128, 64, 68]),
    "norm_store": (PRO_RMSNORM, EPI_STORE, 0, [300]),
    "residual": (PRO_NONE, EPI_RESIDUAL, 0, [300]),
    "norm_swiglu": (PRO_RMSNORM, EPI_SWIGLU, 0, None),
    "swiglu_single": (PRO_NONE, EPI_SWIGLU, 1, None),
    "store_qkv": (PRO_NONE, EPI_STORE, 0, [64, 32, 36]),
}
N_SWIGLU = 204                                          # ragged: not a multiple of a block's rows


def _case(omx, bits, M, form, K, group, sb, seed):
    """(rows kernel output, reference output, inputs) for one case."""
    lib = _bind(omx)
    T = omx.ops.Tensor
    pro, epi, single, members = FORMS[form]
    sizes = [N_SWIGLU, N_SWIGLU] if members is None else members
    N = N_SWIGLU if members is None else sum(members)
    mats = [_triplet(rand((n, K), seed + 3 + j) * 0.05, group, bits) for j, n in enumerate(sizes)]
    dev = [(T.from_numpy(np.ascontiguousarray(pack_bits(q, bits)), "u32"), T.from_numpy(s), T.from_numpy(b)) for q, s, b in mats]
    x = rc.bf16_round(rand((M, K), seed))
    nw = rc.bf16_round(1.0 + 0.1 * rand((K,), seed + 1))
    resid = rc.bf16_round(rand((M, N), seed + 2))
    xd, nwd, rd = T.from_numpy(x), T.from_numpy(nw), T.from_numpy(resid)
    vp = ctypes.c_void_p
    W = (vp * 3)(*[d[0].ptr for d in dev]); S = (vp * 3)(*[d[1].ptr for d in dev]); B = (vp * 3)(*[d[2].ptr for d in dev])
    ns = (ctypes.c_int * 3)(*sizes)
    outs = []
    for reference in (0, 1):
        out = T.from_numpy(np.zeros((M, N), np.float32))
        omx.check(lib.omx_debug_qgemv_rows(out.ptr, xd.ptr, nwd.ptr, rd.ptr, W, S, B, ns, len(sizes), M, N, K, group, bits, pro, epi,
                                           1e-6, single, int(sb), reference, None))
        omx.check(omx.lib.omx_synchronize(None))
        outs.append(out.numpy())
    return outs[0], outs[1], (x, nw, resid, mats)


@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 8])
@pytest.mark.parametrize("M", [1, 2, 5, 8])
@pytest.mark.parametrize("form", list(FORMS))
def test_rows_kernel_bit_identical_to_per_row_gemv(omx, bits, M, form):
    got, want, _ = _case(omx, bits, M, form, 4096, 64, sb=(M + bits) % 2 == 0, seed=2000 + 17 * bits + M)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 8])
@pytest.mark.parametrize("K", [512, 1536, 12288])
@pytest.mark.parametrize("M", [5, 8])
@pytest.mark.parametrize("form,sb", [("residual", True), ("norm_store_qkv", False), ("norm_swiglu", True)])
def test_rows_kernel_bit_identical_across_k(omx, bits, K, M, form, sb):
    got, want, _ = _case(omx, bits, M, form, K, 64, sb=sb, seed=2100 + bits + K % 97 + M)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("bits", [3, 4, 6, 8])
@pytest.mark.parametrize("group", [32, 128])
@pytest.mark.parametrize("form", ["norm_store", "residual", "swiglu_single"])
def test_rows_kernel_bit_identical_across_groups(omx, bits, group, form):
    got, want, _ = _case(omx, bits, 5, form, 2048, group, sb=group == 128, seed=2200 + bits + group)
    np.testing.assert_array_equal(got, want)


def _hold_rows_to_numpy(omx, form, bits, group, M, K, seed):
    """test_fused_packed_gemv_forms_match_numpy's tolerances against a float64 reference."""
    pro, epi, single, _ = FORMS[form]
    got, _, (x, nw, resid, mats) = _case(omx, bits, M, form, K, group, sb=False, seed=seed)
    got = got.astype(np.float64)
    xin = (rc.rms_norm(x, nw, 1e-6, "bf16") if pro == PRO_RMSNORM else x).astype(np.float64)
    ws = [dequantize_any(m[0], m[1], m[2], group, "f32").astype(np.float64) for m in mats]
    ys = [xin @ w.T for w in ws]
    noise = [4 * 2.0 ** -9 * np.sqrt((xin ** 2) @ (w ** 2).T) for w in ws]
    ulp = 2.0 ** -7
    if epi == EPI_STORE:
        assert (np.abs(got - ys[0]) <= np.abs(ys[0]) * ulp + noise[0] + 1e-6).all()
    elif epi == EPI_RESIDUAL:
        ref = resid.astype(np.float64) + ys[0]
        assert (np.abs(got - ref) <= (np.abs(ref) + np.abs(ys[0])) * ulp + noise[0] + 1e-6).all()
    else:
        g, u = ys
        sg = 1.0 / (1.0 + np.exp(-g))
        ref = g * sg * u
        tol = np.abs(ref) * 4 * ulp + 1.1 * (noise[0] + np.abs(g) * ulp) * np.abs(u) + (noise[1] + np.abs(u) * ulp) * np.abs(g * sg) + 1e-6
        assert (np.abs(got - ref) <= tol).all()


def test_rows_kernel_matches_numpy(omx):
    """5 rows of a 6-bit RMSNorm + store."""
    _hold_rows_to_numpy(omx, "norm_store", 6, 64, 5, 1536, seed=2300)


@pytest.mark.parametrize("form,bits,group,K", [
    ("residual", 4, 64, 2048),
    ("residual", 3, 32, 1024 + 32),          # a chunked width whose last step masks lanes
    ("norm_swiglu", 5, 32, 1024 + 32),
    ("swiglu_single", 4, 64, 2048),
])
def test_rows_kernel_epilogues_match_numpy(omx, form, bits, group, K):
    """The epilogues that only the bit comparison with the single-row kernel reached, 3 rows each."""
    _hold_rows_to_numpy(omx, form, bits, group, 3, K, seed=2310 + bits)


# ---- 2. the engine's verify pass on packed checkpoints ----

def _qmodel(cfg, bits, group, max_context=256, **kw):
    from ominix_mlx_amd import engine
    return engine.Model(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
                        num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim,
                        vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
                        tie_word_embeddings=cfg.tie_word_embeddings, max_context=max_context,
                        quantization={"bits": bits, "group_size": group}, **kw)


def _quantized(cfg, bits, group):
    """(checkpoint at `bits`, oracle): the oracle packs widths that divide 32 only -- 3 / 6 bits are held to their 8-bit re-pack."""
    if 32 % bits == 0:
        w = rq.quantize_weights(cfg, rq.synth_weights(cfg), bits, group)
        return w, rq.Qwen3Oracle(cfg, w, quant=(bits, group))
    wb, w8 = _checkpoints(cfg, bits, group)
    return wb, rq.Qwen3Oracle(cfg, w8, quant=(8, group))


@pytest.mark.parametrize("bits,group", [(4, 64), (8, 64), (3, 32), (6, 64)])
def test_packed_verify_matches_oracle(omx, bits, group):
    w, oracle = _quantized(TARGET, bits, group)
    prompt = synth.prompt_ids(33, TARGET.vocab_size)
    ref_tokens, ref_logits = oracle.generate(prompt, 8, return_logits=True)
    bound = 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(TARGET.num_hidden_layers)
    margins = rc.argmax_margin(ref_logits)
    m = _qmodel(TARGET, bits, group)
    m.load_weights(w)
    first = m.prefill(prompt)
    assert first == ref_tokens[0] or margins[0] <= 2 * bound
    feed = [int(t) for t in ref_tokens[:6]]
    got = m.verify(feed)
    assert m.offset() == 33 + 6
    for i in range(6):
        assert np.abs(m.verify_logits(i) - ref_logits[i + 1]).max() <= 1.5 * bound, f"row {i}"
        assert got[i] == ref_tokens[i + 1] or margins[i + 1] <= 2 * bound
    # drop feed[4], feed[5]: the pending input becomes feed[4] and the next step predicts what verify row 4 did
    m.trim(2, feed[4])
    assert m.offset() == 33 + 4
    nxt = int(m.decode(1)[0])
    assert nxt == got[4] or margins[5] <= 2 * bound
    assert nxt == ref_tokens[5] or margins[5] <= 2 * bound
    m.close()


# ---- 3. SpeculativeGenerate with a 4-bit target and a 4-bit draft ----

def _pair(draft_layers):
    dcfg = dataclasses.replace(TARGET, num_hidden_layers=draft_layers)   # tensors are generated by name: the target's first layers
    wt, oracle = _quantized(TARGET, 4, 64)
    wd = rq.quantize_weights(dcfg, rq.synth_weights(dcfg), 4, 64)
    target, draft = _qmodel(TARGET, 4, 64), _qmodel(dcfg, 4, 64)
    target.load_weights(wt)
    draft.load_weights(wd)
    return target, draft, oracle, wt


@pytest.mark.parametrize("k", [2, 4])
def test_speculative_generate_on_4bit_target_equals_target_greedy(omx, k):
    from ominix_mlx_amd import speculative
    prompt = synth.prompt_ids(48, TARGET.vocab_size)
    n = 32
    target, draft, oracle, wt = _pair(1)
    want, want_logits = oracle.generate(prompt, n, return_logits=True)
    bound = 2.0 ** -7 * np.abs(want_logits).max() * np.sqrt(TARGET.num_hidden_layers)
    margins = rc.argmax_margin(want_logits)
    gen = speculative.SpeculativeGenerate(target, draft, k, 0.0, prompt)
    got = [next(gen).token for _ in range(n)]
    div = next((i for i in range(n) if got[i] != int(want[i])), None)
    if div is not None:
        assert margins[div] <= 2 * bound, f"token {div}: got {got[div]} want {int(want[div])} with margin {margins[div]:.4f}"
    assert (n if div is None else div) >= 8
    assert gen.rounds > 0
    # the 4-bit engine's own greedy run, up to the first near-tie between its decode step and the verify pass
    plain = _qmodel(TARGET, 4, 64)
    plain.load_weights(wt)
    mine = np.concatenate([[plain.prefill(prompt)], plain.decode(n - 1)])
    plain.close()
    same = next((i for i in range(n) if got[i] != mine[i]), n)
    assert same >= (n if div is None else div) or margins[same] <= 2 * bound
    target.close(); draft.close()


def test_speculative_sampling_on_4bit_target_draws_from_one_key_sequence(omx):
    """test_speculative_sampling_draws_from_one_key_sequence on the packed target and draft."""
    from ominix_mlx_amd import speculative
    from oracle import mlx_rng
    k, temp, seed = 3, 0.7, 5
    prompt = synth.prompt_ids(40, TARGET.vocab_size)
    target, draft, _, _ = _pair(1)
    gen = speculative.SpeculativeGenerate(target, draft, k, temp, prompt, seed=seed, record=True)
    n = 24
    toks = [next(gen) for _ in range(n)]
    state = mlx_rng.RandomState(seed)
    want_first = int(rc.sample(gen.first_logits[None, :], temp, state.next())[0])
    assert toks[0].token == want_first
    emitted = [want_first]
    for r in gen.record:
        d_want = [int(rc.sample(row[None, :], temp, state.next())[0]) for row in r["draft_logits"]]
        assert r["drafts"] == d_want
        t_want = [int(rc.sample(row[None, :], temp, state.next())[0]) for row in r["target_logits"]]
        assert r["target_tokens"] == t_want
        acc = 0
        while acc < k and d_want[acc] == t_want[acc]:
            acc += 1
        assert r["accepted"] == acc
        emitted += d_want[:acc] + [t_want[acc]]
    assert [t.token for t in toks] == emitted[:n]
    target.close(); draft.close()


# ---- 4. no dequantised weights on the verify route ----

def test_packed_verify_dequantises_no_weight(omx):
    w, _ = _quantized(TARGET, 4, 64)
    m = _qmodel(TARGET, 4, 64)
    m.load_weights(w)
    assert m.dequant_bytes() == 0
    m.verify([int(t) for t in synth.prompt_ids(6, TARGET.vocab_size)])    # the first call on a fresh model
    assert m.offset() == 6
    assert m.dequant_bytes() == 0
    m.prefill(synth.prompt_ids(33, TARGET.vocab_size))                     # the prompt pass keeps its dequantising route
    assert m.dequant_bytes() > 0
    m.close()


# ---- 5. refusals ----

def test_packed_verify_refuses_float16_triplets_and_experts(omx):
    from ominix_mlx_amd import engine
    cfg = CONFIGS["gqa4_d128"]
    m = engine.Model(
        hidden_size=cfg.hidden_size, num_hidden_layers=1, intermediate_size=cfg.intermediate_size, num_attention_heads=cfg.num_attention_heads,
        num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, vocab_size=cfg.vocab_size, max_context=256,
        quantization={"bits": 4, "group_size": 64, "scales_dtype": "float16"})
    with pytest.raises(omx.OmxError, match="float16 triplets"):
        m.verify([1, 2, 3])
    m.close()
    m = engine.Model(hidden_size=1024, num_hidden_layers=1, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                     vocab_size=1024, max_context=256, num_experts=4, num_experts_per_tok=2, moe_intermediate_size=512,
                     quantization={"bits": 4, "group_size": 64})
    with pytest.raises(omx.OmxError, match="experts"):
        m.verify([1, 2, 3])
    m.close()
