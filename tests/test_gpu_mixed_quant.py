"""Mixed-precision MLX checkpoints on the device: per-matrix (bits, group_size) through the packed decode GEMV (a q | k | v stack whose
members differ, as one launch of qgemv_stack_kernel), the Qwen3 engine (synthesised and uploaded weights,
hipGraph decode step, verify, batched decode on bf16 and 8-bit K/V, a checkpoint directory through the loader) and the refusals.

The reference of a mixed model is its 8-bit re-pack at the table's smallest group (mixed_quant_helpers)."""
import ctypes
import json

import numpy as np
import pytest

from oracle import ref_core as rc, synth
from mixed_quant_helpers import checkpoints, oracle_of, quantization, table_a, table_b
from test_gpu_primitives import rand
from test_gpu_quant import EPI_STORE, PRO_NONE, PRO_RMSNORM, _bind_debug
from test_gpu_quant_widths import CONFIGS, _hold_to_oracle, _model, _triplet, dequantize_any, pack_bits

pytestmark = pytest.mark.gpu

N_PROMPT, N_NEW = 48, 10


def _bind_mixed(omx):
    lib = _bind_debug(omx)
    vp, pvp, pi = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int)
    lib.omx_debug_qgemv_mixed.restype = ctypes.c_int
    lib.omx_debug_qgemv_mixed.argtypes = [vp, vp, vp, pvp, pvp, pvp, pi, pi, pi, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp]
    return lib


# ---- 1. the stack kernel ----

def _mixed_launch(omx, lib, out, xd, nwd, dev, members, K, pro):
    n = len(members)
    arr = lambda j: (ctypes.c_void_p * n)(*[d[j].ptr for d in dev])
    ints = lambda j: (ctypes.c_int * n)(*[m[j] for m in members])
    omx.check(lib.omx_debug_qgemv_mixed(out.ptr, xd.ptr, nwd.ptr, arr(0), arr(1), arr(2), ints(0), ints(1), ints(2), n, K, pro, 1e-6, None))
    omx.check(omx.lib.omx_synchronize(None))
    return out.numpy()


@pytest.mark.parametrize("K,pro,members", [
    (1536, PRO_RMSNORM, [(1024, 4, 64), (256, 4, 64), (256, 6, 64)]),     # no scale | bias words; 4-bit at W = 1; the 6-bit row (48 chunks in its one step) masks 16 lanes
    (4096, PRO_RMSNORM, [(1000, 4, 64), (264, 8, 32), (250, 3, 128)]),    # interleaved words, register-resident prologue, members ending mid-block
    (6144, PRO_RMSNORM, [(512, 5, 64), (128, 2, 64), (128, 6, 128)]),     # the two-pass prologue
    (4096, PRO_NONE, [(512, 4, 64), (512, 8, 64)]),                       # two members, no prologue
])
def test_mixed_stack_kernel(omx, K, pro, members):
    lib = _bind_mixed(omx)
    T = omx.ops.Tensor
    seed = 2100 + K % 97 + len(members) + pro
    x = rc.bf16_round(rand((1, K), seed))
    nw = rc.bf16_round(1.0 + 0.1 * rand((K,), seed + 1))
    xin = (rc.rms_norm(x, nw, 1e-6, "bf16") if pro == PRO_RMSNORM else x).astype(np.float64)
    trip = [_triplet(rand((n, K), seed + 3 + j) * 0.05, group, bits) for j, (n, bits, group) in enumerate(members)]
    dev = [(T.from_numpy(np.ascontiguousarray(pack_bits(q, bits)), "u32"), T.from_numpy(s, "bf16"), T.from_numpy(b, "bf16"))
           for (q, s, b), (_, bits, _) in zip(trip, members)]
    N = sum(m[0] for m in members)
    xd, nwd = T.from_numpy(x), T.from_numpy(nw)
    got = _mixed_launch(omx, lib, T.from_numpy(np.zeros((N,), np.float32)), xd, nwd, dev, members, K, pro)
    # (a) float64 x . dequantised(w)^T under the bound of test_fused_packed_gemv_forms_match_numpy's EPI_STORE
    w = np.concatenate([dequantize_any(q, s, b, group, "f32").astype(np.float64) for (q, s, b), (_, _, group) in zip(trip, members)])
    ref = (xin @ w.T)[0]
    noise = 4 * 2.0 ** -9 * np.sqrt((xin ** 2) @ (w ** 2).T)[0]
    err = np.abs(got.astype(np.float64) - ref)
    print(f"K {K}: max err / bound {np.max(err / (np.abs(ref) * 2.0 ** -7 + noise + 1e-6)):.3f}")
    assert (err <= np.abs(ref) * 2.0 ** -7 + noise + 1e-6).all()
    # (b) every member's rows == that member alone through the VALU kernel
    row = 0
    for (n, bits, group), d in zip(members, dev):
        alone = T.from_numpy(np.zeros((n,), np.float32))
        lib.omx_debug_qgemv_mfma(0)
        try:
            omx.check(lib.omx_debug_qgemv(alone.ptr, None, None, xd.ptr, nwd.ptr, None, d[0].ptr, d[1].ptr, d[2].ptr, None, None, None, 0, n, K,
                                          group, bits, pro, EPI_STORE, 1e-6, 0, None))
            omx.check(omx.lib.omx_synchronize(None))
        finally:
            lib.omx_debug_qgemv_mfma(-1)
        np.testing.assert_array_equal(got[row:row + n], alone.numpy(), err_msg=f"member ({n}, {bits}, {group})")
        row += n


# ---- 2. the engine against the repack oracle ----

_REF = {}


def _reference(name, which, n_prompt=N_PROMPT, seed_shift=0):
    """(cfg, base, table, checkpoint, prompt, oracle tokens, oracle logits), computed once per (config, table, prompt)"""
    key = (name, which, n_prompt, seed_shift)
    if key not in _REF:
        cfg = CONFIGS[name]
        base, table = (table_a if which == "A" else table_b)(cfg)
        wm, w8, g_min = checkpoints(cfg, base, table)
        prompt = (synth.prompt_ids(n_prompt, cfg.vocab_size) + seed_shift) % cfg.vocab_size
        tokens, logits = oracle_of(cfg, w8, g_min).generate(prompt, N_NEW, return_logits=True)
        _REF[key] = (cfg, base, table, wm, prompt.astype(np.uint32), tokens, logits)
    return _REF[key]


def _generate(m, prompt, n_new=N_NEW):
    first = m.prefill(prompt)
    logits0 = m.last_logits()
    got = np.concatenate([[first], m.decode(n_new - 1)]).astype(np.uint32)
    return got, logits0, m.last_logits()


@pytest.mark.parametrize("name", ["gqa4_d128", "gqa2_d64"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_engine_decode_matches_the_repack_oracle(omx, name, which):
    cfg, base, table, wm, prompt, ref_tokens, ref_logits = _reference(name, which)
    outs = {}
    for upload in (True, False):
        m = _model(cfg, quantization(base, table))
        for prefix, fmt in table.items():
            assert m.quant_format(prefix) == fmt
        assert m.quant_format("model.layers.0.self_attn.q_proj") == table.get("model.layers.0.self_attn.q_proj", base)
        m.load_weights(wm) if upload else m.synth_weights()
        outs[upload] = _generate(m, prompt)
        assert m.decode_path() == "graph"
        m.close()
    np.testing.assert_array_equal(outs[True][0], outs[False][0])      # uploaded == synthesised: tokens and first logits
    np.testing.assert_array_equal(outs[True][1], outs[False][1])
    _hold_to_oracle(outs[True][0], outs[True][1], ref_tokens, ref_logits, cfg.num_hidden_layers)


# ---- 3. the format decides the route, not the base ----

def test_every_matrix_overridden_to_4bit_equals_the_uniform_4bit_model(omx):
    cfg = CONFIGS["gqa4_d128"]
    table = {f"model.layers.{i}.{sub}": (4, 64) for i in range(cfg.num_hidden_layers)
             for sub in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")}
    table["model.embed_tokens"] = (4, 64)
    prompt = synth.prompt_ids(N_PROMPT, cfg.vocab_size)
    res = []
    for quant in (quantization((8, 64), table), {"bits": 4, "group_size": 64}):
        m = _model(cfg, quant)
        m.synth_weights()
        first = m.prefill(prompt)
        toks, logits = [first], [m.last_logits()]
        for _ in range(N_NEW):
            toks.append(int(m.decode(1)[0]))
            logits.append(m.last_logits())
        res.append((np.array(toks, np.uint32), np.stack(logits), m.step_forms()))
        m.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]          # the same in-launch folds (the O projection inside the attention launch)


# ---- 4. verify and the batched decode on table A ----

def test_verify_on_a_mixed_checkpoint(omx):
    """tests/test_gpu_quant_verify.py's rule for a uniform checkpoint, on table A: the rows' greedy tokens are the decode's, the rows'
    logits lie within 1.5 x the decoder's bound of the oracle's."""
    cfg, base, table, wm, prompt, ref_tokens, ref_logits = _reference("gqa4_d128", "A")
    bound = 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(cfg.num_hidden_layers)
    margins = rc.argmax_margin(ref_logits)
    m = _model(cfg, quantization(base, table))
    m.load_weights(wm)
    greedy, _, _ = _generate(m, prompt)
    m.reset()
    first = m.prefill(prompt)
    assert first == greedy[0]
    feed = [int(t) for t in greedy[:4]]
    got = m.verify(feed)
    np.testing.assert_array_equal(got, greedy[1:5])          # the target tokens of the draft == the greedy decode
    # row i saw prompt + greedy[: i + 1]: it is the oracle's position i + 1 for as long as the greedy tokens are the oracle's.  Every such
    # row is held to the rule; the first token that leaves the oracle's must be a near-tie (the rows behind it have no reference)
    checked = 0
    for i in range(4):
        if any(int(a) != int(b) for a, b in zip(greedy[: i + 1], ref_tokens[: i + 1])):
            d = next(j for j in range(i + 1) if greedy[j] != ref_tokens[j])
            assert margins[d] <= 2 * bound, f"token {d}: got {greedy[d]} want {ref_tokens[d]} with margin {margins[d]:.4f}"
            break
        assert np.abs(m.verify_logits(i) - ref_logits[i + 1]).max() <= 1.5 * bound, f"row {i}"
        assert got[i] == ref_tokens[i + 1] or margins[i + 1] <= 2 * bound
        checked += 1
    print(f"verify rows held to the oracle: {checked} of 4")
    m.close()


@pytest.mark.parametrize("kv_bits", [0, 8])
def test_batched_decode_on_a_mixed_checkpoint(omx, kv_bits):
    refs = [_reference("gqa4_d128", "A"), _reference("gqa4_d128", "A", 21, 7), _reference("gqa4_d128", "A")]
    cfg, base, table, wm = refs[0][:4]
    m = _model(cfg, quantization(base, table))
    m.load_weights(wm)
    b = m.batch(3, 256, kv_bits=kv_bits)
    firsts = [b.prefill(s, refs[s][4]) for s in range(3)]
    logits0 = [b.logits(s) for s in range(3)]
    among = b.decode(N_NEW - 1)
    last = [b.logits(s) for s in range(3)]
    for s in (0, 1):       # a slot alone equals itself among three, bit for bit
        a = m.batch(3, 256, kv_bits=kv_bits)
        assert a.prefill(s, refs[s][4]) == firsts[s]
        np.testing.assert_array_equal(a.logits(s), logits0[s])
        np.testing.assert_array_equal(a.decode(N_NEW - 1, [s])[:, 0], among[:, s])
        np.testing.assert_array_equal(a.logits(s), last[s])
        a.close()
    if kv_bits == 0:       # the bf16-slab slots hold to the oracle
        for s in range(3):
            got = np.concatenate([[firsts[s]], among[:, s]]).astype(np.uint32)
            _hold_to_oracle(got, logits0[s], refs[s][5], refs[s][6], cfg.num_hidden_layers)
    b.close()
    m.close()


# ---- 5. a checkpoint directory ----

def test_load_model_from_a_mixed_checkpoint_directory(omx, tmp_path):
    from ominix_mlx_amd import loader
    cfg, base, table, wm, prompt, _, _ = _reference("gqa4_d128", "A")
    d = str(tmp_path)
    json.dump({"hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_hidden_layers, "intermediate_size": cfg.intermediate_size,
               "num_attention_heads": cfg.num_attention_heads, "num_key_value_heads": cfg.num_key_value_heads, "head_dim": cfg.head_dim,
               "vocab_size": cfg.vocab_size, "rms_norm_eps": cfg.rms_norm_eps, "rope_theta": cfg.rope_theta,
               "tie_word_embeddings": cfg.tie_word_embeddings, "quantization": quantization(base, table)},
              open(f"{d}/config.json", "w"))
    names = sorted(wm)
    shards = {"model-00001-of-00002.safetensors": names[: len(names) // 2], "model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for fn, keys in shards.items():
        raw = lambda k: wm[k].dtype == np.uint32
        tensors = {k: (wm[k] if raw(k) else rc.to_bf16_bits(wm[k])) for k in keys}
        loader.write_safetensors(f"{d}/{fn}", tensors, bf16_names=tuple(k for k in keys if not raw(k)))
    json.dump({"metadata": {}, "weight_map": {k: fn for fn, keys in shards.items() for k in keys}}, open(f"{d}/model.safetensors.index.json", "w"))
    m = loader.load_model(d, max_context=256)
    assert m.quant_format("model.layers.0.self_attn.v_proj") == (6, 64) and m.quant_format("model.layers.1.self_attn.v_proj") == (4, 64)
    got, logits0, _ = _generate(m, prompt)
    m.close()
    ref = _model(cfg, quantization(base, table))
    ref.load_weights(wm)
    want, want0, _ = _generate(ref, prompt)
    ref.close()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(logits0, want0)


def test_drop_in_route_takes_each_module_format(omx):
    """The per-op replay of the mlx-c route on the engine's own tensors passes every QuantizedLinear's own (group_size, bits), as the crate
    does.  Teacher-forced with the engine's greedy tokens on table B (every kind of matrix in another format) and table A: the route's
    logits rows lie within two decoder bounds of the engine's rows at the same positions -- each side is one bound from the exact
    value (the engine is held to the oracle above) -- and its greedy tokens are the engine's up to a near-tie.  A Linear read in the base
    format instead of its own gives noise, not a near-tie."""
    for which in ("B", "A"):
        cfg, base, table, wm, prompt, ref_tokens, ref_logits = _reference("gqa4_d128", which)
        bound = 2.0 ** -7 * np.abs(ref_logits).max() * np.sqrt(2 * cfg.num_hidden_layers)
        m = _model(cfg, quantization(base, table))
        m.load_weights(wm)
        toks, rows = [int(m.prefill(prompt))], [m.last_logits()]
        for _ in range(N_NEW - 1):
            toks.append(int(m.decode(1)[0]))
            rows.append(m.last_logits())
        steps = [0, 1, 4, N_NEW - 1]
        r = m.per_op_route_forced(prompt, toks[:-1], steps)
        m.close()
        for k, step in enumerate(steps):
            err = np.abs(r["logits"][k] - rows[step]).max()
            print(f"table {which} step {step}: route - engine {err:.4f}, 2 x bound {2 * bound:.4f}")
            assert err <= 2 * bound, f"table {which} step {step}"
        for i in range(N_NEW):
            if int(r["tokens"][i]) != toks[i]:
                top2 = np.sort(rows[i])[-2:]
                assert top2[1] - top2[0] <= 2 * bound, f"table {which} token {i}: route {r['tokens'][i]} engine {toks[i]}"


# ---- 6. refusals ----

def _set_format(omx, m, prefix, bits, group):
    omx.check(omx.lib.omx_qwen3_set_quant_format(m._h, prefix.encode(), bits, group))


def test_refusals(omx):
    from ominix_mlx_amd import engine
    cfg = CONFIGS["gqa4_d128"]
    over = {"bits": 4, "group_size": 64, "model.layers.0.self_attn.v_proj": {"bits": 8, "group_size": 64}}
    dims = dict(hidden_size=1024, num_hidden_layers=2, intermediate_size=3072, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                vocab_size=2048, max_context=256)
    with pytest.raises(omx.OmxError, match=r"set_quant_format: model\.layers\.0\.self_attn\.v_proj: .*experts"):
        engine.Model(**dims, quantization=over, num_experts=4, num_experts_per_tok=2, moe_intermediate_size=512)
    with pytest.raises(omx.OmxError, match=r"set_quant_format: model\.layers\.0\.self_attn\.v_proj: .*tensor / expert parallelism"):
        engine.Model(**dims, quantization=over, tp_size=2)
    with pytest.raises(omx.OmxError, match=r"set_quant_format: model\.layers\.0\.self_attn\.v_proj: .*float16 triplets"):
        engine.Model(**dims, quantization=dict(over, scales_dtype="float16"))
    with pytest.raises(omx.OmxError, match="no base quantization"):
        m = engine.Model(**dims)
        _set_format(omx, m, "model.layers.0.self_attn.v_proj", 6, 64)
    m = _model(cfg, {"bits": 4, "group_size": 64})
    for prefix in ("model.layers.9.self_attn.v_proj", "model.layers.0.self_attn.q_norm", "model.norm", "lm_head", "model.layers.x.mlp.up_proj"):
        with pytest.raises(omx.OmxError, match="unknown prefix " + prefix.replace(".", r"\.")):      # (lm_head: the config ties it)
            _set_format(omx, m, prefix, 6, 64)
    with pytest.raises(omx.OmxError, match="bits must be 2, 3, 4, 5, 6 or 8 .got 7."):
        _set_format(omx, m, "model.layers.0.self_attn.v_proj", 7, 64)
    with pytest.raises(omx.OmxError, match="group_size must be 32, 64 or 128 .got 48."):
        _set_format(omx, m, "model.layers.0.self_attn.v_proj", 6, 48)
    _set_format(omx, m, "model.layers.0.self_attn.v_proj", 6, 64)
    assert m.quant_format("model.layers.0.self_attn.v_proj") == (6, 64) and m.quant_format("model.layers.0.self_attn.k_proj") == (4, 64)
    m.synth_weights()
    with pytest.raises(omx.OmxError, match=r"model\.layers\.1\.mlp\.down_proj\.weight is already set"):
        _set_format(omx, m, "model.layers.1.mlp.down_proj", 6, 64)
    m.close()
    # gate and up of one layer in different formats: refused when the weights are resolved, naming the layer
    m = _model(cfg, {"bits": 4, "group_size": 64, "model.layers.1.mlp.up_proj": {"bits": 8, "group_size": 64}})
    m.synth_weights()
    with pytest.raises(omx.OmxError, match=r"layer 1: mlp\.gate_proj .4-bit group 64. and mlp\.up_proj .8-bit group 64. must share"):
        m.prefill(synth.prompt_ids(8, cfg.vocab_size))
    m.close()
    # a weight whose shape fits the base but not its override
    base, table = table_a(cfg)
    uniform, _, _ = checkpoints(cfg, base, {})
    m = _model(cfg, quantization(base, table))
    with pytest.raises(omx.OmxError, match=r"ShapeMismatch: model\.layers\.0\.(self_attn\.v_proj|mlp\.down_proj)\.weight"):
        m.load_weights(uniform)
    t = omx.ops.Tensor.from_numpy(uniform["model.layers.0.self_attn.v_proj.weight"], "u32")
    with pytest.raises(omx.OmxError, match=r"ShapeMismatch: model\.layers\.0\.self_attn\.v_proj\.weight"):      # ... at the C entry point too
        omx.check(omx.lib.omx_qwen3_set_weight(m._h, b"model.layers.0.self_attn.v_proj.weight", t.ptr, t.nbytes))
    m.close()


def test_a_group_that_does_not_divide_k_is_refused(omx):
    """The engine's contraction widths are multiples of 512, which every legal group divides: omx_qwen3_set_quant_format's check cannot
    fire on a model the engine accepts, so the refusal is reached through the launch (K = 1568 = 49 x 32 at 6 bits, group 64)."""
    lib = _bind_mixed(omx)
    T = omx.ops.Tensor
    K, members = 1568, [(64, 6, 32), (64, 6, 64)]
    dev = [(T.from_numpy(np.zeros((n, K * bits // 32), np.uint32), "u32"), T.from_numpy(np.zeros((n, K // 32), np.float32)),
            T.from_numpy(np.zeros((n, K // 32), np.float32))) for n, bits, _ in members]
    x = T.from_numpy(np.zeros((1, K), np.float32))
    out = T.from_numpy(np.zeros((128,), np.float32))
    with pytest.raises(omx.OmxError, match="1568.*divisible by the group size .64."):
        _mixed_launch(omx, lib, out, x, x, dev, members, K, PRO_NONE)
