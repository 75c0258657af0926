"""The Fun-ASR-Nano audio tower on the device (csrc/sensevoice_encoder.hip; audio.FunASRNanoEncoder) against tests/funasr_nano_rule.py, a
numpy float64 restatement of funasr-nano-mlx/src/sensevoice_encoder.rs and adaptor.rs.

Tolerance: the project's float32 form (tests/test_gpu_paraformer.py, TOL["f32"]): error <= 1e-4 x the largest magnitude of the float64
result, PER UTTERANCE.  Every test prints its measured worst ratio error / (1e-4 x max|ref|); DESIGN 4.14 quotes them."""
import functools

import numpy as np
import pytest

import funasr_nano_rule as rule

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _worst(got, ref, lengths):
    """largest error / (TOL * max|ref|) over the utterances, each held to its own largest magnitude"""
    worst = 0.0
    for lo, hi in rule.segments(lengths):
        worst = max(worst, float(np.abs(got[lo:hi] - ref[lo:hi]).max() / (TOL * np.abs(ref[lo:hi]).max())))
    return worst


# ---- 1. segment attention alone ----

SEGMENT_LISTS = [(1,), (16,), (17,), (1, 1, 1), (5, 16, 33), (512,), (511, 1), (96, 200, 7, 300)]


@pytest.mark.parametrize("lengths", SEGMENT_LISTS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("heads", [4, 8])
def test_segment_attention(omx, heads, lengths):
    """q | k | v read in place from a stacked projection whose rows are 3 dim + 8 floats apart; compared with the per-utterance form and
    with full attention under a block-diagonal -1e9 mask (the two agree to float64 rounding: exp(-1e9 - max) is 0)"""
    from ominix_mlx_amd import audio
    dim, T = heads * 128, int(sum(lengths))
    g = np.random.default_rng(100 * heads + T)
    qkv = np.zeros((T, 3 * dim + 8), np.float32)
    qkv[:, :3 * dim] = g.standard_normal((T, 3 * dim)).astype(np.float32)
    qkv[:, 3 * dim:] = np.nan                                        # the padding columns are nobody's operand
    x = qkv.astype(np.float64)
    q, k, v = x[:, :dim], x[:, dim:2 * dim], x[:, 2 * dim:3 * dim]
    ref = rule.attention(q, k, v, heads, lengths)
    masked = rule.attention(q, k, v, heads, mask=rule.block_mask(lengths))
    assert np.abs(ref - masked).max() <= 1e-12 * np.abs(ref).max()
    got = audio.segment_attention_f32(omx.ops.Tensor.from_numpy(qkv, "f32"), heads, lengths).numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    w = _worst(got, ref, lengths)
    print(f"segment attention heads={heads} segments={lengths}: worst ratio {w:.4f}")
    assert w <= 1.0


# ---- 2. one layer ----

def _layer_weights(in_dim, dim, ffn, k, seed):
    g = np.random.default_rng(seed)
    r = lambda *s, sc=1.0: (g.standard_normal(s) * sc).astype(np.float32)
    return {"norm1_w": r(in_dim, sc=0.1) + 1, "norm1_b": r(in_dim, sc=0.1), "qkv_w": r(3 * dim, in_dim, sc=in_dim ** -0.5), "qkv_b": r(3 * dim, sc=0.1),
            "out_w": r(dim, dim, sc=dim ** -0.5), "out_b": r(dim, sc=0.1), "fsmn_w": r(dim, k, sc=0.3), "norm2_w": r(dim, sc=0.1) + 1,
            "norm2_b": r(dim, sc=0.1), "ffn_up_w": r(ffn, dim, sc=dim ** -0.5), "ffn_up_b": r(ffn, sc=0.1), "ffn_down_w": r(dim, ffn, sc=ffn ** -0.5),
            "ffn_down_b": r(dim, sc=0.1)}


@pytest.mark.parametrize("lengths", [(3,), (5, 11, 1, 40)], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("in_dim,dim,heads,ffn", [(512, 512, 4, 2048), (560, 512, 4, 2048), (256, 256, 2, 512)],
                         ids=["real", "first_560", "narrow_unfused"])
def test_one_layer(omx, in_dim, dim, heads, ffn, lengths):
    """utterances shorter than the FSMN's 5-tap reach and one of a single row; the 560 -> 512 layer without its residual; a width (256)
    the fused epilogue does not take.  The reference of an utterance is that utterance through the layer ALONE."""
    from ominix_mlx_amd import paraformer
    k, T = 11, int(sum(lengths))
    w = _layer_weights(in_dim, dim, ffn, k, 7)
    x = np.random.default_rng(8).standard_normal((T, in_dim)).astype(np.float32)
    ref = np.concatenate([rule.encoder_layer(x[lo:hi], w, heads) for lo, hi in rule.segments(lengths)])
    got = paraformer.SanmEncoderLayer(w, heads, k, "f32").forward_segments(omx.ops.Tensor.from_numpy(x, "f32"), lengths).numpy()
    assert got.shape == ref.shape
    ws = _worst(got, ref, lengths)
    print(f"layer {in_dim}->{dim} segments={lengths}: worst ratio {ws:.4f}")
    assert ws <= 1.0
    if len(lengths) > 1:
        # a leak across a boundary is an O(1) error: the layer over the rows as ONE utterance is far outside the tolerance
        leak = rule.encoder_layer(x, w, heads)
        assert _worst(leak, ref, lengths) > 100.0


# ---- 3. the tiny tower end to end ----

TOWER_SEGMENTS = [(37,), (1,), (20, 84, 3), (9, 1, 33, 16, 17, 2, 48, 5)]
STAGES = ("after_norm", "tp_norm", "linear2")


@functools.lru_cache(maxsize=None)
def _tiny():
    cfg = rule.TINY_CFG
    w = rule.synth_weights(cfg, 3)
    return cfg, w


_ENC = {}


def _encoder():
    from ominix_mlx_amd import audio
    if "e" not in _ENC:
        cfg, w = _tiny()
        e = audio.FunASRNanoEncoder(**cfg)
        e.load_weights(w)
        _ENC["e"] = e
    return _ENC["e"]


def _rows(T, seed=21):
    return np.random.default_rng(seed).standard_normal((T, rule.TINY_CFG["lfr_dim"])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _alone_ref(length, offset):
    """float64 stages of one utterance alone (rows [offset, offset + length) of the shared input)"""
    cfg, w = _tiny()
    return rule.tower(_rows(200)[offset:offset + length], w, cfg)


@pytest.mark.parametrize("lengths", TOWER_SEGMENTS, ids=lambda v: "-".join(map(str, v)))
def test_tiny_tower(omx, lengths):
    cfg, w = _tiny()
    e = _encoder()
    T = int(sum(lengths))
    x = _rows(200)[:T]
    out = e.forward(x, lengths)
    assert out.shape == (T, cfg["llm_dim"])
    got = {"out": out.numpy()}
    for name in STAGES:
        width = cfg["llm_dim"] if name == "linear2" else cfg["output_size"]
        got[name] = e.debug_read(name, (T, width))
    got["pos"] = e.debug_read("pos", (T, cfg["lfr_dim"]))
    spans = rule.segments(lengths)
    ref = {name: np.concatenate([_alone_ref(hi - lo, lo)[name] for lo, hi in spans]) for name in got}
    for name in ("pos",) + STAGES + ("out",):
        ws = _worst(got[name], ref[name], lengths)
        print(f"tower segments={lengths} stage {name}: worst ratio {ws:.4f}")
        assert ws <= 1.0, name
    # each utterance of the joint pass against the SAME utterance passed alone on the device
    for lo, hi in spans:
        alone = e.forward(x[lo:hi], [hi - lo]).numpy()
        r = _alone_ref(hi - lo, lo)["out"]
        assert np.abs(alone - r).max() <= TOL * np.abs(r).max()
        assert np.abs(got["out"][lo:hi] - alone).max() <= TOL * np.abs(r).max()


# ---- 4. refusals ----

def test_refusals_are_named(omx):
    from ominix_mlx_amd import audio
    cfg, w = _tiny()
    e = _encoder()
    x = _rows(600, seed=5)
    with pytest.raises(omx.OmxError, match="InvalidConfig.*513 rows"):
        e.forward(x[:513], [513])
    with pytest.raises(omx.OmxError, match="InvalidConfig.*513 rows"):
        e.forward(x[:520], [7, 513])
    with pytest.raises(omx.OmxError, match="InvalidConfig.*9 utterances"):
        e.forward(x[:18], [2] * 9)
    with pytest.raises(omx.OmxError, match="utterance 1 has 0 rows"):
        e.forward(x[:4], [4, 0])
    with pytest.raises(omx.OmxError, match="ShapeMismatch"):
        e.forward(np.zeros((4, cfg["lfr_dim"] + 1), np.float32), [4])
    with pytest.raises(omx.OmxError, match="InvalidConfig.*head width"):
        audio.FunASRNanoEncoder(**dict(cfg, attention_heads=4))      # 256 / 4 = 64
    with pytest.raises(omx.OmxError, match="InvalidConfig.*adaptor: head width"):
        audio.FunASRNanoEncoder(**dict(cfg, llm_dim=2560))           # funasr-qwen4b's width: 2560 / 8 = 320
    with pytest.raises(omx.OmxError, match="InvalidConfig.*kernel_size 10"):
        audio.FunASRNanoEncoder(**dict(cfg, kernel_size=10))
    with pytest.raises(omx.OmxError, match="InvalidConfig.*kernel_size 33"):
        audio.FunASRNanoEncoder(**dict(cfg, kernel_size=33))
    with pytest.raises(omx.OmxError, match="ShapeMismatch.*encoder.after_norm.weight"):
        e.load_weights({"encoder.after_norm.weight": np.zeros(cfg["output_size"] + 4, np.float32)})
    with pytest.raises(omx.OmxError, match="not a tensor of this model"):
        e.load_weights({"encoder.encoders.7.norm1.weight": np.zeros(cfg["output_size"], np.float32)})   # the tiny tower has 2 of them
    import ctypes
    with pytest.raises(omx.OmxError, match="encoder.after_norm.weight: null tensor"):
        omx.check(omx.lib.omx_funasr_nano_encoder_load(e._h, b"encoder.after_norm.weight", None, (ctypes.c_int64 * 1)(cfg["output_size"]), 1))
    fresh = audio.FunASRNanoEncoder(**cfg)
    with pytest.raises(omx.OmxError, match="WeightNotFound"):
        fresh.forward(x[:4], [4])
    fresh.close()
    # the handle still works: nothing was launched or replaced by the refused calls
    r = _alone_ref(37, 0)["out"]
    assert np.abs(e.forward(_rows(200)[:37], [37]).numpy() - r).max() <= TOL * np.abs(r).max()
