"""CPU: the 8-bit K/V cache rule (tests/kv_quant_rule.py) by itself -- what the round trip costs per element, its edge groups, trim,
and the condition the GPU parity test (tests/test_gpu_batch_kv8.py) rests on: the kv8 oracle's own near-ties are a minority."""
import numpy as np
import pytest

import kv_quant_rule as kq
from oracle import ref_core as rc


def _rows(seed, scale=1.0, shape=(512, 128)):
    return rc.bf16_round(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale)


def _errors(x):
    """(|x - x_hat| per element, |scale| / 2, rounding slack of scale and bias) of rows x, groups of 64 on their own axis"""
    q, s, b = rc.quantize(x, kq.GROUP, kq.BITS)
    err = np.abs(kq.kv8_round_trip(x).astype(np.float64) - x).reshape(*s.shape, kq.GROUP)
    half = (np.abs(s).astype(np.float64) / 2)[..., None]
    # scale and bias each move by at most half a bf16 ulp (8 significand bits: 2^-8 relative); the code multiplies the scale's by up to 255
    slack = ((255 * np.abs(s) + np.abs(b)).astype(np.float64) * 2.0 ** -8)[..., None]
    codes = ((q[..., None] >> (np.arange(4, dtype=np.uint32) * np.uint32(8))) & np.uint32(0xFF)).reshape(*s.shape, kq.GROUP)
    t = (x.reshape(*s.shape, kq.GROUP).astype(np.float64) - b[..., None]) / s[..., None]     # the unclipped code of every element
    return err, half, slack, codes, t


@pytest.mark.parametrize("scale", [1.0, 0.1, 30.0])
def test_round_trip_error_is_within_half_a_step(scale):
    """Per element |x - x_hat| <= |scale| / 2 + the bf16 rounding of scale and bias (half an ulp each, 2^-8 relative; the scale's
    is multiplied by a code of up to 255).  The rounding terms are not a formality: together they are about |scale| to 1.5 |scale|,
    and they are what covers the one element the half step alone does not -- see test_round_trip_error_by_element_kind."""
    err, half, slack, _, _ = _errors(_rows(11, scale))
    ratio = err / (half + slack)
    print(f"scale {scale}: worst error {ratio.max():.3f} x bound, {(err / (2 * half)).max():.3f} |scale|")
    assert (ratio <= 1).all()


@pytest.mark.parametrize("scale", [1.0, 0.1, 30.0])
def test_round_trip_error_by_element_kind(scale):
    """Where the error comes from.  MLX makes the group's larger-magnitude extreme an exact code (q0 = rint(edge / scale), scale :=
    edge / q0), which moves the OTHER extreme to an unclipped code (x - bias) / scale of up to 256.0: above 255.5 it is clipped to 255
    and sits up to one |scale| off before any rounding (a fifth of these groups hold such an element) -- the reference's own bound
    range / 2^bits (ops/quantization.rs:289-305).  Every other element is within half a step of its code."""
    x = _rows(11, scale)
    q, s, b = rc.quantize(x, kq.GROUP, kq.BITS)
    exact = np.abs(kq.dequantize64(q, s, b) - x).reshape(*s.shape, kq.GROUP)      # scale and bias NOT rounded to bf16
    _, half, _, codes, t = _errors(x)
    inside = (t >= -0.5) & (t <= 255.5)
    f32 = 2.0 ** -20 * (np.abs(x).reshape(exact.shape) + 256 * 2 * half)             # the float32 steps of the quantiser itself
    assert (exact <= half + f32)[inside].all()
    assert (t <= 256.0 + 1e-3).all() and (t >= -0.5 - 1e-3).all()
    assert (codes[~inside] == 255).all()
    assert (exact <= 2 * half + f32)[~inside].all()
    clipped = int((~inside).any(axis=-1).sum())
    print(f"scale {scale}: {clipped} of {inside.shape[0] * inside.shape[1]} groups hold a clipped far extreme")
    assert clipped > 0, "these rows are meant to hold clipped extremes"


def test_constant_and_zero_groups():
    """A constant group: scale falls to the 1e-7 floor, every code is the edge's, the value comes back as bias (exact on the bf16
    grid).  An all-zero group: bias 0, codes 0, exact zeros; no NaN or inf anywhere."""
    x = np.zeros((3, 128), dtype=np.float32)
    x[1, :64] = 0.375
    x[2, 64:] = -2.5
    q, s, b = kq.kv8_triplet(x)
    back = kq.kv8_round_trip(x)
    assert np.isfinite(s).all() and np.isfinite(b).all() and np.isfinite(back).all()
    np.testing.assert_array_equal(back[0], 0.0)
    np.testing.assert_array_equal(q[0], 0)
    np.testing.assert_allclose(back[1, :64], 0.375, rtol=0, atol=255 * 1e-7 * 1.01)
    np.testing.assert_allclose(back[2, 64:], -2.5, rtol=0, atol=255 * 1e-7 * 1.01)
    np.testing.assert_array_equal(back[1, 64:], 0.0)
    np.testing.assert_array_equal(back[2, :64], 0.0)


def test_cache_stores_the_round_trip_and_trims():
    g = np.random.default_rng(5)
    k1, v1 = (rc.bf16_round(g.standard_normal((1, 2, 7, 64)).astype(np.float32)) for _ in range(2))
    k2, v2 = (rc.bf16_round(g.standard_normal((1, 2, 3, 64)).astype(np.float32)) for _ in range(2))
    c = kq.KV8Cache()
    k, v = c.update_and_fetch(k1, v1)
    np.testing.assert_array_equal(k, kq.kv8_round_trip(k1))
    np.testing.assert_array_equal(v, kq.kv8_round_trip(v1))
    assert k.dtype == np.float32 and (k != k1).any()
    k, v = c.update_and_fetch(k2, v2)
    assert c.offset() == 10 and k.shape == (1, 2, 10, 64)
    np.testing.assert_array_equal(k[:, :, 7:], kq.kv8_round_trip(k2))
    # a row's codes depend on that row alone: appended after a trim, the same rows give the same cache
    assert c.trim(3) == 3 and c.offset() == 7
    k, v = c.update_and_fetch(k2, v2)
    np.testing.assert_array_equal(k[:, :, :7], kq.kv8_round_trip(k1))
    np.testing.assert_array_equal(v[:, :, 7:], kq.kv8_round_trip(v2))
    # the stored value is a fixed point of the rule up to one code: quantising it again moves no element by more than a step
    again = kq.kv8_round_trip(rc.bf16_round(k))
    s = np.repeat(np.abs(kq.kv8_triplet(rc.bf16_round(k))[1]), kq.GROUP, axis=-1)
    assert (np.abs(again - k) <= 1.5 * s + np.abs(k) * 2.0 ** -8).all()


@pytest.mark.parametrize("name,want", [("narrow", 39), ("wide", 34), ("narrow_q4", 38)])
def test_the_kv8_oracle_alone_is_mostly_decided(name, want):
    """The GPU parity test lets a token differ where the oracle's margin is <= 2 x bound, so such positions must be a minority of
    the 96 for the oracle alone: 39 (narrow), 34 (wide), 38 (narrow_q4) with exactly the cache class the GPU test uses."""
    n = kq.near_ties(name)
    print(f"{name}: {n} of {8 * kq.N_POS} positions of the kv8 oracle are near-ties")
    assert n <= 8 * kq.N_POS // 2
    assert n == want
