"""CPU: tests/mlx_ops_rule.py, the numpy statement of the mlx-c array ops that tests/test_gpu_mlx_ops_sweep.py holds the kernels to, pinned
on answers known without it: hand-computed small cases for every rule, numpy's own stable sort / cumsum / floor_divide / remainder, and a
direct-loop convolution."""
import numpy as np
import pytest

import mlx_ops_rule as R


def test_promotion_table_is_symmetric_and_matches_its_description():
    """mlx-rs/src/dtype.rs:119-204 in words: bool yields; f32 wins among floats, f16 x bf16 -> f32; a float beats an integer; one
    signedness -> the wider; signed x unsigned -> the signed type holding both, uint64 x signed -> float32."""
    size = {"uint8": 1, "int8": 1, "uint16": 2, "int16": 2, "uint32": 4, "int32": 4, "uint64": 8, "int64": 8}
    signed_of = {1: "int8", 2: "int16", 4: "int32", 8: "int64"}

    def described(a, b):
        if a == b:
            return a
        if a == "bool" or b == "bool":
            return b if a == "bool" else a
        fa, fb = R.is_float(a), R.is_float(b)
        if fa and fb:
            return "float32"
        if fa or fb:
            return a if fa else b
        sa, sb = a.startswith("int"), b.startswith("int")
        if sa == sb:
            return a if size[a] >= size[b] else b
        sg, us = (a, b) if sa else (b, a)
        if size[us] == 8:
            return "float32"
        return sg if size[sg] > size[us] else signed_of[2 * size[us]]

    for a in R.DTYPES:
        for b in R.DTYPES:
            assert R.promote(a, b) == R.promote(b, a) == described(a, b), (a, b)
    # the rows the issue names, by hand
    assert R.promote("int32", "uint32") == "int64" and R.promote("uint8", "int8") == "int16" and R.promote("uint64", "int64") == "float32"
    assert R.promote("float16", "bfloat16") == "float32" and R.promote("int64", "float16") == "float16" and R.promote("bool", "uint8") == "uint8"


def test_casts_wrap_round_and_truncate():
    np.testing.assert_array_equal(R.cast(np.array([2 ** 31, -1, 2 ** 32 + 5], np.int64), "int32"), np.array([-2 ** 31, -1, 5], np.int32))
    np.testing.assert_array_equal(R.cast(np.array([-1, 256], np.int64), "uint8"), np.array([255, 0], np.uint8))
    np.testing.assert_array_equal(R.cast(np.array([-1], np.int64), "uint64"), np.array([2 ** 64 - 1], np.uint64))
    np.testing.assert_array_equal(R.cast(np.array([-2.7, 2.7], np.float32), "int32"), np.array([-2, 2], np.int32))          # toward zero
    # bfloat16: 8 significand bits, ties to even -- 1 + 2^-8 is a tie between 1 and 1 + 2^-7 (even: 1); 1 + 3 * 2^-8 ties up to 1 + 2^-6
    np.testing.assert_array_equal(R.bf16_round(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], np.float32)),
                                  np.array([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7], np.float32))
    assert R.bf16_round(np.float32(1.5)).shape == () and R.bf16_round(np.ones((2, 0, 3), np.float32)).shape == (2, 0, 3)
    assert np.isnan(R.bf16_round(np.array([np.nan], np.float32))[0]) and R.bf16_round(np.array([np.inf], np.float32))[0] == np.inf


def test_arithmetic_rules():
    a = np.array([2 ** 25 + 1, 2 ** 31 - 1, -2 ** 31], np.int32)
    v, dt = R.arith("add", a, "int32", np.array([0, 1, -1], np.int32), "int32")
    assert dt == "int32"
    np.testing.assert_array_equal(v, np.array([2 ** 25 + 1, -2 ** 31, 2 ** 31 - 1], np.int32))           # exact past 2^24; wraps at the limits
    v, dt = R.arith("multiply", np.array([2 ** 16 + 1], np.uint32), "uint32", np.array([2 ** 16 + 1], np.uint32), "uint32")
    assert dt == "uint32" and v.tolist() == [(2 ** 16 + 1) ** 2 % 2 ** 32]
    v, dt = R.arith("subtract", np.array([0], np.uint32), "uint32", np.array([1], np.int32), "int32")
    assert dt == "int64" and v.tolist() == [-1]
    v, dt = R.arith("divide", np.array([7, -7, 1, 0], np.int32), "int32", np.array([2, 2, 0, 0], np.int32), "int32")
    assert dt == "float32" and v[:2].tolist() == [3.5, -3.5] and np.isinf(v[2]) and np.isnan(v[3])
    v, dt = R.arith("add", np.array([1.0], np.float32), "bfloat16", np.array([2.0 ** -8], np.float32), "bfloat16")
    assert dt == "bfloat16" and v.tolist() == [1.0]                                                      # float32 sum, then ties-to-even
    v, dt = R.arith("add", np.array([True, False]), "bool", np.array([True, False]), "bool")
    assert dt == "bool" and v.tolist() == [True, False]


def test_comparison_maxmin_division_power_rules():
    nan = np.float32(np.nan)
    x, y = np.array([1, nan, 3, -0.0], np.float32), np.array([nan, 2, 2, 0.0], np.float32)
    v, _dt = R.maxmin("maximum", x, "float32", y, "float32")
    assert np.isnan(v[0]) and np.isnan(v[1]) and v[2] == 3
    v, _dt = R.maxmin("minimum", x, "float32", y, "float32")
    assert np.isnan(v[0]) and np.isnan(v[1]) and v[2] == 2
    assert R.compare("equal", x, "float32", y, "float32")[0].tolist() == [False, False, False, True]                  # NaN != NaN, -0 == +0
    assert R.compare("less", np.array([2 ** 53 + 1], np.int64), "int64", np.array([2 ** 53 + 2], np.int64), "int64")[0].tolist() == [True]
    a, b = np.array([7, -7, 7, -7, 5], np.int32), np.array([2, 2, -2, -2, 0], np.int32)
    assert R.floor_divide(a, "int32", b, "int32")[0].tolist() == [3, -4, -4, 3, 0]                                   # floor; x / 0 = 0
    assert R.remainder(a, "int32", b, "int32")[0].tolist() == [1, 1, -1, -1, 0]                                      # the divisor's sign
    safe = b.copy(); safe[-1] = 3
    np.testing.assert_array_equal(R.floor_divide(a, "int32", safe, "int32")[0], np.floor_divide(a, safe))
    np.testing.assert_array_equal(R.remainder(a, "int32", safe, "int32")[0], np.remainder(a, safe))
    f, g = np.array([5.5, -5.5, 5.5, -5.5], np.float32), np.array([2, 2, -2, -2], np.float32)
    np.testing.assert_array_equal(R.floor_divide(f, "float32", g, "float32")[0], np.floor_divide(f, g))
    np.testing.assert_array_equal(R.remainder(f, "float32", g, "float32")[0], np.remainder(f, g))
    assert R.remainder(f, "float32", g, "float32")[0].tolist() == [1.5, 0.5, -0.5, -1.5]
    v, dt = R.int_power(np.array([2, 3, 1, -1, -1, 5, 2], np.int32), "int32", np.array([10, 3, -4, -3, -2, -1, 31], np.int32), "int32")
    assert dt == "int32" and v.tolist() == [1024, 27, 1, -1, 1, 0, -2 ** 31]
    assert R.logical("logical_and", np.array([2, 0]), np.array([1, 1]))[0].tolist() == [True, False]
    assert R.logical("logical_not", np.array([2.5, 0.0]))[0].tolist() == [False, True]
    v, dt = R.where(np.array([1, 0]), np.array([5], np.uint8), "uint8", np.array([-1], np.int8), "int8")
    assert dt == "int16" and v.tolist() == [5, -1]


def test_unary_rules():
    v, dt = R.unary_exact("round", np.array([0.5, 1.5, 2.5, -0.5, -1.5], np.float32), "float32")
    assert dt == "float32" and v.tolist() == [0.0, 2.0, 2.0, -0.0, -2.0]                                              # half to even
    v, dt = R.unary_exact("abs", np.array([-2 ** 25 - 1, -128], np.int32), "int32")
    assert dt == "int32" and v.tolist() == [2 ** 25 + 1, 128]
    assert R.unary_exact("abs", np.array([-128], np.int8), "int8")[0].tolist() == [-128]                             # wraps in int8
    assert R.unary_exact("negative", np.array([1], np.uint8), "uint8")[0].tolist() == [255]
    assert R.unary_exact("sign", np.array([-3.0, 0.0, 2.0], np.float32), "bfloat16")[0].tolist() == [-1.0, 0.0, 1.0]
    assert R.unary_exact("isposinf", np.array([np.inf, -np.inf, np.nan], np.float32), "float32") [0].tolist() == [True, False, False]
    assert R.unary_dtype("exp", "int32") == "float32" and R.unary_dtype("exp", "float16") == "float16" and R.unary_dtype("isnan", "int8") == "bool"
    assert R.unary_dtype("floor", "int16") == "int16"
    np.testing.assert_allclose(R.unary_f64("sigmoid", np.array([0.0], np.float32), "float32")[0], [0.5])
    np.testing.assert_allclose(R.erf_f64(np.array([0.5], np.float32)), [0.5204998778130465], rtol=1e-15)


def test_reduction_rules():
    b = np.array([[True, True, False], [True, True, True]])
    v, dt = R.reduce("sum", b, "bool", axis=1)
    assert dt == "int32" and v.tolist() == [2, 3]                                                                   # bools count
    assert R.reduce("all", b, "bool", axis=1)[0].tolist() == [False, True] and R.reduce("any", b, "bool", axis=0)[1] == "bool"
    i = np.array([[1, 2], [3, 5]], np.int32)
    v, dt = R.reduce("mean", i, "int32", axis=0)
    assert dt == "float32" and v.tolist() == [2.0, 3.5]
    assert R.reduce_dtype("logsumexp", "uint8") == "float32" and R.reduce_dtype("logsumexp", "bfloat16") == "bfloat16"
    assert R.reduce("sum", np.array([2 ** 31 - 1, 1], np.int32), "int32")[0].tolist() == -2 ** 31                        # wraps in the dtype
    assert R.reduce("prod", np.array([16, 16], np.uint8), "uint8")[0].tolist() == 0
    f = np.array([[1, np.nan, 3], [4, 5, 6]], np.float32)
    v, _dt = R.reduce("max", f, "float32", axis=1)
    assert np.isnan(v[0]) and v[1] == 6                                                                             # NaN in one line only
    v, _dt = R.reduce("logsumexp", np.array([[-np.inf, -np.inf], [0, 0]], np.float32), "float32", axis=1)
    assert v[0] == -np.inf and abs(v[1] - np.log(2)) < 1e-15
    t = np.array([1, 7, 7, 0, 0], np.float32)
    assert R.argextreme("argmax", t)[0] == 1 and R.argextreme("argmin", t)[0] == 3                                 # ties: the first
    v, dt = R.var(np.array([1, 2, 3, 4], np.float32), "float32", ddof=1)
    assert dt == "float32" and abs(v - 5 / 3) < 1e-15


def test_scan_rules():
    a = np.array([[3, 1, 4, 1, 5]], np.int8)
    np.testing.assert_array_equal(R.scan("sum", a, "int8", 1)[0], np.cumsum(a, 1, dtype=np.int8))
    assert R.scan("sum", a, "int8", 1, reverse=True)[0].tolist() == [[14, 11, 10, 6, 5]]
    assert R.scan("sum", a, "int8", 1, inclusive=False)[0].tolist() == [[0, 3, 4, 8, 9]]
    assert R.scan("sum", a, "int8", 1, reverse=True, inclusive=False)[0].tolist() == [[11, 10, 6, 5, 0]]
    assert R.scan("max", a, "int8", 1, inclusive=False)[0].tolist() == [[-128, 3, 3, 4, 4]]                        # the dtype's own lowest
    assert R.scan("min", a, "int8", 1, inclusive=False)[0].tolist() == [[127, 3, 1, 1, 1]]
    assert R.scan("min", np.array([5], np.uint16), "uint16", 0, inclusive=False)[0].tolist() == [65535]
    assert R.scan("prod", np.array([100, 3], np.int8), "int8", 0)[0].tolist() == [100, 44]                          # 300 wraps to 44
    f = np.array([1, np.nan, 3, 2], np.float32)
    v, _dt = R.scan("max", f, "float32", 0)
    assert v[0] == 1 and np.isnan(v[1:]).all()                                                                      # NaN stays
    v, _dt = R.scan("max", f, "float32", 0, reverse=True)
    assert v[3] == 2 and v[2] == 3 and np.isnan(v[:2]).all()
    assert R.scan("max", np.array([1.0], np.float32), "float32", 0, inclusive=False)[0].tolist() == [-np.inf]
    x = np.random.default_rng(0).standard_normal((3, 7)).astype(np.float32)
    np.testing.assert_array_equal(R.scan("sum", x, "float32", 0)[0], np.cumsum(x.astype(np.float64), 0))


def test_order_and_gather_rules():
    g = np.random.default_rng(1)
    a = g.integers(0, 4, (3, 50)).astype(np.int64)
    np.testing.assert_array_equal(R.argsort(a, 1)[0], np.argsort(a, 1, kind="stable"))
    np.testing.assert_array_equal(R.sort(a, 0), np.sort(a, 0, kind="stable"))
    f = np.array([2, np.nan, -0.0, 0.0, 1, -0.0], np.float32)
    assert R.argsort(f)[0].tolist() == [2, 3, 5, 4, 0, 1]                                                            # zeros tie in index order; NaN last
    s = R.sort(f)
    assert R.is_partition(s, 2, s) and R.is_partition(f[[2, 5, 3, 1, 0, 4]], 2, s) and not R.is_partition(f[[0, 5, 3, 1, 2, 4]], 2, s)
    t = np.arange(12).reshape(4, 3)
    assert R.wrap_index([-1, -4, 3, 9, -9], 4).tolist() == [3, 0, 3, 3, 0]                                            # wrap, then clamp
    np.testing.assert_array_equal(R.take_axis(t, np.array([[-1, 0], [2, 2]]), 0), t[[[3, 0], [2, 2]]])
    np.testing.assert_array_equal(R.take(t, np.array([-1, 5])), np.array([11, 5]))
    np.testing.assert_array_equal(R.take_along_axis(t, np.array([[0, -1]]), 1), t[:, [0, 2]])                       # indices broadcast over rows


@pytest.mark.parametrize("stride,padding,dilation,groups", [(1, 0, 1, 1), (2, 2, 2, 2), (1, 2, 1, 4)])
def test_convolution_against_a_direct_loop(stride, padding, dilation, groups):
    g = np.random.default_rng(2)
    B, L, Cin, Cout, K = 2, 9, 4, 8, 3
    x, w = g.standard_normal((B, L, Cin)).astype(np.float32), g.standard_normal((Cout, K, Cin // groups)).astype(np.float32)
    got, mag = R.conv1d_f64(x, w, stride, padding, dilation, groups)
    Lout = (L + 2 * padding - dilation * (K - 1) - 1) // stride + 1
    want = np.zeros((B, Lout, Cout))
    cig, cog = Cin // groups, Cout // groups
    for b in range(B):
        for t in range(Lout):
            for co in range(Cout):
                for k in range(K):
                    p = t * stride - padding + k * dilation
                    if 0 <= p < L:
                        for ci in range(cig):
                            want[b, t, co] += float(x[b, p, (co // cog) * cig + ci]) * float(w[co, k, ci])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    assert got.shape == (B, Lout, Cout) and (mag >= np.abs(got) - 1e-13).all()
    # the 2-D form on a non-square image and kernel reduces to the 1-D one along each axis
    x2, w2 = g.standard_normal((1, 5, 7, 2)).astype(np.float32), g.standard_normal((2, 1, 3, 2)).astype(np.float32)
    y2, _m = R.conv2d_f64(x2, w2, (1, stride), (0, padding), (1, dilation), 1)
    for row in range(5):
        np.testing.assert_allclose(y2[:, row], R.conv1d_f64(x2[:, row], w2[:, 0], stride, padding, dilation, 1)[0], atol=1e-13)


def test_softmax_and_bounds():
    p = R.softmax_f64(np.array([[1e4, 1e4 - 1], [-np.inf, 0]], np.float32), 1)
    np.testing.assert_allclose(p, [[1 / (1 + np.exp(-1)), np.exp(-1) / (1 + np.exp(-1))], [0, 1]], rtol=1e-15)
    assert R.out_rounding(1.0, "bfloat16") > 2.0 ** -9 and R.out_rounding(1.0, "float16") < 2.0 ** -10 and R.U == 2.0 ** -24
