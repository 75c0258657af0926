"""GPU: the mlx-c handle layer's own array ops (csrc/mlxc.hip, mlxc_glue.hpp, mlxc_glue2.hpp and their generic kernels) held to
tests/mlx_ops_rule.py across dtypes, operand layouts and the sizes at which each kernel's structure changes.  Every case is built from a
fixed seed.  Integer, boolean, layout, order, gather and IEEE-exact float results are compared bit for bit; the rest under the bounds
derived next to each family (u = 2^-24, plus half an ulp of the result dtype for the final rounding).

Left out on purpose: uint64 values of 2^63 and above (the integer kernels hold every integer in a signed 64-bit word), float -> integer
casts of out-of-range values (undefined), NaN in argmax / argmin inputs, maximum / minimum of two zeros of opposite sign."""
import numpy as np
import pytest

import mlx_ops_rule as R

pytestmark = pytest.mark.gpu

# Maximum error of the device math functions, in float32 ulp of |ref|.  No copy of the ROCm math-function accuracy tables ships with the
# toolchain this suite builds against, so every figure is the ASSUMED 4 ulp (never tuned to what the kernels return).
ULP32 = 2.0 ** -23
TRANSCENDENTAL_ULP = {op: 4 for op in ("exp", "sigmoid", "log", "log2", "log10", "log1p", "expm1", "sin", "cos", "tan", "tanh", "sinh", "cosh",
                                       "arcsin", "arccos", "arctan", "arcsinh", "arccosh", "arctanh", "erf", "sqrt", "rsqrt", "power", "logaddexp")}
# where each function is well-conditioned (no poles, no domain edges, no zero crossings of the result other than at 0)
DOMAIN = {"exp": (-10, 10), "sigmoid": (-10, 10), "log": (1.5, 100), "log2": (1.5, 100), "log10": (1.5, 100), "log1p": (0.1, 10), "expm1": (-5, 5),
          "sin": (-1.5, 1.5), "cos": (-1.2, 1.2), "tan": (-1.2, 1.2), "tanh": (-3, 3), "sinh": (-5, 5), "cosh": (-5, 5), "arcsin": (-0.9, 0.9),
          "arccos": (-0.9, 0.9), "arctan": (-10, 10), "arcsinh": (-10, 10), "arccosh": (1.5, 50), "arctanh": (-0.9, 0.9), "erf": (-2, 2),
          "sqrt": (0.01, 100), "rsqrt": (0.01, 100)}
BIG = 2 ** 21 + 257          # past grid_for()'s 8192 x 256 threads: the second trip of every grid-stride loop
AXIS_N = [1, 2, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def mx(omx):
    from ominix_mlx_amd import mlx_c
    return mlx_c


def code(mx, dt):
    return getattr(mx, dt.upper())


def up(mx, a, dt):
    return mx.Array.from_numpy(np.asarray(a), code(mx, dt))


def rng(*key):
    return np.random.default_rng([2024, *key])


def in_dtype(x, dt):
    """Host values as the device will hold them: rounded into `dt` (bfloat16 as float32 values)."""
    with np.errstate(all="ignore"):
        return R.bf16_round(x) if dt == "bfloat16" else np.asarray(x).astype(R.NP[dt])


_INT_POOL = [0, 1, 2, 3, 7, -1, -2, -7, 100, -100, 127, -128, 255, 2 ** 15 - 1, -2 ** 15, 2 ** 16 - 1, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 25 + 1, -2 ** 25 - 1,
             2 ** 31 - 1, -2 ** 31, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 53 + 1, -2 ** 53 - 1, 2 ** 62 + 3]


def vals(g, shape, dt, specials=True):
    """Seeded values of `dt`: integers on both sides of 2^24 and next to the type's limits; floats with NaN, +-inf, +-0.0 up front."""
    n = int(np.prod(shape))
    if dt == "bool":
        return g.integers(0, 2, shape).astype(bool)
    if dt in R.INTS:
        info = np.iinfo(R.NP[dt])
        lo, hi = (int(info.min), int(info.max)) if info.bits < 64 else (-2 ** 62 - 3 if info.min else 0, 2 ** 62 + 3)   # (64-bit: clear of -2^63 / -1 and 2^63)
        pool = [v for v in _INT_POOL if lo <= v <= hi] + [lo, hi]
        flat = np.array([pool[i] for i in g.integers(0, len(pool), n)], dtype=object)
        if specials:
            flat[:min(n, len(pool))] = pool[:n]
        return np.array(flat.tolist(), dtype=R.NP[dt]).reshape(shape)
    flat = (g.standard_normal(n) * 4).astype(np.float32)
    if specials:
        sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, 1.5, 2.5, -0.5, -2.5, 1.0], np.float32)
        flat[:min(n, sp.size)] = sp[:n]
    return in_dtype(flat.reshape(shape), dt)


def bits_equal(got, want, dt, msg=""):
    """Bit for bit (every NaN counts as the same NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} vs {want.shape}"
    if dt in R.FLOATS:
        g32, w32 = got.astype(np.float32), want.astype(np.float32)          # exact widenings
        nan = np.isnan(w32)
        np.testing.assert_array_equal(np.isnan(g32), nan, err_msg=msg)
        np.testing.assert_array_equal(np.where(nan, np.float32(0), g32).view(np.uint32), np.where(nan, np.float32(0), w32).view(np.uint32), err_msg=msg)
    else:
        np.testing.assert_array_equal(got, want.astype(R.NP[dt]), err_msg=msg)


def same(mx, arr, want, dt, msg=""):
    assert arr.dtype == code(mx, dt), f"{msg}: result dtype {arr.dtype}, the rule says {dt} ({code(mx, dt)})"
    bits_equal(arr.numpy(), want, dt, msg)


def close(mx, arr, ref64, bound, dt, msg=""):
    """|got - ref| <= bound + the rounding into dt; where the reference is not finite the result must be the same non-finite value."""
    assert arr.dtype == code(mx, dt), f"{msg}: result dtype {arr.dtype}, the rule says {dt}"
    got, ref = arr.numpy().astype(np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref.shape, f"{msg}: shape {got.shape} vs {ref.shape}"
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(got[~fin], ref[~fin], err_msg=msg)
    err, lim = np.abs(got[fin] - ref[fin]), (np.broadcast_to(bound, ref.shape)[fin] + R.out_rounding(ref[fin], dt))
    worst = int(np.argmax(err - lim)) if err.size else 0
    assert (err <= lim).all(), f"{msg}: error {err[worst]:.3e} over the bound {lim[worst]:.3e} at reference {ref[fin][worst]!r}"


# ---- operand layouts, built with the ABI's own view ops ----------------------------------------------------------------------
LAYOUTS = ["contiguous", "transposed", "strided", "broadcast", "scalar", "offset1"]


def lay(mx, a, dt, kind):
    """(handle, logical values): `a` presented through the layout `kind`."""
    a = np.asarray(a)
    if kind == "contiguous":
        return up(mx, a, dt), a
    if kind == "transposed":
        rev = list(range(a.ndim))[::-1]
        return mx.transpose_axes(up(mx, np.ascontiguousarray(a.transpose(rev)), dt), rev), a
    if kind == "strided":                                   # [1::2] along axis 0 of a buffer twice as long
        buf = np.zeros((2 * a.shape[0] + 1,) + a.shape[1:], a.dtype)
        buf[1::2] = a
        return mx.slice(up(mx, buf, dt), [1] + [0] * (a.ndim - 1), list(buf.shape), [2] + [1] * (a.ndim - 1)), a
    if kind == "broadcast":                                 # stride 0 along axis 0
        return mx.broadcast_to(up(mx, a[:1], dt), list(a.shape)), np.broadcast_to(a[:1], a.shape)
    if kind == "scalar":
        v = a.reshape(-1)[-1]
        return up(mx, np.asarray(v), dt), np.asarray(v)
    flat = a.reshape(-1)                                    # offset1: contiguous, 1-D, one element into its buffer
    buf = np.concatenate([flat[:1], flat])
    return mx.slice(up(mx, buf, dt), [1], [buf.size]), flat


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------
ARITH = {"add": "add", "subtract": "subtract", "multiply": "multiply", "divide": "divide"}


@pytest.mark.parametrize("op", list(ARITH))
def test_arithmetic_every_dtype_pair_in_every_mode(mx, op):
    """Every pair of the promotion table, broadcast both ways; integer results exact modulo 2^width, float results one float32 operation
    rounded once.  Immediate, deferred and deferred + fused execution agree bit for bit."""
    fn = getattr(mx, op)
    try:
        for ia, adt in enumerate(R.DTYPES):
            for ib, bdt in enumerate(R.DTYPES):
                g = rng(1, ia, ib)
                for sa, sb in (((5, 8), (8,)), ((5, 1), (1, 8))):
                    a, b = vals(g, sa, adt), vals(g, sb, bdt)
                    with np.errstate(all="ignore"):
                        want, rdt = R.arith(op, a, adt, b, bdt)
                    outs = []
                    for lazy, fuse in ((False, False), (True, False), (True, True)):
                        mx.lazy_mode(lazy, fuse)
                        got = fn(up(mx, a, adt), up(mx, b, bdt))
                        same(mx, got, want, rdt, f"{op} {adt} {sa} x {bdt} {sb} lazy={lazy} fuse={fuse}")
                        outs.append(got.numpy())
                    bits_equal(outs[1], outs[0], rdt), bits_equal(outs[2], outs[0], rdt)
    finally:
        mx.lazy_mode(True, True)


def test_integer_arithmetic_is_exact_past_2_24_and_wraps(mx):
    """The cases of the issue, by hand: int32(2^25 + 1) + 0; products and sums past 2^31 wrap in the result dtype."""
    a = np.array([2 ** 25 + 1, 2 ** 31 - 1, -2 ** 31, 46341, 2 ** 24 + 1], np.int32)
    b = np.array([0, 1, -1, 46341, 2 ** 24 + 1], np.int32)
    A, B = up(mx, a, "int32"), up(mx, b, "int32")
    assert mx.add(A, B).numpy().tolist() == [2 ** 25 + 1, -2 ** 31, 2 ** 31 - 1, 92682, 2 ** 25 + 2]
    assert mx.subtract(A, B).numpy().tolist() == [2 ** 25 + 1, 2 ** 31 - 2, -2 ** 31 + 1, 0, 0]
    assert mx.multiply(A, B).numpy().tolist() == [0, 2 ** 31 - 1, -2 ** 31, 46341 ** 2 - 2 ** 32, (2 ** 24 + 1) ** 2 % 2 ** 32]
    mixed = mx.add(up(mx, np.array([2 ** 32 - 1], np.uint32), "uint32"), up(mx, np.array([-1], np.int32), "int32"))
    assert mixed.dtype == mx.INT64 and mixed.numpy().tolist() == [2 ** 32 - 2]                       # int32 x uint32 -> int64
    q = mx.divide(up(mx, np.array([7, -7, 1], np.int32), "int32"), up(mx, np.array([2, 2, 0], np.int32), "int32"))
    assert q.dtype == mx.FLOAT32 and q.numpy().tolist() == [3.5, -3.5, np.inf]                       # integer / integer -> float32


# (a 1-D view at offset 1 only meets 1-D partners: itself, a whole 1-D array, a scalar)
LAYOUT_PAIRS = [(a, b) for a in LAYOUTS for b in LAYOUTS if "offset1" not in (a, b) or {a, b} <= {"offset1", "scalar", "contiguous"}]


@pytest.mark.parametrize("kind_a,kind_b", LAYOUT_PAIRS)
def test_arithmetic_operand_layouts(mx, kind_a, kind_b):
    """Each layout on each side; a 1-D contiguous view at element offset 1 (length a multiple of the vector width: only the alignment
    term of vec_ok() sends it to the general kernel) gives the bits of the aligned run of the same values."""
    one_d = "offset1" in (kind_a, kind_b)
    for dt in ("float32", "bfloat16", "float16", "int32", "uint8"):
        g = rng(2, LAYOUTS.index(kind_a), LAYOUTS.index(kind_b), R.DTYPES.index(dt))
        shape = (64,) if one_d else (6, 8)
        a, b = vals(g, shape, dt), vals(g, shape, dt)
        (A, la), (B, lb) = lay(mx, a, dt, kind_a), lay(mx, b, dt, kind_b)
        for op in ("add", "multiply", "divide"):
            with np.errstate(all="ignore"):
                want, rdt = R.arith(op, la, dt, lb, dt)
            got = getattr(mx, op)(A, B)
            same(mx, got, want, rdt, f"{op} {dt} {kind_a} x {kind_b}")
            if one_d and la.shape == lb.shape:
                aligned = getattr(mx, op)(up(mx, la, dt), up(mx, lb, dt))
                bits_equal(got.numpy(), aligned.numpy(), rdt, f"{op} {dt}: offset view vs aligned run")
        if dt in R.FLOATS:                                  # the unary pair of kernels on the same views
            for name, fn in (("negative", mx.negative), ("exp", mx.exp), ("sigmoid", mx.sigmoid)):
                got = fn(A)
                assert got.dtype == code(mx, dt)
                bits_equal(got.numpy(), fn(up(mx, la, dt)).numpy(), dt, f"{name} {dt} {kind_a} vs the contiguous aligned run")


# ---- comparison, logical and the rest --------------------------------------------------------------------------------------------
BINARY2 = ["greater", "greater_equal", "less", "less_equal", "equal", "not_equal", "logical_and", "logical_or", "maximum", "minimum",
           "floor_divide", "remainder"]


def _binary2_rule(op, a, adt, b, bdt):
    if op in R.COMPARISONS:
        return R.compare(op, a, adt, b, bdt)
    if op.startswith("logical"):
        return R.logical(op, a, b)
    if op in ("maximum", "minimum"):
        return R.maxmin(op, a, adt, b, bdt)
    return (R.floor_divide if op == "floor_divide" else R.remainder)(a, adt, b, bdt)


@pytest.mark.parametrize("op", BINARY2)
def test_comparison_logical_maxmin_division_every_dtype_pair(mx, op):
    """NaN, +-inf, +-0.0, negative operands and zero divisors on both sides, every dtype pair, broadcast; exact."""
    for ia, adt in enumerate(R.DTYPES):
        for ib, bdt in enumerate(R.DTYPES):
            g = rng(3, ia, ib)
            a, b = vals(g, (4, 16), adt), vals(g, (16,), bdt)
            if op in ("maximum", "minimum"):                # no zero meets a zero of the other sign (the pick is unspecified)
                a, b = (np.where((t == 0) & np.signbit(t), -1, t).astype(t.dtype) if t.dtype.kind == "f" else t for t in (a, b))
            if op in ("floor_divide", "remainder") and (R.is_float(adt) or R.is_float(bdt)):
                # a float quotient that lands exactly on an integer is well defined; one a rounding away from it is not robust: keep
                # the float cases to the divisors +-2 (the division is exact) plus zero, inf and NaN
                fin = np.isfinite(b.astype(np.float32)) & (b.astype(np.float32) != 0)
                b = np.where(fin, in_dtype(np.where(b.astype(np.float32) < 0, -2.0, 2.0), bdt), b).astype(b.dtype)
            with np.errstate(all="ignore"):
                want, rdt = _binary2_rule(op, a, adt, b, bdt)
            same(mx, mx.binary_op(op, up(mx, a, adt), up(mx, b, bdt)), want, rdt, f"{op} {adt} x {bdt}")


def test_logical_not_power_logaddexp_where_clip(mx):
    g = rng(4)
    for dt in R.DTYPES:
        a = vals(g, (3, 11), dt)
        same(mx, mx.unary_op("logical_not", up(mx, a, dt)), R.logical("logical_not", a)[0], "bool", f"logical_not {dt}")
    # integer power: by squaring, wrapping; negative exponents
    for adt, bdt in (("int32", "int32"), ("int8", "uint8"), ("int64", "int32"), ("uint32", "uint32"), ("int16", "int64")):
        base = in_dtype(np.array([[2], [3], [1], [-1 if not adt.startswith("u") else 5], [7], [0]]), adt)
        e = in_dtype(np.array([0, 1, 2, 5, 10, 31, 33, -1, -2, -3] if not bdt.startswith("u") else [0, 1, 2, 5, 10, 31, 33, 40, 63, 64]), bdt)
        want, rdt = R.int_power(base, adt, e, bdt)
        same(mx, mx.binary_op("power", up(mx, base, adt), up(mx, e, bdt)), want, rdt, f"power {adt} ** {bdt}")
    # float power and logaddexp: float64 reference, TRANSCENDENTAL_ULP float32 ulp of |ref| (logaddexp: of the larger of |ref| and |max operand|)
    for dt in R.FLOATS:
        x, y = in_dtype(g.uniform(0.5, 4, (5, 9)), dt), in_dtype(g.uniform(-3, 3, (9,)), dt)
        ref = np.power(R.f32(x).astype(np.float64), R.f32(y).astype(np.float64))
        close(mx, mx.binary_op("power", up(mx, x, dt), up(mx, y, dt)), ref, TRANSCENDENTAL_ULP["power"] * ULP32 * np.abs(ref), dt, f"power {dt}")
        p, q = in_dtype(g.uniform(-20, 20, (5, 9)), dt), in_dtype(g.uniform(-20, 20, (9,)), dt)
        p[0, 0], q[0] = -np.inf, -np.inf
        p[0, 1] = -np.inf
        p64, q64 = np.broadcast_arrays(R.f32(p).astype(np.float64), R.f32(q).astype(np.float64))
        ref = np.logaddexp(p64, q64)
        scale = np.maximum(np.abs(ref), np.where(np.isfinite(np.maximum(p64, q64)), np.abs(np.maximum(p64, q64)), 0))
        close(mx, mx.binary_op("logaddexp", up(mx, p, dt), up(mx, q, dt)), ref, TRANSCENDENTAL_ULP["logaddexp"] * ULP32 * scale, dt, f"logaddexp {dt}")
    got = mx.binary_op("logaddexp", up(mx, np.array([1, 2], np.int32), "int32"), up(mx, np.array([1, 3], np.int32), "int32"))
    close(mx, got, np.logaddexp([1.0, 2.0], [1.0, 3.0]), 4 * ULP32 * 3.5, "float32", "logaddexp of integers is float32")
    # where: three different broadcast shapes; the result takes the promoted dtype of x and y
    for cdt, xdt, ydt in (("bool", "float32", "float32"), ("int32", "uint8", "int8"), ("float32", "int64", "int32"), ("uint8", "bfloat16", "float16"),
                          ("bool", "int32", "uint32"), ("float16", "bool", "int16")):
        c, x, y = vals(g, (5, 1, 8), cdt), vals(g, (3, 1), xdt), vals(g, (8,), ydt)
        want, rdt = R.where(c, x, xdt, y, ydt)
        same(mx, mx.where(up(mx, c, cdt), up(mx, x, xdt), up(mx, y, ydt)), want, rdt, f"where {cdt} ? {xdt} : {ydt}")
    # clip = minimum(maximum(a, lo), hi), each with the promotion of its operands
    for dt, lo_dt in (("float32", "float32"), ("int32", "int32"), ("bfloat16", "float32"), ("int8", "int32"), ("uint8", "uint8")):
        a = vals(g, (4, 9), dt, specials=dt not in R.FLOATS)
        lo, hi = in_dtype(np.array(2), lo_dt), in_dtype(np.array([5, 6, 7, 100, 3, 4, 50, 9, 10]), lo_dt)
        mid, mdt = R.maxmin("maximum", a, dt, lo, lo_dt)
        want, rdt = R.maxmin("minimum", mid, mdt, hi, lo_dt)
        same(mx, mx.clip(up(mx, a, dt), up(mx, lo, lo_dt), up(mx, hi, lo_dt)), want, rdt, f"clip {dt} by {lo_dt}")


# ---- unary and astype ------------------------------------------------------------------------------------------------------------
def test_astype_every_dtype_pair(mx):
    """In-range values only (an out-of-range float -> integer cast is undefined); int64 <-> int32 <-> uint32 exact at full width."""
    g = rng(5)
    for sdt in R.DTYPES:
        for ddt in R.DTYPES:
            unsigned = any(t.startswith("u") for t in (sdt, ddt))
            lo = 0 if unsigned else -100
            if sdt == "bool":
                a = g.integers(0, 2, (3, 13)).astype(bool)
            elif sdt in R.INTS:
                a = g.integers(lo, 101, (3, 13)).astype(R.NP[sdt])
            else:
                a = in_dtype(g.integers(lo * 4, 401, (3, 13)) / 4.0, sdt)           # quarters: fractions every float type holds, truncated by the casts
            for kind in ("contiguous", "transposed"):
                A, la = lay(mx, a, sdt, kind)
                same(mx, mx.astype(A, code(mx, ddt)), R.cast_between(la, sdt, ddt), ddt, f"astype {sdt} -> {ddt} ({kind})")
    wide = np.array([0, 1, 2 ** 24 + 1, 2 ** 25 + 1, 2 ** 31 - 1], np.int64)
    for sdt, ddt in (("int64", "int32"), ("int32", "int64"), ("int64", "uint32"), ("uint32", "int64"), ("int32", "uint32"), ("uint32", "int32")):
        same(mx, mx.astype(up(mx, wide.astype(R.NP[sdt]), sdt), code(mx, ddt)), wide.astype(R.NP[ddt]), ddt, f"astype {sdt} -> {ddt} at full width")
    same(mx, mx.astype(up(mx, np.array([2 ** 32 - 1, 2 ** 31], np.int64), "int64"), mx.UINT32), np.array([2 ** 32 - 1, 2 ** 31], np.uint32), "uint32")
    same(mx, mx.astype(up(mx, np.array([-1, -2 ** 31], np.int32), "int32"), mx.INT64), np.array([-1, -2 ** 31], np.int64), "int64")


EXACT_UNARY = ["isnan", "isinf", "isfinite", "isposinf", "isneginf", "sign", "floor", "ceil", "round", "abs", "square", "negative", "reciprocal"]


@pytest.mark.parametrize("op", EXACT_UNARY)
def test_exact_unary_ops_every_dtype(mx, op):
    for i, dt in enumerate(R.DTYPES):
        if dt == "bool" and op == "negative":
            continue
        a = vals(rng(6, i), (3, 17), dt)
        for kind in ("contiguous", "strided"):
            A, la = lay(mx, a, dt, kind)
            want, rdt = R.unary_exact(op, la, dt)
            got = mx.round_(A) if op == "round" else mx.negative(A) if op == "negative" else mx.unary_op(op, A)
            same(mx, got, want, rdt, f"{op} {dt} ({kind})")


@pytest.mark.parametrize("op", sorted(DOMAIN))
def test_transcendental_unary_ops_against_float64(mx, op):
    """Float inputs keep their dtype, integer inputs give float32; TRANSCENDENTAL_ULP[op] float32 ulp of |ref| plus the output rounding."""
    lo, hi = DOMAIN[op]
    for i, dt in enumerate(R.FLOATS + ["int32"]):
        g = rng(7, i)
        a = in_dtype(g.uniform(lo, hi, (7, 37)), dt) if dt in R.FLOATS else g.integers(max(int(np.ceil(lo)), -9), min(int(hi), 9) + 1, (7, 37)).astype(np.int32)
        if dt == "int32" and op in ("arcsin", "arccos", "arctanh"):
            a = np.zeros_like(a)                            # the only integer inside (-0.9, 0.9)
        ref, rdt = R.unary_f64(op, a, dt) if op != "erf" else (R.erf_f64(a), R.unary_dtype("erf", dt))
        fn = mx.exp if op == "exp" else mx.sigmoid if op == "sigmoid" else (lambda t: mx.unary_op(op, t))
        close(mx, fn(up(mx, a, dt)), ref, TRANSCENDENTAL_ULP[op] * ULP32 * np.abs(ref), rdt, f"{op} {dt}")


# ---- reductions --------------------------------------------------------------------------------------------------------------------
def _reduce_call(mx, op, A, axis, keepdims):
    if axis is None:
        return mx.prod_axes(A, None, keepdims) if op == "prod" else mx.reduce_all_op(op, A, keepdims)
    if isinstance(axis, tuple):
        return getattr(mx, op + "_axes")(A, list(axis), keepdims)
    return mx.prod_axes(A, axis, keepdims) if op == "prod" else mx.reduce_axis_op(op + "_axis", A, axis, keepdims)


def _check_reduction(mx, op, a, dt, axis, keepdims, msg):
    """sum / mean / prod of floats and logsumexp: the loops accumulate k ascending in float32, so with n accumulated terms
         sum   (n - 1) u sum|x|            mean  the same / n, one more rounding for the division
         prod  (n - 1) u |ref|             logsumexp  the sum inside the log carries (n + 7) u of itself (n terms, the expf calls and the
                                                      final logf and add stand in the 7, as for softmax), i.e. that much absolute error
    everything else is exact."""
    got = _reduce_call(mx, op, up(mx, a, dt), axis, keepdims)
    ref, rdt = R.reduce(op, a, dt, axis, keepdims)
    n = a.size // max(np.asarray(ref).size, 1)
    if op in ("max", "min", "all", "any") or (op in ("sum", "prod") and dt not in R.FLOATS):
        return same(mx, got, ref, rdt, msg)
    mag = np.abs(R.f32(a).astype(np.float64)).sum(axis=axis, keepdims=keepdims)
    if op == "sum":
        bound = (n - 1) * R.U * mag
    elif op == "mean":
        bound = (n - 1) * R.U * mag / n + R.U * np.abs(ref)
    elif op == "prod":
        bound = (n - 1) * R.U * np.abs(ref)
    else:
        bound = (n + 7) * R.U + 2 * ULP32 * np.abs(np.where(np.isfinite(ref), ref, 0))
    close(mx, got, ref, bound, rdt, msg)


def _reduction_input(g, shape, dt, op):
    if dt in R.FLOATS:
        a = in_dtype(g.uniform(0.5, 1.5, shape) * g.choice([-1, 1], shape), dt) if op == "prod" else in_dtype(g.standard_normal(shape) * 3, dt)
        if op in ("max", "min"):
            a[0, 0, 0] = np.nan                             # NaN in one line only
        if op == "logsumexp":
            a[-1, :, -1] = -np.inf                          # a line that is all -inf along axis 1
        return a
    if dt == "bool":
        a = g.integers(0, 2, shape).astype(bool)
        a[0] = True
        a[-1] = False
        return a
    return vals(g, shape, dt) if op in ("max", "min") else g.integers(0 if dt.startswith("u") else -9, 10, shape).astype(R.NP[dt])


REDUCTIONS = ["sum", "mean", "max", "min", "prod", "all", "any", "logsumexp"]


@pytest.mark.parametrize("op", REDUCTIONS)
def test_reductions_on_every_axis_whole_array_and_two_axes(mx, op):
    for i, dt in enumerate(["float32", "bfloat16", "float16", "int32", "int8", "uint8", "int64", "uint16", "bool"]):
        g = rng(8, i)
        a = _reduction_input(g, (5, 65, 3), dt, op)
        for axis in (0, 1, 2, -1, None, (0, 2), (1, 2)):
            for keepdims in (False, True):
                _check_reduction(mx, op, a, dt, axis, keepdims, f"{op} {dt} axis={axis} keepdims={keepdims}")


@pytest.mark.parametrize("n", AXIS_N)
def test_reductions_along_axis_lengths(mx, n):
    """[outer, n, inner] with outer in {1, 5} and inner in {1, 3}."""
    for outer, inner in ((1, 1), (5, 3), (5, 1), (1, 3)):
        for i, dt in enumerate(["float32", "bfloat16", "int32"]):
            for op in REDUCTIONS:
                a = _reduction_input(rng(9, n, outer, inner, i), (outer, n, inner), dt, op)
                _check_reduction(mx, op, a, dt, 1, False, f"{op} {dt} [{outer}, {n}, {inner}]")


def test_reduce_axis_refuses_an_empty_axis_and_sum_gives_zero(mx):
    e = up(mx, np.zeros((3, 0), np.float32), "float32")
    for op in ("max_axis", "min_axis", "mean_axis", "logsumexp_axis", "all_axis"):
        with pytest.raises(Exception, match="empty reduction axis"):
            mx.reduce_axis_op(op, e, 1)
    assert mx.sum_axis(e, 1).numpy().tolist() == [0, 0, 0] and mx.sum_axis(e, 0).shape == (0,)


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("std", [False, True])
def test_var_and_std(mx, ddof, std):
    """var = sum((x - mean)^2) / (N - ddof): float32 inside whatever the input's dtype, rounded once into the result dtype.  The bound is
    the sequential one over the N accumulated terms (x - mean)^2 / (N - ddof): (N - 1) u var, plus the output rounding.  std is its square
    root: an error e of var becomes e / (2 std), sqrtf's (assumed) ulp and the output rounding come on top."""
    for i, dt in enumerate(["float32", "int32", "bfloat16", "float16"]):
        g = rng(10, i)
        a = in_dtype(g.standard_normal((4, 33, 3)) * 2 + 1, dt) if dt in R.FLOATS else g.integers(-20, 21, (4, 33, 3)).astype(np.int32)
        for axes in (None, (1,), (0, 2), (1, 2)):
            for keepdims in (False, True):
                v, rdt = R.var(a, dt, axes, keepdims, ddof, False)
                N = a.size // np.asarray(v).size
                bound = (N - 1) * R.U * v
                ref = v
                if std:
                    ref = np.sqrt(v)
                    bound = bound / (2 * ref) + TRANSCENDENTAL_ULP["sqrt"] * ULP32 * ref
                close(mx, mx.var(up(mx, a, dt), None if axes is None else list(axes), keepdims, ddof, std), ref, bound, rdt,
                      f"{'std' if std else 'var'} {dt} axes={axes} ddof={ddof} keepdims={keepdims}")


def test_argmax_argmin_every_axis_with_planted_ties(mx):
    for i, dt in enumerate(R.FLOATS):
        a = in_dtype(rng(11, i).integers(-3, 4, (5, 66, 3)).astype(np.float32), dt)     # few distinct values: every line has ties
        a[2, 10, 1] = a[2, 40, 1] = 9
        a[2, 11, 1] = a[2, 41, 1] = -9
        A = up(mx, a, dt)
        for keepdims in (False, True):
            for axis in (0, 1, 2, -2):
                same(mx, mx.argmax_axis(A, axis, keepdims), R.argextreme("argmax", a, axis, keepdims)[0], "uint32", f"argmax {dt} axis={axis}")
                same(mx, mx.argmin(A, axis, keepdims), R.argextreme("argmin", a, axis, keepdims)[0], "uint32", f"argmin {dt} axis={axis}")
            want_max = np.asarray(R.argextreme("argmax", a)[0]).reshape((1, 1, 1) if keepdims else ())
            want_min = np.asarray(R.argextreme("argmin", a)[0]).reshape((1, 1, 1) if keepdims else ())
            same(mx, mx.argmax_all(A, keepdims), want_max, "uint32", f"argmax {dt} whole array")
            same(mx, mx.argmin(A, None, keepdims), want_min, "uint32", f"argmin {dt} whole array")


# ---- the long-line block reduction ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4095, 4096, 4097, 2 * 4096 + 1])
def test_long_line_sums_cross_the_block_reduction_threshold(mx, n):
    """Lines of 4096 elements and more, few of them, are summed by blocks (4096-element chunks: 16 terms per thread, an 8-level tree, then
    one block over the chunk sums: at most 32 + ceil(chunks / 256) roundings on any term's way); shorter ones, and 257 lines, by one thread
    each (n - 1 roundings).  Integer and boolean sums are exact either way; the result does not change from run to run.  Uniform(0, 1)
    values do not tell the two orders apart (the one-thread loop's error random-walks well inside either bound); constant lines do."""
    for outer in (1, 5, 257):
        g = rng(12, n, outer)
        x = g.uniform(0, 1, (outer, n)).astype(np.float32)
        blocks = n >= 4096 and outer <= 256
        chunks = -(-n // 4096)
        depth = 32 + -(-chunks // 256) if blocks else n - 1
        for dt in ("float32", "bfloat16"):
            a = in_dtype(x, dt)
            ref = R.f32(a).astype(np.float64).sum(1)
            first = mx.sum_axis(up(mx, a, dt), 1)
            close(mx, first, ref, depth * R.U * ref, dt, f"sum {dt} [{outer}, {n}]")
            bits_equal(mx.sum_axis(up(mx, a, dt), 1).numpy(), first.numpy(), dt, "sum: run to run")
            close(mx, mx.mean_axis(up(mx, a, dt), -1, True), ref[:, None] / n, (depth + 1) * R.U * ref[:, None] / n, dt, f"mean {dt} [{outer}, {n}]")
        # every element float32(0.1): one thread adding them in turn drifts (0.0158 off at n = 4096, against 33 u sum = 0.0008 for the
        # block order, which is off by 0.00006 -- both computed on the CPU), so this case fails if long lines go back to the one-thread loop
        c = np.full((outer, n), np.float32(0.1), np.float32)
        cref = c.astype(np.float64).sum(1)
        close(mx, mx.sum_axis(up(mx, c, "float32"), 1), cref, depth * R.U * cref, "float32", f"sum of {n} x 0.1, {outer} lines")
        close(mx, mx.mean_axis(up(mx, c, "float32"), 1), cref / n, (depth + 1) * R.U * cref / n, "float32", f"mean of {n} x 0.1, {outer} lines")
        i = g.integers(-2 ** 31, 2 ** 31, (outer, n)).astype(np.int32)
        same(mx, mx.sum_axis(up(mx, i, "int32"), 1), R.reduce("sum", i, "int32", 1)[0], "int32", f"sum int32 [{outer}, {n}] wraps exactly")
        b = g.integers(0, 2, (outer, n)).astype(bool)
        same(mx, mx.sum_axis(up(mx, b, "bool"), 1), b.sum(1).astype(np.int32), "int32", f"sum bool [{outer}, {n}] counts")
        close(mx, mx.mean_axis(up(mx, i, "int32"), 1), R.f32(i).astype(np.float64).mean(1),
              (depth + 1) * R.U * np.abs(R.f32(i).astype(np.float64)).sum(1) / n, "float32", f"mean int32 [{outer}, {n}]")


def test_whole_array_sum_and_mean_hold_the_tree_bound(mx):
    """2^21 + 257 float32 values against the tree-reduction bound (ceil(log2 n) + 1) u sum|x|, two inputs.
      uniform(0, 1) from default_rng(7): the bound is 1.44.  One thread adding every element in turn is off by 0.0629 here (numpy's float32
        cumsum on the CPU; the 6.09 the issue quotes for that order did not reproduce), the block order by 0.0621: this input holds the
        kernel to the bound but does not tell the two orders apart.
      every element float32(0.1): the bound is 0.29.  The one-thread order drifts to 3584 off, the block order is off by 0.034 (both
        computed on the CPU): this input fails if the whole-array forms go back to the one-thread loop.
    Two runs give the same bits."""
    inputs = {"uniform": np.random.default_rng(7).uniform(0, 1, BIG).astype(np.float32), "constant 0.1": np.full(BIG, np.float32(0.1), np.float32)}
    for name, x in inputs.items():
        ref = x.astype(np.float64).sum()
        bound = (int(np.ceil(np.log2(BIG))) + 1) * R.U * ref
        assert (1.43 < bound < 1.45) if name == "uniform" else (0.28 < bound < 0.29)
        for shape in ((BIG,), (17, 123377)):                # 1-D, and 2-D flattened by the op
            A = up(mx, x.reshape(shape), "float32")
            s1, s2 = mx.reduce_all_op("sum", A), mx.reduce_all_op("sum", A)
            close(mx, s1, ref, bound, "float32", f"whole-array sum, {name} {shape}")
            bits_equal(s2.numpy(), s1.numpy(), "float32", "whole-array sum: run to run")
            m1, m2 = mx.reduce_all_op("mean", A, True), mx.reduce_all_op("mean", A, True)
            close(mx, m1, np.full((1,) * len(shape), ref / BIG), bound / BIG + R.U * ref / BIG, "float32", f"whole-array mean, {name} {shape}")
            bits_equal(m2.numpy(), m1.numpy(), "float32", "whole-array mean: run to run")


# ---- total size 2^21 + 257: the second trip of every grid-stride kernel ----------------------------------------------------------------
def _big_i32():
    return np.random.default_rng(21).integers(-2 ** 31, 2 ** 31, BIG).astype(np.int32)


def _big_f32(n=BIG):
    return np.random.default_rng(22).standard_normal(n).astype(np.float32)


def test_big_binary_kernel(mx):
    a = _big_i32()
    same(mx, mx.add(up(mx, a, "int32"), up(mx, np.int32(3), "int32")), a + np.int32(3), "int32", "binary_kernel")


def test_big_binary_and_unary_vec_kernels(mx):
    x = _big_f32(BIG - 1)                                   # 2^21 + 256: stays a whole number of 16-byte vectors
    X = up(mx, x, "float32")
    same(mx, mx.add(X, X), x + x, "float32", "binary_vec_kernel")
    same(mx, mx.negative(X), -x, "float32", "unary_vec_kernel")


def test_big_unary_binary2_unary2_kernels(mx):
    a, x = _big_i32(), _big_f32()
    A = up(mx, a, "int32")
    same(mx, mx.negative(A), R.unary_exact("negative", a, "int32")[0], "int32", "unary_kernel")
    same(mx, mx.maximum(A, up(mx, np.int32(-5), "int32")), np.maximum(a, np.int32(-5)), "int32", "binary2_kernel")
    same(mx, mx.unary_op("abs", up(mx, x, "float32")), np.abs(x), "float32", "unary2_kernel")


def test_big_strided_copy_both_directions(mx):
    x = _big_f32().reshape(BIG // 1, 1)
    pair = np.concatenate([x, -x], 1)                       # [BIG, 2]; its transpose, made contiguous, is a strided gather of 2 * BIG elements
    same(mx, mx.contiguous(mx.transpose(up(mx, pair, "float32"))), np.ascontiguousarray(pair.T), "float32", "strided_copy_kernel, gather")
    want = np.zeros(2 * BIG, np.float32)
    want[::2] = x[:, 0]
    got = mx.slice_update(mx.zeros([2 * BIG], mx.FLOAT32), up(mx, x[:, 0], "float32"), [0], [2 * BIG], [2])
    same(mx, got, want, "float32", "strided_copy_kernel, scatter")


def test_big_where_fill_arange(mx):
    a = _big_i32()
    same(mx, mx.where(up(mx, a > 0, "bool"), up(mx, a, "int32"), up(mx, np.int32(-1), "int32")), np.where(a > 0, a, np.int32(-1)), "int32", "where_kernel")
    same(mx, mx.full([BIG], up(mx, np.int32(2 ** 25 + 1), "int32"), mx.INT32), np.full(BIG, 2 ** 25 + 1, np.int32), "int32", "fill_value_kernel")
    same(mx, mx.arange(5, 5 + BIG, 1, mx.INT32), np.arange(5, 5 + BIG, dtype=np.int32), "int32", "arange_kernel")


def test_big_take_along_and_take_axis(mx):
    a = _big_i32()
    idx = np.random.default_rng(23).integers(-BIG, BIG, BIG).astype(np.int32)
    A, I = up(mx, a, "int32"), up(mx, idx, "int32")
    same(mx, mx.take_along_axis(A, I, 0), R.take_along_axis(a, idx, 0), "int32", "take_along_kernel")
    same(mx, mx.take_axis(A, I, 0), R.take_axis(a, idx, 0), "int32", "take_axis_kernel")


def test_big_sum_and_reduce_axis_with_a_long_inner(mx):
    """[2, 2^21 + 257] reduced over axis 0: n = 2, inner = 2^21 + 257.  One float32 addition (and an exact halving) per output: bit-equal."""
    x = np.stack([_big_f32(), np.random.default_rng(24).standard_normal(BIG).astype(np.float32)])
    X = up(mx, x, "float32")
    same(mx, mx.sum_axis(X, 0), x[0] + x[1], "float32", "sum_axis_kernel")
    same(mx, mx.mean_axis(X, 0), (x[0] + x[1]) / np.float32(2), "float32", "reduce_axis_kernel, mean")
    same(mx, mx.max_axis(X, 0), np.maximum(x[0], x[1]), "float32", "reduce_axis_kernel, max")


# ---- scans ---------------------------------------------------------------------------------------------------------------------------
SCANS = ["sum", "prod", "max", "min"]


def _check_scan(mx, kind, a, dt, axis, reverse, inclusive, msg):
    """Float cumsum: (n - 1) u of the running sum of |x| (k ascending from the scan's start); cumprod: (n - 1) u |ref|.  The rest is exact."""
    got = mx.scan(kind, up(mx, a, dt), axis, reverse, inclusive)
    ref, rdt = R.scan(kind, a, dt, axis, reverse, inclusive)
    if dt not in R.FLOATS or kind in ("max", "min"):
        return same(mx, got, ref, rdt, msg)
    n = a.shape[axis]
    if kind == "sum":
        bound = (n - 1) * R.U * R.scan("sum", np.abs(R.f32(a)), "float32", axis, reverse, inclusive)[0]
    else:
        bound = (n - 1) * R.U * np.abs(np.where(np.isfinite(ref), ref, 0))
    close(mx, got, ref, bound, rdt, msg)


@pytest.mark.parametrize("kind", SCANS)
def test_scans_every_dtype_axis_direction_and_form(mx, kind):
    """Exclusive running max / min start from the dtype's own lowest / highest value; a NaN in the middle of a line stays."""
    for i, dt in enumerate(R.INTS + R.FLOATS):
        g = rng(13, i)
        if dt in R.FLOATS:
            a = in_dtype(g.uniform(0.5, 1.5, (3, 7, 2)) * g.choice([-1, 1], (3, 7, 2)), dt)
            a[1, 3, 0] = np.nan
        else:
            a = vals(g, (3, 7, 2), dt) if kind in ("max", "min") else g.integers(0 if dt.startswith("u") else -5, 6, (3, 7, 2)).astype(R.NP[dt])
        for axis in (0, 1, 2, -1):
            for reverse in (False, True):
                for inclusive in (True, False):
                    _check_scan(mx, kind, a, dt, axis, reverse, inclusive, f"cum{kind} {dt} axis={axis} reverse={reverse} inclusive={inclusive}")
    with pytest.raises(Exception, match="boolean input is not supported"):
        mx.scan(kind, up(mx, np.array([True, False]), "bool"), 0)


@pytest.mark.parametrize("n", AXIS_N)
def test_scans_along_axis_lengths(mx, n):
    for outer, inner in ((1, 1), (5, 3)):
        g = rng(14, n, outer)
        ai = g.integers(-5, 6, (outer, n, inner)).astype(np.int32)
        af = (g.uniform(0.5, 1.5, (outer, n, inner)) * g.choice([-1, 1], (outer, n, inner))).astype(np.float32)
        for kind in SCANS:
            for reverse, inclusive in ((False, True), (True, False)):
                _check_scan(mx, kind, ai, "int32", 1, reverse, inclusive, f"cum{kind} int32 [{outer}, {n}, {inner}]")
                _check_scan(mx, kind, af, "float32", 1, reverse, inclusive, f"cum{kind} float32 [{outer}, {n}, {inner}]")


# ---- order ---------------------------------------------------------------------------------------------------------------------------
def _order_input(g, shape, dt):
    if dt in R.FLOATS:
        a = in_dtype(g.integers(-4, 5, shape) / 2.0, dt)    # heavy ties
        flat = a.reshape(-1)
        if flat.size > 8:
            flat[[1, flat.size // 2]] = np.nan
            flat[[2, 5]] = -0.0
            flat[[3, 7]] = 0.0
        return a
    return g.integers(0 if dt.startswith("u") else -3, 4, shape).astype(R.NP[dt]) * (2 ** 40 + 1 if dt == "int64" else 1)


@pytest.mark.parametrize("n", [1, 2, 257, 1000])
def test_argsort_sort_argpartition_topk(mx, n):
    """Stable (ties keep index order), NaN last, -0.0 and +0.0 tie; along the last axis and along a middle one.  argpartition and topk
    promise a partition, not an order: position kth holds what the sort puts there, no larger value before it, no smaller one after."""
    for i, dt in enumerate(["float32", "bfloat16", "int64", "uint8", "float16", "int32"]):
        for shape, axis in (((3, n), -1), ((2, n, 3), 1)):
            a = _order_input(rng(15, n, i, len(shape)), shape, dt)
            A = up(mx, a, dt)
            same(mx, mx.argsort_axis(A, axis), R.argsort(a, axis)[0], "uint32", f"argsort {dt} {shape} axis={axis}")
            same(mx, mx.sort_axis(A, axis), R.sort(a, axis), dt, f"sort {dt} {shape} axis={axis}")
            srt = np.moveaxis(R.sort(a, axis), axis, -1)
            for kth in sorted({0, n // 2, n - 1}):
                part = mx.argpartition_axis(A, kth, axis)
                assert part.dtype == mx.UINT32 and part.shape == a.shape
                picked = np.take_along_axis(a, part.numpy().astype(np.int64), axis)
                assert R.is_partition(np.moveaxis(picked, axis, -1), kth, srt), f"argpartition {dt} {shape} kth={kth}"
                vals_part = mx.partition(A, kth, axis)
                assert vals_part.dtype == code(mx, dt) and R.is_partition(np.moveaxis(vals_part.numpy(), axis, -1), kth, srt), f"partition {dt} kth={kth}"
            for k in sorted({1, (n + 1) // 2, n}):
                top = mx.topk(A, k, axis)
                assert top.dtype == code(mx, dt)
                got = np.sort(np.moveaxis(top.numpy(), axis, -1), -1)
                bits_equal(got, np.sort(srt[..., n - k:], -1), dt, f"topk {dt} {shape} k={k}: the k largest, in any order")
    if n == 1:
        a = _order_input(rng(15, 0), (4, 9), "float32")
        same(mx, mx.sort(up(mx, a, "float32")), R.sort(a.reshape(-1), -1), "float32", "sort without an axis: of the flattened array")
        same(mx, mx.argsort(mx.transpose(up(mx, a, "float32"))), R.argsort(a.T, -1)[0], "uint32", "argsort of a transposed view")


# ---- gathers -------------------------------------------------------------------------------------------------------------------------
def test_take_and_take_along_axis(mx):
    g = rng(16)
    for dt in ("float32", "int8", "int64", "bfloat16"):
        a = vals(g, (4, 5, 6), dt, specials=False)
        A = up(mx, a, dt)
        for idt in ("int32", "uint32", "int64", "uint8"):
            lo = 0 if idt.startswith("u") else -120
            idx = g.integers(lo, 120, (3, 7)).astype(R.NP[idt])
            same(mx, mx.take(A, up(mx, idx, idt)), R.take(a, idx), dt, f"take {dt} by {idt}")
            same(mx, mx.take(mx.transpose_axes(A, [2, 0, 1]), up(mx, idx, idt)), R.take(a.transpose(2, 0, 1), idx), dt, f"take of a view {dt} by {idt}")
        for axis, ishape in ((0, (3, 1, 6)), (1, (4, 2, 1)), (2, (1, 5, 9)), (-1, (4, 5, 2))):          # indices broadcast against the array
            n = a.shape[axis]
            idx = g.integers(-n, n, ishape).astype(np.int32)
            same(mx, mx.take_along_axis(A, up(mx, idx, "int32"), axis), R.take_along_axis(a, idx, axis), dt, f"take_along_axis {dt} axis={axis} {ishape}")


def test_take_axis_general_route(mx):
    g = rng(17)
    for dt, shape in (("int32", (6, 5)), ("float32", (4, 6, 5)), ("uint8", (7,)), ("int64", (3, 4)), ("bfloat16", (5, 6))):
        a = vals(g, shape, dt, specials=False)
        for axis in range(len(shape)):
            if len(shape) == 2 and axis == 0 and dt in R.FLOATS:
                continue                                    # the embedding route: below
            n = shape[axis]
            for idt in ("int32", "uint32", "int64", "uint8"):
                for ishape in ((), (5,), (2, 3)):
                    idx = g.integers(0, n, ishape).astype(R.NP[idt])
                    if not idt.startswith("u") and ishape:
                        idx.reshape(-1)[:2] = [-1, -n]      # negative indices wrap
                    if len(ishape) == 1:
                        idx[-2:] = idx[0]                   # duplicates
                    for kind in ("contiguous", "transposed"):
                        A, la = lay(mx, a, dt, kind)
                        same(mx, mx.take_axis(A, up(mx, idx, idt), axis), R.take_axis(la, idx, axis), dt, f"take_axis {dt} {shape} axis={axis} by {idt} {ishape} ({kind})")


def test_take_axis_embedding_route_wraps_and_bounds_its_indices(mx):
    """A 2-D float table, axis 0 (take_rows_kernel): rows of a whole number of 16-byte vectors and not; int32 indices of -1 and -n wrap like
    on every other route; an index past the table is clamped into it, never read."""
    g = rng(18)
    for dt, shape in (("float32", (9, 8)), ("float32", (9, 5)), ("bfloat16", (9, 16)), ("bfloat16", (9, 3)), ("float16", (300, 8))):
        a = vals(g, shape, dt, specials=False)
        n = shape[0]
        for idt in ("int32", "uint32", "int64"):            # (64-bit indices take the general route: the row gather reads 32-bit words)
            for ishape in ((), (6,), (2, 4)):
                idx = g.integers(0, n, ishape).astype(R.NP[idt])
                flat = idx.reshape(-1)
                if flat.size > 1:
                    flat[-1] = flat[0]                      # a duplicate
                    if idt != "uint32":
                        flat[:4] = [-1, -n, -n - 3, n + 5][:flat.size]
                    else:
                        flat[:2] = [n, 2 ** 32 - 1]         # too large, and what -1 looks like unsigned: both clamp to the last row
                for kind in ("contiguous", "transposed"):
                    A, la = lay(mx, a, dt, kind)
                    same(mx, mx.take_axis(A, up(mx, idx, idt), 0), R.take_axis(la, idx, 0), dt, f"take_axis {dt} {shape} rows by {idt} {ishape} ({kind})")


# ---- softmax -------------------------------------------------------------------------------------------------------------------------
def _check_softmax(mx, got, a, dt, axes, msg):
    """64 lanes each add ceil(n / 64) terms, then six butterfly adds and one divide: |d| <= (ceil(n / 64) + 7) u ref plus the output
    rounding; and every line sums to 1 within n ulps of the output dtype (at 1).  The bound leaves no room for the rounding of x - max,
    which exp turns into up to u |x - max| of relative error: softmax_kernel gives that rounding back (exp_shifted); before it did, the
    float32 cases missed the bound by up to 1.6x (2.6e-15 against 1.7e-15 at a probability of 2.8e-9, n = 65)."""
    ref = R.softmax_f64(a, axes)
    axes = (axes,) if isinstance(axes, int) else tuple(axes)
    n = int(np.prod([a.shape[x] for x in axes]))
    close(mx, got, ref, (-(-n // 64) + 7) * R.U * ref, dt, msg)
    ulp1 = {"float32": 2.0 ** -23, "float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}[dt]
    sums = got.numpy().astype(np.float64).sum(axis=axes)
    assert (np.abs(sums - 1) <= n * ulp1).all(), f"{msg}: a line sums to {sums.reshape(-1)[np.argmax(np.abs(sums - 1))]!r}"


@pytest.mark.parametrize("n", AXIS_N + [1000])
def test_softmax_along_axis_lengths(mx, n):
    """rows % 4 != 0 (5 and 15 rows, 4 to a block), inner in {1, 3}; values around 1e4 (the max shift must hold); a line that is -inf but
    for one entry."""
    for i, dt in enumerate(R.FLOATS):
        for shape, axis in (((5, n), 1), ((5, n, 3), 1), ((1, n), -1)):
            g = rng(19, n, i, len(shape))
            a = g.standard_normal(shape).astype(np.float32) * 3
            a[0] += 1e4
            if shape[0] > 2:
                line = np.moveaxis(a, axis, -1)[2]
                line[...] = -np.inf
                line[..., n // 2] = 0.25
            a = in_dtype(a, dt)
            _check_softmax(mx, mx.softmax_axis(up(mx, a, dt), axis), a, dt, axis, f"softmax_axis {dt} {shape} axis={axis}")


def test_softmax_every_axis_axes_and_whole_array(mx):
    for i, dt in enumerate(R.FLOATS):
        a = in_dtype(rng(20, i).standard_normal((5, 9, 3)) * 2, dt)
        A = up(mx, a, dt)
        for axis in (0, 1, 2, -1):
            _check_softmax(mx, mx.softmax_axis(A, axis), a, dt, axis % 3, f"softmax_axis {dt} axis={axis}")
        for axes in ((0, 1), (1, 2), (0, 2), (2,)):
            _check_softmax(mx, mx.softmax_axes(A, list(axes)), a, dt, axes, f"softmax_axes {dt} {axes}")
        _check_softmax(mx, mx.softmax_axes(A, None), a, dt, (0, 1, 2), f"softmax {dt}")
        _check_softmax(mx, mx.softmax_axis(mx.transpose_axes(A, [2, 0, 1]), 1), a.transpose(2, 0, 1), dt, 1, f"softmax_axis of a view {dt}")
    with pytest.raises(Exception, match="floating arrays only"):
        mx.softmax_axis(up(mx, np.arange(4, dtype=np.int32), "int32"), 0)


def test_softmax_one_vocabulary_row(mx):
    a = (np.random.default_rng(25).standard_normal((1, 151936)) * 4).astype(np.float32)
    for dt in R.FLOATS:
        b = in_dtype(a, dt)
        _check_softmax(mx, mx.softmax_axis(up(mx, b, dt), -1), b, dt, 1, f"softmax {dt} [1, 151936]")


# ---- layout: bit-equal to numpy ----------------------------------------------------------------------------------------------------------
def test_slice_and_slice_update(mx):
    g = rng(26)
    for dt in ("float32", "bfloat16", "int8", "int64"):
        a = vals(g, (7, 6, 5), dt, specials=False)
        for step in (1, 2, 3):
            for start in range(7):
                got = mx.slice(up(mx, a, dt), [start, 1, 0], [7, 6, 5], [step, 2, 1])
                same(mx, got, a[start::step, 1::2, :], dt, f"slice {dt} [{start}::{step}, 1::2]")
        view = mx.slice(mx.transpose_axes(up(mx, a, dt), [2, 0, 1]), [1, 0, 1], [5, 7, 6], [2, 3, 2])
        same(mx, view, a.transpose(2, 0, 1)[1:5:2, 0:7:3, 1:6:2], dt, f"slice of a transposed view {dt}")
        # an update into a strided region of a contiguous source ...
        u = vals(g, (3, 3, 5), dt, specials=False)
        want = a.copy()
        want[1::2, 0:6:2] = u
        same(mx, mx.slice_update(up(mx, a, dt), up(mx, u, dt), [1, 0, 0], [7, 6, 5], [2, 2, 1]), want, dt, f"slice_update {dt}, strided region")
        # ... and into a region of a transposed source, from an update that is itself a view
        t = a.transpose(1, 0, 2)
        u2 = vals(g, (5, 2, 3), dt, specials=False)
        want = t.copy()
        want[1:6:2, 2:4] = u2.transpose(2, 1, 0)
        got = mx.slice_update(mx.transpose_axes(up(mx, a, dt), [1, 0, 2]), mx.transpose_axes(up(mx, u2, dt), [2, 1, 0]), [1, 2, 0], [6, 4, 5], [2, 1, 1])
        same(mx, got, want, dt, f"slice_update {dt}, transposed source")


def test_concatenate_stack_pad_repeat_tile_broadcast_flatten_triangles(mx):
    g = rng(27)
    for dt in ("float32", "float16", "uint8", "int64", "bool"):
        a, b = vals(g, (4, 3, 5), dt, specials=False), vals(g, (4, 3, 5), dt, specials=False)
        parts = [lay(mx, a, dt, "transposed"), lay(mx, b, dt, "strided"), lay(mx, a, dt, "broadcast")]
        H, V = [p[0] for p in parts], [p[1] for p in parts]
        for axis in (0, 1, 2, -1):
            same(mx, mx.concatenate_axis(H, axis), np.concatenate(V, axis), dt, f"concatenate {dt} axis={axis}")
        for axis in (0, 1, 2, 3, -1):
            same(mx, mx.stack_axis(H, axis), np.stack(V, axis), dt, f"stack {dt} axis={axis}")
        T, lt = parts[0]
        fill = vals(g, (), dt, specials=False)
        same(mx, mx.pad(T, [0, 2], [1, 0], [2, 3], up(mx, fill, dt)), np.pad(lt, [(1, 2), (0, 0), (0, 3)], constant_values=fill), dt, f"pad {dt}")
        same(mx, mx.repeat(T, 3, 1), np.repeat(lt, 3, 1), dt, f"repeat {dt} axis 1")
        same(mx, mx.repeat(T, 2), np.repeat(lt, 2), dt, f"repeat {dt} flattened")
        same(mx, mx.tile(T, [2, 1, 3]), np.tile(lt, (2, 1, 3)), dt, f"tile {dt}")
        same(mx, mx.tile(T, [2, 2]), np.tile(lt, (2, 2)), dt, f"tile {dt}, fewer reps than axes")
        same(mx, mx.broadcast_to(mx.slice(T, [0, 1, 0], [4, 2, 5]), [2, 4, 3, 5]), np.broadcast_to(lt[:, 1:2], (2, 4, 3, 5)), dt, f"broadcast_to {dt}")
        same(mx, mx.flatten(T), lt.reshape(-1), dt, f"flatten {dt}")
        same(mx, mx.flatten(parts[1][0], 1, 2), V[1].reshape(4, 15), dt, f"flatten {dt} axes 1..2")
        m = vals(g, (5, 8), dt, specials=False)
        for k in (-2, 0, 3):
            same(mx, mx.tri(5, 8, k, code(mx, dt)), np.tri(5, 8, k).astype(R.NP[dt]), dt, f"tri {dt} k={k}")
            same(mx, mx.tril(up(mx, m, dt), k), np.tril(m, k), dt, f"tril {dt} k={k}")
            same(mx, mx.triu(mx.transpose(up(mx, np.ascontiguousarray(m.T), dt)), k), np.triu(m, k), dt, f"triu of a view {dt} k={k}")


def test_zero_element_arrays_launch_nothing(mx):
    """Ops whose wrappers guard their launch with the result's size."""
    e = up(mx, np.zeros((0, 4), np.float32), "float32")
    row = up(mx, np.ones((1, 4), np.float32), "float32")
    for got, dt in ((mx.add(e, row), "float32"), (mx.exp(e), "float32"), (mx.greater(e, row), "bool"), (mx.unary_op("abs", e), "float32"),
                    (mx.astype(e, mx.INT32), "int32"), (mx.where(e, row, e), "float32"), (mx.argsort_axis(e, 0), "uint32"),
                    (mx.sum_axis(e, 1), "float32"), (mx.scan("sum", e, 0), "float32"), (mx.contiguous(mx.transpose(e)), "float32")):
        assert got.dtype == code(mx, dt) and got.numpy().size == 0
    assert mx.full([0, 3], up(mx, np.float32(1), "float32"), mx.FLOAT32).shape == (0, 3) and mx.arange(3, 3, 1, mx.INT32).shape == (0,)


# ---- convolution -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("padding", [0, 2])
@pytest.mark.parametrize("dilation", [1, 2])
def test_conv1d_and_conv2d_general_kernels_against_a_direct_loop(mx, stride, padding, dilation):
    """float32 accumulation in (k, ci) order: (n - 1) u sum|terms| with n accumulated terms (taps outside the input do not count, the bound
    takes the full count), plus the output rounding.  groups in {1, 2, C}; non-square kernels and images."""
    for i, dt in enumerate(("float32", "bfloat16")):
        for groups in (1, 2, 4):
            g = rng(28, stride, padding, dilation, i, groups)
            x, w = in_dtype(g.standard_normal((2, 11, 4)), dt), in_dtype(g.standard_normal((8, 3, 4 // groups)), dt)
            ref, mag = R.conv1d_f64(x, w, stride, padding, dilation, groups)
            n = 3 * (4 // groups)
            close(mx, mx.conv1d(up(mx, x, dt), up(mx, w, dt), stride, padding, dilation, groups), ref, (n - 1) * R.U * mag, dt,
                  f"conv1d {dt} s={stride} p={padding} d={dilation} g={groups}")
            x2, w2 = in_dtype(g.standard_normal((2, 7, 9, 4)), dt), in_dtype(g.standard_normal((4, 2, 3, 4 // groups)), dt)
            s2, p2, d2 = (stride, 3 - stride), (padding, 2 - padding), (dilation, 3 - dilation)
            ref, mag = R.conv2d_f64(x2, w2, s2, p2, d2, groups)
            n = 2 * 3 * (4 // groups)
            close(mx, mx.conv2d(up(mx, x2, dt), up(mx, w2, dt), s2, p2, d2, groups), ref, (n - 1) * R.U * mag, dt,
                  f"conv2d {dt} s={s2} p={p2} d={d2} g={groups}")
