"""The mlx-c array ops (csrc/mlxc.hip, mlxc_glue.hpp, mlxc_glue2.hpp) restated in numpy: for every op of tests/test_gpu_mlx_ops_sweep.py
the result dtype and the value MLX gives.  Shared by tests/test_mlx_ops_rule.py (CPU: the rules pinned on known answers) and the sweep (GPU).

Dtypes are names ("int32", "bfloat16", ...).  A bfloat16 array is held as float32 values that are exactly representable in bfloat16, which
is also what `Array.numpy()` reads back.  Integer results are computed in 64-bit integers and wrap into the result dtype; float results
are computed in float64 (`*_f64`, compared under a bound) or, where the kernel's float32 operation is itself IEEE-exact, in float32
(compared bit for bit) -- and rounded once to the result dtype.

Where each rule comes from:
  promotion table           reference mlx-rs/src/dtype.rs:119-204 (`TypePromotion::promote_with`)
  divide of non-floats      float32: reference mlx-rs/src/ops/arithmetic.rs:2644-2658 (bool / bool items read as f32: 1, 0, inf, NaN)
  NaN in maximum / minimum  mlxc_glue.hpp binary2_kernel "NaN propagates like MLX's maximum"; reduce_axis_kernel "NaN propagates in max / min";
                            mlxc_glue2.hpp scan_axis_kernel (the running max / min turn NaN and stay NaN)
  NaN sorts last, stable    mlxc_glue.hpp argsort_kernel "stable ascending argsort ... NaN last"
  argmax / argmin ties      elementwise.hip "argmax over the last axis, first index on ties"; mlxc_glue2.hpp mlx_argmin_axis "ties: the lowest index"
  floor_divide / remainder  mlxc_glue.hpp binary2_kernel "sign of the divisor (numpy / MLX remainder); division by zero gives 0",
                            "floor division (numpy / MLX semantics for negative operands); division by zero gives 0"
  integer power             mlxc_glue.hpp binary2_kernel "a negative exponent gives 0 (1 for a base of 1)"
  round                     mlxc_glue.hpp unary2_apply "round half to even, as MLX (numpy) does"
  sum of bools is int32     mlxc_glue.hpp mlx_sum_axis "sums of booleans count"
  mean / logsumexp of ints  float32: mlxc_glue.hpp reduce_axis "the mean of integers is float32 in MLX"
  sign                      mlxc_glue.hpp unary2_apply: (x > 0) - (x < 0), so 0 for NaN and +0.0 for -0.0 (kept as it is: no source for MLX's)
  unary result dtypes       mlxc_glue.hpp unary2 "abs / square / sign / floor / ceil / round keep an integer input's dtype in MLX", unary2_apply
                            "float results for float inputs, float32 for integer inputs; predicates and logical_not give bool"
  negative gather indices   mlxc_glue.hpp take_axis_kernel / take_along_kernel (t < 0: t += n, then clamped); tests/test_gpu_mlx_glue.py
                            "negative indices wrap"
  exclusive scans           start from the operation's identity in the array's own dtype (0, 1, the dtype's lowest / highest, -inf / +inf)
  conv1d / conv2d layout    mlxc_glue.hpp conv1d_kernel, mlxc_glue2.hpp conv2d_kernel: channels-last input, weight [Cout, k..., Cin / groups]"""
import numpy as np

DTYPES = ["bool", "uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64", "float16", "bfloat16", "float32"]
INTS = ["uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64"]
FLOATS = ["float16", "bfloat16", "float32"]
NP = {"bool": np.bool_, "uint8": np.uint8, "uint16": np.uint16, "uint32": np.uint32, "uint64": np.uint64, "int8": np.int8, "int16": np.int16,
      "int32": np.int32, "int64": np.int64, "float16": np.float16, "bfloat16": np.float32, "float32": np.float32}

_ = {"b": "bool", "u8": "uint8", "u16": "uint16", "u32": "uint32", "u64": "uint64", "i8": "int8", "i16": "int16", "i32": "int32",
     "i64": "int64", "f16": "float16", "bf": "bfloat16", "f32": "float32"}
# PROMOTION[row][column], both in the order of DTYPES (mlx-rs/src/dtype.rs:119-204, written out)
_TABLE = """
b   u8  u16 u32 u64 i8  i16 i32 i64 f16 bf  f32
u8  u8  u16 u32 u64 i16 i16 i32 i64 f16 bf  f32
u16 u16 u16 u32 u64 i32 i32 i32 i64 f16 bf  f32
u32 u32 u32 u32 u64 i64 i64 i64 i64 f16 bf  f32
u64 u64 u64 u64 u64 f32 f32 f32 f32 f16 bf  f32
i8  i16 i32 i64 f32 i8  i16 i32 i64 f16 bf  f32
i16 i16 i32 i64 f32 i16 i16 i32 i64 f16 bf  f32
i32 i32 i32 i64 f32 i32 i32 i32 i64 f16 bf  f32
i64 i64 i64 i64 f32 i64 i64 i64 i64 f16 bf  f32
f16 f16 f16 f16 f16 f16 f16 f16 f16 f16 f32 f32
bf  bf  bf  bf  bf  bf  bf  bf  bf  f32 bf  f32
f32 f32 f32 f32 f32 f32 f32 f32 f32 f32 f32 f32
"""
PROMOTION = {a: {b: _[cell] for b, cell in zip(DTYPES, row.split())} for a, row in zip(DTYPES, _TABLE.strip().splitlines())}


def promote(a: str, b: str) -> str:
    return PROMOTION[a][b]


def is_float(dt: str) -> bool:
    return dt in FLOATS


def bf16_round(x) -> np.ndarray:
    """float32 -> the nearest bfloat16 (ties to even), held as float32; NaN and the infinities pass through."""
    shape = np.shape(x)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    u = x.view(np.uint32).astype(np.uint64)
    r = (((u + ((u >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7FFF)) >> np.uint64(16)) << np.uint64(16)).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r).astype(np.float32).reshape(shape)


def cast(x, dt: str) -> np.ndarray:
    """One rounding (floats) or one two's-complement wrap (integers) into `dt`.  x is float32 / float64 / any integer / bool.
    A float -> integer cast truncates toward zero and is defined for in-range values only."""
    x = np.asarray(x)
    if dt == "bool":
        return x != 0
    if dt == "bfloat16":
        # float64 -> float32 -> bfloat16 would round twice: go through float32 only when x already is float32 or an exact integer
        return bf16_round(x.astype(np.float32))
    if dt in FLOATS:
        return x.astype(NP[dt])
    if x.dtype.kind == "f":
        return np.trunc(x).astype(np.int64).astype(NP[dt]) if dt != "uint64" else np.trunc(x).astype(np.uint64)
    if x.dtype.kind == "b":
        return x.astype(NP[dt])
    return x.astype(np.uint64 if x.dtype == np.uint64 else np.int64).astype(NP[dt])      # C-style wrap


def f32(x, dt: str = None) -> np.ndarray:
    """What the kernels' ld_f gives: the element as float32 (one rounding for 64-bit integers)."""
    return np.asarray(x).astype(np.float32)


def _u64(x) -> np.ndarray:
    x = np.asarray(x)
    return x if x.dtype == np.uint64 else x.astype(np.int64).view(np.uint64)


# ---- arithmetic -------------------------------------------------------------------------------------------------------------
def arith_dtype(op: str, adt: str, bdt: str) -> str:
    r = promote(adt, bdt)
    return "float32" if op == "divide" and not is_float(r) else r


def arith(op: str, a, adt: str, b, bdt: str):
    """add / subtract / multiply / divide -> (value, dtype).  Integer results are exact modulo 2^width; float results are ONE float32
    IEEE operation on the float32 operands, rounded once to the result dtype -- exact, compared bit for bit."""
    rdt = arith_dtype(op, adt, bdt)
    if not is_float(rdt):
        with np.errstate(over="ignore"):
            x, y = np.broadcast_arrays(_u64(a), _u64(b))
            v = x + y if op == "add" else x - y if op == "subtract" else x * y
        return cast(v, rdt), rdt
    x, y = f32(a), f32(b)
    with np.errstate(all="ignore"):
        v = (x + y if op == "add" else x - y if op == "subtract" else x * y if op == "multiply" else x / y).astype(np.float32)
    return cast(v, rdt), rdt


# ---- comparison, logical, max / min, floor_divide, remainder, power -----------------------------------------------------------
COMPARISONS = {"greater": np.greater, "greater_equal": np.greater_equal, "less": np.less, "less_equal": np.less_equal, "equal": np.equal,
               "not_equal": np.not_equal}


def _operands(a, adt, b, bdt):
    """Both integer (or bool): exact int64 (values below 2^63).  Otherwise float32, like the kernels."""
    if not is_float(adt) and not is_float(bdt):
        return np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64), True
    return f32(a), f32(b), False


def compare(op: str, a, adt, b, bdt):
    x, y, _i = _operands(a, adt, b, bdt)
    return COMPARISONS[op](x, y), "bool"


def logical(op: str, a, b=None):
    if op == "logical_not":
        return np.asarray(a) == 0, "bool"
    x, y = np.asarray(a) != 0, np.asarray(b) != 0
    return (x & y if op == "logical_and" else x | y), "bool"


def maxmin(op: str, a, adt, b, bdt):
    """maximum / minimum: a NaN on either side gives NaN."""
    rdt = promote(adt, bdt)
    x, y, _i = _operands(a, adt, b, bdt)
    with np.errstate(invalid="ignore"):
        v = np.maximum(x, y) if op == "maximum" else np.minimum(x, y)        # numpy's maximum propagates NaN too
    return cast(v, rdt), rdt


def floor_divide(a, adt, b, bdt):
    """Integers: floor (toward -inf), 0 where the divisor is 0.  Floats: floor(float32(x / y)), one float32 division then floor."""
    rdt = promote(adt, bdt)
    x, y, ints = _operands(a, adt, b, bdt)
    if ints:
        x, y = np.broadcast_arrays(x, y)
        safe = np.where(y == 0, 1, y)
        return cast(np.where(y == 0, 0, np.floor_divide(x, safe)), rdt), rdt
    with np.errstate(all="ignore"):
        return cast(np.floor((x / y).astype(np.float32)), rdt), rdt


def remainder(a, adt, b, bdt):
    """The result takes the divisor's sign; integers give 0 for a zero divisor.  Floats: fmod (exact) and, where the signs differ, one
    float32 addition of the divisor."""
    rdt = promote(adt, bdt)
    x, y, ints = _operands(a, adt, b, bdt)
    if ints:
        x, y = np.broadcast_arrays(x, y)
        safe = np.where(y == 0, 1, y)
        return cast(np.where(y == 0, 0, np.remainder(x, safe)), rdt), rdt
    with np.errstate(all="ignore"):
        v = np.fmod(x, y).astype(np.float32)
        v = np.where((v != 0) & ((v < 0) != (y < 0)), (v + y).astype(np.float32), v)
    return cast(v, rdt), rdt


def int_power(a, adt, b, bdt):
    """Integer power, wrapping; a negative exponent gives 0 except for the bases 1 (1) and -1 (+-1 by the exponent's parity)."""
    rdt = promote(adt, bdt)
    x, y = np.broadcast_arrays(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64))
    out = np.empty(x.shape, np.int64)
    for i in np.ndindex(x.shape):
        base, e = int(x[i]), int(y[i])
        if e < 0:
            v = 1 if base == 1 else ((-1 if e & 1 else 1) if base == -1 else 0)
        else:
            v = pow(base, e, 1 << 64)
        out[i] = np.array(v & 0xFFFFFFFFFFFFFFFF, np.uint64).astype(np.int64)
    return cast(out, rdt), rdt


def where(c, x, xdt, y, ydt):
    rdt = promote(xdt, ydt)
    return np.where(np.asarray(c) != 0, cast_between(x, xdt, rdt), cast_between(y, ydt, rdt)), rdt


def cast_between(x, sdt: str, ddt: str) -> np.ndarray:
    """astype on in-range values: integer -> integer wraps exactly, anything -> float rounds once, float -> integer truncates."""
    if sdt == ddt:
        return np.asarray(x)
    return cast(np.asarray(x), ddt)


# ---- unary ------------------------------------------------------------------------------------------------------------------
KEEPS_INT = ("abs", "square", "sign", "floor", "ceil", "round", "negative")
PREDICATES = ("isnan", "isinf", "isfinite", "isposinf", "isneginf", "logical_not")
EXACT_UNARY = {"abs": np.abs, "square": lambda v: v * v, "sign": lambda v: (v > 0).astype(np.float32) - (v < 0).astype(np.float32), "floor": np.floor, "ceil": np.ceil, "round": np.rint,
               "negative": np.negative, "reciprocal": lambda v: np.float32(1) / v, "isnan": np.isnan, "isinf": np.isinf, "isfinite": np.isfinite,
               "isposinf": np.isposinf, "isneginf": np.isneginf, "logical_not": lambda v: v == 0}
F64_UNARY = {"exp": np.exp, "sigmoid": lambda v: 1 / (1 + np.exp(-v)), "log": np.log, "log2": np.log2, "log10": np.log10, "log1p": np.log1p,
             "expm1": np.expm1, "sin": np.sin, "cos": np.cos, "tan": np.tan, "tanh": np.tanh, "sinh": np.sinh, "cosh": np.cosh,
             "arcsin": np.arcsin, "arccos": np.arccos, "arctan": np.arctan, "arcsinh": np.arcsinh, "arccosh": np.arccosh, "arctanh": np.arctanh,
             "sqrt": np.sqrt, "rsqrt": lambda v: 1 / np.sqrt(v)}


def unary_dtype(op: str, dt: str) -> str:
    if op in PREDICATES:
        return "bool"
    return dt if is_float(dt) or op in KEEPS_INT else "float32"


def unary_exact(op: str, a, dt: str):
    """The IEEE-exact ones: integers stay integers (wrapping), floats are one float32 operation rounded once.  round is half-to-even."""
    rdt = unary_dtype(op, dt)
    if not is_float(dt) and op in KEEPS_INT:
        x = np.asarray(a).astype(np.int64)
        if dt == "bool" or dt.startswith("u"):
            v = {"abs": x, "square": x * x, "sign": (x > 0).astype(np.int64), "negative": -x}.get(op, x)
        else:
            with np.errstate(over="ignore"):
                v = {"abs": np.abs(x), "square": x * x, "sign": np.sign(x), "negative": -x}.get(op, x)
        return cast(v, rdt), rdt
    with np.errstate(all="ignore"):
        v = EXACT_UNARY[op](f32(a))
    return (np.asarray(v, bool), rdt) if rdt == "bool" else (cast(np.asarray(v, np.float32), rdt), rdt)


def unary_f64(op: str, a, dt: str):
    """The transcendental ones: float64 of the float32 operand, unrounded -- the caller's bound covers the kernel's error and the rounding."""
    with np.errstate(all="ignore"):
        return F64_UNARY[op](f32(a).astype(np.float64)), unary_dtype(op, dt)


def erf_f64(a):
    import math
    return np.vectorize(math.erf, otypes=[np.float64])(f32(a).astype(np.float64))


# ---- reductions -------------------------------------------------------------------------------------------------------------
def reduce_dtype(op: str, dt: str) -> str:
    if op in ("all", "any"):
        return "bool"
    if op in ("sum", "prod"):
        return "int32" if dt == "bool" else dt
    if op in ("mean", "logsumexp", "var", "std"):
        return dt if is_float(dt) else "float32"
    return dt                                            # max / min


def reduce(op: str, a, dt: str, axis=None, keepdims=False):
    """-> (value, dtype).  Integer sum / prod / max / min, all / any and float max / min (NaN propagates) are exact; float sum / prod, mean,
    logsumexp come back as float64 of the float32 operands, for the caller's bound."""
    rdt = reduce_dtype(op, dt)
    a = np.asarray(a)
    if op in ("all", "any"):
        return getattr(np, op)(a != 0, axis=axis, keepdims=keepdims), rdt
    if op in ("max", "min"):
        with np.errstate(invalid="ignore"):
            return getattr(np, op)(a, axis=axis, keepdims=keepdims), rdt
    if op in ("sum", "prod") and not is_float(dt):
        with np.errstate(over="ignore"):
            return cast(getattr(np, op)(_u64(a), axis=axis, keepdims=keepdims, dtype=np.uint64), rdt), rdt
    x = f32(a).astype(np.float64)
    with np.errstate(all="ignore"):
        if op == "logsumexp":
            m = x.max(axis=axis, keepdims=True)
            ms = np.where(np.isfinite(m), m, 0.0)
            v = np.log(np.exp(x - ms).sum(axis=axis, keepdims=True)) + ms
            v = np.where(m == -np.inf, -np.inf, v)
            return (v if keepdims else np.squeeze(v, axis=axis) if axis is not None else v.reshape(())), rdt
        return getattr(np, op)(x, axis=axis, keepdims=keepdims), rdt


def var(a, dt: str, axes=None, keepdims=False, ddof=0, std=False):
    x = f32(a).astype(np.float64)
    v = np.var(x, axis=axes, keepdims=keepdims, ddof=ddof)
    return (np.sqrt(v) if std else v), reduce_dtype("var", dt)


def argextreme(op: str, a, axis=None, keepdims=False):
    """argmax / argmin: the first index among ties; uint32.  (numpy's argmax / argmin take the first occurrence too.)"""
    a = np.asarray(a)
    v = (np.argmax if op == "argmax" else np.argmin)(a, axis=axis, keepdims=keepdims)
    return np.asarray(v).astype(np.uint32), "uint32"


# ---- scans ------------------------------------------------------------------------------------------------------------------
def _identity(kind: str, dt: str):
    if kind == "sum":
        return 0
    if kind == "prod":
        return 1
    if is_float(dt):
        return -np.inf if kind == "max" else np.inf
    info = np.iinfo(NP[dt])
    return info.min if kind == "max" else info.max


def scan(kind: str, a, dt: str, axis: int, reverse=False, inclusive=True):
    """cumsum / cumprod / cummax / cummin along `axis`.  Integers wrap in their own dtype; float cummax / cummin are exact and a NaN, once
    met, stays; float cumsum / cumprod come back as float64.  The exclusive form starts from the identity in the array's dtype."""
    a = np.moveaxis(np.asarray(a), axis, -1)
    if reverse:
        a = a[..., ::-1]
    ints = not is_float(dt)
    x = (a.astype(np.uint64) if dt == "uint64" else a.astype(np.int64)) if ints else f32(a).astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == "sum":
            inc = np.cumsum(x, -1)
        elif kind == "prod":
            inc = np.cumprod(x, -1)
        else:
            inc = (np.maximum if kind == "max" else np.minimum).accumulate(x, -1)        # NaN propagates and stays
    if not inclusive:
        first = np.full(x.shape[:-1] + (1,), _identity(kind, dt), dtype=x.dtype)
        inc = np.concatenate([first, inc[..., :-1]], -1)
    if reverse:
        inc = inc[..., ::-1]
    inc = np.moveaxis(inc, -1, axis)
    if ints:
        return cast(inc, dt), dt
    return (cast(inc, dt) if kind in ("max", "min") else inc), dt


# ---- order ------------------------------------------------------------------------------------------------------------------
def argsort(a, axis=-1):
    """Stable, ascending, NaN last, -0.0 == +0.0 (a tie: index order); uint32."""
    return np.argsort(np.asarray(a), axis=axis, kind="stable").astype(np.uint32), "uint32"


def sort(a, axis=-1):
    a = np.asarray(a)
    return np.take_along_axis(a, np.argsort(a, axis=axis, kind="stable"), axis)


def is_partition(values_in_result_order, kth: int, sorted_line) -> bool:
    """The partition promise along the last axis: position kth holds what a sort would put there, nothing before it is larger and nothing
    after it smaller (NaN counts as largest)."""
    v = np.where(np.isnan(values_in_result_order), np.inf, values_in_result_order) if values_in_result_order.dtype.kind == "f" else values_in_result_order
    s = np.where(np.isnan(sorted_line), np.inf, sorted_line) if sorted_line.dtype.kind == "f" else sorted_line
    pivot = s[..., kth:kth + 1]
    return bool((v[..., kth:kth + 1] == pivot).all() and (v[..., :kth] <= pivot).all() and (v[..., kth + 1:] >= pivot).all()
                and (np.sort(v, -1) == np.sort(s, -1)).all())


# ---- gathers ----------------------------------------------------------------------------------------------------------------
def wrap_index(idx, n: int) -> np.ndarray:
    """Negative indices count from the end; what is still outside [0, n) is clamped."""
    t = np.asarray(idx).astype(np.int64)
    t = np.where(t < 0, t + n, t)
    return np.clip(t, 0, n - 1)


def take_axis(a, idx, axis: int):
    a = np.asarray(a)
    return np.take(a, wrap_index(idx, a.shape[axis]), axis=axis)


def take(a, idx):
    a = np.asarray(a).reshape(-1)
    return a[wrap_index(idx, a.size)]


def take_along_axis(a, idx, axis: int):
    a, idx = np.asarray(a), np.asarray(idx)
    shape = list(np.broadcast_shapes(tuple(1 if d == axis % a.ndim else s for d, s in enumerate(a.shape)),
                                     tuple(1 if d == axis % a.ndim else s for d, s in enumerate(idx.shape))))
    sa, si = list(shape), list(shape)
    sa[axis], si[axis] = a.shape[axis], idx.shape[axis]
    return np.take_along_axis(np.broadcast_to(a, sa), wrap_index(np.broadcast_to(idx, si), a.shape[axis]), axis)


# ---- softmax, convolution -----------------------------------------------------------------------------------------------------
def softmax_f64(a, axes):
    x = f32(a).astype(np.float64)
    axes = tuple(axes) if not isinstance(axes, int) else (axes,)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=axes, keepdims=True))
        return e / e.sum(axis=axes, keepdims=True)


def conv1d_f64(x, w, stride=1, padding=0, dilation=1, groups=1):
    """x [B, L, Cin], w [Cout, K, Cin / groups] -> ([B, Lout, Cout] float64, sum of |terms| per output): a direct loop."""
    x, w = f32(x).astype(np.float64), f32(w).astype(np.float64)
    y, mag = conv2d_f64(x[:, None], w[:, None], (1, stride), (0, padding), (1, dilation), groups)
    return y[:, 0], mag[:, 0]


def conv2d_f64(x, w, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1):
    """x [B, H, W, Cin], w [Cout, kH, kW, Cin / groups] -> ([B, Ho, Wo, Cout] float64, sum of |terms| per output): a direct loop."""
    x, w = f32(x).astype(np.float64), f32(w).astype(np.float64)
    B, H, W, Cin = x.shape
    Cout, kH, kW, cig = w.shape
    cog = Cout // groups
    Ho = (H + 2 * padding[0] - dilation[0] * (kH - 1) - 1) // stride[0] + 1
    Wo = (W + 2 * padding[1] - dilation[1] * (kW - 1) - 1) // stride[1] + 1
    y, mag = np.zeros((B, Ho, Wo, Cout)), np.zeros((B, Ho, Wo, Cout))
    for oy in range(Ho):
        for ox in range(Wo):
            for kh in range(kH):
                iy = oy * stride[0] - padding[0] + kh * dilation[0]
                if iy < 0 or iy >= H:
                    continue
                for kw in range(kW):
                    ixx = ox * stride[1] - padding[1] + kw * dilation[1]
                    if ixx < 0 or ixx >= W:
                        continue
                    for co in range(Cout):
                        g = co // cog
                        t = x[:, iy, ixx, g * cig:(g + 1) * cig] * w[co, kh, kw]
                        y[:, oy, ox, co] += t.sum(-1)
                        mag[:, oy, ox, co] += np.abs(t).sum(-1)
    return y, mag


# ---- bounds -----------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24                      # float32 unit roundoff


def out_rounding(ref, dt: str):
    """Half an ulp of the result dtype at |ref|: the final rounding of a float32 value into `dt`."""
    eps = {"float32": 2.0 ** -24, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}[dt]
    tiny = {"float32": 2.0 ** -150, "float16": 2.0 ** -25, "bfloat16": 2.0 ** -134}[dt]      # half the smallest subnormal
    return np.abs(ref) * eps + tiny
