"""GPU: the packed-weight matrix-core GEMM (csrc/qgemm.hip) against its definition, out = x . dequant(W)^T in float64, at the edges
the DiT's own shapes never reach: one, three and five 64-k steps (the even / odd pipeline pair), widths that are no multiple of 4 (the
scalar epilogue) or of the 256-column tile, a ragged plain segment in front of SwiGLU tiles, SwiGLU widths below and just above one
128-pair tile, biases == None, the row edges of the 128-row kernel, and the 256-row kernel with an XCD-remap remainder and a one-member
row-tile group.  test_gpu_klein_quant.py holds the same kernel to dequantise + the pinned bf16 GEMM bit for bit at the DiT's shapes.

Weights: every (row, group) block is a normal draw (sigma 0.05) shifted by its own offset (up to +-0.15) and multiplied by its own
2^u; the u of a row are a permutation of linspace(-2, 2, groups), so the scales of a row span a factor of 16 before the block's range
enters, and scales and biases of neighbouring groups differ by integer factors: a kernel that read the wrong group's scale or bias, the
wrong 32-k half or a swapped index is off by whole codes.  Every test asserts max |scale| / min |scale| >= 4 on every row that has
more than one group.  The triplets come from omx.ops.quantize; the reference reads the same triplets back,
wd = ref_core.dequantize(q, s, b, group, bits, "bf16"): the kernel's B operand exactly (test_dequantize_is_exact holds omx_dequantize to
it).  Activations are seeded standard normals on the bf16 grid.

  1. identity activations: the output IS wd^T, no tolerance;  2. plain and gated forms against float64 at M x N x K edges of the 128-row
  kernel, with and without biases, through the C entry with a sentinel tail behind the output;  3. the 256-row kernel;  4. SwiGLU
  against float64;  5. refusals.
Every bound is derived in the docstring of its test, none is tuned; each float64 test prints its largest error / bound."""
import numpy as np
import pytest

from oracle import ref_core as rc
from test_gpu_klein_quant import FORMATS, _pin_bf16_kernel

pytestmark = pytest.mark.gpu

SENT, PAD = 7.0, 64          # the C-entry launches write into a buffer PAD elements longer than the output, pre-filled with SENT


def _weight(N, K, group, seed):
    """bf16 [N, K] whose (row, group) blocks have their own factor 2^u and their own offset (module docstring)"""
    g = np.random.default_rng(seed)
    ng = K // group
    w = 0.05 * g.standard_normal((N, ng, group))
    u = g.permuted(np.tile(np.linspace(-2.0, 2.0, ng), (N, 1)), axis=1) if ng > 1 else g.uniform(-2.0, 2.0, (N, 1))
    off = g.uniform(-0.15, 0.15, (N, ng, 1))
    return rc.bf16_round(((w + off) * np.exp2(u)[..., None]).reshape(N, K).astype(np.float32))


class Case:
    """one problem: the device operands, and in float64 the activations and the dequantised weight with (wd) and without (wd0) biases"""

    def __init__(self, omx, M, N, K, group, bits, seed, x=None):
        T = omx.ops.Tensor
        self.M, self.N, self.K, self.group, self.bits = M, N, K, group, bits
        self.q, self.s, self.b = omx.ops.quantize(T.from_numpy(_weight(N, K, group, seed)), group, bits)
        qh, sh, bh = self.q.numpy(), self.s.numpy(), self.b.numpy()
        if K // group > 1:       # (one group per row: nothing to tell apart)
            spread = np.abs(sh).max(axis=1) / np.abs(sh).min(axis=1)
            assert (spread >= 4).all(), f"the scales of row {spread.argmin()} differ by {spread.min():.2f} only"
            assert (np.abs(bh).max(axis=1) > 0).all()
        self.wd = rc.dequantize(qh, sh, bh, group, bits, "bf16").astype(np.float64)
        self.wd0 = rc.dequantize(qh, sh, np.zeros_like(bh), group, bits, "bf16").astype(np.float64)   # bf16(q * s) from the unpacked codes
        assert np.isfinite(self.wd).all() and np.abs(self.wd - self.wd0).max() > 0
        if x is None:
            xh = rc.bf16_round(np.random.default_rng(seed + 1).standard_normal((M, K)).astype(np.float32))
            x = T.from_numpy(xh)
            self.xs = xh.astype(np.float64)
        self.x = x

    def biases(self, on):
        return self.b if on else None

    def weight(self, on):
        return self.wd if on else self.wd0


def _ulp(v):
    """one bf16 ulp of v: 2^(floor(log2 |v|) - 7)"""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 7)


def _linear_bound(K, acc, mag, resid=None, gate=None):
    """(reference, bound) of bf16(resid + acc * gate[col]), acc one f32 chain over K products (the plain form: resid 0, gate 1):
    one bf16 ulp of the reference  +  K 2^-23 (|x| @ |wd|^T) |gate|  (the f32 accumulation: K roundings, each below 2^-24 of a partial
    sum that (|x| @ |wd|^T) bounds, with a factor 2 to spare)  +  2^-23 (|resid| + |acc gate|)  (the epilogue's f32 multiply and add).
    At K <= 3072 the f32 terms are below 2^-11 of the magnitudes, a bf16 ulp is 2^-7..2^-8: about one output ulp and nothing more."""
    resid = np.zeros_like(acc) if resid is None else resid.astype(np.float64)
    gate = np.ones(acc.shape[1]) if gate is None else gate.astype(np.float64)
    ref = resid + acc * gate
    return ref, _ulp(ref) + K * 2.0 ** -23 * mag * np.abs(gate) + 2.0 ** -23 * (np.abs(resid) + np.abs(acc * gate))


def _ratio(got, ref, bound, what):
    """largest error / bound; fails with the worst element when it exceeds 1 (a NaN fails too)"""
    err = np.abs(got.astype(np.float64) - ref)
    r = err / bound
    ok = err <= bound
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, 0.0, np.where(np.isnan(r), np.inf, r))), r.shape)
        raise AssertionError(f"{what}: {np.count_nonzero(~ok)} of {ok.size} elements outside the bound, worst at {i}: got {got[i]} "
                             f"want {ref[i]} error / bound {r[i]:.3f}")
    return float(r.max())


def _resid_gate(M, N, seed):
    g = np.random.default_rng(seed)
    return (rc.bf16_round(g.standard_normal((M, N)).astype(np.float32)), rc.bf16_round(g.standard_normal(N).astype(np.float32)))


def _exact(got, want, what):
    """got == want value for value (IEEE ==: a zero equals a zero)"""
    assert got.shape == want.shape, what
    bad = np.argwhere(~(got == want))
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} elements differ, first at row {bad[0][0]} column {bad[0][1]}: got "
                           f"{got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


# ---- 1. exact probe ----

_EYES = {}


def _eye(omx, K):
    if K not in _EYES:
        _EYES[K] = omx.ops.Tensor.from_numpy(np.eye(K, dtype=np.float32))
    return _EYES[K]


def _probe_ks(group):
    """nt = K / 64 of 1, 2, 3 and 5 (K a multiple of the group); at group 128: 2 and 6"""
    return (128, 384) if group == 128 else (64, 128, 192, 320)


@pytest.mark.parametrize("bits,group", FORMATS)
def test_identity_rows_read_the_dequantised_weight_back(omx, bits, group):
    """x = the K x K identity (M = K: 64 .. 384 rows, whole and ragged 128-row tiles): out[m, n] = 1.0 * wd[n, m] + zeros, exact in
    f32 and already a bf16 value, so the output equals wd^T with no tolerance -- the swizzle, the 32-k halves, word and field order, the
    group index and the row clamp against the definition.  N = 37 (scalar epilogue, one ragged tile), 256 (one tile), 261 (tile + 5)."""
    for K in _probe_ks(group):
        for N in (37, 256, 261):
            c = Case(omx, K, N, K, group, bits, 1000 + K + N, x=_eye(omx, K))
            got = omx.ops.quantized_linear(c.x, c.q, c.s, c.b, group, bits).numpy()
            _exact(got, c.wd.T.astype(np.float32), f"K {K} N {N}")


@pytest.mark.parametrize("bits,group", FORMATS)
def test_identity_rows_without_biases(omx, bits, group):
    """biases = None: the output equals bf16(q * s) of the unpacked codes (and differs from the weight with biases)"""
    K, N = (384 if group == 128 else 192), 261
    c = Case(omx, K, N, K, group, bits, 2000 + K, x=_eye(omx, K))
    got = omx.ops.quantized_linear(c.x, c.q, c.s, None, group, bits).numpy()
    _exact(got, c.wd0.T.astype(np.float32), f"K {K} N {N}")


@pytest.mark.parametrize("bits,group", FORMATS)
@pytest.mark.parametrize("n_plain,half", [(132, 124), (260, 4)])
def test_identity_rows_through_the_swiglu_launch(omx, bits, group, n_plain, half):
    """the plain segment of the segmented launch, ragged against the 256-column tile and followed by one partial SwiGLU tile, equals
    wd[:n_plain]^T exactly: its clamped tail columns sit next to act_tile0 and read neither gate nor up rows"""
    K = 128 if group == 128 else 320
    c = Case(omx, K, n_plain + 2 * half, K, group, bits, 3000 + n_plain, x=_eye(omx, K))
    for on in (True, False):
        plain, act = omx.ops.quantized_linear_swiglu(c.x, c.q, c.s, c.biases(on), n_plain, group, bits)
        _exact(plain.numpy(), c.weight(on)[:n_plain].T.astype(np.float32), f"biases {on}")
        assert act.shape == (K, half) and np.isfinite(act.numpy()).all()


# ---- 2. plain and gated forms against float64, the 128-row kernel ----

def _launch_guarded(omx, c, on, resid, gate):
    """omx_quantized_linear_mfma into a buffer with a sentinel tail; returns [M, N] float32"""
    T = omx.ops.Tensor
    out = T.from_numpy(np.full((c.M * c.N + PAD,), SENT, np.float32))
    b = c.biases(on)
    omx.check(omx.lib.omx_quantized_linear_mfma(out.ptr, c.x.ptr, c.q.ptr, c.s.ptr, b.ptr if b is not None else None,
                                                resid.ptr if resid is not None else None, gate.ptr if gate is not None else None,
                                                c.M, c.N, c.K, c.group, c.bits, None))
    got = out.numpy()
    assert (got[c.M * c.N:] == SENT).all(), "the launch wrote past its output"
    return got[:c.M * c.N].reshape(c.M, c.N)


# (bits, group, M, N, K): per width every M of {1, 16, 127, 128, 129, 255, 256, 257}, every N of {4, 37, 131, 256, 261, 515} (4: scalar
# epilogue off, one run; 37, 131: scalar epilogue; 256: one tile; 261, 515: tiles + 5 / + 3 through the scalar epilogue) and every K
# of {64, 192, 320, 3072} (nt 1, 3, 5, 48); each case runs plain and gated, with and without biases
LINEAR_CASES = [
    (4, 64, 1, 37, 64), (4, 32, 16, 4, 192), (4, 64, 127, 261, 320), (4, 128, 128, 131, 3072),
    (4, 32, 129, 515, 64), (4, 64, 255, 256, 192), (4, 32, 256, 37, 320), (4, 32, 257, 261, 3072),
    (8, 128, 1, 515, 3072), (8, 32, 16, 261, 64), (8, 32, 127, 4, 192), (8, 32, 128, 256, 320),
    (8, 64, 129, 37, 3072), (8, 64, 255, 131, 64), (8, 64, 256, 515, 192), (8, 64, 257, 4, 320),
]


def test_linear_cases_cover_every_edge():
    for bits in (4, 8):
        mine = [c for c in LINEAR_CASES if c[0] == bits]
        assert {c[2] for c in mine} == {1, 16, 127, 128, 129, 255, 256, 257}
        assert {c[3] for c in mine} == {4, 37, 131, 256, 261, 515}
        assert {c[4] for c in mine} == {64, 192, 320, 3072}
        assert {c[1] for c in mine} == {32, 64, 128}
    for _, _, M, N, _ in LINEAR_CASES:
        assert ((M + 255) // 256) * ((N + 255) // 256) < 160     # pick_rows: the 128-row kernel


@pytest.mark.parametrize("bits,group,M,N,K", LINEAR_CASES)
def test_plain_and_gated_against_float64(omx, bits, group, M, N, K):
    """acc = x64 @ wd^T; plain bf16(acc), gated bf16(resid + acc * gate[col]); the bound of _linear_bound: one bf16 ulp of the
    reference + K 2^-23 (|x| @ |wd|^T) |gate| + 2^-23 (|resid| + |acc gate|)"""
    T = omx.ops.Tensor
    c = Case(omx, M, N, K, group, bits, 4000 + 7 * M + N + K)
    resid, gate = _resid_gate(M, N, M + N)
    rd, gd = T.from_numpy(resid), T.from_numpy(gate)
    worst = {"plain": 0.0, "gated": 0.0}
    for on in (True, False):
        w = c.weight(on)
        acc, mag = c.xs @ w.T, np.abs(c.xs) @ np.abs(w).T
        ref, bound = _linear_bound(K, acc, mag)
        worst["plain"] = max(worst["plain"], _ratio(_launch_guarded(omx, c, on, None, None), ref, bound, f"plain, biases {on}"))
        ref, bound = _linear_bound(K, acc, mag, resid, gate)
        worst["gated"] = max(worst["gated"], _ratio(_launch_guarded(omx, c, on, rd, gd), ref, bound, f"gated, biases {on}"))
    print(f"qgemm {bits}-bit group {group} M {M} N {N} K {K}: largest error / bound plain {worst['plain']:.3f} gated {worst['gated']:.3f}")


# ---- 3. the 256-row kernel ----

@pytest.mark.parametrize("bits,group", [(4, 32), (8, 64)])
def test_256_row_kernel_tall_and_narrow(omx, monkeypatch, bits, group):
    """M = 10243, N = 805, K = 192: 41 x 4 = 164 tiles of 256 rows (>= 160: pick_rows takes the 256-row kernel), 164 % 8 = 4 (the XCD
    remap has a remainder), 41 = 5 * 8 + 1 (the last row-tile group has one member), the last row tile holds 3 rows, N has a scalar
    tail, nt = 3.  Plain and gated against float64 with the bound of _linear_bound; plain also equals dequantise + the pinned bf16
    16x16x32 kernel bit for bit."""
    M, N, K = 10243, 805, 192
    assert ((M + 255) // 256, (N + 255) // 256) == (41, 4) and M % 256 == 3
    T = omx.ops.Tensor
    c = Case(omx, M, N, K, group, bits, 5000 + bits)
    resid, gate = _resid_gate(M, N, 5)
    acc, mag = c.xs @ c.wd.T, np.abs(c.xs) @ np.abs(c.wd).T
    plain = omx.ops.quantized_linear(c.x, c.q, c.s, c.b, group, bits).numpy()
    gated = omx.ops.quantized_linear(c.x, c.q, c.s, c.b, group, bits, resid=T.from_numpy(resid), gate=T.from_numpy(gate)).numpy()
    rp = _ratio(plain, *_linear_bound(K, acc, mag), "plain")
    rg = _ratio(gated, *_linear_bound(K, acc, mag, resid, gate), "gated")
    print(f"qgemm 256-row {bits}-bit group {group} M {M} N {N} K {K}: largest error / bound plain {rp:.3f} gated {rg:.3f}")
    _pin_bf16_kernel(monkeypatch)
    pinned = omx.ops.linear(c.x, omx.ops.dequantize(c.q, c.s, c.b, group, bits)).numpy()
    np.testing.assert_array_equal(plain, pinned)


@pytest.mark.parametrize("bits,group", [(4, 64), (8, 32)])
def test_256_row_kernel_one_column_tile(omx, bits, group):
    """M = 40961, N = 8, K = 64: grid_n = 1, 161 row tiles of 256 (161 % 8 = 1, 161 = 20 * 8 + 1), the last of one row, nt = 1;
    with and without biases"""
    M, N, K = 40961, 8, 64
    assert ((M + 255) // 256) * ((N + 255) // 256) >= 160
    T = omx.ops.Tensor
    c = Case(omx, M, N, K, group, bits, 6000 + bits)
    resid, gate = _resid_gate(M, N, 6)
    rd, gd = T.from_numpy(resid), T.from_numpy(gate)
    rp = rg = 0.0
    for on in (True, False):
        w = c.weight(on)
        acc, mag = c.xs @ w.T, np.abs(c.xs) @ np.abs(w).T
        plain = omx.ops.quantized_linear(c.x, c.q, c.s, c.biases(on), group, bits).numpy()
        gated = omx.ops.quantized_linear(c.x, c.q, c.s, c.biases(on), group, bits, resid=rd, gate=gd).numpy()
        rp = max(rp, _ratio(plain, *_linear_bound(K, acc, mag), f"plain, biases {on}"))
        rg = max(rg, _ratio(gated, *_linear_bound(K, acc, mag, resid, gate), f"gated, biases {on}"))
    print(f"qgemm 256-row {bits}-bit group {group} M {M} N {N} K {K}: largest error / bound plain {rp:.3f} gated {rg:.3f}")


# ---- 4. SwiGLU ----

# (M, n_plain, half, K): one partial tile of 4; a ragged plain segment + one tile and 4; plain tile + 4 in front of a partial tile;
# three tiles and 4 behind a 4-column plain segment; two plain tiles + 4 and two full SwiGLU tiles at the DiT's K
SWIGLU_SHAPES = [(17, 0, 4, 64), (129, 132, 132, 192), (40, 260, 124, 320), (257, 4, 388, 128), (300, 516, 256, 3072)]
SWIGLU_CASES = [(M, n_plain, half, K, bits, group) for M, n_plain, half, K in SWIGLU_SHAPES for bits, group in FORMATS if K % group == 0]


@pytest.mark.parametrize("M,n_plain,half,K,bits,group", SWIGLU_CASES)
def test_swiglu_against_float64(omx, M, n_plain, half, K, bits, group):
    """W = [n_plain plain | half gate | half up] rows.  Reference: float64 accumulations g and u, ref = g sigmoid(g) u.  The kernel
    rounds both f32 accumulators to bf16, evaluates silu(g) * u in f32 and rounds once.  With
        eg = ulp_bf16(g) + K 2^-23 (|x| @ |wg|^T)     (the distance of the rounded accumulator from g; eu likewise)
    the kernel's gate operand g' lies within eg of g and silu(g') within 1.1 eg of silu(g) (|silu'| <= 1.0998), its up operand u'
    within eu of u, so  silu(g') u' - silu(g) u = (silu(g') - silu(g)) u + silu(g) (u' - u) + (silu(g') - silu(g)) (u' - u)  gives
        bound = ulp_bf16(ref) + 1.1 eg |u| + |g sigmoid(g)| eu + 1.1 eg eu + 2^-20 |ref|
    the first term the output rounding, the last expf, the f32 divide and multiply.  The plain segment: _linear_bound."""
    c = Case(omx, M, n_plain + 2 * half, K, group, bits, 7000 + M + K)
    ra = rp = 0.0
    for on in (True, False):
        plain, act = omx.ops.quantized_linear_swiglu(c.x, c.q, c.s, c.biases(on), n_plain, group, bits)
        w = c.weight(on)
        acc, mag = c.xs @ w.T, np.abs(c.xs) @ np.abs(w).T
        g, u = acc[:, n_plain:n_plain + half], acc[:, n_plain + half:]
        eg = _ulp(g) + K * 2.0 ** -23 * mag[:, n_plain:n_plain + half]
        eu = _ulp(u) + K * 2.0 ** -23 * mag[:, n_plain + half:]
        sg = g / (1.0 + np.exp(-g))
        ref = sg * u
        bound = _ulp(ref) + 1.1 * eg * np.abs(u) + np.abs(sg) * eu + 1.1 * eg * eu + 2.0 ** -20 * np.abs(ref)
        assert act.shape == (M, half)
        ra = max(ra, _ratio(act.numpy(), ref, bound, f"swiglu, biases {on}"))
        if n_plain:
            assert plain.shape == (M, n_plain)
            rp = max(rp, _ratio(plain.numpy(), *_linear_bound(K, acc[:, :n_plain], mag[:, :n_plain]), f"plain segment, biases {on}"))
        else:
            assert plain is None
    print(f"qgemm swiglu {bits}-bit group {group} M {M} n_plain {n_plain} half {half} K {K}: largest error / bound swiglu {ra:.3f} "
          f"plain segment {rp:.3f}")


# ---- 5. refusals ----

def test_refusals(omx):
    T = omx.ops.Tensor

    def operands(M, N, K, group, bits=8):      # refused before any launch: the values do not matter
        return (T.from_numpy(np.zeros((M, K), np.float32)), T.from_numpy(np.zeros((N, K * bits // 32), np.uint32), "u32"),
                T.from_numpy(np.ones((N, K // group), np.float32)), T.from_numpy(np.zeros((N, K // group), np.float32)))

    x, q, s, b = operands(20, 16, 96, 32)      # K % group == 0, but the kernel steps 64 k
    with pytest.raises(omx.OmxError, match="K=96 must be a multiple of 64"):
        omx.ops.quantized_linear(x, q, s, b, 32, 8)
    with pytest.raises(omx.OmxError, match="K=96 must be a multiple of 64"):
        omx.ops.quantized_linear_swiglu(x, q, s, b, 8, 32, 8)
    x, q, s, b = operands(20, 16, 128, 64)
    with pytest.raises(omx.OmxError, match="must be multiples of 4"):      # half = 6
        omx.ops.quantized_linear_swiglu(x, q, s, b, 4, 64, 8)
    with pytest.raises(omx.OmxError, match="must be multiples of 4"):      # n_plain = 2 (half = 7)
        omx.ops.quantized_linear_swiglu(x, q, s, b, 2, 64, 8)
    x, q, s, b = operands(20, 10, 128, 64)
    with pytest.raises(omx.OmxError, match="must be multiples of 4"):      # n_plain = 2, half = 4
        omx.ops.quantized_linear_swiglu(x, q, s, b, 2, 64, 8)
    x, q, s, b = operands(20, 16, 128, 64)
    resid, gate = T.from_numpy(np.zeros((20, 16), np.float32)), T.from_numpy(np.ones(16, np.float32))
    with pytest.raises(omx.OmxError, match="both resid and gate"):
        omx.ops.quantized_linear(x, q, s, b, 64, 8, resid=resid)
    with pytest.raises(omx.OmxError, match="both resid and gate"):
        omx.ops.quantized_linear(x, q, s, b, 64, 8, gate=gate)
    out = omx.ops.quantized_linear(x, q, s, b, 64, 8, resid=resid, gate=gate).numpy()      # ... and both are taken
    assert (out == 0).all()
