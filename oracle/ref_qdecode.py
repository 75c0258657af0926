"""Float64 reference and derived error bound of the packed-weight decode GEMV: csrc/quant.hip with qgemv_body.inc (the VALU kernel,
and bit for bit behind it qgemv_rows.hip) and csrc/qgemv_mfma.hip (4-bit group 64 on the matrix cores).  ref_decode.py's checks
(check_plain, check_residual, check_swiglu, check_argmax) take a per-row magnitude and a chain depth; this module supplies both for the
packed arithmetic.  Both are read off the kernels, line by line below; neither is fitted.  u = 2^-24.

What a row adds up (qgemv_body.inc, `consume`).  A row of K elements is cut into lane chunks c of EPL elements, each inside one
quantisation group g (scale s_g, bias b_g, both exact 16-bit values widened to f32).  Per chunk the lane forms

    d    = sum_k x_k (m + q_k)            l. 138-157: EPL / 2 v_dot2 instructions (8 bits: EPL fmas) from d = 0
    b'   = fma(-m, s_g, b_g)              l. 158     (m = 0: b' = b_g, no rounding)
    acc  = fma(s_g, d, acc)               l. 159
    acc  = fma(b', xsum_c, acc)           l. 160     xsum_c = sum_k x_k in f32, staged once per block (stage_chunk, quant.hpp)

and the 64 lanes' acc meet in wave_sum (l. 165).  m is the "magic" the unpack leaves in every weight: a field q becomes the bf16 value
0x4300 | q = 128 + q by bit assembly, so m = 128 on bfloat16 triplets at 4 bits and at the chunked widths (2, 3, 5, 6); m = 0 at 8 bits
((float)q) and on float16 triplets, where A::unmagic takes the 1024 of 0x6400 | q off again exactly before the product (act16.hpp).

Magnitude.  The kernel does not add x_k w_k = x_k (s q_k + b): it adds s x_k (m + q_k) and (b - m s) x_k, two streams whose m s x_k
parts cancel only in exact arithmetic.  Every rounding is relative to what is actually added, so the magnitude of a row is

    M_r = sum_c ( |s_g| sum_k |x_k| (m + q_k)  +  |b_g - m s_g| sum_k |x_k| )

-- with m = 128 an order of magnitude above sum |x| |w| for a 4-bit matrix (q <= 15), which is why sum |x| |w| is NOT a valid magnitude
here: a bound n u sum|x||w| with the true n would fail on a correct kernel, and one fitted to pass hides the factor in n.

Depth (VALU kernel), the longest chain of f32 roundings any addend passes through, term by term:
  * d: bfloat16 v_dot2c_f32_bf16 adds two exact products (8 x 8 significant bits) to the accumulator, at most one rounding per
    product (ref_decode.gemv_acc_depth's model of the same instruction): EPL.  8 bits: one fma per element: EPL.  float16
    v_dot2_f32_f16 rounds its two products and the accumulator in ONE unspecified step (gemv_parts.hpp:14): bounded as one rounding
    per product plus one per instruction, EPL + EPL / 2.
  * xsum_c (stage_chunk): per 16-byte vector `sv += lo + hi` four times -- an element passes the pair add and at most four running
    adds: 5 -- then log2(EPL / 8) DPP levels.  b' adds one rounding to the same product: 5 + log2(EPL / 8) + 1.
    The two streams are separate addends, so a chunk costs max(d, xsum + b') roundings before it joins acc.
  * acc: two fmas per step of the lane, steps = K / (64 EPL) (chunked widths: ceil(K / 2048), EPL = 32): 2 steps.
  * wave_sum: 6 levels.
  * + 1 for the second-order terms of (1 + u)^n (n u < 2^-17 here).
The 16-bit store of the sum is ref_decode's "rounding of the stored point", outside the depth.

Depth (matrix-core kernel, qgemv_mfma.hip), bfloat16 4-bit group 64 only, m = 128; a lane chunk is a whole group (EPL = 64 staging,
l. 136) and a wave owns one 1024-column superchunk of 16 rows:
  * group sum D: four v_mfma_f32_16x16x32_bf16 per accumulator (l. 159-166), each adding 16 live exact products (the other 16 meet
    staged zeros) to it with an unspecified internal order: one rounding per product plus one per instruction, 64 + 4.
  * xsum over 64 elements: 5 + 3 DPP levels, + 1 for the fold fma(-128, s, b) (l. 175): 9.  max(68, 9) = 68.
  * r: two fmas for each of the lane's 4 groups (l. 176-177): 8; the two __shfl_xor adds over the k-block quarters (l. 180-181): 2.
  * the KS superchunk partials summed in order from 0 (l. 199): KS.
  * + 1 second order.

One-hot rows (the dequantise-through-the-GEMV probe): every sum has ONE non-zero term, so d, xsum_c, every later add of an exact zero
and the matrix cores' sum are exact; what rounds is fma(s, d, 0), the fold b', fma(b', xsum, acc): 3, taken as PROBE_DEPTH = 4.
"""
import numpy as np

from . import ref_decode as rd

U24 = rd.U24
PROBE_DEPTH = 4
CHUNKED = (2, 3, 5, 6)


def magic(bits, dt):
    """m: what the unpack leaves added to every code (128 on bf16 triplets at 4 bits and the chunked widths, else 0)"""
    return 128.0 if dt == "bf16" and bits != 8 else 0.0


def words(bits, K, group):
    """qgemv_words (quant.hip): u32 words per lane and step; 0: no kernel"""
    if bits in CHUNKED:
        return bits if (K > 0 and K % 32 == 0 and group >= 32) else 0
    epw = 32 // bits
    W = 4
    while W * epw > 8 and (K % (64 * W * epw) != 0 or W * epw > group):
        W >>= 1
    return W if (K % (64 * W * epw) == 0 and W * epw <= group and W * epw >= 8) else 0


def epl(bits, K, group):
    """elements of a lane chunk"""
    return 32 if bits in CHUNKED else words(bits, K, group) * (32 // bits)


def steps(bits, K, group):
    e = epl(bits, K, group)
    return -(-K // (64 * e))


def valu_depth(bits, K, group, dt, x_span=None):
    """chain depth of the VALU kernel (module docstring).  x_span: the number of binades the activations are known to span (rand16's
    hi - lo + 1; None: unknown, e.g. behind the RMSNorm prologue).  On bfloat16 triplets every product x (m + q) is an integer
    (m + q < 2^8) times x's ulp, a multiple of 2^(emin - 7), and every partial sum of a chunk stays below EPL 2^(emax + 1) 2^8: while
    EPL 2^x_span <= 2^9 all of them are f32 values and d is EXACT whatever the instruction's internal order; xsum_c (8-bit values) is
    exact a fortiori.  The chunk then costs the fold's one rounding instead of max(d, xsum + b').  float16 products carry 11 + bits
    significant bits and get no such pass."""
    e = epl(bits, K, group)
    d = e if (dt == "bf16" or bits == 8) else e + e // 2
    xs = 5 + int(np.log2(e // 8)) + 1
    chunk = max(d, xs)
    if dt == "bf16" and x_span is not None and e * 2 ** x_span <= 2 ** 9:
        chunk = 1
    return chunk + 2 * steps(bits, K, group) + 6 + 1


def mfma_depth(K):
    """chain depth of the matrix-core kernel, KS = K / 1024 (module docstring)"""
    return max(64 + 4, 5 + 3 + 1) + 8 + 2 + K // 1024 + 1


# ---- triplets built from codes ----

def make_triplet(rng, N, K, bits, group, dt, s_exp=None, b_exp=(-7, -3)):
    """(codes [N, K] uint8, scales [N, K / group], biases [N, K / group]): codes uniform over the full range with row 0 all zero and
    row 1 all maximum (where there are that many rows); scales exact in dt with both signs (MLX stores negative scales), three
    binades from 2^(-3 - bits) so that the weights s q + b are of one size at every width; biases exact in dt, one in eight exactly 0"""
    if s_exp is None:
        s_exp = (-3 - bits, -1 - bits)
    q = rng.integers(0, 1 << bits, size=(N, K), dtype=np.uint8)
    q[0] = 0
    if N > 1:
        q[1] = (1 << bits) - 1
    G = K // group
    s = rd.rand16(rng, (N, G), dt, *s_exp)
    b = rd.rand16(rng, (N, G), dt, *b_exp)
    b[rng.integers(0, 8, size=(N, G)) == 0] = 0.0
    return q, s, b


def pack(q, bits):
    """codes [N, K] -> u32 words [N, K * bits / 32]: element j is the bits-wide field at bit j * bits of the row's little-endian bit
    string (MLX's layout at every width; a 3 / 5 / 6-bit field may straddle two words)"""
    N, K = q.shape
    out = np.empty((N, K * bits // 32), np.uint32)
    for r in range(0, N, 4096):
        if 32 % bits == 0:      # whole fields per word
            sh = (np.arange(32 // bits, dtype=np.uint32) * np.uint32(bits))
            out[r:r + 4096] = (q[r:r + 4096].reshape(-1, K * bits // 32, 32 // bits).astype(np.uint32) << sh).sum(-1, dtype=np.uint32)
        else:                   # through the bit string
            b = ((q[r:r + 4096, :, None] >> np.arange(bits, dtype=np.uint8)) & 1).reshape(-1, K * bits // 32, 32)
            out[r:r + 4096] = (b.astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
    return out


def dequant(q, s, b, group):
    """float64 [N, K]: s q + b"""
    return np.repeat(s.astype(np.float64), group, axis=1) * q + np.repeat(b.astype(np.float64), group, axis=1)


def rows_ref(q, s, b, group, x, m, chunk=4096):
    """(exact [N], M_r [N]) of x against the triplet, float64: exact = sum_k x_k (s q_k + b); M_r as in the module docstring (the sums
    over chunks of a group add up to the sums over the group).  Row-chunked like ref_decode.rows_dot: a vocabulary-sized matrix does not
    fit in float64 at once."""
    N, K = q.shape
    G = K // group
    xg = np.asarray(x, np.float64).reshape(G, group)
    xa = np.abs(xg)
    sx, sa = xg.sum(1), xa.sum(1)
    exact, mag = np.empty(N), np.empty(N)
    for r in range(0, N, chunk):
        qg = q[r:r + chunk].reshape(-1, G, group).astype(np.float64)
        sd, bd = s[r:r + chunk].astype(np.float64), b[r:r + chunk].astype(np.float64)
        exact[r:r + chunk] = (sd * np.einsum("ngk,gk->ng", qg, xg) + bd * sx).sum(1)
        mag[r:r + chunk] = (np.abs(sd) * (np.einsum("ngk,gk->ng", qg, xa) + m * sa) + np.abs(bd - m * sd) * sa).sum(1)
    return exact, mag


def norm_slack_q(q, s, b, group, x, nw, eps, dt):
    """ref_decode.norm_slack for a triplet, without the dense matrix: (xn, slack per row) -- only the columns whose RMSNorm rounding
    can flip are dequantised.  The flips move the kernel's row by sum_k |hi_k - lo_k| |w_rk| with the TRUE weight w = s q + b: the
    two streams' m s x parts cancel exactly in what a changed x adds."""
    mid, lo, hi = rd.norm_candidates(x, nw, eps, dt, rd.gemv_norm_depth(np.asarray(x).size))
    d = hi - lo
    idx = np.nonzero(d)[0]
    if not idx.size:
        return mid, np.zeros(q.shape[0])
    g = idx // group
    w = s[:, g].astype(np.float64) * q[:, idx] + b[:, g].astype(np.float64)
    return mid, np.abs(w) @ d[idx]


def probe_ref(q, s, b, group, m, xv=0.125):
    """the one-hot probe: row k of x is xv at column k.  (want [K, N], tol [K, N], step [K, N]): want = xv (s q + b) of element
    (r, k), tol = PROBE_DEPTH u xv (|s| (m + q) + |b - m s|), step = xv |s|, one code step"""
    sd, bd = np.repeat(s.astype(np.float64), group, axis=1), np.repeat(b.astype(np.float64), group, axis=1)
    want = xv * (sd * q + bd)
    tol = PROBE_DEPTH * U24 * xv * (np.abs(sd) * (m + q) + np.abs(bd - m * sd))
    return want.T, tol.T, (xv * np.abs(sd)).T


def ratio(got, exact, mag, n, extra=0.0, dt=None):
    """largest error / bound of a plain comparison (the figure the GPU tests print); dt: the stored 16-bit point's half ulp joins the
    bound as in ref_decode.check_plain, None: f32 outputs"""
    acc = n * U24 * mag + extra
    tol = acc if dt is None else 0.5 * rd.ulp16(np.abs(exact) + acc, dt) + acc
    return float((np.abs(got - exact) / np.maximum(tol, 1e-300)).max())


def check_f32(got, exact, mag, n, extra=0.0):
    """EPI_F32: the unrounded row sums within n u M_r"""
    tol = n * U24 * mag + extra
    bad = np.nonzero(np.abs(got - exact) > tol)[0]
    assert bad.size == 0, f"{bad.size} f32 rows off, e.g. row {bad[0]}: got {got[bad[0]]} exact {exact[bad[0]]} tol {tol[bad[0]]}"


# ---- a plain float32 emulation of the VALU kernel's lane order (tests/test_qdecode_ref.py holds the bound against it) ----

def emulate_valu(q, s, b, group, x, bits, dt, code_bump=None, scale_shift_chunk=None, drop_fold=False):
    """f32 row sums in the kernel's order: per lane chunk a sequential f32 sum of the products x (m + q), a sequential f32 chunk sum of
    x, the two fmas per chunk (an fma = the float64 expression rounded once to f32: the operands' product is exact in float64), lanes
    summed by a 6-level tree.  Deliberately wrong variants: code_bump = (row, column): that code + 1 (- 1 at the maximum);
    scale_shift_chunk = (row, chunk): that chunk takes the next group's scale (the previous at the row's end); drop_fold: b' = b."""
    N, K = q.shape
    m = np.float32(magic(bits, dt))
    e = epl(bits, K, group)
    st = steps(bits, K, group)
    nch = K // e
    qf = q.astype(np.float32)
    if code_bump is not None:
        r, k = code_bump
        qf[r, k] += -1.0 if qf[r, k] == (1 << bits) - 1 else 1.0
    x32 = np.asarray(x, np.float32)
    gi = (np.arange(nch) * e) // group
    sc, bc = s[:, gi].astype(np.float32), b[:, gi].astype(np.float32)           # [N, nch]
    if scale_shift_chunk is not None:
        r, c = scale_shift_chunk
        g2 = gi[c] + 1 if gi[c] + 1 < s.shape[1] else gi[c] - 1
        sc = sc.copy()
        sc[r, c] = s[r, g2]
    xc = x32.reshape(nch, e)
    d = np.zeros((N, nch), np.float32)
    xs = np.zeros(nch, np.float32)
    qc = qf.reshape(N, nch, e)
    for j in range(e):
        d = (d + (xc[None, :, j] * (m + qc[:, :, j])).astype(np.float32)).astype(np.float32)   # products exact in f32 (8 x 8 bits)
        xs = (xs + xc[:, j]).astype(np.float32)
    fold = bc if drop_fold else (bc.astype(np.float64) - np.float64(m) * sc).astype(np.float32)
    acc = np.zeros((N, 64), np.float32)
    pad = st * 64 - nch
    dz, sz, fz, xz = (np.pad(a, ((0, 0), (0, pad))) for a in (d, sc, fold, np.broadcast_to(xs, (N, nch))))
    for t in range(st):
        sl = slice(t * 64, t * 64 + 64)
        acc = (sz[:, sl].astype(np.float64) * dz[:, sl] + acc).astype(np.float32)
        acc = (fz[:, sl].astype(np.float64) * xz[:, sl] + acc).astype(np.float32)
    w = 64
    while w > 1:
        w //= 2
        acc = (acc[:, :w] + acc[:, w:2 * w]).astype(np.float32)
    return acc[:, 0].astype(np.float64)
