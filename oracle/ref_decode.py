"""Float64 references and derived error bounds of the two decode-step kernel families, in bfloat16 ("bf16") and float16 ("f16"):
the dense GEMV forms (csrc/gemv.hip) and the step attention (csrc/attn_step.hip).  The references model the kernels' rounding
points as their comments state them; every bound is derived below, none is fitted.  u = 2^-24 is the f32 unit roundoff."""
import numpy as np

from . import ref_core as rc

U24 = 2.0 ** -24


def rnd(v, dt):
    """f32 value rounded to the 16-bit grid (RNE), as float64 -- the kernels round f32 results, so the model goes through f32"""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    if dt == "bf16":
        return rc.bf16_round(v32).astype(np.float64)
    return v32.astype(np.float16).astype(np.float64)


def ulp16(v, dt="f16"):
    """ulp of the 16-bit grid at |v| (float16: subnormal spacing 2^-24 below 2^-14)"""
    a = np.abs(np.asarray(v, np.float64))
    if dt == "f16":
        return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -14))) - 10)
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 7)


def rand16(rng, shape, dt, lo, hi):
    """float32 values exact in dt with random sign and mantissa, binary exponent in [lo, hi] (|v| in [2^lo, 2^(hi+1)))"""
    u = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16).astype(np.uint32)
    mb, bias = (7, 127) if dt == "bf16" else (10, 15)
    e = (lo + bias + (u >> np.uint32(mb)) % np.uint32(hi - lo + 1)).astype(np.uint32)
    bits = (u & np.uint32(0x8000 | ((1 << mb) - 1))) | (e << np.uint32(mb))
    if dt == "bf16":
        return (bits << np.uint32(16)).view(np.float32)
    return bits.astype(np.uint16).view(np.float16).astype(np.float32)


def rows_dot(W, x, chunk=8192):
    """exact W @ x (float64) and sum |W| |x| per row, chunked (the vocabulary-sized matrix does not fit in float64 at once)"""
    xd, xa = np.asarray(x).astype(np.float64), np.abs(np.asarray(x).astype(np.float64))
    out, mag = np.empty(W.shape[0]), np.empty(W.shape[0])
    for r in range(0, W.shape[0], chunk):
        Wd = W[r:r + chunk].astype(np.float64)
        out[r:r + chunk] = Wd @ xd
        mag[r:r + chunk] = np.abs(Wd) @ xa
    return out, mag


def rmsnorm16(x, nw, eps, dt="f16"):
    """the GEMV prologue as the host computes it in f32: ss, rstd = 1/sqrt(ss/K + eps), xn = dt((x * rstd) * w)"""
    x32, w32 = np.asarray(x, np.float32), np.asarray(nw, np.float32)
    ss = np.float32(np.sum(x32.astype(np.float64) ** 2))
    rstd = np.float32(1.0) / np.sqrt(ss / np.float32(x32.size) + np.float32(eps))
    return rnd((x32 * rstd) * w32, dt)


def flip_slack(W, xn, dt="f16"):
    """RMSNorm output rounding may flip a few roundings of xn against the host's f32 rstd: 4 flips of the widest ulp, per row"""
    return 4.0 * ulp16(np.abs(np.asarray(xn, np.float64)).max(), dt) * np.abs(W.astype(np.float32)).max(axis=1)


def norm_eps(depth):
    """relative error of the kernel's f32 x * rstd * w against the exact value: the sum of squares is a chain of `depth` f32
    roundings of positive terms (<= depth u), the square root halves it; ss / K, + eps, sqrt and the division are one correctly
    rounded operation each (hipcc's default) and (x * rstd) * w two more: (depth / 2 + 6) u, taken as (depth / 2 + 8) u"""
    return (depth / 2.0 + 8.0) * U24


def norm_candidates(x, nw, eps, dt, depth):
    """RMSNorm output rounded to dt: (mid, lo, hi).  mid = dt(exact); the kernel's element is lo or hi, the two roundings of the
    exact value moved by the relative error norm_eps(depth) (equal unless the value sits that close to a rounding midpoint)"""
    x64, w64 = np.asarray(x, np.float64), np.asarray(nw, np.float64)
    rstd = 1.0 / np.sqrt(np.mean(x64 * x64, axis=-1, keepdims=True) + np.float64(np.float32(eps)))
    t = x64 * rstd * w64
    e = norm_eps(depth)
    a, b = rnd(t * (1 - e), dt), rnd(t * (1 + e), dt)
    return rnd(t, dt), np.minimum(a, b), np.maximum(a, b)


def gemv_norm_depth(K):
    """longest f32 chain of the GEMV prologue's sum of squares: 8 fmas per 2048 columns a thread stages, a 6-level wave sum and the
    4-wave block sum (+ 6 spare levels)"""
    return 8 * ((K + 2047) // 2048) + 16


def rows_norm_depth(K):
    """longest f32 chain of the few-row kernel's in-launch RMSNorm (gemv_rows.hip, K <= 4096): one wave per activation row, lane l
    runs `s += lo * lo; s += hi * hi` (the squares of bf16 values are exact in f32: one rounding per add) over the 8 elements of each of
    its vectors l, l + 64, ... -- ceil(K / 512) vectors that are not staged zeros -- then the 6-level wave sum"""
    return 8 * ((K + 511) // 512) + 6


def norm_slack(W, x, nw, eps, dt):
    """(xn, slack per row): xn = dt(exact RMSNorm); the kernel's W . xn' differs from W . xn by at most sum_k |hi_k - lo_k| |W_rk| --
    only the elements whose rounding can flip (norm_candidates) contribute"""
    mid, lo, hi = norm_candidates(x, nw, eps, dt, gemv_norm_depth(np.asarray(x).size))
    d = hi - lo
    idx = np.nonzero(d)[0]
    slack = np.abs(W[:, idx].astype(np.float64)) @ d[idx] if idx.size else np.zeros(W.shape[0])
    return mid, slack


def gemv_acc_depth(K):
    """longest chain of f32 roundings in a GEMV row's accumulation: a lane's fma chain over its 16-byte vectors (at most
    8 ceil(K / 512) products in every kernel: K / 64 per lane, a quarter of that per wave when the K is split), the 6-level wave sum
    and the 4-part sum of a K split (+ 6 spare).
    The few-row kernel (gemv_rows.hip) is covered too, read off its loop: per 4096-column chunk a lane owns vectors lane, lane + 64, ...
    of the chunk's nv <= 512 -- 8 of a whole chunk, ceil(nv / 64) of the last; the others meet a staged zero row of x and add an exact
    0 -- ceil(K / 512) vectors in all, chunk after chunk in ONE accumulator, 8 products each through four v_dot2c_f32_bf16 (two exact
    products and the accumulator per instruction: at most one rounding per product), then the 6-level wave sum and the bias add:
    8 ceil(K / 512) + 7"""
    return 8 * ((K + 511) // 512) + 16


def check_exact16(got, dt):
    assert np.array_equal(got, rnd(got, dt)), f"outputs must be exact {dt} values"


def check_plain(got, exact, mag, n, extra=0.0, dt="f16"):
    """|got - dt(exact)| <= 1/2 ulp of the stored point + the f32 accumulation bound n 2^-24 sum|x w| (+ the prologue's rounding
    flips): the products are exact in f32 and summed in chains of at most n roundings (gamma_n ~ n u; n = K always holds,
    gemv_acc_depth(K) is the kernels' chain), then rounded once to dt"""
    acc = n * U24 * mag + extra
    err = np.abs(got - exact)
    tol = 0.5 * ulp16(np.abs(exact) + acc, dt) + acc
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, f"{bad.size} rows off, e.g. row {bad[0]}: got {got[bad[0]]} exact {exact[bad[0]]} tol {tol[bad[0]]}"
    check_exact16(got, dt)


def stored_candidates(exact, err, dt):
    """the two dt values an f32 accumulation within `err` of `exact` can round to (equal away from rounding midpoints)"""
    a, b = rnd(exact - err, dt), rnd(exact + err, dt)
    return np.minimum(a, b), np.maximum(a, b)


def check_residual(got, resid, exact, mag, n, dt, extra=0.0, relu=False):
    """EPI_RESIDUAL: out = dt(r + dt(acc)).  dt(acc) lies in [lo, hi], the stored candidates of an accumulation within
    n u sum|x w| (+ extra) of the exact value, and y -> dt(r + y) (one f32 add of two dt values, one rounding) is monotone: got must
    lie in [dt(r + lo), dt(r + hi)] -- a single value away from rounding midpoints.  relu: max(acc, 0) before the rounding (exact and
    monotone, it commutes with the rounding: the candidates are clamped)"""
    lo, hi = stored_candidates(exact, n * U24 * mag + extra, dt)
    if relu:
        lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    r32 = np.asarray(resid, np.float32)
    c_lo, c_hi = rnd(r32 + lo.astype(np.float32), dt), rnd(r32 + hi.astype(np.float32), dt)
    bad = np.nonzero((got < c_lo) | (got > c_hi))[0]
    assert bad.size == 0, f"{bad.size} residual rows off, e.g. {bad[0]}: got {got[bad[0]]} want {c_lo[bad[0]]} .. {c_hi[bad[0]]}"
    check_exact16(got, dt)


def check_gate(got, resid, gate, exact, mag, n, dt, extra=0.0, relu=False):
    """the gated residual of the GEMM epilogues: out = dt(r + acc * g), g per output column, no rounding in between.  acc lies within
    E = n u sum|x w| (+ extra) of the exact value (clamped at 0 under relu: exact and monotone), so acc * g lies between the products
    of the interval ends with g; the f32 product and the f32 add are one rounding each, relative u of |acc g| and of |r + acc g|: the
    f32 sum lies in [r + p_lo - e, r + p_hi + e] with e = 4 u (|r| + max|p|) (2 u needed), and got must lie between the roundings of
    the two ends (stored_candidates' argument, the rounding being monotone) -- a single value away from rounding midpoints"""
    E = n * U24 * mag + extra
    a, b = exact - E, exact + E
    if relu:
        a, b = np.maximum(a, 0.0), np.maximum(b, 0.0)
    g, r = np.asarray(gate, np.float64), np.asarray(resid, np.float64)
    p_lo, p_hi = np.minimum(a * g, b * g), np.maximum(a * g, b * g)
    e = 4 * U24 * (np.abs(r) + np.maximum(np.abs(p_lo), np.abs(p_hi)))
    c_lo, c_hi = rnd(r + p_lo - e, dt), rnd(r + p_hi + e, dt)
    bad = np.nonzero((got < c_lo) | (got > c_hi))[0]
    assert bad.size == 0, f"{bad.size} gated rows off, e.g. {bad[0]}: got {got[bad[0]]} want {c_lo[bad[0]]} .. {c_hi[bad[0]]}"
    check_exact16(got, dt)


def act_mode_single_round(act_mode):
    """GemmSegs.act_mode (gemm.hpp) -> check_swiglu's single_round.  act_mode 0 (fused_swiglu): dt(g / (1 + expf(-g)) * u) on the
    rounded g and u, one rounding -- single_round.  act_mode 1 (nn::silu(gate) * up, every primitive rounded): g = dt(acc_gate),
    u = dt(acc_up), s = dt(1 / (1 + expf(-g))), dt(dt(g s) u) -- the four rounded values (gate, sigmoid, silu, up) are exactly
    check_swiglu's "three roundings" form, whose g and u are already stored candidates: the sigmoid, the silu and the output."""
    assert act_mode in (0, 1)
    return 1 if act_mode == 0 else 0


def check_swiglu(got, exact_g, mag_g, exact_u, mag_u, n, dt, single_round, extra_g=0.0, extra_u=0.0):
    """EPI_SWIGLU on g = dt(acc_gate), u = dt(acc_up) (each one of its stored candidates, chains of n roundings):
    single_round: dt(g * sigmoid(g) * u) in f32 -- expf (a few ulp), the add, the division and the product keep the f32 value
    within 16 u of the exact one, so the output is one of the two roundings of that interval;
    three roundings: dt(dt(g * dt(sigmoid(g))) * u) -- the sigmoid rounding likewise within 16 u, the two products of dt values
    are exact in f32.  got must be one of the candidate outputs.
    f32 range: where sigmoid(g) < 2^-125 (g < -86.6) the relative bounds do not hold -- expf(-g) overflows to inf beyond 88.72 and
    the quotient goes subnormal or to 0 -- so the f32 sigmoid is anywhere in [0, 2^-125] and the output anywhere between 0 and
    |g u| 2^-124 with the sign of g u."""
    gl, gh = stored_candidates(exact_g, n * U24 * mag_g + extra_g, dt)
    ul, uh = stored_candidates(exact_u, n * U24 * mag_u + extra_u, dt)
    e = 16 * U24
    ok = np.zeros(got.shape, bool)
    # (lo, dt(exact), hi) are every value in between while an interval spans at most three grid points
    for g in (gl, rnd(exact_g, dt), gh):
        sig = 1.0 / (1.0 + np.exp(-g))
        for u in (ul, rnd(exact_u, dt), uh):
            if single_round:
                y = g * sig * u
                cands = [rnd(y * (1 - e), dt), rnd(y * (1 + e), dt)]
            else:
                cands = [rnd(rnd(g * s, dt) * u, dt) for s in (rnd(sig * (1 - e), dt), rnd(sig * (1 + e), dt))]
            for c in cands:
                ok |= got == c
    # a wider interval (the grid finer than the accumulation bound): silu(g) u is linear in u and, in g, monotone on each side of
    # silu's minimum at g* = -1.2785, so the output lies between its values at the interval ends (and at g* when inside), moved by
    # the roundings (1 or 3 half ulps) and e
    wide = (gh - gl > 2 * ulp16(np.maximum(np.abs(gl), np.abs(gh)), dt)) | (uh - ul > 2 * ulp16(np.maximum(np.abs(ul), np.abs(uh)), dt))
    if wide.any():
        gs = np.clip(-1.2785, gl, gh)
        c = np.stack([g / (1.0 + np.exp(-g)) * u for g in (gl, rnd(exact_g, dt), gs, gh) for u in (ul, uh)])
        half = 2.0 ** -8 if dt == "bf16" else 2.0 ** -11
        slack = ((1 if single_round else 3) * half + e) * np.abs(c).max(0)
        ok |= wide & (got >= c.min(0) - slack) & (got <= c.max(0) + slack)
    tiny = 1.0 / (1.0 + np.exp(-gh)) < 2.0 ** -125
    if tiny.any():
        lim = np.abs(gl) * np.maximum(np.abs(ul), np.abs(uh)) * 2.0 ** -124
        ok |= tiny & (np.abs(got) <= lim) & (got * np.sign(exact_g * exact_u) >= 0)
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, f"{bad.size} SwiGLU rows off, e.g. {bad[0]}: got {got[bad[0]]} gate {exact_g[bad[0]]} up {exact_u[bad[0]]}"
    check_exact16(got, dt)


def argmax_from_keys(keys, n_blocks):
    """the row the kernel's per-block partial keys (orderable logit << 32 | ~row) select: the largest key"""
    best = int(np.asarray(keys, np.uint64)[:n_blocks].max())
    return (~best) & 0xFFFFFFFF


def check_argmax(got_logits, row, row_offset=0):
    """greedy argmax over the stored logits: the LOWEST index of the maximum, plus the shard's row offset"""
    want = int(np.argmax(got_logits)) + row_offset
    assert row == want, f"argmax row {row}, want {want} (lowest index of the maximum {got_logits.max()})"


# ---- step attention (attn_step.hip) ----

def rope_cur(pos, D, theta=1e6):
    """cos | sin of position `pos` as f32 (the engine's rope_cur row): angle pos * theta^(-2i/D), i < D/2"""
    i = np.arange(D // 2, dtype=np.float64)
    ang = pos * theta ** (-2.0 * i / D)
    return np.concatenate([np.cos(ang), np.sin(ang)]).astype(np.float32)


def norm_rope_candidates(rows, nw, eps, rope, dt):
    """the kernel's q/k row: dt(rope(dt(rmsnorm(x))))) per head row ([n, D]).  Returns (mid, cands [4, n, D]): mid from the exact
    norm; the kernel's element must be one of the 4 candidates (the element's and its partner's norm rounding flips, norm_candidates
    with a depth of 8 fmas + a 4-level lane sum + 4 spare).  Without a norm (nw None) x goes to RoPE as it is: one candidate."""
    rows = np.asarray(rows, np.float64)
    n, D = rows.shape
    h = D // 2
    cs, sn = rope[:h].astype(np.float32), rope[h:].astype(np.float32)
    if nw is None:
        mid = lo = hi = rows
    else:
        mid, lo, hi = norm_candidates(rows, nw, eps, dt, 16)

    def cand(own, partner):   # first half: own cs - partner sn; second half: partner sn + own cs (f32, no contraction)
        y1 = own[:, :h].astype(np.float32) * cs - partner[:, h:].astype(np.float32) * sn
        y2 = partner[:, :h].astype(np.float32) * sn + own[:, h:].astype(np.float32) * cs
        return rnd(np.concatenate([y1, y2], axis=1), dt)

    m = cand(mid, mid)
    cands = np.stack([cand(a, b) for a in (lo, hi) for b in (lo, hi)])
    return m, cands


def check_row(got, cands, what):
    ok = np.any(np.asarray(got, np.float64)[None] == cands, axis=0)
    bad = np.argwhere(~ok)
    assert bad.size == 0, f"{what}: {len(bad)} elements off, e.g. {tuple(bad[0])}: got {got[tuple(bad[0])]}"


def attn_step_ref(qkv, Kslab, Vslab, pos, H, Hkv, D, q_nw, k_nw, rope, eps, scale, dt, chunk, nsplit, skip=()):
    """float64 attention of query heads (modelled q) over slab rows [0, pos] with row pos = the modelled k row and v_raw.
    Returns (out [H, D], bound [H, D], k_cands [4, Hkv, D], k_mid [Hkv, D]).  `skip`: token indices left out (for mutants).

    Bound, per output element: 1/2 ulp of the stored point + E, E = A * rel with A = sum_t w_t |v_t| (w the exact softmax weights):
      * scores: |s' - s| <= eps_s = scale (D u sum|q k| + sum dq |k| + [t = pos] sum |q| dk + sum dq dk) + 2 u |s|  (an f32 dot over
        D products, the q / k rounding flips dq / dk of norm_rope_candidates, the f32 scale and its multiply); perturbed scores move each
        normalised weight by a factor within exp(+-2 eps_s);
      * exp and rescales: every exp argument is an f32 difference (one rounding, relative u |arg|) that __expf multiplies by
        log2(e) (another), and __expf is accurate to 2 u; along a token's chain the arguments telescope to |s_t - M| <= S (the live
        score range) over at most R + 3 exp calls (R rounds of a lane, the wave merge, the split merge): weights move within
        exp(+-2 (2 u S + 3 (R + 3) u));
      * sums: o and l are f32 chains of at most 4 R (a rescale and 3 fmas per round) + TPW + 8 + nsplit + 8 roundings each:
        2 (that) u relative; the division u.
    """
    G = H // Hkv
    TPW = 64 // (D // 8)
    R = -(-chunk // (TPW * 8 * 3)) + 1
    q_raw = np.asarray(qkv[:H * D], np.float64).reshape(H, D)
    k_raw = np.asarray(qkv[H * D:(H + Hkv) * D], np.float64).reshape(Hkv, D)
    v_raw = np.asarray(qkv[(H + Hkv) * D:], np.float64).reshape(Hkv, D)
    q_mid, q_c = norm_rope_candidates(q_raw, q_nw, eps, rope, dt)
    k_mid, k_c = norm_rope_candidates(k_raw, k_nw, eps, rope, dt)
    dq = q_c.max(0) - q_c.min(0)
    dk = k_c.max(0) - k_c.min(0)
    Tk = pos + 1
    live = np.array([t for t in range(Tk) if t not in set(skip)])
    out, bound = np.empty((H, D)), np.empty((H, D))
    for h in range(H):
        kv = h // G
        Kt = np.asarray(Kslab[kv, :Tk], np.float64).copy()
        Vt = np.asarray(Vslab[kv, :Tk], np.float64).copy()
        Kt[pos], Vt[pos] = k_mid[kv], v_raw[kv]
        Kt, Vt = Kt[live], Vt[live]
        q = q_mid[h]
        s = scale * (Kt @ q)
        dkt = np.zeros_like(Kt)
        if pos in set(live.tolist()):
            dkt[live == pos] = dk[kv]
        eps_s = scale * (D * U24 * (np.abs(Kt) @ np.abs(q)) + np.abs(Kt) @ dq[h] + dkt @ np.abs(q) + dkt @ dq[h]) + 2 * U24 * np.abs(s)
        M = s.max()
        p = np.exp(s - M)
        w = p / p.sum()
        o = w @ Vt
        A = w @ np.abs(Vt)
        S = M - s.min()
        rel = np.expm1(2 * eps_s.max() + 2 * (2 * U24 * S + 3 * (R + 3) * U24)) + 2 * (4 * R + TPW + nsplit + 16) * U24 + U24
        E = A * rel
        out[h] = o
        bound[h] = 0.5 * ulp16(np.abs(o) + E, dt) + E
    return out, bound, k_c, k_mid


def check_attn(got, ref, bound, dt):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"attention: {len(bad)} elements off, e.g. head/dim {tuple(bad[0])}: got {got[tuple(bad[0])]} "
                           f"ref {ref[tuple(bad[0])]} bound {bound[tuple(bad[0])]}")
    check_exact16(np.asarray(got, np.float64), dt)
