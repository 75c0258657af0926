"""CPU-only: the references and bound checkers of oracle/ref_decode.py (used by the GPU tests of the bf16 / float16 decode GEMV and the
step attention) accept a correct kernel's output and reject each plausible wrong kernel -- simulated on the host.  This is the
evidence that the GPU tests would catch a subtle bug."""
import numpy as np
import pytest

from oracle import ref_decode as rd

EPS = 1e-6
f32 = np.float32


def rejects(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def gemv_inputs(dt, N, K, seed):
    rng = np.random.default_rng(seed)
    W = rd.rand16(rng, (N, K), dt, -6, -2)
    x = rd.rand16(rng, (K,), dt, -2, 1)
    nw = rd.rand16(rng, (K,), dt, -1, 0)
    return rng, W, x, nw


def acc32(W, x):
    """an f32 accumulation of W . x (a valid kernel's pre-rounding value)"""
    return (W.astype(f32) @ np.asarray(x, f32)).astype(np.float64)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [4096, 12288, 1000])
def test_plain_store_mutants(dt, K):
    N = 512
    rng, W, x, _ = gemv_inputs(dt, N, K, K)
    exact, mag = rd.rows_dot(W, x)
    n = rd.gemv_acc_depth(K)
    good = rd.rnd(acc32(W, x), dt)
    rd.check_plain(good, exact, mag, n, 0.0, dt)
    # one 8-element vector dropped: at the tail, and at a K-split wave boundary (the first vector of wave 1's quarter)
    tail = x.copy()
    tail[K - 8:] = 0
    rejects(rd.check_plain, rd.rnd(acc32(W, tail), dt), exact, mag, n, 0.0, dt)
    if K == 12288:
        wb = x.copy()
        wb[3072:3080] = 0
        rejects(rd.check_plain, rd.rnd(acc32(W, wb), dt), exact, mag, n, 0.0, dt)
    # the neighbouring row at every row-group boundary (rows 8 g + 7 -> 8 g + 8) and at the member boundaries of a 300 | 100 | 112 stack
    for rows in (np.arange(7, N - 1, 8), np.array([299, 399])):
        bad = good.copy()
        bad[rows] = rd.rnd(acc32(W[rows + 1], x), dt)
        rejects(rd.check_plain, bad, exact, mag, n, 0.0, dt)
    # outputs that are not exact 16-bit values
    rejects(rd.check_plain, acc32(W, x), exact, mag, n, 0.0, dt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_bias_after_rounding_rejected(dt):
    N, K = 2048, 2048
    rng, W, x, _ = gemv_inputs(dt, N, K, 11)
    n = rd.gemv_acc_depth(K)
    a = acc32(W, x)
    b = rd.rand16(rng, (N,), dt, -4, 0)
    exact, mag = rd.rows_dot(W, x)
    exact = exact + b
    rd.check_plain(rd.rnd(a + b, dt), exact, mag, n, 0.0, dt)
    rejects(rd.check_plain, rd.rnd(rd.rnd(a, dt) + b, dt), exact, mag, n, 0.0, dt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [4096, 1000])
def test_rmsnorm_prologue_mutants(dt, K):
    N = 1024
    rng, W, x, nw = gemv_inputs(dt, N, K, 3 * K)
    n = rd.gemv_acc_depth(K)
    xin, slack = rd.norm_slack(W, x, nw, EPS, dt)
    exact, mag = rd.rows_dot(W, xin)
    # the kernel's prologue as the host computes it in f32 (an rstd within a few f32 ulp of the exact one) passes
    good = rd.rnd(acc32(W, rd.rmsnorm16(x, nw, EPS, dt)), dt)
    rd.check_plain(good, exact, mag, n, slack, dt)
    # rstd over K - 8 elements
    x32, w32 = x.astype(f32), nw.astype(f32)
    ss = f32(np.sum(x32[:K - 8].astype(np.float64) ** 2))
    rstd = f32(1) / np.sqrt(ss / f32(K) + f32(EPS))
    rejects(rd.check_plain, rd.rnd(acc32(W, rd.rnd((x32 * rstd) * w32, dt)), dt), exact, mag, n, slack, dt)
    # the norm weight shifted by one element
    rejects(rd.check_plain, rd.rnd(acc32(W, rd.rmsnorm16(x, np.roll(nw, -1), EPS, dt)), dt), exact, mag, n, slack, dt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("single_round", [0, 1])
def test_swiglu_rounding_count_mutants(dt, single_round):
    N, K = 2048, 4096
    rng, W, x, _ = gemv_inputs(dt, N, K, 40 + single_round)
    U = rd.rand16(rng, (N, K), dt, -6, -2)
    n = rd.gemv_acc_depth(K)
    eg, mg = rd.rows_dot(W, x)
    eu, mu = rd.rows_dot(U, x)
    g, u = f32(rd.rnd(acc32(W, x), dt)), f32(rd.rnd(acc32(U, x), dt))
    one = rd.rnd(g / (f32(1) + np.exp(-g)) * u, dt)
    three = rd.rnd(f32(rd.rnd(g * f32(rd.rnd(f32(1) / (f32(1) + np.exp(-g)), dt)), dt)) * u, dt)
    good, bad = (one, three) if single_round else (three, one)
    rd.check_swiglu(good, eg, mg, eu, mu, n, dt, single_round)
    rejects(rd.check_swiglu, bad, eg, mg, eu, mu, n, dt, single_round)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("single_round", [0, 1])
def test_swiglu_gate_beyond_f32_range(dt, single_round):
    """gate far below -87: expf(-g) overflows in f32 and the kernel's sigmoid is 0, its output -0.0 where the exact one is ~ -1e-36
    -- accepted; a wrong sign or a value of normal size is not"""
    g = np.array([-90.5, -88.0, -86.0, -20.0], f32)
    u = np.array([35.5, -3.0, 2.0, 1.5], f32)
    with np.errstate(over="ignore"):
        sig = f32(1) / (f32(1) + np.exp(-g))
        out = rd.rnd(g / (f32(1) + np.exp(-g)) * u, dt) if single_round else rd.rnd(f32(rd.rnd(g * f32(rd.rnd(sig, dt)), dt)) * u, dt)
    z = np.zeros(4)
    rd.check_swiglu(out, g.astype(np.float64), z, u.astype(np.float64), z, 1, dt, single_round)
    bad = out.copy()
    bad[0] = rd.rnd(np.array([1e-30]), dt)[0] if dt == "bf16" else 0.5
    rejects(rd.check_swiglu, bad, g.astype(np.float64), z, u.astype(np.float64), z, 1, dt, single_round)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_residual_mutants(dt):
    N, K = 2048, 4096
    rng, W, x, _ = gemv_inputs(dt, N, K, 77)
    r = rd.rand16(rng, (N,), dt, -3, 1)
    n = rd.gemv_acc_depth(K)
    a = acc32(W, x)
    exact, mag = rd.rows_dot(W, x)
    rd.check_residual(rd.rnd(f32(r) + f32(rd.rnd(a, dt)), dt), r, exact, mag, n, dt)
    # the product left unrounded: one rounding where the kernel does two
    rejects(rd.check_residual, rd.rnd(r + a, dt), r, exact, mag, n, dt)


def test_fold_rounded_twice_rejected():
    """x := bf16(x + bf16(p_0 + p_1 + p_2)) (x_out bit for bit): rounding each slot's partial before the sum is caught"""
    rng = np.random.default_rng(5)
    K = 4096
    x = rd.rand16(rng, (K,), "bf16", -2, 1)
    p = (rng.standard_normal((3, K)) * 0.5).astype(f32)
    good = rd.rnd(x + f32(rd.rnd((p[0] + p[1]) + p[2], "bf16")), "bf16")
    twice = rd.rnd(x + f32(rd.rnd(f32(rd.rnd(p[0], "bf16")) + f32(rd.rnd(p[1], "bf16")) + f32(rd.rnd(p[2], "bf16")), "bf16")), "bf16")
    assert not np.array_equal(good, twice)


def test_argmax_tie_mutant():
    logits = rd.rnd(np.array([0.5, 3.0, -1.0, 3.0, 2.0, 3.0]), "bf16")
    rd.check_argmax(logits, 1)
    rd.check_argmax(logits, 1 + 640, row_offset=640)
    rejects(rd.check_argmax, logits, 5)             # the highest index of the tie
    rejects(rd.check_argmax, logits, 1, row_offset=640)
    # the kernel's keys: orderable logit << 32 | ~row, the largest wins -> the lowest row of a tie
    keys = []
    for r, v in enumerate(logits):
        u = int(np.float32(v).view(np.uint32))
        u = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
        keys.append((u << 32) | (~r & 0xFFFFFFFF))
    assert rd.argmax_from_keys(np.array(keys, np.uint64), len(keys)) == 1


# ---- step attention ----

def attn_setup(dt, pos=40, H=4, Hkv=2, D=64, cap=64, seed=9):
    rng = np.random.default_rng(seed)
    qkv = rd.rand16(rng, ((H + 2 * Hkv) * D,), dt, -3, 1)
    qn, kn = rd.rand16(rng, (D,), dt, -1, 0), rd.rand16(rng, (D,), dt, -1, 0)
    K = rd.rand16(rng, (Hkv, cap, D), dt, -2, 0)
    V = rd.rand16(rng, (Hkv, cap, D), dt, -2, 0)
    return dict(qkv=qkv, qn=qn, kn=kn, K=K, V=V, pos=pos, H=H, Hkv=Hkv, D=D)


def sim_attn(s, chunk, dt, rope_pos=None, drop_split=None, drop_appended=False, rescale=True):
    """a host split-KV kernel: q/k modelled at rope_pos, per-split (m, l, o) in f32, merged with or without exp(m_j - M)"""
    H, Hkv, D, pos = s["H"], s["Hkv"], s["D"], s["pos"]
    rope = rd.rope_cur(pos if rope_pos is None else rope_pos, D)
    q, _ = rd.norm_rope_candidates(s["qkv"][:H * D].reshape(H, D), s["qn"], EPS, rope, dt)
    k, _ = rd.norm_rope_candidates(s["qkv"][H * D:(H + Hkv) * D].reshape(Hkv, D), s["kn"], EPS, rope, dt)
    v = s["qkv"][(H + Hkv) * D:].reshape(Hkv, D)
    Kx, Vx = s["K"].astype(f32).copy(), s["V"].astype(f32).copy()
    Kx[:, pos], Vx[:, pos] = k, v
    out = np.empty((H, D))
    for h in range(H):
        kv = h // (H // Hkv)
        parts = []
        for j in range(-(-(pos + 1) // chunk)):
            toks = [t for t in range(j * chunk, min(pos + 1, (j + 1) * chunk)) if not (drop_appended and t == pos)]
            if j == drop_split or not toks:
                continue
            sc = (Kx[kv, toks] @ f32(q[h])) * f32(D ** -0.5)
            m = sc.max()
            p = np.exp(sc - m)
            parts.append((m, p.sum(), p @ Vx[kv, toks]))
        M = max(m for m, _, _ in parts)
        f = [np.exp(f32(m - M)) if rescale else f32(1) for m, _, _ in parts]
        out[h] = sum(fj * o for fj, (_, _, o) in zip(f, parts)) / sum(fj * l for fj, (_, l, _) in zip(f, parts))
    return rd.rnd(out, dt), Kx[:, pos]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_attention_mutants(dt):
    s = attn_setup(dt)
    chunk = 8
    nsplit = -(-(s["pos"] + 1) // chunk)
    args = (s["qkv"], s["K"], s["V"], s["pos"], s["H"], s["Hkv"], s["D"], s["qn"], s["kn"], rd.rope_cur(s["pos"], s["D"]), EPS,
            s["D"] ** -0.5, dt, chunk, nsplit)
    ref, bound, k_c, _ = rd.attn_step_ref(*args)
    good, krow = sim_attn(s, chunk, dt)
    rd.check_attn(good, ref, bound, dt)
    rd.check_row(krow, k_c, "K row")
    rejects(rd.check_attn, sim_attn(s, chunk, dt, drop_split=2)[0], ref, bound, dt)          # one split dropped
    rejects(rd.check_attn, sim_attn(s, chunk, dt, drop_appended=True)[0], ref, bound, dt)    # the appended row left out
    rejects(rd.check_attn, sim_attn(s, chunk, dt, rescale=False)[0], ref, bound, dt)         # merge without the rescale
    bad_out, bad_k = sim_attn(s, chunk, dt, rope_pos=s["pos"] - 1)                           # RoPE at pos - 1
    rejects(rd.check_row, bad_k, k_c, "K row")
    rejects(rd.check_attn, bad_out, ref, bound, dt)
