"""CPU-only: the float64 checks of the few-row bf16 Linear (oracle/ref_gemv_rows.py, used by tests/test_gpu_gemv_rows.py on the
kernel's output) accept a correct kernel and reject each plausible wrong one, on the GPU tests' own inputs (same seeds).  The correct
kernel is a host emulation of csrc/gemv_rows.hip: f32 accumulation in the kernel's order (per 4096-column chunk, lane l takes vectors
l, l + 64, ..., eight products each, one accumulator across the chunks, then a 6-level sum over the lanes), its RMSNorm and its
epilogues in f32.  Every case of M rows is the first M of the same 8 rows, so a mutant that is rejected on row 0 is rejected in every
parametrised case of the GPU test; each test prints how many of the 8 rows reject it (the mutant table, `pytest -s`)."""
import numpy as np
import pytest

from oracle import ref_decode as rd
from oracle import ref_gemv_rows as rg

f32 = np.float32
BF = rg.BF


def bf(v):
    return f32(rd.rnd(v, BF))


def emu_acc(W, X):
    """[M, N] f32: sum_k x[t, k] w[n, k] in the kernel's order"""
    (M, K), N = X.shape, W.shape[0]
    acc = np.zeros((M, N, 64), f32)
    lane = np.arange(64)
    for k0 in range(0, K, 4096):
        nv = min(512, (K - k0) // 8)
        for j in range(8):
            v = j * 64 + lane
            live = v < nv
            if not live.any():
                break
            for e in range(8):
                cols = k0 + np.minimum(v, nv - 1) * 8 + e
                xv = np.where(live, X[:, cols], f32(0))                     # [M, 64]: lanes past the row's end see a staged zero
                acc = acc + xv[:, None, :] * W[:, cols][None, :, :]         # the product of two bf16 values is exact in f32
    for s in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :s] + acc[..., s:2 * s]
    return acc[..., 0]


def emu_norm(X, nw, K_div=None):
    """the in-launch RMSNorm: per row, lane l squares its vectors' elements in order, the lanes are summed, y = bf16((x rstd) w)"""
    M, K = X.shape
    nv = K // 8
    s = np.zeros((M, 64), f32)
    lane = np.arange(64)
    for k in range(8):
        v = k * 64 + lane
        live = v < nv
        for e in range(8):
            xv = np.where(live, X[:, np.minimum(v, nv - 1) * 8 + e], f32(0))
            s = s + xv * xv
    for w in (32, 16, 8, 4, 2, 1):
        s = s[:, :w] + s[:, w:2 * w]
    rstd = f32(1) / np.sqrt(s / f32(K if K_div is None else K_div) + f32(rg.EPS))   # [M, 1]
    return bf((X * rstd) * nw[None, :].astype(f32))


def epi_plain(acc, c, M=8, round_before_resid=True):
    v = acc if c["bias"] is None else acc + c["bias"][None, :].astype(f32)
    if c["relu"]:
        v = np.maximum(v, f32(0))
    if c["gate"] is not None:
        v = c["resid"][:M].astype(f32) + v * c["gate"][None, :].astype(f32)
    elif c["resid"] is not None:
        v = c["resid"][:M].astype(f32) + (bf(v) if round_before_resid else v)
    return rd.rnd(v, BF)


def epi_act(acc_g, acc_u, act_mode):
    gt, up = bf(acc_g), bf(acc_u)
    with np.errstate(over="ignore"):   # a gate below -88.7: expf overflows, the sigmoid is 0 (check_swiglu's f32 range)
        den = f32(1) + np.exp(-gt)
    if act_mode == 1:
        return rd.rnd(bf(gt * bf(f32(1) / den)) * up, BF)
    return rd.rnd(gt / den * up, BF)


def rejected_rows(check, rows):
    """how many of the rows the check rejects; row 0 -- part of every case -- must be among them"""
    n = 0
    for t, row in enumerate(rows):
        try:
            check(t, row)
        except AssertionError:
            n += 1
        else:
            assert t != 0, "the mutant stays inside the bound on row 0"
    return n


def drop_tail(X):
    """the last 16-byte vector of K dropped"""
    Xd = X.copy()
    Xd[:, -8:] = 0
    return Xd


def mm32(W, X):
    """an f32 accumulation in another order (a valid kernel's value; the mutants are built on it)"""
    return X.astype(f32) @ W.astype(f32).T


@pytest.mark.parametrize("N,K,form", [(rg.PLAIN_N, K, f) for K in rg.PLAIN_KS for f in rg.PLAIN_FORMS] +
                         [(rg.WIDE_N, rg.WIDE_K, f) for f in rg.WIDE_FORMS])
def test_plain_cases(N, K, form):
    c = rg.plain_case(form, N, K)
    good = epi_plain(emu_acc(c["W"], c["X"]), c)
    for t in range(8):
        rg.check_plain_row(c, t, good[t])
    table = {"tail vector dropped": rejected_rows(lambda t, r: rg.check_plain_row(c, t, r), epi_plain(mm32(c["W"], drop_tail(c["X"])), c))}
    if c["resid"] is not None and c["gate"] is None:
        table["residual added without the rounding"] = rejected_rows(
            lambda t, r: rg.check_plain_row(c, t, r), epi_plain(mm32(c["W"], c["X"]), c, round_before_resid=False))
    print(f"plain {form} N={N} K={K}: rows rejecting, of 8: {table}")


@pytest.mark.parametrize("K", rg.SEG_KS)
@pytest.mark.parametrize("cols", rg.SEG_COLS)
def test_three_segment_cases(cols, K):
    c = rg.seg_case(cols, K)
    segments(c, c["X"], f"q|k|v {cols} K={K}")


def segments(c, xin, what):
    """the plain segments of a case on the kernel-side input rows xin: emulation inside, mutants outside"""
    table = {}
    for i, W in enumerate(c["W"]):
        b = 0 if c["bias"][i] is None else c["bias"][i][None, :].astype(f32)
        good = rd.rnd(emu_acc(W, xin) + b, BF)
        for t in range(8):
            rg.check_segment_row(c, t, i, good[t])
        table[f"segment {i}: tail vector dropped"] = rejected_rows(lambda t, r: rg.check_segment_row(c, t, i, r),
                                                                   rd.rnd(mm32(W, drop_tail(xin)) + b, BF))
    if len(c["W"]) == 3:
        other = np.resize(c["bias"][1], c["cols"][2])[None, :].astype(f32)
        table["segment 1's bias on segment 2"] = rejected_rows(lambda t, r: rg.check_segment_row(c, t, 2, r),
                                                               rd.rnd(mm32(c["W"][2], xin) + other, BF))
    print(f"{what}: rows rejecting, of 8: {table}")


def act_segment(c, xin, modes, what):
    ag, au = emu_acc(c["Wg"], xin), emu_acc(c["Wu"], xin)
    mg, mu = mm32(c["Wg"], xin), mm32(c["Wu"], xin)
    pair = np.arange(c["half"]) ^ 1                    # up column c + 1 with gate column c (and back)
    for mode in modes:
        good = epi_act(ag, au, mode)
        for t in range(8):
            rg.check_act_row(c, t, mode, good[t])
        chk = lambda t, r: rg.check_act_row(c, t, mode, r)   # noqa: E731
        table = {"tail vector dropped": rejected_rows(chk, epi_act(mm32(c["Wg"], drop_tail(xin)), mm32(c["Wu"], drop_tail(xin)), mode)),
                 f"act_mode {1 - mode} computed": rejected_rows(chk, epi_act(mg, mu, 1 - mode)),
                 "up columns c, c + 1 exchanged": rejected_rows(chk, epi_act(mg, mu[:, pair], mode))}
        print(f"{what} act_mode {mode}: rows rejecting, of 8: {table}")


@pytest.mark.parametrize("K", rg.ACT_KS)
@pytest.mark.parametrize("n_plain", [0, 1])
@pytest.mark.parametrize("half", rg.ACT_HALVES)
def test_swiglu_cases(half, n_plain, K):
    c = rg.act_case(half, n_plain, K)
    segments(c, c["X"], f"swiglu half={half} plain={n_plain} K={K}")
    act_segment(c, c["X"], (0, 1), f"swiglu half={half} plain={n_plain} K={K}")


@pytest.mark.parametrize("K", rg.NORM_KS)
def test_norm_cases(K):
    """the in-launch RMSNorm in front of the q | k | v triple and of the SwiGLU pair (act_mode 1)"""
    for c, what in ((rg.seg_case(rg.NORM_QKV_COLS, K, True), "q|k|v"), (rg.act_case(rg.NORM_HALF, 0, K, True), "swiglu")):
        xn = emu_norm(c["X"], c["nw"])
        segments(c, xn, f"norm + {what} K={K}")
        if what == "swiglu":
            act_segment(c, xn, (1,), f"norm + swiglu K={K}")
        if K % 512:   # rstd over K rounded up to 512 (where that is another K)
            bad = emu_norm(c["X"], c["nw"], K_div=-(-K // 512) * 512)
            if what == "swiglu":
                n = rejected_rows(lambda t, r: rg.check_act_row(c, t, 1, r), epi_act(mm32(c["Wg"], bad), mm32(c["Wu"], bad), 1))
            else:
                n = rejected_rows(lambda t, r: rg.check_segment_row(c, t, 0, r),
                                  rd.rnd(mm32(c["W"][0], bad) + c["bias"][0][None, :].astype(f32), BF))
            print(f"norm + {what} K={K}: rstd from K rounded up to 512: rows rejecting, of 8: {n}")


def test_gate_and_relu_references():
    """check_gate and the relu clamp on hand-made values"""
    z = np.zeros(3)
    r, g, acc = np.array([1.0, -2.0, 0.5]), np.array([0.5, 0.25, -1.5]), np.array([3.0, -1.0, 2.0])
    rd.check_gate(rd.rnd(r + acc * g, BF), r, g, acc, z, 1, BF)
    rd.check_gate(rd.rnd(r + np.maximum(acc, 0) * g, BF), r, g, acc, z, 1, BF, relu=True)
    with pytest.raises(AssertionError):   # relu asked, not applied (element 1)
        rd.check_gate(rd.rnd(r + acc * g, BF), r, g, acc, z, 1, BF, relu=True)
    with pytest.raises(AssertionError):   # the product rounded before the add: 257/128 -> 2, then 1/256 + 2 -> 2, not 2 + 3/256 -> 2.015625
        rd.check_gate(rd.rnd(np.array([1 / 256 + 2.0]), BF), np.array([1 / 256]), np.array([1.0]), np.array([257 / 128]), np.zeros(1), 1, BF)
    rd.check_residual(rd.rnd(r + np.maximum(acc, 0), BF), r, acc, z, 1, BF, relu=True)
    with pytest.raises(AssertionError):
        rd.check_residual(rd.rnd(r + acc, BF), r, acc, z, 1, BF, relu=True)


def test_probe_weights_are_the_formula():
    N, K = 37, 1032
    w = (rg.probe_weights(N, K).astype(np.uint32) << np.uint32(16)).view(f32)
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    np.testing.assert_array_equal(w, ((n * K + k) % 251 - 125) / 64.0)
    np.testing.assert_array_equal(rg.probe_expected(N, K, 8), w[:, 3 * np.arange(8) + 1].T)
    Wg, Wu, X, g, u = rg.column_probe(102, 512)
    assert np.array_equal(Wg, rd.rnd(Wg, BF)) and np.array_equal(Wu, rd.rnd(Wu, BF))
    assert np.all(g[1:] != g[:-1]) and np.all(np.abs(u[1:] - u[:-1]) >= 1 / 16)
