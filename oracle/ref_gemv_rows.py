"""The cases of the few-row bf16 Linear (csrc/gemv_rows.hip, M <= 8 activation rows) and their float64 checks, shared by the GPU test
(tests/test_gpu_gemv_rows.py, the kernel's output) and the CPU test (tests/test_gemv_rows_bounds.py, a host emulation and its mutants):
both draw the same inputs from the same seeds and go through the same check_* below.  References and bounds are oracle/ref_decode.py's,
applied per activation row; the accumulation depth is gemv_acc_depth(K), the in-launch RMSNorm's rows_norm_depth(K) (both derived in
their docstrings).  Inputs are keyed without the row count: a case of M rows takes the first M of 8, so row t is the same in every case."""
import functools
import zlib

import numpy as np

from . import ref_decode as rd

BF = "bf16"
EPS = 1e-6
SENTINEL = -1024.0           # pre-fill of the padding columns (ld > cols): exact in bf16, far from every output

PLAIN_FORMS = ("store", "bias", "bias_relu", "residual", "residual_inplace", "gate")
PLAIN_N, PLAIN_KS = 300, (512, 1032, 4096, 4104, 12288)
WIDE_N, WIDE_K, WIDE_MS, WIDE_FORMS = 12300, 512, (1, 4, 8), ("store", "residual")
SEG_COLS, SEG_MS, SEG_KS = ((128, 64, 68), (1000, 300, 300)), (1, 3, 5, 8), (512, 1032, 4096, 12288)
ACT_HALVES, ACT_MS, ACT_KS, ACT_PLAIN_COLS = (102, 2050), (1, 4, 8), (512, 4096, 4104), 64
NORM_MS, NORM_KS = (1, 2, 3, 4), (512, 1032, 4096)
NORM_QKV_COLS, NORM_HALF = (128, 64, 68), 102


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in ("gemv_rows",) + key).encode()))


def dots(W, X):
    """exact X . W^T [M, N] (float64) and sum_k |x| |w| of each element"""
    Wd, Xd = W.astype(np.float64), np.asarray(X, np.float64)
    return Xd @ Wd.T, np.abs(Xd) @ np.abs(Wd).T


# ---- plain mode: out = x . w^T (+ bias) (relu) (+ resid | resid + . * gate) ----

@functools.lru_cache(maxsize=4)
def plain_case(form, N, K):
    """inputs (8 activation rows) and the exact products of one plain case"""
    rng = _rng("plain", form, N, K)
    c = {"form": form, "N": N, "K": K, "W": rd.rand16(rng, (N, K), BF, -6, -2), "X": rd.rand16(rng, (8, K), BF, -2, 1),
         "bias": None, "resid": None, "gate": None, "relu": int(form == "bias_relu")}
    if form in ("bias", "bias_relu"):
        c["bias"] = rd.rand16(rng, (N,), BF, -4, 0)
    if form in ("residual", "residual_inplace", "gate"):
        c["resid"] = rd.rand16(rng, (8, N), BF, -3, 1)
    if form == "gate":
        c["gate"] = rd.rand16(rng, (N,), BF, -2, 1)
    c["exact"], c["mag"] = dots(c["W"], c["X"])
    if c["bias"] is not None:   # the bias joins the f32 sum as one more term (one more rounding, inside gemv_acc_depth's spare)
        c["exact"] = c["exact"] + c["bias"].astype(np.float64)
        c["mag"] = c["mag"] + np.abs(c["bias"].astype(np.float64))
    return c


def check_plain_row(c, t, got):
    """row t of a plain case's output [N] against float64"""
    n = rd.gemv_acc_depth(c["K"])
    exact, mag = c["exact"][t], c["mag"][t]
    if c["gate"] is not None:
        rd.check_gate(got, c["resid"][t], c["gate"], exact, mag, n, BF, relu=bool(c["relu"]))
    elif c["resid"] is not None:
        rd.check_residual(got, c["resid"][t], exact, mag, n, BF, relu=bool(c["relu"]))
    else:   # |max(v, 0) - max(exact, 0)| <= |v - exact|: the plain bound holds on the clamped reference
        rd.check_plain(got, np.maximum(exact, 0.0) if c["relu"] else exact, mag, n, 0.0, BF)


def probe_weights(N, K):
    """w[n, k] = ((n K + k) % 251 - 125) / 64 as bf16 BIT patterns [N, K] (every value is exact in bf16), built from one period"""
    period = ((np.arange(251) - 125) / 64.0).astype(np.float32)
    bits = (period.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    line = np.tile(bits, K // 251 + 2)
    out = np.empty((N, K), np.uint16)
    for r in range(N):
        o = (r * K) % 251
        out[r] = line[o:o + K]
    return out


def probe_expected(N, K, M):
    """x row t one-hot at column 3 t + 1: out[t, n] = w[n, 3 t + 1] exactly"""
    n, t = np.arange(N, dtype=np.int64)[None, :], np.arange(M, dtype=np.int64)[:, None]
    return (((n * K + 3 * t + 1) % 251 - 125) / 64.0).astype(np.float32)


# ---- segmented mode ----

@functools.lru_cache(maxsize=2)
def seg_case(cols, K, norm=False):
    """q | k | v: three plain segments with biases (norm: the in-launch RMSNorm in front)"""
    rng = _rng("seg", cols, K, norm)
    c = {"cols": cols, "K": K, "X": rd.rand16(rng, (8, K), BF, -2, 1), "W": [rd.rand16(rng, (n, K), BF, -6, -2) for n in cols],
         "bias": [rd.rand16(rng, (n,), BF, -4, 0) for n in cols], "nw": rd.rand16(rng, (K,), BF, -1, 0) if norm else None}
    return c


@functools.lru_cache(maxsize=2)
def act_case(half, n_plain, K, norm=False):
    """a SwiGLU pair (gate / up [half, K]) behind n_plain segments of ACT_PLAIN_COLS columns without bias"""
    rng = _rng("act", half, n_plain, K, norm)
    c = {"half": half, "K": K, "X": rd.rand16(rng, (8, K), BF, -2, 1), "cols": (ACT_PLAIN_COLS,) * n_plain,
         "W": [rd.rand16(rng, (ACT_PLAIN_COLS, K), BF, -6, -2) for _ in range(n_plain)], "bias": [None] * n_plain,
         "Wg": rd.rand16(rng, (half, K), BF, -6, -2), "Wu": rd.rand16(rng, (half, K), BF, -6, -2),
         "nw": rd.rand16(rng, (K,), BF, -1, 0) if norm else None}
    return c


@functools.lru_cache(maxsize=2)
def _case_ref(kind, key):
    """for all 8 activation rows at once: per weight matrix the exact products [8, n], their magnitudes and the norm's flip slack.
    Under a norm the kernel-side input is the exact RMSNorm rounded to bf16 (norm_candidates' mid at rows_norm_depth(K)); the kernel's
    element is lo or hi, so its product differs by at most sum_k |hi_k - lo_k| |W_nk| (the way norm_slack counts it for one row)"""
    c = seg_case(*key) if kind == "seg" else act_case(*key)
    mats = list(c["W"]) + ([c["Wg"], c["Wu"]] if kind == "act" else [])
    if c["nw"] is not None:
        xin, lo, hi = rd.norm_candidates(c["X"], c["nw"], EPS, BF, rd.rows_norm_depth(c["K"]))
        d = hi - lo
    else:
        xin, d = c["X"].astype(np.float64), None
    out = []
    for W in mats:
        exact, mag = dots(W, xin)
        out.append((exact, mag, np.zeros_like(exact) if d is None else d @ np.abs(W.astype(np.float64)).T))
    return out


def case_key(c):
    return ("act", (c["half"], len(c["cols"]), c["K"], c["nw"] is not None)) if "half" in c else ("seg", (c["cols"], c["K"], c["nw"] is not None))


def check_segment_row(c, t, i, got):
    """row t of plain segment i [cols_i] against float64 (bias as one more term of the sum)"""
    exact, mag, slack = (a[t] for a in _case_ref(*case_key(c))[i])
    if c["bias"][i] is not None:
        b = c["bias"][i].astype(np.float64)
        exact, mag = exact + b, mag + np.abs(b)
    rd.check_plain(got, exact, mag, rd.gemv_acc_depth(c["K"]), slack, BF)


def check_act_row(c, t, act_mode, got):
    """row t of the SwiGLU output [half] against float64, act_mode as in gemm.hpp"""
    ref = _case_ref(*case_key(c))
    (eg, mg, sg), (eu, mu, su) = ((a[t] for a in m) for m in ref[-2:])
    rd.check_swiglu(got, eg, mg, eu, mu, rd.gemv_acc_depth(c["K"]), BF, rd.act_mode_single_round(act_mode), sg, su)


def column_probe(half, K):
    """gate / up weights with one distinctive row per column: row c of w_gate is g_c at column c % K and zero elsewhere, row c of w_up
    is u_c at the same column; activation row t is 2^-t everywhere.  Then acc_gate[t, c] = g_c 2^-t and acc_up[t, c] = u_c 2^-t
    EXACTLY (one non-zero product per row, nothing to round), and out_act[t, c] is the epilogue of exactly the pair (gate c, up c).
    g_c = (1 + c % 127) / 32, u_c = (1 + c // 127 + 2 (c % 5)) / 16 (exact in bf16): both differ between c and c + 1 by far more than
    a bf16 ulp, so a wrong pairing of neighbouring gate / up rows is a hard failure.  Returns (Wg, Wu, X [8, K], g, u)."""
    cidx = np.arange(half)
    g = ((1 + cidx % 127) / 32.0).astype(np.float32)
    u = ((1 + cidx // 127 + 2 * (cidx % 5)) / 16.0).astype(np.float32)
    Wg, Wu = np.zeros((half, K), np.float32), np.zeros((half, K), np.float32)
    Wg[cidx, cidx % K], Wu[cidx, cidx % K] = g, u
    X = np.repeat((2.0 ** -np.arange(8, dtype=np.float64))[:, None], K, axis=1).astype(np.float32)
    return Wg, Wu, X, g, u


def column_probe_expected(g, u, t, act_mode):
    """the kernel's epilogue on the exact factors g 2^-t, u 2^-t, in f32 as the kernel computes it: (candidates lo, hi) per column --
    the f32 expf / divide may sit 16 u off (check_swiglu's e), everything else is exact or a rounding to bf16"""
    f32 = np.float32
    gt, up = (g * f32(2.0 ** -t)).astype(np.float64), (u * f32(2.0 ** -t)).astype(np.float64)
    sig = 1.0 / (1.0 + np.exp(-gt))
    e = 16 * rd.U24
    if act_mode == 1:
        a, b = (rd.rnd(rd.rnd(gt * s, BF) * up, BF) for s in (rd.rnd(sig * (1 - e), BF), rd.rnd(sig * (1 + e), BF)))
    else:
        y = gt * sig * up
        a, b = rd.rnd(y * (1 - e), BF), rd.rnd(y * (1 + e), BF)
    return np.minimum(a, b), np.maximum(a, b)
