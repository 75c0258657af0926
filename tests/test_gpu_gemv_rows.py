"""GPU: the few-row bf16 Linear (csrc/gemv_rows.hip, gemv_rows_kernel<T, SEG, RPW>) at kernel level against float64, through
omx_debug_gemv_rows -- straight into launch_gemv_rows / launch_gemv_rows_segmented, no N * K routing threshold in between.  Every row
count T = 1..8 with every plain epilogue, both rows-per-wave layouts (asserted per launch through route_rpw), one-hot probes, the
three-segment q | k | v launch with biases and padded outputs, the SwiGLU pair in both act_modes with a column probe, the in-launch
RMSNorm (bit for bit against rms_norm + the same launch, and against float64) and the launcher's refusals.  Inputs, references and
bounds: oracle/ref_gemv_rows.py (oracle/ref_decode.py per activation row); tests/test_gemv_rows_bounds.py shows on the CPU that these
checks pass a correct kernel and fail the plausible wrong ones."""
import ctypes

import numpy as np
import pytest

from oracle import ref_gemv_rows as rg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hook(omx):
    from ominix_mlx_amd import engine   # (its binding table declares the hook)
    assert "omx_debug_gemv_rows" in engine.ENGINE_SIGNATURES
    return Hook(omx)


class Hook:
    def __init__(self, omx):
        self.omx, self.T = omx, omx.ops.Tensor

    def dev(self, a, keep):
        if a is None:
            return None
        t = self.T.from_numpy(a)
        keep.append(t)
        return t

    def call(self, d):
        self.omx.check(self.omx.lib.omx_debug_gemv_rows(ctypes.byref(d), None))
        return d

    def filled(self, shape, keep):
        return self.dev(np.full(shape, rg.SENTINEL, np.float32), keep)


def plain_args(M, N, K, x, w, out, bias=None, resid=None, gate=None, relu=0):
    from ominix_mlx_amd.engine import GemvRowsDbg
    d = GemvRowsDbg()
    d.x, d.M, d.K, d.segmented, d.w, d.N, d.out, d.relu = x, M, K, 0, w, N, out, relu
    d.bias, d.resid, d.gate = bias, resid, gate
    return d


def seg_args(M, K, x, segs=(), act=None, act_mode=0, norm_w=None):
    """segs: (w, bias, out, cols, ld) device pointers per plain segment; act: (w_gate, w_up, out_act, half, ld_act)"""
    from ominix_mlx_amd.engine import GemvRowsDbg
    d = GemvRowsDbg()
    d.x, d.M, d.K, d.segmented, d.n_plain = x, M, K, 1, len(segs)
    for i, (w, b, o, cols, ld) in enumerate(segs):
        d.seg[i].w, d.seg[i].bias, d.seg[i].out, d.seg[i].cols, d.seg[i].ld = w, b, o, cols, ld
    if act is not None:
        d.w_gate, d.w_up, d.out_act, d.half, d.ld_act = act
    d.act_mode, d.pre_norm_w, d.pre_norm_eps = act_mode, norm_w, rg.EPS
    return d


def ptr(t):
    return None if t is None else t.ptr


# ---- plain mode ----

def run_plain_case(hook, c, Ms, want_rpw):
    keep = []
    N, K = c["N"], c["K"]
    x, w = hook.dev(c["X"], keep), hook.dev(c["W"], keep)
    bias, gate, resid = hook.dev(c["bias"], keep), hook.dev(c["gate"], keep), hook.dev(c["resid"], keep)
    for M in Ms:   # the first M of the 8 rows: the same device buffers, a prefix of them
        if c["form"] == "residual_inplace":   # out == resid, as the engine calls the o and down projections
            out = res = hook.dev(c["resid"][:M], keep)
        else:
            out, res = hook.filled((M, N), keep), resid
        d = hook.call(plain_args(M, N, K, x.ptr, w.ptr, out.ptr, ptr(bias), ptr(res), ptr(gate), c["relu"]))
        assert d.route_rpw == want_rpw
        got = out.numpy().astype(np.float64)
        for t in range(M):
            rg.check_plain_row(c, t, got[t])


@pytest.mark.parametrize("form", rg.PLAIN_FORMS)
@pytest.mark.parametrize("K", rg.PLAIN_KS)
def test_rows_plain_every_row_count(hook, K, form):
    """T = 1..8 at N = 300 (two rows per wave, 8 per block: the trailing waves own one row or none); K: one partial chunk, a masked last
    vector row, exactly one chunk, a chunk plus one vector, three chunks"""
    run_plain_case(hook, rg.plain_case(form, rg.PLAIN_N, K), range(1, 9), 2)


@pytest.mark.parametrize("form", rg.WIDE_FORMS)
def test_rows_plain_four_rows_per_wave(hook, form):
    """N = 12300 >= 12288: four rows per wave, 16 per block, 12300 % 16 != 0"""
    run_plain_case(hook, rg.plain_case(form, rg.WIDE_N, rg.WIDE_K), rg.WIDE_MS, 4)


@pytest.mark.parametrize("K", [4104, 12288])
@pytest.mark.parametrize("N,rpw", [(rg.PLAIN_N, 2), (rg.WIDE_N, 4)])
def test_rows_one_hot_probes(hook, N, rpw, K):
    """row t of x one-hot at column 3 t + 1 against w[n, k] = ((n K + k) % 251 - 125) / 64: the picked weights, exactly -- transposes, the
    chunk seam (everything past column 22 must add nothing) and the min(j * 64 + lane, nv - 1) clamp of the short last chunk"""
    from ominix_mlx_amd.loader import Bf16Bits
    M, keep = 8, []
    x = np.zeros((M, K), np.float32)
    x[np.arange(M), 3 * np.arange(M) + 1] = 1.0
    xd, wd, out = hook.dev(x, keep), hook.dev(rg.probe_weights(N, K).view(Bf16Bits), keep), hook.filled((M, N), keep)
    d = hook.call(plain_args(M, N, K, xd.ptr, wd.ptr, out.ptr))
    assert d.route_rpw == rpw
    np.testing.assert_array_equal(out.numpy(), rg.probe_expected(N, K, M))


# ---- segmented mode ----

def upload(hook, c, keep):
    """the weights and biases of a segmented case on the device, once per test"""
    dw = {"W": [hook.dev(W, keep) for W in c["W"]], "bias": [hook.dev(b, keep) for b in c["bias"]]}
    if "half" in c:
        dw["Wg"], dw["Wu"] = hook.dev(c["Wg"], keep), hook.dev(c["Wu"], keep)
    return dw


def run_segmented(hook, c, dw, M, x, act_mode=0, norm_w=None, pad=8):
    """one segmented launch of case c (device weights dw) on the device rows x: (plain outputs [M, cols_i] each, act output [M, half] or
    None, route_rpw); every output has a row stride of cols + pad, pre-filled with a sentinel that the padding must keep"""
    keep, segs, outs = [], [], []
    for W, b, cols in zip(dw["W"], dw["bias"], c["cols"]):
        o = hook.filled((M, cols + pad), keep)
        outs.append(o)
        segs.append((W.ptr, ptr(b), o.ptr, cols, cols + pad))
    act = oa = None
    if "half" in c:
        oa = hook.filled((M, c["half"] + pad), keep)
        act = (dw["Wg"].ptr, dw["Wu"].ptr, oa.ptr, c["half"], c["half"] + pad)
    d = hook.call(seg_args(M, c["K"], x.ptr, segs, act, act_mode, ptr(norm_w)))
    res = []
    for o, cols in list(zip(outs, c["cols"])) + ([(oa, c["half"])] if oa is not None else []):
        full = o.numpy()
        assert np.all(full[:, cols:] == rg.SENTINEL), "a padding column was written"
        res.append(full[:, :cols].astype(np.float64))
    return res[:len(outs)], (res[-1] if oa is not None else None), d.route_rpw


@pytest.mark.parametrize("K", rg.SEG_KS)
@pytest.mark.parametrize("cols", rg.SEG_COLS)
def test_rows_three_segments_with_biases(hook, cols, K):
    """q | k | v in one launch (Qwen2: a bias per segment), every output padded; each segment against float64 on its own"""
    c = rg.seg_case(cols, K)
    keep = []
    x, dw = hook.dev(c["X"], keep), upload(hook, c, keep)
    for M in rg.SEG_MS:
        plain, _, rpw = run_segmented(hook, c, dw, M, x)
        assert rpw == 2
        for i in range(3):
            for t in range(M):
                rg.check_segment_row(c, t, i, plain[i][t])


@pytest.mark.parametrize("K", rg.ACT_KS)
@pytest.mark.parametrize("n_plain", [0, 1])
@pytest.mark.parametrize("half", rg.ACT_HALVES)
def test_rows_swiglu_pair(hook, half, n_plain, K):
    """gate / up with the SwiGLU epilogue in both act_modes (four rows per wave: 2 gate + 2 up rows, a block owns 8 activation columns;
    102 % 8 != 0, and a 64-column plain segment in front of 2050 puts the block's seam inside the pair)"""
    c = rg.act_case(half, n_plain, K)
    keep = []
    x, dw = hook.dev(c["X"], keep), upload(hook, c, keep)
    for M in rg.ACT_MS:
        for act_mode in (0, 1):
            plain, act, rpw = run_segmented(hook, c, dw, M, x, act_mode)
            assert rpw == 4
            for t in range(M):
                for i in range(n_plain):
                    rg.check_segment_row(c, t, i, plain[i][t])
                rg.check_act_row(c, t, act_mode, act[t])


@pytest.mark.parametrize("act_mode", [0, 1])
@pytest.mark.parametrize("half,K", [(102, 512), (2050, 4104)])
def test_rows_swiglu_column_probe(hook, half, K, act_mode):
    """one distinctive gate and up row per column (rg.column_probe): out_act[t, c] is the epilogue of exactly (gate c, up c)"""
    Wg, Wu, X, g, u = rg.column_probe(half, K)
    c = {"W": [], "bias": [], "cols": (), "half": half, "K": K, "Wg": Wg, "Wu": Wu}
    keep = []
    _, act, rpw = run_segmented(hook, c, upload(hook, c, keep), 8, hook.dev(X, keep), act_mode)
    assert rpw == 4
    for t in range(8):
        lo, hi = rg.column_probe_expected(g, u, t, act_mode)
        bad = np.nonzero((act[t] < lo) | (act[t] > hi))[0]
        assert bad.size == 0, f"row {t}: {bad.size} columns are not their own (gate, up) pair, e.g. {bad[0]}: {act[t][bad[0]]}, want {lo[bad[0]]}"


@pytest.mark.parametrize("K", rg.NORM_KS)
@pytest.mark.parametrize("what", ["qkv", "swiglu"])
def test_rows_in_launch_rmsnorm(omx, hook, what, K):
    """pre_norm_w: bit for bit the two-launch composition (rms_norm, then the same launch without it), and against float64 with the
    norm's rounding flips counted at rows_norm_depth(K)"""
    c = rg.seg_case(rg.NORM_QKV_COLS, K, True) if what == "qkv" else rg.act_case(rg.NORM_HALF, 0, K, True)
    act_mode = 1
    keep = []
    nw, dw = hook.dev(c["nw"], keep), upload(hook, c, keep)
    for M in rg.NORM_MS:
        x = hook.dev(c["X"][:M], keep)
        plain, act, rpw = run_segmented(hook, c, dw, M, x, act_mode, nw)
        assert rpw == (2 if what == "qkv" else 4)
        xn = omx.ops.rms_norm(x, nw, rg.EPS)
        plain2, act2, _ = run_segmented(hook, c, dw, M, xn, act_mode)
        for a, b in zip(plain, plain2):
            np.testing.assert_array_equal(a, b)
        if act is not None:
            np.testing.assert_array_equal(act, act2)
        for t in range(M):
            for i in range(len(plain)):
                rg.check_segment_row(c, t, i, plain[i][t])
            if act is not None:
                rg.check_act_row(c, t, act_mode, act[t])


# ---- refusals: the launcher's host checks, nothing is launched ----

def test_rows_refusals(omx, hook):
    keep = []
    K, N = 4104, 304
    x, w = hook.filled((9, K), keep), hook.filled((N, K), keep)   # (large enough for every shape below, were a check missing)
    out, nw = hook.filled((9, N + 8), keep), hook.filled((K,), keep)

    def refused(d, text):
        with pytest.raises(omx.OmxError, match=text):
            hook.call(d)

    seg = [(w.ptr, None, out.ptr, 64, N + 8)]
    act = (w.ptr, w.ptr, out.ptr, 102, N + 8)
    refused(seg_args(2, K, x.ptr, seg, norm_w=nw.ptr), r"in-launch RMSNorm needs the whole row staged at once \(K = 4104 > 4096\)")
    refused(plain_args(9, N, K, x.ptr, w.ptr, out.ptr), r"gemv_rows: unsupported shape M=9 N=304 K=4104")
    refused(seg_args(9, K, x.ptr, seg), r"gemv_rows: unsupported segmented shape M=9 K=4104")
    refused(plain_args(2, N, 12, x.ptr, w.ptr, out.ptr), r"gemv_rows: unsupported shape M=2 N=304 K=12")
    refused(seg_args(2, 12, x.ptr, seg), r"gemv_rows: unsupported segmented shape M=2 K=12")
    refused(seg_args(2, K, x.ptr, [(w.ptr, None, out.ptr, 6, N + 8)]), r"gemv_rows: unsupported segmented shape M=2 K=4104")
    refused(seg_args(2, K, x.ptr, seg, (w.ptr, w.ptr, out.ptr, 101, N + 8)), r"gemv_rows: unsupported segmented shape M=2 K=4104")
    refused(plain_args(2, N, K, x.ptr + 2, w.ptr, out.ptr), r"gemv_rows: unsupported shape M=2 N=304 K=4104")
    refused(plain_args(2, N, K, x.ptr, w.ptr + 2, out.ptr), r"gemv_rows: unsupported shape M=2 N=304 K=4104")
    refused(seg_args(2, K, x.ptr, [(w.ptr + 2, None, out.ptr, 64, N + 8)]), r"gemv_rows: operands must be 16-byte aligned")
    refused(seg_args(2, K, x.ptr, seg, (w.ptr, w.ptr + 2, out.ptr, 102, N + 8)), r"gemv_rows: operands must be 16-byte aligned")
    refused(seg_args(2, 4096, x.ptr, seg, act, norm_w=nw.ptr + 2), r"gemv_rows: operands must be 16-byte aligned")
    assert np.all(out.numpy() == rg.SENTINEL), "a refused call wrote its output"
