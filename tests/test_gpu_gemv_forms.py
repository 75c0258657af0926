"""GPU: the bf16 decode GEMV (csrc/gemv.hip) at kernel level against float64 (oracle/ref_decode.py), through omx_debug_gemv_ex --
every prologue / epilogue form at every width class (tuned, K split, masked tail, generic), with the route the launch takes asserted
per case; one-hot probes, rows_per_wave overrides, argmax ties and shard offsets, the x_partial fold, EPI_F32 and batched /
expert-selected entries."""
import ctypes
import zlib

import numpy as np
import pytest

from oracle import ref_decode as rd

pytestmark = pytest.mark.gpu

PRO_NONE, PRO_RMSNORM = 0, 1
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU, EPI_ARGMAX, EPI_F32 = 0, 1, 2, 3, 4
EPS = 1e-6
BF = "bf16"

# K: (route of PRO_NONE launches, route with a prologue), a route = (nv, ksplit, tail); nv 0 is the generic kernel
ROUTES = {
    512: ((1, 1, 0), (1, 1, 0)), 1024: ((2, 1, 0), (2, 1, 0)), 1536: ((3, 1, 0), (3, 1, 0)), 2048: ((4, 1, 0), (4, 1, 0)),
    3072: ((6, 1, 0), (6, 1, 0)), 3584: ((7, 1, 0), (7, 1, 0)), 4096: ((8, 1, 0), (8, 1, 0)),
    6144: ((12, 4, 0), (12, 4, 0)), 8192: ((16, 4, 0), (16, 4, 0)), 12288: ((24, 4, 0), (24, 4, 0)),
    14336: ((28, 4, 0), (28, 4, 0)), 16384: ((32, 4, 0), (32, 4, 0)), 20480: ((40, 4, 0), (40, 4, 0)),
    1000: ((2, 1, 1), (0, 1, 0)), 2560: ((6, 1, 1), (0, 1, 0)),
    4608: ((12, 4, 1), (0, 1, 0)), 5120: ((12, 4, 1), (0, 1, 0)), 9728: ((24, 4, 1), (0, 1, 0)),
    17408: ((40, 4, 1), (0, 1, 0)), 18944: ((40, 4, 1), (0, 1, 0)),
    25600: ((0, 1, 0), (0, 1, 0)),
}
# form: (prologue, epilogue, member rows, swiglu_single_round, bias)
FORMS = {
    "store": (PRO_NONE, EPI_STORE, (520,), 0, False),
    "store_bias": (PRO_NONE, EPI_STORE, (520,), 0, True),
    "rms_qkv": (PRO_RMSNORM, EPI_STORE, (1000, 300, 300), 0, False),
    "residual": (PRO_NONE, EPI_RESIDUAL, (520,), 0, False),
    "rms_swiglu3": (PRO_RMSNORM, EPI_SWIGLU, (300, 300), 0, False),
    "rms_swiglu1": (PRO_RMSNORM, EPI_SWIGLU, (300, 300), 1, False),
    "swiglu": (PRO_NONE, EPI_SWIGLU, (300, 300), 0, False),
    "rms_argmax": (PRO_RMSNORM, EPI_ARGMAX, (700,), 0, False),
}


@pytest.fixture(scope="module")
def lib(omx):
    from ominix_mlx_amd import engine   # (its binding table declares the hook)
    assert "omx_debug_gemv_ex" in engine.ENGINE_SIGNATURES
    return omx.lib


def mk_args(**kw):
    from ominix_mlx_amd.engine import GemvEx
    a = GemvEx()
    a.eps = EPS
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def launch(omx, lib, mats, x, pro, epi, nw=None, resid=None, bias=None, single_round=0, rows_per_wave=0, row_offset=0,
           out_dtype="bf16", fill=None, **extra):
    """one launch on the device copies of the host arrays; returns (output, argmax row or None, GemvEx with the route)"""
    from ominix_mlx_amd.ops import Tensor
    N = mats[0].shape[0] if epi == EPI_SWIGLU else sum(m.shape[0] for m in mats)
    K = x.shape[-1]
    keep = []

    def dev(a, dt="bf16"):
        if a is None:
            return None
        t = Tensor.from_numpy(a, dt)
        keep.append(t)
        return t.ptr

    n_out = N * max(1, extra.get("n_batch", 1))
    out = Tensor((n_out,), out_dtype) if fill is None else Tensor.from_numpy(fill, out_dtype)
    a = mk_args(N=N, K=K, pro=pro, epi=epi, single_round=single_round, rows_per_wave=rows_per_wave, row_offset=row_offset,
                n0=mats[0].shape[0], n1=mats[1].shape[0] if len(mats) > 2 else 0)
    a.dry_run = 1
    omx.check(lib.omx_debug_gemv_ex(ctypes.byref(a), None))
    slots = Tensor((max(1, a.route_blocks) * 2,), "u32")
    a.dry_run = 0
    a.out, a.argmax_slot, a.argmax_slot_n = out.ptr, slots.ptr, a.route_blocks
    a.x, a.norm_w, a.resid, a.bias = dev(x), dev(nw), dev(resid), dev(bias)
    a.w0, a.w1, a.w2 = dev(mats[0]), dev(mats[1]) if len(mats) > 1 else None, dev(mats[2]) if len(mats) > 2 else None
    for k, v in extra.items():
        if isinstance(v, np.ndarray):
            v = dev(v, "f32" if v.dtype == np.float32 and k == "x_partial" else ("u32" if v.dtype == np.uint32 else "bf16"))
        setattr(a, k, v)
    omx.check(lib.omx_debug_gemv_ex(ctypes.byref(a), None))
    got = out.numpy().astype(np.float64)
    row = None
    if epi == EPI_ARGMAX:
        row = rd.argmax_from_keys(slots.numpy().view(np.uint64), a.route_blocks)
    return got, row, a


def assert_route(a, want, rows_per_wave=None):
    assert (a.route_nv, a.route_ksplit, a.route_tail) == want, f"route {(a.route_nv, a.route_ksplit, a.route_tail)}, want {want}"
    if rows_per_wave is not None:
        assert a.route_rows_per_wave == rows_per_wave


def check_form(got, row, mats, x, pro, epi, nw, resid, bias, single_round, K):
    """the float64 reference and bound of each form (oracle/ref_decode.py)"""
    n = rd.gemv_acc_depth(K)
    W = mats[0] if len(mats) == 1 else np.concatenate(mats)
    if pro == PRO_RMSNORM:
        xin, slack_all = rd.norm_slack(W, x, nw, EPS, BF)
    else:
        xin, slack_all = x.astype(np.float64), np.zeros(sum(m.shape[0] for m in mats))
    if epi == EPI_SWIGLU:
        m = mats[0].shape[0]
        eg, mg = rd.rows_dot(mats[0], xin)
        eu, mu = rd.rows_dot(mats[1], xin)
        rd.check_swiglu(got, eg, mg, eu, mu, n, BF, single_round, slack_all[:m], slack_all[m:])
        return
    exact, mag = rd.rows_dot(W, xin)
    if epi == EPI_RESIDUAL:
        rd.check_residual(got, resid, exact, mag, n, BF, slack_all)
        return
    if bias is not None:
        exact = exact + bias.astype(np.float64)
    rd.check_plain(got, exact, mag, n, slack_all, BF)
    if epi == EPI_ARGMAX:
        rd.check_argmax(got, row)


def make_inputs(rng, pro, epi, ns, K, bias):
    mats = [rd.rand16(rng, (n, K), BF, -6, -2) for n in ns]
    x = rd.rand16(rng, (K,), BF, -2, 1)
    nw = rd.rand16(rng, (K,), BF, -1, 0) if pro == PRO_RMSNORM else None
    N = ns[0] if epi == EPI_SWIGLU else sum(ns)
    resid = rd.rand16(rng, (N,), BF, -3, 1) if epi == EPI_RESIDUAL else None
    b = rd.rand16(rng, (N,), BF, -4, 0) if bias else None
    return mats, x, nw, resid, b


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("K", list(ROUTES))
def test_gemv_form_at_width(omx, lib, K, form):
    pro, epi, ns, single_round, bias = FORMS[form]
    rng = np.random.default_rng(zlib.crc32(f"{form}/{K}".encode()))
    mats, x, nw, resid, b = make_inputs(rng, pro, epi, ns, K, bias)
    got, row, a = launch(omx, lib, mats, x, pro, epi, nw, resid, b, single_round)
    assert_route(a, ROUTES[K][1 if pro == PRO_RMSNORM else 0])
    check_form(got, row, mats, x, pro, epi, nw, resid, b, single_round, K)


def test_gemv_real_qkv_members(omx, lib):
    """Qwen3-8B's q | k | v stack (4096 | 1024 | 1024 rows) with the RMSNorm prologue"""
    rng = np.random.default_rng(8)
    mats, x, nw, _, _ = make_inputs(rng, PRO_RMSNORM, EPI_STORE, (4096, 1024, 1024), 4096, False)
    got, _, a = launch(omx, lib, mats, x, PRO_RMSNORM, EPI_STORE, nw)
    assert_route(a, (8, 1, 0))
    check_form(got, None, mats, x, PRO_RMSNORM, EPI_STORE, nw, None, None, 0, 4096)


# ---- exact probes: a one-hot x gives W[:, k] bit for bit ----

def probe_columns(K):
    nv, ks, _ = ROUTES[K][0]
    cols = {0, K - 1}
    if ks > 1:   # each wave's K slice starts at w * NVW * 512
        for w in range(1, 4):
            c = w * (nv // 4) * 512
            if c < K:
                cols |= {c - 1, c}
    return sorted(cols)


@pytest.mark.parametrize("K", [4096, 12288, 4608, 20480, 1000, 25600])
def test_gemv_one_hot_probes(omx, lib, K):
    rng = np.random.default_rng(K)
    W = rd.rand16(rng, (130, K), BF, -6, 3)
    for k in probe_columns(K):
        x = np.zeros(K, np.float32)
        x[k] = 1.0
        got, _, a = launch(omx, lib, [W], x, PRO_NONE, EPI_STORE)
        assert_route(a, ROUTES[K][0])
        np.testing.assert_array_equal(got, W[:, k].astype(np.float64), err_msg=f"column {k}")


# ---- row grouping: rows_per_wave overrides, N around whole grids ----

@pytest.mark.parametrize("rpw", [1, 2, 3, 5, 7, 8, 16, 256, 300])
@pytest.mark.parametrize("K", [4096, 12288, 1000])
def test_gemv_rows_per_wave(omx, lib, K, rpw):
    ks = ROUTES[K][0][1]
    eff = min(rpw, 256) if ks > 1 else rpw
    rows_per_block = eff * (1 if ks > 1 else 4)
    whole = rows_per_block * (3 if rpw < 256 else 1)
    rng = np.random.default_rng(zlib.crc32(f"rpw/{K}/{rpw}".encode()))
    for N in (1, 3, whole - 1, whole + 1):
        for pro, epi in ((PRO_NONE, EPI_STORE), (PRO_RMSNORM, EPI_SWIGLU)):
            ns = (N,) if epi == EPI_STORE else (N, N)
            mats, x, nw, _, _ = make_inputs(rng, pro, epi, ns, K, False)
            got, _, a = launch(omx, lib, mats, x, pro, epi, nw, rows_per_wave=rpw)
            assert_route(a, ROUTES[K][1 if pro == PRO_RMSNORM else 0], eff if a.route_nv else rpw)
            check_form(got, None, mats, x, pro, epi, nw, None, None, 0, K)


# ---- argmax: ties inside and across blocks, the last row of a ragged grid, the shard offset ----

@pytest.mark.parametrize("K", [4096, 12288, 1000])
def test_gemv_argmax_ties_and_offset(omx, lib, K):
    rng = np.random.default_rng(zlib.crc32(f"argmax/{K}".encode()))
    N = 2051   # ragged: no whole number of row groups
    W = rd.rand16(rng, (N, K), BF, -6, -2)
    x = rd.rand16(rng, (K,), BF, -2, 1)
    nw = rd.rand16(rng, (K,), BF, -1, 0)
    xin, _ = rd.norm_slack(W, x, nw, EPS, BF)
    top = (np.sign(xin) * 2.0 ** -1).astype(np.float32)   # the dominant row: every product positive
    rpb = None
    for case, rows in (("in_block", (9, 10)), ("across_blocks", (1, N - 2)), ("last_row", (N - 1,)), ("tie_3", (700, 5, 2000))):
        Wc = W.copy()
        for r in rows:
            Wc[r] = top
        for off in (0, 151936 - N):
            got, row, a = launch(omx, lib, [Wc], x, PRO_RMSNORM, EPI_ARGMAX, nw, row_offset=off)
            assert_route(a, ROUTES[K][1])
            rpb = a.route_rows_per_wave * (1 if a.route_ksplit > 1 else 4)
            check_form(got, row - off, [Wc], x, PRO_RMSNORM, EPI_ARGMAX, nw, None, None, 0, K)
            assert row - off == min(rows), f"{case}: argmax {row - off}, want the lowest tied row {min(rows)}"
    assert 9 // rpb == 10 // rpb and 1 // rpb != (N - 2) // rpb, "the in-block tie shares a block, the other spans blocks"


def test_gemv_argmax_vocabulary(omx, lib):
    """one vocabulary-sized head (Qwen3: 151936 rows of 4096) with the RMSNorm prologue; a tie across far blocks"""
    rng = np.random.default_rng(151936)
    N, K = 151936, 4096
    W = np.empty((N, K), np.float32)
    for r in range(0, N, 16384):   # (in slices: the generator's temporaries of the whole matrix would take several GB)
        W[r:r + 16384] = rd.rand16(rng, (min(16384, N - r), K), BF, -6, -2)
    x = rd.rand16(rng, (K,), BF, -2, 1)
    nw = rd.rand16(rng, (K,), BF, -1, 0)
    xin, _ = rd.norm_slack(W[:1], x, nw, EPS, BF)
    top = (np.sign(xin) * 2.0 ** -2).astype(np.float32)
    W[100000] = top
    W[77777] = top
    got, row, a = launch(omx, lib, [W], x, PRO_RMSNORM, EPI_ARGMAX, nw)
    assert_route(a, (8, 1, 0))
    assert row == 77777
    check_form(got, row, [W], x, PRO_RMSNORM, EPI_ARGMAX, nw, None, None, 0, K)


# ---- the x_partial fold: x := bf16(x + bf16(p_0 + p_1 + ...)), x_out = the folded x ----

@pytest.mark.parametrize("n_part", [1, 2, 3])
@pytest.mark.parametrize("K,pro", [(4096, PRO_RMSNORM), (4096, PRO_NONE), (1000, PRO_RMSNORM), (2560, PRO_NONE)])
def test_gemv_x_partial_fold(omx, lib, K, pro, n_part):
    from ominix_mlx_amd.ops import Tensor
    rng = np.random.default_rng(zlib.crc32(f"fold/{K}/{pro}/{n_part}".encode()))
    mats, x, nw, _, _ = make_inputs(rng, pro, EPI_STORE, (600,), K, False)
    parts = (rng.standard_normal((n_part, K)) * 0.5).astype(np.float32)
    pp = parts[0].copy()
    for j in range(1, n_part):
        pp = pp + parts[j]   # f32, slot order
    xf = rd.rnd(x.astype(np.float32) + rd.rnd(pp, BF).astype(np.float32), BF).astype(np.float32)
    x_out = Tensor((K,), "bf16")
    got, _, a = launch(omx, lib, mats, x, pro, EPI_STORE, nw, x_partial=parts.reshape(-1), x_partial_n=n_part, x_out=x_out.ptr)
    want_route = ROUTES[K][1] if K % 512 == 0 else (0, 1, 0)   # x_partial stages like a prologue: K % 512 == 0 or generic
    assert_route(a, want_route)
    np.testing.assert_array_equal(x_out.numpy(), xf)
    check_form(got, None, mats, xf, pro, EPI_STORE, nw, None, None, 0, K)


# ---- EPI_F32: the un-rounded f32 total, or bf16(bf16(acc) * out_scale) stored as f32 ----

@pytest.mark.parametrize("K", [4096, 12288, 1000, 25600])
@pytest.mark.parametrize("scaled", [False, True])
def test_gemv_epi_f32(omx, lib, K, scaled):
    rng = np.random.default_rng(zlib.crc32(f"f32/{K}/{scaled}".encode()))
    W = rd.rand16(rng, (520, K), BF, -6, -2)
    x = rd.rand16(rng, (K,), BF, -2, 1)
    sc = rd.rand16(rng, (1,), BF, -2, 0)
    extra = {"out_scale": sc} if scaled else {}
    got, _, a = launch(omx, lib, [W], x, PRO_NONE, EPI_F32, out_dtype="f32", **extra)
    assert_route(a, ROUTES[K][0])
    exact, mag = rd.rows_dot(W, x)
    acc = rd.gemv_acc_depth(K) * rd.U24 * mag
    if not scaled:
        assert np.all(np.abs(got - exact) <= acc), "f32 output off the exact dot by more than the accumulation bound"
        return
    check_scaled(got, exact, acc, float(sc[0]))


def check_scaled(got, exact, acc, s):
    """EPI_F32 with out_scale: bf16(bf16(acc) * s) -- bf16(acc) in [lo, hi] (stored_candidates), the product of two bf16 values is
    exact in f32 and the rounding monotone: got lies between bf16(lo s) and bf16(hi s) and is a bf16 value"""
    lo, hi = rd.stored_candidates(exact, acc, BF)
    a, b = rd.rnd(lo * s, BF), rd.rnd(hi * s, BF)
    ok = (got >= np.minimum(a, b)) & (got <= np.maximum(a, b))
    assert ok.all(), f"{(~ok).sum()} scaled rows off"
    rd.check_exact16(got, BF)


# ---- batched, expert-selected entries (MoE decode): x row j / x_div, expert w_sel[j], shard [w_sel_lo, + w_sel_n) ----

@pytest.mark.parametrize("K", [2048, 1000])
@pytest.mark.parametrize("form", ["swiglu", "f32_scaled"])
def test_gemv_batched_expert_entries(omx, lib, K, form):
    from ominix_mlx_amd.ops import Tensor
    rng = np.random.default_rng(zlib.crc32(f"batch/{K}/{form}".encode()))
    E, N, x_div = 4, 300, 2
    sel = np.array([3, 1, 1, 0, 2, 3, 2, 1], np.uint32)   # repeated and out-of-order expert ids
    nb = sel.size
    lo_e, n_e = 1, 2                                       # this rank holds experts 1 and 2
    f32 = form == "f32_scaled"
    xs = rd.rand16(rng, (nb // x_div, K), BF, -2, 1)
    gate = rd.rand16(rng, (E, N, K), BF, -6, -2)
    up = rd.rand16(rng, (E, N, K), BF, -6, -2)
    scales = rd.rand16(rng, (nb,), BF, -2, 0)
    sentinel = -1024.0
    out = Tensor.from_numpy(np.full(nb * N, sentinel, np.float32), "f32" if f32 else "bf16")
    keep = [Tensor.from_numpy(xs.reshape(-1)), Tensor.from_numpy(gate[lo_e:lo_e + n_e].reshape(-1)),
            Tensor.from_numpy(up[lo_e:lo_e + n_e].reshape(-1)), Tensor.from_numpy(sel, "u32"), Tensor.from_numpy(scales)]
    epi = EPI_F32 if f32 else EPI_SWIGLU
    a = mk_args(N=N, K=K, pro=PRO_NONE, epi=epi, n0=N, out=out.ptr, x=keep[0].ptr, w0=keep[1].ptr, w1=None if f32 else keep[2].ptr,
                n_batch=nb, x_div=x_div, x_bstride=K, out_bstride_bytes=N * (4 if f32 else 2), w_sel=keep[3].ptr, w_estride=N * K,
                w_sel_lo=lo_e, w_sel_n=n_e, out_scale=keep[4].ptr if f32 else None)
    omx.check(lib.omx_debug_gemv_ex(ctypes.byref(a), None))
    assert_route(a, ROUTES[K][0])
    got = out.numpy().astype(np.float64).reshape(nb, N)
    for j in range(nb):
        e = int(sel[j])
        if not lo_e <= e < lo_e + n_e:
            assert np.all(got[j] == sentinel), f"entry {j} (expert {e}, another rank's) must leave its output untouched"
            continue
        x = xs[j // x_div]
        eg, mg = rd.rows_dot(gate[e], x)
        if f32:
            check_scaled(got[j], eg, rd.gemv_acc_depth(K) * rd.U24 * mg, float(scales[j]))
        else:
            eu, mu = rd.rows_dot(up[e], x)
            rd.check_swiglu(got[j], eg, mg, eu, mu, rd.gemv_acc_depth(K), BF, 0)
