"""GPU: the packed-weight decode GEMV (csrc/quant.hip + qgemv_body.inc, csrc/qgemv_mfma.hip) at kernel level against float64
(oracle/ref_qdecode.py), through omx_debug_qgemv_ex -- every launch with the fields the engines set (interleaved scale | bias words,
float16 triplets, row_offset, batches, expert selection) and its route asserted.  Triplets are built from random codes (row 0 all
zero, row 1 all maximum, scales of both signs, some biases exactly 0), not by quantising a matrix.

a/b. dequantise through the GEMV: one-hot activation rows read every single field back, within a few u -- far below one code step;
c.   every prologue / epilogue form at each of the 36 (bits, group, triplet dtype) formats, SB on and off (bit-identical), the
     two-pass RMSNorm prologue, the rolled staging; d. argmax: rows_per_wave 16, row_offset, ties, the matrix cores' streaming route;
e.   the matrix-core forms at every built KS; f. expert selection.
Every bound is n 2^-24 M_r (+ the rounding of the stored point), n and M_r derived in ref_qdecode.py.  Each test prints its largest
error / bound ratio."""
import ctypes
import zlib

import numpy as np
import pytest

from oracle import ref_decode as rd
from oracle import ref_qdecode as rq

pytestmark = pytest.mark.gpu

PRO_NONE, PRO_RMSNORM = 0, 1
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU, EPI_ARGMAX, EPI_F32 = 0, 1, 2, 3, 4
VALU, MFMA = 1, 3          # route_kernel (2: the mixed-format stack kernel, held in test_gpu_mixed_quant.py)
EPS = 1e-6
BITS, GROUPS, DTS = (2, 3, 4, 5, 6, 8), (32, 64, 128), ("bf16", "f16")
# the smallest K of every W class (4 bits: W 4, 2, 1; 8 bits: W 4, 2); the chunked widths: one full step, and 80 chunks = a second step
# with 16 live lanes
CLASS_K = {2: (2048, 2560), 3: (2048, 2560), 5: (2048, 2560), 6: (2048, 2560), 4: (2048, 1024, 512), 8: (1024, 512)}
X_EXP = (-3, 0)          # activations over four binades (ref_qdecode.valu_depth's x_span = 4)
SENT, PAD = 7.0, 8       # every output buffer is PAD elements longer than the launch writes, pre-filled with SENT
FORMATS = [(b, g, dt) for b in BITS for g in GROUPS for dt in DTS]


def case_rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@pytest.fixture(scope="module")
def lib(omx):
    from ominix_mlx_amd import engine   # (its binding table declares the hook)
    assert "omx_debug_qgemv_ex" in engine.ENGINE_SIGNATURES
    omx.require_device()
    omx.lib.omx_debug_qgemv_grid.restype, omx.lib.omx_debug_qgemv_grid.argtypes = ctypes.c_int, [ctypes.c_int]
    return omx.lib


class Mat:
    """one packed matrix on the host and (lazily, once) on the device"""

    def __init__(self, rng, n, K, bits, group, dt, stack=1):
        self.n, self.K, self.bits, self.group, self.dt = n, K, bits, group, dt
        self.q, self.s, self.b = rq.make_triplet(rng, n * stack, K, bits, group, dt)
        self._dev = None

    def dev(self):
        if self._dev is None:
            from ominix_mlx_amd.ops import Tensor
            self._dev = (Tensor.from_numpy(rq.pack(self.q, self.bits), "u32"), Tensor.from_numpy(self.s, self.dt), Tensor.from_numpy(self.b, self.dt))
        return self._dev


def launch(omx, lib, mats, x, pro, epi, *, nw=None, resid=None, single_round=0, use_sb=0, use_tiles=0, mfma=0, row_offset=0,
           rolled_stage=0, n_batch=0, x_div=0, w_sel=None, w_sel_lo=0, w_sel_n=0, n_experts=0, x_dev=None, x_off=0,
           slot_cap=None):
    """one launch; returns (output as float64 [rows, N] WITHOUT the sentinel tail (checked here), argmax row or None, the QGemvEx).
    x: host array (uploaded) or, with x_dev, a device tensor read from element x_off."""
    from ominix_mlx_amd.engine import QGemvEx
    from ominix_mlx_amd.ops import Tensor
    m0 = mats[0]
    dt, K = m0.dt, m0.K
    N = m0.n if epi == EPI_SWIGLU else sum(m.n for m in mats)
    keep = []

    def up(a, d):
        if a is None:
            return None
        t = Tensor.from_numpy(a, d)
        keep.append(t)
        return t.ptr

    a = QGemvEx()
    for i, m in enumerate(mats):
        w, s, b = m.dev()
        a.m[i].w, a.m[i].scales, a.m[i].biases, a.m[i].n = w.ptr, s.ptr, b.ptr, m.n
    a.N, a.K, a.group, a.bits, a.pro, a.epi, a.eps, a.single_round = N, K, m0.group, m0.bits, pro, epi, EPS, single_round
    a.scales_f16, a.use_sb, a.use_tiles, a.mfma, a.row_offset, a.rolled_stage = int(dt == "f16"), use_sb, use_tiles, mfma, row_offset, rolled_stage
    a.n_batch, a.x_div, a.w_sel_lo, a.w_sel_n, a.n_experts = n_batch, x_div, w_sel_lo, w_sel_n, n_experts
    if w_sel is not None:
        a.w_sel = up(np.asarray(w_sel, np.uint32), "u32")
        a.w_estride, a.s_estride = m0.n * (K * m0.bits // 32), m0.n * (K // m0.group)
    a.dry_run = 1
    omx.check(lib.omx_debug_qgemv_ex(ctypes.byref(a), None))
    a.dry_run = 0
    rows = max(1, n_batch)
    f32 = epi == EPI_F32
    out = Tensor.from_numpy(np.full((rows * N + PAD,), SENT, np.float32), "f32" if f32 else dt)
    # (the matrix-core kernel also clears the slots up to qgemv_grid(N), the partials the engines reduce)
    cap = slot_cap if slot_cap is not None else max(1, a.route_blocks, lib.omx_debug_qgemv_grid(N) if a.route_kernel == MFMA else 0)
    slots = Tensor.from_numpy(np.full((2 * cap,), 0xFFFFFFFF, np.uint32), "u32")
    if f32:
        a.out_f32 = out.ptr
    else:
        a.out = out.ptr
    a.argmax_slot, a.argmax_slot_n = slots.ptr, cap
    a.x = x_dev.ptr + 2 * x_off if x_dev is not None else up(x, dt)
    a.norm_w, a.resid = up(nw, dt), up(resid, dt)
    omx.check(lib.omx_debug_qgemv_ex(ctypes.byref(a), None))
    got = out.numpy().astype(np.float64)
    assert (got[rows * N:] == SENT).all(), "the launch wrote past its output"
    row = None
    if epi == EPI_ARGMAX:
        a.keys = slots.numpy().view(np.uint64)
        row = rd.argmax_from_keys(a.keys, a.route_blocks)
    return got[:rows * N].reshape(rows, N), row, a


def cat(mats):
    return np.concatenate([m.q for m in mats]), np.concatenate([m.s for m in mats]), np.concatenate([m.b for m in mats])


def check_form(got, row, mats, x, pro, epi, nw, resid, single_round, n, row_offset=0):
    """the float64 reference and bound of one single-row launch; returns the error / bound ratio where the check is a distance"""
    m0 = mats[0]
    dt, group, m = m0.dt, m0.group, rq.magic(m0.bits, m0.dt)
    got = got[0]

    def ref(q, s, b):
        if pro == PRO_RMSNORM:
            xin, slack = rq.norm_slack_q(q, s, b, group, x, nw, EPS, dt)
        else:
            xin, slack = x.astype(np.float64), np.zeros(q.shape[0])
        return rq.rows_ref(q, s, b, group, xin, m) + (slack,)

    if epi == EPI_SWIGLU:
        eg, mg, sg = ref(mats[0].q, mats[0].s, mats[0].b)
        eu, mu, su = ref(mats[1].q, mats[1].s, mats[1].b)
        rd.check_swiglu(got, eg, mg, eu, mu, n, dt, single_round, sg, su)
        return None
    exact, mag, slack = ref(*cat(mats))
    if epi == EPI_RESIDUAL:
        rd.check_residual(got, resid, exact, mag, n, dt, slack)
        return None
    if epi == EPI_F32:
        rq.check_f32(got, exact, mag, n, slack)
        return rq.ratio(got, exact, mag, n, slack)
    rd.check_plain(got, exact, mag, n, slack, dt)
    if epi == EPI_ARGMAX:
        rd.check_argmax(got, row, row_offset)
    return rq.ratio(got, exact, mag, n, slack, dt)


def sb_route(bits, W, use_sb):
    """the interleaved-words kernel exists for the four-word class and the chunked widths"""
    return int(bool(use_sb) and (W == 4 or bits in rq.CHUNKED))


# ---- a. dequantise through the VALU kernel ----

_EYES = {}


def eye_dev(K, dt):
    """[K, K] one-hot rows times 2^-3, on the device once per (K, dtype)"""
    from ominix_mlx_amd.ops import Tensor
    if (K, dt) not in _EYES:
        _EYES[K, dt] = Tensor.from_numpy(np.eye(K, dtype=np.float32) * 0.125, dt)
    return _EYES[K, dt]


@pytest.mark.parametrize("bits,group,dt", FORMATS)
def test_dequantise_through_the_gemv(omx, lib, bits, group, dt):
    """x = the K one-hot rows times 2^-3 as one batch (n_batch = K, x_div = 1), PRO_NONE, EPI_F32: out_f32[k, r] is 2^-3 (s q + b) of
    element (r, k), N = 21 rows ragged against a block's 8.  Every sum has one non-zero term (ref_qdecode.PROBE_DEPTH), and the
    tolerance is asserted below 2^-10 of one code step: a wrong field, pairing, group index or fold fails by orders of magnitude."""
    N, worst = 21, 0.0
    for K in CLASS_K[bits]:
        mat = Mat(case_rng("probe", bits, group, dt, K), N, K, bits, group, dt)
        want, tol, step = rq.probe_ref(mat.q, mat.s, mat.b, group, rq.magic(bits, dt))
        assert (tol < 2.0 ** -10 * step).all()
        W = rq.words(bits, K, group)
        outs = []
        for use_sb in (0, 1):
            got, _, a = launch(omx, lib, [mat], None, PRO_NONE, EPI_F32, use_sb=use_sb, n_batch=K, x_div=1, x_dev=eye_dev(K, dt))
            assert (a.route_kernel, a.route_bits, a.route_w, a.route_f16s) == (VALU, bits, W, int(dt == "f16"))
            assert a.route_sb == sb_route(bits, W, use_sb)
            err = np.abs(got - want)
            bad = np.argwhere(err > tol)
            assert bad.size == 0, (f"K {K} sb {use_sb}: {len(bad)} elements off, e.g. column {bad[0][0]} row {bad[0][1]}: got "
                                   f"{got[tuple(bad[0])]} want {want[tuple(bad[0])]} (one code step {step[tuple(bad[0])]})")
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))    # (tol == 0: all-zero codes under a zero bias, err == 0 asserted)
            outs.append(got)
        assert np.array_equal(outs[0], outs[1]), "interleaved and separate scale / bias words must agree bit for bit"
    print(f"probe {bits}-bit group {group} {dt}: largest error / bound {worst:.3f}")


# ---- b. ... and through the matrix-core kernel (one launch per one-hot column: it takes one activation row) ----

@pytest.mark.parametrize("K,N,ncols", [(1024, 40, 1024), (2048, 40, 64), (12288, 40, 64)])
def test_dequantise_through_the_matrix_cores(omx, lib, K, N, ncols):
    """K = 1024: every column, N = 40 = two 16-row blocks and half a third.  K = 2048 / 12288: 64 columns, one of every residue mod 64,
    alternating between the first and the last 1024-column tile and walking the tile's 16 groups."""
    from ominix_mlx_amd.ops import Tensor
    mat = Mat(case_rng("mprobe", K), N, K, 4, 64, "bf16")
    want, tol, step = rq.probe_ref(mat.q, mat.s, mat.b, 64, 128.0)
    assert (tol < 2.0 ** -10 * step).all()
    if ncols == K:
        cols = np.arange(K)
    else:
        j = np.arange(64)
        cols = np.where(j % 2 == 0, 0, K - 1024) + 64 * ((5 * j) % 16) + j
        assert sorted(cols % 64) == list(range(64)) and (cols < 1024).any() and (cols >= K - 1024).any()
    xh = np.zeros((len(cols), K), np.float32)
    xh[np.arange(len(cols)), cols] = 0.125
    xd = Tensor.from_numpy(xh, "bf16")
    worst = 0.0
    for i, k in enumerate(cols):
        got, _, a = launch(omx, lib, [mat], None, PRO_NONE, EPI_F32, use_tiles=1, mfma=1, x_dev=xd, x_off=i * K)
        assert (a.route_kernel, a.route_ks, a.route_nu, a.route_nbuf, a.route_blocks) == (MFMA, K // 1024, 1, 1, 3)
        err = np.abs(got[0] - want[k])
        bad = np.nonzero(err > tol[k])[0]
        assert bad.size == 0, f"column {k}: rows {bad[:8]} off, e.g. got {got[0][bad[0]]} want {want[k][bad[0]]} (one code step {step[k][bad[0]]})"
        worst = max(worst, float((err[tol[k] > 0] / tol[k][tol[k] > 0]).max()))
    print(f"matrix-core probe K {K}: largest error / bound {worst:.3f}")


# ---- c. every form at every format ----

# form: (prologue, epilogue, member rows, swiglu_single_round); boundaries of the q | k | v stack (21, 34) fall inside 8-row blocks
FORMS = {
    "store": (PRO_NONE, EPI_STORE, (77,), 0),
    "rms_qkv": (PRO_RMSNORM, EPI_STORE, (21, 13, 11), 0),
    "residual": (PRO_NONE, EPI_RESIDUAL, (77,), 0),
    "swiglu3": (PRO_NONE, EPI_SWIGLU, (52, 52), 0),
    "swiglu1": (PRO_NONE, EPI_SWIGLU, (52, 52), 1),
    "rms_swiglu3": (PRO_RMSNORM, EPI_SWIGLU, (52, 52), 0),
    "rms_swiglu1": (PRO_RMSNORM, EPI_SWIGLU, (52, 52), 1),
    "rms_argmax": (PRO_RMSNORM, EPI_ARGMAX, (77,), 0),
    "f32": (PRO_NONE, EPI_F32, (77,), 0),
}
# the branches beyond the class widths: the two-pass RMSNorm prologue (K > 4096), the rolled PRO_NONE staging (K > 16384)
LONG_K = {"rms_qkv": (5120,), "rms_swiglu1": (8192,), "rms_argmax": (8192,), "residual": (17408,)}


def form_inputs(rng, K, dt, pro, epi, N):
    x = rd.rand16(rng, (K,), dt, *X_EXP)
    nw = rd.rand16(rng, (K,), dt, -1, 0) if pro == PRO_RMSNORM else None
    resid = rd.rand16(rng, (N,), dt, -2, 1) if epi == EPI_RESIDUAL else None
    return x, nw, resid


@pytest.mark.parametrize("bits,group,dt", FORMATS)
def test_forms_at_every_format(omx, lib, bits, group, dt):
    """store, RMSNorm + store over a q | k | v stack, residual, SwiGLU (with / without RMSNorm, both roundings), RMSNorm + argmax and
    f32, at every class width of the format and at the long widths of LONG_K; the VALU kernel with separate and with interleaved
    scale | bias words (which must agree bit for bit), rolled_stage 1 against 0 bit for bit."""
    worst = 0.0
    mats = {}
    for name, (pro, epi, ns, single_round) in FORMS.items():
        for K in CLASS_K[bits] + LONG_K.get(name, ()):
            key = (K, ns)
            if key not in mats:     # a form's matrices are shared with the forms of the same heights
                mats[key] = [Mat(case_rng("form", bits, group, dt, K, ns, i), n, K, bits, group, dt) for i, n in enumerate(ns)]
            ms = mats[key]
            N = ns[0] if epi == EPI_SWIGLU else sum(ns)
            x, nw, resid = form_inputs(case_rng("x", name, bits, group, dt, K), K, dt, pro, epi, N)
            W = rq.words(bits, K, group)
            n = rq.valu_depth(bits, K, group, dt, x_span=4 if pro == PRO_NONE else None)
            outs = []
            for use_sb, rolled in ((0, 0), (1, 0), (1, 1)):
                got, row, a = launch(omx, lib, ms, x, pro, epi, nw=nw, resid=resid, single_round=single_round, use_sb=use_sb,
                                     rolled_stage=rolled)
                want_rb = 2      # N <= 8192: two rows per wave (SwiGLU: four, as row pairs)
                assert (a.route_kernel, a.route_bits, a.route_w, a.route_rb, a.route_f16s) == (VALU, bits, W, want_rb, int(dt == "f16")), name
                assert a.route_rows_per_wave == (4 if epi == EPI_SWIGLU else 2) and a.route_sb == sb_route(bits, W, use_sb)
                outs.append((got, row))
            # the reference once: the three launches must agree bit for bit, winner included
            worst = max(worst, check_form(outs[0][0], outs[0][1], ms, x, pro, epi, nw, resid, single_round, n) or 0.0)
            assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], f"{name} K {K}: interleaved and separate scale / bias words differ"
            assert np.array_equal(outs[1][0], outs[2][0]) and outs[1][1] == outs[2][1], f"{name} K {K}: rolled staging differs"
    print(f"forms {bits}-bit group {group} {dt}: largest error / bound {worst:.3f}")


# ---- d. argmax ----

def test_argmax_vocabulary_rows_per_wave_16(omx, lib):
    """N = 65552 >= 65536: sixteen rows per wave (asserted from the route), K = 512 (the 4-bit one-word class), a shard's row_offset in
    the key; the winner is the first maximum of the logits the launch itself stored"""
    N, K, off = 65552, 512, 1000
    rng = case_rng("vocab")
    mat = Mat(rng, N, K, 4, 64, "bf16")
    x, nw = rd.rand16(rng, (K,), "bf16", *X_EXP), rd.rand16(rng, (K,), "bf16", -1, 0)
    got, row, a = launch(omx, lib, [mat], x, PRO_RMSNORM, EPI_ARGMAX, nw=nw, use_sb=1, row_offset=off)
    assert (a.route_kernel, a.route_w, a.route_rows_per_wave, a.route_rb, a.route_blocks) == (VALU, 1, 16, 4, 1025)
    r = check_form(got, row, [mat], x, PRO_RMSNORM, EPI_ARGMAX, nw, None, 0, rq.valu_depth(4, K, 64, "bf16"), row_offset=off)
    print(f"argmax N {N}: largest error / bound {r:.3f}")


@pytest.mark.parametrize("kernel", [VALU, MFMA])
def test_argmax_ties_go_to_the_lower_row(omx, lib, kernel):
    """the row with the largest logit, copied to rows of another wave of its block and of another block: equal logits, and the lowest
    of the copies wins.  VALU: 8-row blocks of four 2-row waves; matrix cores: 16-row blocks."""
    N, K = 77, 1024
    rng = case_rng("ties", kernel)
    mat = Mat(rng, N, K, 4, 64, "bf16")
    x, nw = rd.rand16(rng, (K,), "bf16", *X_EXP), rd.rand16(rng, (K,), "bf16", -1, 0)
    # a row that wins by far more than any rounding -- the maximum code wherever the normalised activation and the group's scale
    # agree in sign, 0 elsewhere -- at row `top` and, copied, at rows 3 and 6 (one block, waves 1 and 3 of the VALU kernel) and 30, 70
    # (other blocks)
    top, copies = 41, [3, 6, 30, 70]
    xn, _ = rq.norm_slack_q(mat.q, mat.s, mat.b, 64, x, nw, EPS, "bf16")
    mat.q[top] = np.where(xn * np.repeat(mat.s[top].astype(np.float64), 64) > 0, 15, 0)
    for r in copies:
        mat.q[r], mat.s[r], mat.b[r] = mat.q[top], mat.s[top], mat.b[top]
    mfma = int(kernel == MFMA)
    got, row, a = launch(omx, lib, [mat], x, PRO_RMSNORM, EPI_ARGMAX, nw=nw, use_tiles=mfma, mfma=mfma, row_offset=5)
    assert a.route_kernel == kernel
    if kernel == MFMA:
        assert (a.route_ks, a.route_nbuf, a.route_blocks) == (1, 1, 5)
    n = rq.mfma_depth(K) if mfma else rq.valu_depth(4, K, 64, "bf16")
    r = check_form(got, row, [mat], x, PRO_RMSNORM, EPI_ARGMAX, nw, None, 0, n, row_offset=5)
    g = got[0]
    assert len({g[i] for i in copies + [top]}) == 1 and g[3] == g.max(), "identical rows must give identical, maximal logits"
    assert row == min(copies + [top]) + 5
    print(f"argmax ties kernel {kernel}: largest error / bound {r:.3f}")


def test_argmax_matrix_core_streaming(omx, lib):
    """the matrix-core kernel's streaming argmax at KS = 2: three task buffers per wave (NBUF = 3) once every block has at least three
    16-row tasks, so N comes from the grid a vocabulary-sized launch gets on this device (two blocks per CU).  The launch owns
    qgemv_grid(N) slots: those beyond its grid come back 0 ("no candidate") from all-ones."""
    from ominix_mlx_amd.engine import QGemvEx
    K = 2048
    probe = QGemvEx()
    probe.m[0].n, probe.N, probe.K, probe.bits, probe.group = 1 << 20, 1 << 20, K, 4, 64
    probe.pro, probe.epi, probe.use_tiles, probe.mfma, probe.dry_run = PRO_RMSNORM, EPI_ARGMAX, 1, 1, 1
    omx.check(lib.omx_debug_qgemv_ex(ctypes.byref(probe), None))
    grid = probe.route_blocks
    assert probe.route_kernel == MFMA and probe.route_nbuf == 3 and grid % 2 == 0
    N = grid * 3 * 16 + 5          # 3 grid + 1 row blocks, the last one ragged: some blocks run a fourth task
    slots = lib.omx_debug_qgemv_grid(N)
    assert slots > grid
    rng = case_rng("stream")
    mat = Mat(rng, N, K, 4, 64, "bf16")
    x, nw = rd.rand16(rng, (K,), "bf16", *X_EXP), rd.rand16(rng, (K,), "bf16", -1, 0)
    got, row, a = launch(omx, lib, [mat], x, PRO_RMSNORM, EPI_ARGMAX, nw=nw, use_tiles=1, mfma=1, row_offset=3, slot_cap=slots)
    assert (a.route_kernel, a.route_ks, a.route_nu, a.route_nbuf, a.route_blocks) == (MFMA, 2, 1, 3, grid)
    assert (a.keys[grid:slots] == 0).all() and (a.keys[:grid] != np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    r = check_form(got, row, [mat], x, PRO_RMSNORM, EPI_ARGMAX, nw, None, 0, rq.mfma_depth(K), row_offset=3)
    print(f"streaming argmax N {N} grid {grid}: largest error / bound {r:.3f}")


# ---- e. the matrix-core forms at every built KS ----

# ragged N where the form allows it: a stack's members but the last sit on 16-row blocks, SwiGLU heights are multiples of 16
MFORMS = {
    "store": (PRO_NONE, EPI_STORE, (40,), 0),
    "rms_qkv": (PRO_RMSNORM, EPI_STORE, (32, 16, 21), 0),
    "residual": (PRO_NONE, EPI_RESIDUAL, (40,), 0),
    "swiglu3": (PRO_NONE, EPI_SWIGLU, (48, 48), 0),
    "swiglu1": (PRO_NONE, EPI_SWIGLU, (48, 48), 1),
    "rms_swiglu3": (PRO_RMSNORM, EPI_SWIGLU, (48, 48), 0),
    "rms_swiglu1": (PRO_RMSNORM, EPI_SWIGLU, (48, 48), 1),
    "rms_argmax": (PRO_RMSNORM, EPI_ARGMAX, (40,), 0),
    "f32": (PRO_NONE, EPI_F32, (40,), 0),
}


@pytest.mark.parametrize("KS", [1, 2, 3, 4, 6, 8, 12])
def test_matrix_core_forms(omx, lib, KS):
    K, worst = KS * 1024, 0.0
    mats = {}
    for name, (pro, epi, ns, single_round) in MFORMS.items():
        if ns not in mats:
            mats[ns] = [Mat(case_rng("mform", KS, ns, i), n, K, 4, 64, "bf16") for i, n in enumerate(ns)]
        ms = mats[ns]
        N = ns[0] if epi == EPI_SWIGLU else sum(ns)
        x, nw, resid = form_inputs(case_rng("mx", name, KS), K, "bf16", pro, epi, N)
        got, row, a = launch(omx, lib, ms, x, pro, epi, nw=nw, resid=resid, single_round=single_round, use_tiles=1, mfma=1)
        assert (a.route_kernel, a.route_ks, a.route_nu, a.route_nbuf) == (MFMA, KS, 2 if epi == EPI_SWIGLU else 1, 1), name
        assert a.route_blocks == (N + 15) // 16
        r = check_form(got, row, ms, x, pro, epi, nw, resid, single_round, rq.mfma_depth(K))
        worst = max(worst, r or 0.0)
    print(f"matrix-core forms KS {KS}: largest error / bound {worst:.3f}")


# ---- f. expert selection ----

@pytest.mark.parametrize("bits", [3, 4])
def test_expert_selection(omx, lib, bits):
    """w_sel picks an expert of the stack per batch entry, entry j reads activation row j / 2 (x_div = 2); with w_sel_lo / w_sel_n only
    the experts [lo, lo + n) live here, at index w_sel - lo of the stack, and the other entries' rows keep the sentinel"""
    N, K, group, dt = 21, 2048, 64, "bf16"
    sel = np.array([0, 3, 1, 2, 3, 1], np.uint32)
    worst = 0.0
    for lo, cnt, E in ((0, 0, 4), (1, 2, 2)):
        rng = case_rng("experts", bits, lo, cnt)
        mat = Mat(rng, N, K, bits, group, dt, stack=E)
        x = rd.rand16(rng, (3, K), dt, *X_EXP)
        n = rq.valu_depth(bits, K, group, dt, x_span=4)
        outs = []
        for use_sb in (0, 1):
            got, _, a = launch(omx, lib, [mat], x, PRO_NONE, EPI_STORE, use_sb=use_sb, n_batch=len(sel), x_div=2, w_sel=sel, w_sel_lo=lo,
                               w_sel_n=cnt, n_experts=E)
            assert (a.route_kernel, a.route_bits, a.route_sb) == (VALU, bits, use_sb)
            for j, e in enumerate(sel):
                local = cnt == 0 or lo <= e < lo + cnt
                if not local:
                    assert (got[j] == SENT).all(), f"entry {j} (expert {e}) is not local: its row must stay untouched"
                    continue
                i = int(e) - (lo if cnt else 0)
                sl = slice(i * N, (i + 1) * N)
                exact, mag = rq.rows_ref(mat.q[sl], mat.s[sl], mat.b[sl], group, x[j // 2], rq.magic(bits, dt))
                rd.check_plain(got[j], exact, mag, n, 0.0, dt)
                worst = max(worst, rq.ratio(got[j], exact, mag, n, 0.0, dt))
            outs.append(got)
        assert np.array_equal(outs[0], outs[1])
    print(f"expert selection {bits}-bit: largest error / bound {worst:.3f}")
