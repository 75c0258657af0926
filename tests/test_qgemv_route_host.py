"""CPU-only: the route launch_qgemv takes, through omx_debug_qgemv_ex's dry run (no device, no pointer read) -- the W class, RB,
rows_per_wave, blocks and LDS bytes for a table of launches; the launchers' refusals as error text; and, for every argmax launch the
engines make, blocks == qgemv_grid(N): the number of partial keys they reduce, whatever the tuning knobs say."""
import ctypes

import pytest

PRO_NONE, PRO_RMSNORM = 0, 1
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU, EPI_ARGMAX, EPI_F32 = 0, 1, 2, 3, 4
VALU, STACK, MFMA = 1, 2, 3


def dry(omx, members, K, pro, epi, bits=0, group=0, N=None, **kw):
    """members: (n, bits, group) each (0: the launch's format); returns the QGemvEx with its route"""
    from ominix_mlx_amd.engine import QGemvEx
    a = QGemvEx()
    for i, (n, b, g) in enumerate(members):
        a.m[i].n, a.m[i].bits, a.m[i].group = n, b, g
    a.N = N if N is not None else (members[0][0] if epi == EPI_SWIGLU else sum(m[0] for m in members))
    a.K, a.bits, a.group, a.pro, a.epi, a.eps, a.dry_run = K, bits, group, pro, epi, 1e-6, 1
    for k, v in kw.items():
        setattr(a, k, v)
    omx.check(omx.lib.omx_debug_qgemv_ex(ctypes.byref(a), None))
    return a


def route(a):
    return (a.route_kernel, a.route_bits, a.route_w, a.route_rb, a.route_rows_per_wave, a.route_blocks, a.route_lds_bytes)


def lds(K, epl):
    return K * 2 + (K // epl) * 4 + 64


# (bits, group, K, N, pro, epi) -> (W, RB, rows_per_wave, blocks, lane chunk)
TABLE = [
    ((4, 64, 2048, 520, PRO_NONE, EPI_STORE), (4, 2, 2, 65, 32)),
    ((4, 64, 1024, 520, PRO_NONE, EPI_STORE), (2, 2, 2, 65, 16)),
    ((4, 64, 512, 520, PRO_NONE, EPI_STORE), (1, 2, 2, 65, 8)),
    ((4, 32, 2048, 77, PRO_RMSNORM, EPI_STORE), (4, 2, 2, 10, 32)),
    ((4, 128, 17408, 77, PRO_NONE, EPI_RESIDUAL), (2, 2, 2, 10, 16)),      # 17408 = 17 x 1024: the two-word class
    ((8, 64, 1024, 21, PRO_NONE, EPI_F32), (4, 2, 2, 3, 16)),
    ((8, 64, 512, 21, PRO_NONE, EPI_F32), (2, 2, 2, 3, 8)),
    ((8, 32, 8192, 9000, PRO_RMSNORM, EPI_STORE), (4, 4, 4, 563, 16)),
    ((2, 32, 2048, 77, PRO_NONE, EPI_STORE), (2, 2, 2, 10, 32)),
    ((3, 64, 2560, 77, PRO_NONE, EPI_STORE), (3, 2, 2, 10, 32)),
    ((5, 128, 2560, 52, PRO_RMSNORM, EPI_SWIGLU), (5, 2, 4, 4, 32)),
    ((6, 64, 5120, 300, PRO_NONE, EPI_SWIGLU), (6, 2, 4, 19, 32)),
    ((4, 64, 512, 65552, PRO_RMSNORM, EPI_ARGMAX), (1, 4, 16, 1025, 8)),
    ((6, 64, 2048, 8193, PRO_RMSNORM, EPI_ARGMAX), (6, 4, 4, 513, 32)),
    ((3, 64, 2048, 8192, PRO_RMSNORM, EPI_ARGMAX), (3, 2, 2, 1024, 32)),
]


@pytest.mark.parametrize("case,want", TABLE)
def test_valu_route_table(omx, case, want):
    bits, group, K, N, pro, epi = case
    W, RB, rpw, blocks, epl = want
    members = [(N, 0, 0)] * (2 if epi == EPI_SWIGLU else 1)
    for f16 in (0, 1):
        for use_sb in (0, 1):
            a = dry(omx, members, K, pro, epi, bits, group, scales_f16=f16, use_sb=use_sb)
            assert route(a) == (VALU, bits, W, RB, rpw, blocks, lds(K, epl))
            # the interleaved-words kernel exists for the four-word class and the chunked widths only
            assert (a.route_sb, a.route_f16s) == (int(bool(use_sb) and (W == 4 or bits in (2, 3, 5, 6))), f16)
            assert (a.route_ks, a.route_nu, a.route_nbuf) == (0, 0, 0)


def test_matrix_core_and_stack_routes(omx):
    def mlds(KS, NU):
        return KS * 1024 * 2 + KS * 16 * 4 + 2 * NU * KS * 16 * 4 + 32 * 8 + 64

    a = dry(omx, [(40, 0, 0)], 4096, PRO_NONE, EPI_STORE, 4, 64, use_tiles=1, mfma=1)
    assert route(a) == (MFMA, 4, 4, 0, 0, 3, mlds(4, 1)) and (a.route_ks, a.route_nu, a.route_nbuf, a.route_sb) == (4, 1, 1, 1)
    a = dry(omx, [(48, 0, 0)] * 2, 12288, PRO_RMSNORM, EPI_SWIGLU, 4, 64, use_tiles=1, mfma=1)
    assert route(a) == (MFMA, 4, 4, 0, 0, 3, mlds(12, 2)) and (a.route_ks, a.route_nu, a.route_nbuf) == (12, 2, 1)
    # what keeps a launch off the matrix cores: the mode, no tiles, another group, float16 triplets, a batch, a stack boundary or a
    # SwiGLU height off the 16-row blocks, fewer than 16 rows
    for kw, members, epi in (({"mfma": 0}, [(40, 0, 0)], EPI_STORE), ({"use_tiles": 0}, [(40, 0, 0)], EPI_STORE),
                             ({"group": 128}, [(40, 0, 0)], EPI_STORE), ({"scales_f16": 1}, [(40, 0, 0)], EPI_STORE),
                             ({"n_batch": 2, "x_div": 1}, [(40, 0, 0)], EPI_STORE), ({}, [(24, 0, 0), (16, 0, 0)], EPI_STORE),
                             ({}, [(40, 0, 0)] * 2, EPI_SWIGLU), ({}, [(15, 0, 0)], EPI_STORE)):
        args = {"use_tiles": 1, "mfma": 1, "bits": 4, "group": 64}
        args.update(kw)
        a = dry(omx, members, 4096, PRO_NONE, epi, **args)
        assert a.route_kernel == VALU and a.route_w == 4, kw
    # members of different formats: one launch of the stack kernel, each member on a block boundary, LDS for the narrowest lane chunk
    a = dry(omx, [(21, 4, 64), (13, 8, 64), (11, 3, 32)], 2048, PRO_RMSNORM, EPI_STORE, 4, 64, use_sb=1)
    assert route(a) == (STACK, 0, 0, 2, 2, 3 + 2 + 2, lds(2048, 16)) and a.route_sb == 1
    # ... and members that agree are the one-format kernel
    a = dry(omx, [(21, 4, 64), (13, 4, 64), (11, 0, 0)], 2048, PRO_RMSNORM, EPI_STORE, 4, 64)
    assert route(a)[:3] == (VALU, 4, 4)


@pytest.mark.parametrize("members,K,pro,epi,kw,text", [
    ([(21, 0, 0)], 256, PRO_NONE, EPI_STORE, {"bits": 8, "group": 64}, r"K=256 unsupported for 8-bit group 64 \(K must be a multiple of 512\)"),
    ([(21, 0, 0)], 768, PRO_NONE, EPI_STORE, {"bits": 4, "group": 64}, r"K=768 unsupported for 4-bit group 64 \(K must be a multiple of 512\)"),
    ([(21, 0, 0)], 2048, PRO_NONE, EPI_STORE, {"bits": 7, "group": 64}, r"bits must be 2, 3, 4, 5, 6 or 8 \(got 7\)"),
    ([(21, 0, 0)], 2048, PRO_NONE, EPI_STORE, {"bits": 4, "group": 96}, r"row width \(2048\) must be divisible by the group size \(96\)"),
    ([(21, 0, 0)], 2048, PRO_RMSNORM, EPI_RESIDUAL, {"bits": 4, "group": 64}, r"unsupported prologue/epilogue combination 1/1"),
    ([(21, 0, 0)], 2048, PRO_RMSNORM, EPI_F32, {"bits": 3, "group": 64}, r"unsupported prologue/epilogue combination 1/4"),
    ([(21, 4, 64), (21, 8, 64)], 2048, PRO_NONE, EPI_SWIGLU, {}, r"gate \(4-bit group 64\) and up \(8-bit group 64\) must share a format"),
    ([(21, 4, 64), (13, 8, 64)], 2048, PRO_NONE, EPI_RESIDUAL, {}, r"a stack of mixed formats is a plain store of one activation row on bf16 triplets"),
    ([(21, 4, 64), (13, 8, 64)], 2048, PRO_NONE, EPI_STORE, {"scales_f16": 1}, r"a stack of mixed formats is a plain store"),
    ([(21, 4, 64), (13, 8, 64)], 256, PRO_NONE, EPI_STORE, {}, r"K=256 unsupported for 4-bit group 64 \(member 0 of a mixed stack\)"),
    ([(21, 0, 0), (13, 0, 0)], 2048, PRO_NONE, EPI_STORE, {"bits": 4, "group": 64, "N": 40}, r"the members hold 34 rows, N = 40"),
])
def test_refusals(omx, members, K, pro, epi, kw, text):
    with pytest.raises(omx.OmxError, match=text):
        dry(omx, members, K, pro, epi, **kw)


def test_real_launch_is_refused_before_it_runs_without_what_it_reads(omx):
    """not a dry run, and no buffers: refused on the host (nothing is launched, so this needs no device either)"""
    from ominix_mlx_amd.engine import QGemvEx
    a = QGemvEx()
    a.m[0].n, a.N, a.K, a.bits, a.group = 21, 21, 2048, 4, 64
    with pytest.raises(omx.OmxError, match="member 0 has no weights / scales"):
        omx.check(omx.lib.omx_debug_qgemv_ex(ctypes.byref(a), None))


@pytest.mark.parametrize("knobs", [{}, {"OMX_QGEMV_RPW_SMALL": "4"}, {"OMX_QGEMV_RPW_LONGK": "8"},
                                   {"OMX_QGEMV_RPW_SMALL": "4", "OMX_QGEMV_RPW_LONGK": "4", "OMX_QGEMV_RPW_GU": "8"}])
def test_argmax_blocks_are_the_partials_the_engines_reduce(omx, monkeypatch, knobs):
    """The engines size and reduce qgemv_grid(N) argmax partials (engine.hip, mlxc_lazy.hpp), a function of N alone; the launch's
    rows_per_wave honoured OMX_QGEMV_RPW_SMALL / _LONGK for EPI_ARGMAX too, so with RPW_SMALL=4 a vocabulary of N <= 8192 wrote half
    the partials the reduction read.  An argmax launch now takes no knob."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    lib = omx.lib
    lib.omx_debug_qgemv_grid.restype, lib.omx_debug_qgemv_grid.argtypes = ctypes.c_int, [ctypes.c_int]
    for N in (2048, 8191, 8192, 8193, 32000, 65535, 65536, 151936):
        for bits, K in ((4, 512), (4, 1024), (4, 4096), (8, 2048), (3, 2560), (6, 12288)):
            a = dry(omx, [(N, 0, 0)], K, PRO_RMSNORM, EPI_ARGMAX, bits, 64, use_sb=1)
            assert a.route_blocks == lib.omx_debug_qgemv_grid(N), (N, bits, K, knobs)
    # the knobs still reach the launches they are for
    a = dry(omx, [(520, 0, 0)], 2048, PRO_NONE, EPI_STORE, 4, 64)
    assert a.route_rows_per_wave == (4 if knobs.get("OMX_QGEMV_RPW_SMALL") == "4" else 2)
