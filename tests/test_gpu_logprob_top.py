"""The top-n form of the per-row log-probability (csrc/logprob.hip; omx_logprob_rows_top / _top_partial / _top_merge,
ops.logprob_rows_top): the ids against a host sort by (logit descending, column ascending), the values against a float64 log-softmax,
the outputs it shares with omx_logprob_rows against that op's bits, a row's bits against its company and the panel widths, and the
refusals."""
import numpy as np
import pytest

from logprob_rule import CHUNK, NO_TARGET, bf16_round, logprob64, logsumexp64
from test_gpu_logprob import SHAPES, TOL, _case

pytestmark = pytest.mark.gpu

TOPS = (1, 5, 20)


def _orderable(x):
    """the samplers' total order on a float32 (random.hpp sample_key): larger float <=> larger word, +0 above -0"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _host_top(x, n):
    """[rows, n] column ids of each row by (logit descending, column ascending)"""
    key = _orderable(x)
    cols = np.arange(x.shape[1])
    return np.stack([np.lexsort((cols, -key[r]))[:n] for r in range(x.shape[0])]).astype(np.uint32)


def _run(omx, x, t, n, **kw):
    Tn = omx.ops.Tensor
    return [a.numpy() for a in omx.ops.logprob_rows_top(Tn.from_numpy(x), Tn.from_numpy(t, "u32"), n, **kw)]


@pytest.mark.parametrize("T,V", SHAPES)
def test_ids_values_and_shared_outputs(omx, T, V):
    """For top_n in {1, 5, 20} (where V allows; (1, 8) runs top_n = 8 too): top_ids equal the host sort exactly; |top_logprobs - ref|
    <= 1e-4 against the float64 log-softmax of the widened bf16 row (TOL of test_gpu_logprob.py: its derivation bounds |lse - ref|,
    the logit is exact, and the one f32 subtraction more rounds at |value| < 64, 4e-6); logprobs, lse and greedy carry the bits of
    ops.logprob_rows on the same inputs."""
    x, t, _ = _case(T, V)
    if V == 151936:
        # the check has teeth at this size: ties inside the top 20 (bf16 spacing at 16 is 0.125) and an entry from the tail chunk
        for r in range(T):
            top = _host_top(x[r:r + 1], 20)[0]
            assert len(np.unique(x[r, top])) < 20, f"row {r}: no tie inside its top 20"
        assert (_host_top(x[:1], 20)[0] >= (V - 1) // CHUNK * CHUNK).any(), "row 0: no entry from the tail chunk"
    Tn = omx.ops.Tensor
    base = [a.numpy() for a in omx.ops.logprob_rows(Tn.from_numpy(x), Tn.from_numpy(t, "u32"))]
    lse_ref = logsumexp64(x)
    for n in sorted({k for k in TOPS if k <= V} | ({8} if V == 8 else set())):
        lp, lse, greedy, ids, tlp = _run(omx, x, t, n)
        assert ids.shape == (T, n) and tlp.shape == (T, n)
        np.testing.assert_array_equal(ids, _host_top(x, n), err_msg=f"top_n {n}")
        ref = np.take_along_axis(x.astype(np.float64), ids.astype(np.int64), axis=1) - lse_ref[:, None]
        print(f"T={T} V={V} top_n={n}: max |top_logprobs - ref| = {np.abs(tlp - ref).max():.3e}")
        assert np.abs(tlp - ref).max() <= TOL
        np.testing.assert_array_equal(ids[:, 0], greedy)
        for got, want, what in zip((lp, lse, greedy), base, ("logprobs", "lse", "greedy")):
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"{what}, top_n {n}")


def test_directed_rows(omx):
    """V = 5248 (5 chunks + 128 columns), ld = 5376 with 1e30 in the padding, top_n = 5.
    row 0: 40, 39, 38 lead and 30 stands three times -- two places are left: the lowest two ids win
    row 1: the same value in two chunks (and twice in one): ascending ids
    row 2: its best entry and its fourth lie in the 128-column tail
    every row: no padding column is ever returned."""
    V, ld, n = 5248, 5376, 5
    g = np.random.default_rng(5)
    x = np.full((3, ld), 1e30, np.float32)
    x[:, :V] = 4.0 * g.standard_normal((3, V)).astype(np.float32)
    x = bf16_round(x)
    x[0, [700, 3100, 4500]] = [40.0, 39.0, 38.0]
    x[0, [4100, 2050, 900]] = 30.0
    x[1, [3333, 1200, 1100, 4800]] = 33.0
    x[2, [5247, 10, 20, 5130]] = [50.0, 49.0, 48.0, 47.0]
    t = np.full(3, NO_TARGET, np.uint32)
    lp, lse, greedy, ids, tlp = _run(omx, x, t, n, V=V)
    np.testing.assert_array_equal(ids[0], [700, 3100, 4500, 900, 2050])
    np.testing.assert_array_equal(ids[1][:4], [1100, 1200, 3333, 4800])
    np.testing.assert_array_equal(ids[2][:4], [5247, 10, 20, 5130])
    assert (ids < V).all()
    np.testing.assert_array_equal(ids, _host_top(x[:, :V], n))
    ref = np.take_along_axis(x[:, :V].astype(np.float64), ids.astype(np.int64), axis=1) - logsumexp64(x[:, :V])[:, None]
    assert np.abs(tlp - ref).max() <= TOL


def test_first_entry_equals_argmax_on_signed_zeros(omx):
    """the rows of test_gpu_logprob.test_greedy_equals_argmax_on_ties (a maximum twice in a chunk, in two chunks, in the tail and an
    earlier chunk, +0 after -0): top_ids[:, 0] is omx_argmax's answer, and the -0 / +0 row lists +0 (column 3000) before -0 (100)."""
    V = 5248
    g = np.random.default_rng(7)
    x = bf16_round(4.0 * g.standard_normal((5, V)).astype(np.float32))
    top = x.max() + 1.0
    x[0, [2900, 2100]] = top
    x[1, [4200, 1500]] = top
    x[2, [5200, 3000]] = top
    x[4] = -np.abs(x[4]) - 1.0
    x[4, 100] = -0.0
    x[4, 3000] = 0.0
    want = omx.ops.argmax(omx.ops.Tensor.from_numpy(x)).numpy()
    lp, lse, greedy, ids, tlp = _run(omx, x, np.full(5, NO_TARGET, np.uint32), 2)
    np.testing.assert_array_equal(ids[:, 0], want)
    np.testing.assert_array_equal(ids[:3], [[2100, 2900], [1500, 4200], [3000, 5200]])
    np.testing.assert_array_equal(ids[4], [3000, 100])
    np.testing.assert_array_equal(ids, _host_top(x, 2))


def test_a_rows_bits_do_not_depend_on_its_company(omx):
    """All five outputs of row r as uint32 bit patterns: alone, among 5 rows, and through the two-phase form with panels of 1024, 2048
    and V columns -- identical.  V = 5248, ld = 5376 > V with 1e30 in the padding, top_n = 20."""
    V, ld, T, n = 5248, 5376, 5, 20
    g = np.random.default_rng(11)
    x = np.full((T, ld), 1e30, np.float32)
    x[:, :V] = 4.0 * g.standard_normal((T, V)).astype(np.float32)
    x = bf16_round(x)
    t = g.integers(0, V, T).astype(np.uint32)
    t[3] = V - 5
    Tn = omx.ops.Tensor
    xd, td = Tn.from_numpy(x), Tn.from_numpy(t, "u32")

    def bits(res, rows=slice(None)):
        return np.concatenate([a.numpy().view(np.uint32).reshape(a.shape[0], -1)[rows] for a in res], axis=1)

    among = bits(omx.ops.logprob_rows_top(xd, td, n, V=V))
    np.testing.assert_array_equal(among[:, 3:3 + n], _host_top(x[:, :V], n))
    for r in range(T):
        alone = bits(omx.ops.logprob_rows_top(xd.slice_rows(r * ld, (1, ld)), td.slice_rows(r, (1,)), n, V=V))
        np.testing.assert_array_equal(alone[0], among[r], err_msg=f"row {r} alone")
    for panels in ([1024] * 5 + [128], [2048, 2048, 1152], [V]):
        np.testing.assert_array_equal(bits(omx.ops.logprob_rows_top(xd, td, n, V=V, panels=panels)), among, err_msg=f"panels {panels}")
        alone = bits(omx.ops.logprob_rows_top(xd.slice_rows(2 * ld, (1, ld)), td.slice_rows(2, (1,)), n, V=V, panels=panels))
        np.testing.assert_array_equal(alone[0], among[2], err_msg=f"row 2 alone, panels {panels}")


def test_refusals_by_name(omx):
    Tn = omx.ops.Tensor
    t = Tn.from_numpy(np.zeros(2, np.uint32), "u32")
    x = Tn.from_numpy(np.zeros((2, 1024), np.float32))
    for n in (0, 21):
        with pytest.raises(omx.OmxError, match=f"omx_logprob_rows_top: top_n = {n} is outside 1..min\\(20, V = 1024\\)"):
            omx.ops.logprob_rows_top(x, t, n)
    with pytest.raises(omx.OmxError, match="omx_logprob_rows_top: top_n = 9 is outside 1..min\\(20, V = 8\\)"):
        omx.ops.logprob_rows_top(Tn.from_numpy(np.zeros((2, 8), np.float32)), t, 9)
    for dt in ("f32", "f16"):
        with pytest.raises(omx.OmxError, match="omx_logprob_rows_top: dtype .* is not supported"):
            omx.ops.logprob_rows_top(Tn.from_numpy(np.zeros((2, 1024), np.float32), dt), t, 5)
    with pytest.raises(omx.OmxError, match="omx_logprob_rows_top: V = 12 must be a positive multiple of 8"):
        omx.ops.logprob_rows_top(Tn.from_numpy(np.zeros((2, 16), np.float32)), t, 5, V=12)
    with pytest.raises(omx.OmxError, match="omx_logprob_rows_top: ld = 1024 is below V = 2048"):
        omx.ops.logprob_rows_top(x, t, 5, V=2048)
    with pytest.raises(omx.OmxError, match="omx_logprob_top_partial: columns"):
        omx.ops.logprob_rows_top(Tn.from_numpy(np.zeros((2, 2048), np.float32)), t, 5, panels=[512, 1536])
