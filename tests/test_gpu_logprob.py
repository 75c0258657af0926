"""Per-row log-probability of a target column (csrc/logprob.hip; omx_logprob_rows / _partial / _merge, ops.logprob_rows): against a
float64 log-softmax, its argmax against omx_argmax, a row's bits against its company and the panel widths, and the refusals."""
import functools

import numpy as np
import pytest

from logprob_rule import CHUNK, NO_TARGET, bf16_round, logprob64

pytestmark = pytest.mark.gpu

# one lane's vector, one full chunk, a chunk with an 8-column tail, a 128-column tail, Qwen3's vocabulary (148 chunks + 384 columns)
SHAPES = [(1, 8), (3, 1024), (5, 1032), (4, 2176), (2, 151936)]
TOL = 1e-4


def _comb(V):
    """one column in every 1024-column chunk (the tail chunk included), at a lane position that changes from chunk to chunk"""
    cols = []
    for j in range((V + CHUNK - 1) // CHUNK):
        width = min(CHUNK, V - j * CHUNK)
        cols.append(j * CHUNK + (37 * j + 5) % width)
    return np.array(cols)


@functools.lru_cache(maxsize=None)
def _case(T, V):
    """bf16 logits N(0, 4^2) [T, V] and targets [T].
    row 0: the comb columns at 24 and the LAST column at 25 -- the row's maximum lies in the tail chunk, and every chunk carries a
           visible share of the row's mass; its target lies in the tail chunk
    row 1: its maximum in column 0
    row min(2, T - 1) (T >= 2): no target (the sentinel)"""
    g = np.random.default_rng(1000 * T + V)
    x = bf16_round(4.0 * g.standard_normal((T, V)).astype(np.float32))
    t = g.integers(0, V, T).astype(np.uint32)
    x[0, _comb(V)] = 24.0
    x[0, V - 1] = 25.0
    t[0] = V - 3
    if T >= 2:
        x[1, 0] = x[1].max() + 2.0
        t[min(2, T - 1)] = NO_TARGET
    assert np.array_equal(x, bf16_round(x))
    x.setflags(write=False); t.setflags(write=False)
    return x, t, logprob64(x, t)


@pytest.mark.parametrize("T,V", SHAPES)
def test_logprob_rows_against_float64(omx, T, V):
    """|logprob - ref| <= 1e-4 and |lse - ref| <= 1e-4 against the float64 log-softmax of the same (exactly widened) bf16 logits.
    Where 1e-4 comes from: l = sum exp(x - m) is an f32 sum of <= 2^18 positive terms in a tree of 16-term lane runs (about 2e-6
    relative with the exp's own error), log adds an ulp, M + log L one rounding at |lse| < 64 (4e-6), the target logit is exact.
    1e-4 is over an order above that arithmetic.  It is far below what a dropped piece of these inputs costs -- checked here on the
    CPU: leaving out any single 1024-column chunk, the last 8-column vector, or any single comb column or the last column moves the
    reference of row 0 by more than 1e-3.  (No input can make EVERY single column worth 1e-3 of some row: a row's probabilities sum to
    1, so at most 1000 columns per row can carry that much, T * 1000 < V for three of these shapes -- hence the comb, which puts such
    a column into every chunk.)"""
    x, t, (lp_ref, lse_ref) = _case(T, V)
    # the power of the check, on the CPU
    comb = _comb(V)
    drops = [np.arange(j * CHUNK, min((j + 1) * CHUNK, V)) for j in range((V + CHUNK - 1) // CHUNK)] if V > CHUNK else []
    drops += [np.arange(V - 8, V)] if V > 8 else []
    drops += [np.array([c]) for c in comb] + [np.array([V - 1])]
    x0 = x[0].astype(np.float64)
    e0 = np.exp(x0 - x0.max())
    for d in drops:
        moved = -np.log1p(-e0[d].sum() / e0.sum())        # lse(row 0) - lse(row 0 without d)
        assert moved > 1e-3, f"dropping columns {d[0]}..{d[-1]} would move the reference by {moved:.2e} only"
    assert np.argmax(x[0]) // CHUNK == (V - 1) // CHUNK and (T < 2 or np.argmax(x[1]) == 0) and t[0] // CHUNK == (V - 1) // CHUNK
    Tn = omx.ops.Tensor
    lp, lse, greedy = omx.ops.logprob_rows(Tn.from_numpy(x), Tn.from_numpy(t, "u32"))
    lp, lse, greedy = lp.numpy(), lse.numpy(), greedy.numpy()
    print(f"T={T} V={V}: max |lse - ref| = {np.abs(lse - lse_ref).max():.3e}, max |logprob - ref| = {np.abs(lp - lp_ref).max():.3e}")
    assert np.abs(lse - lse_ref).max() <= TOL
    assert np.abs(lp - lp_ref).max() <= TOL
    if T >= 2:
        assert lp[min(2, T - 1)] == 0.0 and t[min(2, T - 1)] == NO_TARGET
    np.testing.assert_array_equal(greedy, np.argmax(x, axis=1))


def test_greedy_equals_argmax_on_ties(omx):
    """greedy is omx_argmax's answer bit for bit -- the first index of the maximum, also where the maximum appears twice in one chunk
    (row 0), in two different chunks (row 1), in the tail chunk and an earlier one (row 2), as +0 after -0 (row 4: equal as numbers,
    +0 the larger in omx_argmax's order)."""
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
    Tn = omx.ops.Tensor
    xd = Tn.from_numpy(x)
    want = omx.ops.argmax(xd).numpy()
    np.testing.assert_array_equal(want[:4], [2100, 1500, 3000, np.argmax(x[3])])
    _, _, greedy = omx.ops.logprob_rows(xd, Tn.from_numpy(np.full(5, NO_TARGET, np.uint32), "u32"))
    np.testing.assert_array_equal(greedy.numpy(), want)


def test_a_rows_bits_do_not_depend_on_its_company(omx):
    """(logprob, lse, greedy) of row r as uint32 bit patterns: alone, among 5 rows, and through the two-phase form with panels of 1024,
    2048 and V columns -- identical.  V = 5248 (5 chunks + 128), ld = 5376 > V; the padding columns hold 1e30 (never read as logits)."""
    V, ld, T = 5248, 5376, 5
    g = np.random.default_rng(11)
    x = np.full((T, ld), 1e30, np.float32)
    x[:, :V] = 4.0 * g.standard_normal((T, V)).astype(np.float32)
    x = bf16_round(x)
    t = g.integers(0, V, T).astype(np.uint32)
    t[3] = V - 5                                        # a target in the tail chunk
    Tn = omx.ops.Tensor
    xd, td = Tn.from_numpy(x), Tn.from_numpy(t, "u32")

    def bits(res, rows=slice(None)):
        lp, lse, greedy = res
        return np.stack([lp.numpy().view(np.uint32)[rows], lse.numpy().view(np.uint32)[rows], greedy.numpy()[rows]])

    among = bits(omx.ops.logprob_rows(xd, td, V=V))
    lp_ref, lse_ref = logprob64(x[:, :V], t)
    assert np.abs(among[1].view(np.float32) - lse_ref).max() <= TOL and np.abs(among[0].view(np.float32) - lp_ref).max() <= TOL
    for r in range(T):
        alone = bits(omx.ops.logprob_rows(xd.slice_rows(r * ld, (1, ld)), td.slice_rows(r, (1,)), V=V))
        np.testing.assert_array_equal(alone[:, 0], among[:, r], err_msg=f"row {r} alone")
    for panels in ([1024] * 5 + [128], [2048, 2048, 1152], [V]):
        np.testing.assert_array_equal(bits(omx.ops.logprob_rows(xd, td, V=V, panels=panels)), among, err_msg=f"panels {panels}")
        alone = bits(omx.ops.logprob_rows(xd.slice_rows(2 * ld, (1, ld)), td.slice_rows(2, (1,)), V=V, panels=panels))
        np.testing.assert_array_equal(alone[:, 0], among[:, 2], err_msg=f"row 2 alone, panels {panels}")


def test_a_target_beyond_the_row_is_not_a_number(omx):
    """a target >= V that is not the sentinel: logprob NaN (documented in include/omx.h), the row's lse and greedy as usual"""
    x, _, (_, lse_ref) = _case(3, 1024)
    t = np.array([5, 1024, 4000], np.uint32)
    Tn = omx.ops.Tensor
    lp, lse, greedy = omx.ops.logprob_rows(Tn.from_numpy(x), Tn.from_numpy(t, "u32"))
    lp = lp.numpy()
    assert np.isfinite(lp[0]) and np.isnan(lp[1]) and np.isnan(lp[2])
    assert np.abs(lse.numpy() - lse_ref).max() <= TOL
    np.testing.assert_array_equal(greedy.numpy(), np.argmax(x, axis=1))


def test_refusals_by_name(omx):
    Tn = omx.ops.Tensor
    t = Tn.from_numpy(np.zeros(2, np.uint32), "u32")
    with pytest.raises(omx.OmxError, match="omx_logprob_rows: V = 12 must be a positive multiple of 8"):
        omx.ops.logprob_rows(Tn.from_numpy(np.zeros((2, 16), np.float32)), t, V=12)
    with pytest.raises(omx.OmxError, match="omx_logprob_rows: ld = 1028 must be a multiple of 8"):
        omx.ops.logprob_rows(Tn.from_numpy(np.zeros((2, 1028), np.float32)), t, V=1024)
    for dt in ("f32", "f16"):
        with pytest.raises(omx.OmxError, match="omx_logprob_rows: dtype .* is not supported"):
            omx.ops.logprob_rows(Tn.from_numpy(np.zeros((2, 1024), np.float32), dt), t)
    with pytest.raises(omx.OmxError, match="omx_logprob_rows: ld = 1024 is below V = 2048"):
        omx.ops.logprob_rows(Tn.from_numpy(np.zeros((2, 1024), np.float32)), t, V=2048)
    with pytest.raises(omx.OmxError, match="omx_logprob_rows: V = 1048584 exceeds 2\\^20 columns"):
        omx.ops.logprob_rows(Tn((2, (1 << 20) + 8), "bf16"), t)
    with pytest.raises(omx.OmxError, match="omx_logprob_partial: columns"):
        omx.ops.logprob_rows(Tn.from_numpy(np.zeros((2, 2048), np.float32)), t, panels=[512, 1536])
