"""CPU-only: the packed GEMV's float64 reference and derived bound (oracle/ref_qdecode.py) against a plain float32 emulation of the
kernel's lane order, on the inputs tests/test_gpu_qgemv_forms.py uses, at every format -- the emulation stays inside the bound, three
deliberately wrong emulations leave it.  Shown before any GPU time is spent: the bound is neither too tight nor blind."""
import zlib

import numpy as np
import pytest

from oracle import ref_decode as rd
from oracle import ref_qdecode as rq

BITS, GROUPS, DTS = (2, 3, 4, 5, 6, 8), (32, 64, 128), ("bf16", "f16")
# the smallest K of every W class, and the chunked widths' K with a partly live second step
KS = {2: (2048, 2560), 3: (2048, 2560), 5: (2048, 2560), 6: (2048, 2560), 4: (2048, 1024, 512), 8: (1024, 512)}
N = 24


def case_rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def test_words_classes():
    """the W classes the GPU tests name, as qgemv_words gives them"""
    assert [rq.words(4, K, 64) for K in (2048, 1024, 512)] == [4, 2, 1]
    assert [rq.words(8, K, 64) for K in (1024, 512)] == [4, 2]
    assert rq.words(4, 2048, 32) == 4 and rq.words(8, 1024, 32) == 4
    assert [rq.words(b, 2560, 32) for b in rq.CHUNKED] == [2, 3, 5, 6]
    assert rq.words(8, 256, 64) == 0 and rq.words(4, 2560, 64) == 1 and rq.words(3, 48, 32) == 0
    assert rq.steps(3, 2560, 64) == 2 and rq.steps(4, 2048, 64) == 1 and rq.steps(4, 17408, 64) == 17


def test_pack_layout():
    """element j is the field at bit j * bits of the little-endian bit string, straddling fields included"""
    rng = np.random.default_rng(3)
    for bits in BITS:
        q = rng.integers(0, 1 << bits, size=(3, 64), dtype=np.uint8)
        w = rq.pack(q, bits)
        assert w.shape == (3, 64 * bits // 32) and w.dtype == np.uint32
        for r in range(3):
            big = sum(int(v) << (32 * i) for i, v in enumerate(w[r]))
            assert [(big >> (j * bits)) & ((1 << bits) - 1) for j in range(64)] == q[r].tolist()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("bits", BITS)
def test_emulation_inside_bound_and_mutants_outside(bits, group, dt):
    worst = 0.0
    for K in KS[bits]:
        rng = case_rng("ref", bits, group, dt, K)
        q, s, b = rq.make_triplet(rng, N, K, bits, group, dt)
        x = rd.rand16(rng, (K,), dt, -3, 0)
        m = rq.magic(bits, dt)
        n = rq.valu_depth(bits, K, group, dt, x_span=4)   # x over the binades -3 .. 0
        exact, mag = rq.rows_ref(q, s, b, group, x, m)
        assert np.allclose(exact, rq.dequant(q, s, b, group) @ x.astype(np.float64), rtol=1e-12, atol=1e-12)
        got = rq.emulate_valu(q, s, b, group, x, bits, dt)
        rq.check_f32(got, exact, mag, n)
        worst = max(worst, rq.ratio(got, exact, mag, n))
        # the 16-bit store on top: ref_decode's plain check holds too
        rd.check_plain(rd.rnd(got, dt), exact, mag, n, 0.0, dt)

        row = 5
        e = rq.epl(bits, K, group)
        # one code off by one, at the row's largest |s x| (a single small element is the one-hot probe's business, not this bound's)
        k = int(np.argmax(np.abs(np.repeat(s[row], group) * x)))
        with pytest.raises(AssertionError):
            rq.check_f32(rq.emulate_valu(q, s, b, group, x, bits, dt, code_bump=(row, k)), exact, mag, n)
        # the neighbouring group's scale for one lane chunk, feeding the product and the fold alike as the kernel's one `scl` does:
        # the row moves by (s' - s) sum q x of the chunk -- at the chunk where that is largest (a small one is the probe's business too)
        G = K // group
        gi = np.arange(K // e) * e // group
        other = np.where(gi + 1 < G, gi + 1, gi - 1)
        c = int(np.argmax(np.abs((s[row, other] - s[row, gi]) * (q[row] * x.astype(np.float64)).reshape(-1, e).sum(1))))
        with pytest.raises(AssertionError):
            rq.check_f32(rq.emulate_valu(q, s, b, group, x, bits, dt, scale_shift_chunk=(row, c)), exact, mag, n)
        # the m s fold dropped (only where there is a magic to fold)
        if m:
            with pytest.raises(AssertionError):
                rq.check_f32(rq.emulate_valu(q, s, b, group, x, bits, dt, drop_fold=True), exact, mag, n)
    print(f"bits {bits} group {group} {dt}: worst emulation error / bound {worst:.3f}")


def test_probe_tolerance_resolves_one_code_step():
    """the one-hot probe's tolerance is below 2^-10 of one code step for every element of every format"""
    for bits in BITS:
        for dt in DTS:
            q, s, b = rq.make_triplet(case_rng("probe", bits, dt), 21, 2048, bits, 64, dt)
            want, tol, step = rq.probe_ref(q, s, b, 64, rq.magic(bits, dt))
            assert want.shape == (2048, 21) and (tol < 2.0 ** -10 * step).all()
