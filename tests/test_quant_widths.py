"""The MLX affine bit string at every width (CPU): a row of K elements is ceil(K*bits/32) little-endian u32 words, element j the
`bits`-wide field at bit j*bits, LSB first -- at 3 / 5 / 6 bits a field may straddle two words, and 32 elements fill exactly `bits`
words.  oracle/ref_core.quantize packs only widths that divide 32, so this module carries its own packer / unpacker (the GPU tests of
the 2 / 3 / 5 / 6-bit kernels import them) and pins it: known-answer words, and equality with the oracle's packing at 2 / 4 / 8 bits."""
import numpy as np
import pytest

from oracle import ref_core as rc


def pack_bits(q, bits):
    """q [..., K] integers < 2^bits -> packed u32 [..., K*bits/32] (K a multiple of 32)."""
    q = np.asarray(q, np.uint64)
    K = q.shape[-1]
    assert K % 32 == 0 and (q < (1 << bits)).all()
    pos = np.arange(K, dtype=np.uint64) * np.uint64(bits)
    word, off = pos // np.uint64(32), pos % np.uint64(32)
    out = np.zeros(q.shape[:-1] + (K * bits // 32,), np.uint64)
    lo = (q << off) & np.uint64(0xFFFFFFFF)
    hi = q >> (np.uint64(32) - off)               # the part of a straddling field that lands in the next word (0 otherwise)
    for j in range(K):
        out[..., int(word[j])] |= lo[..., j]
        if int(off[j]) + bits > 32:
            out[..., int(word[j]) + 1] |= hi[..., j]
    return out.astype(np.uint32)


def unpack_bits(packed, bits):
    """packed u32 [..., W] -> q [..., W*32/bits] (uint32)."""
    p = np.asarray(packed, np.uint32).astype(np.uint64)
    K = p.shape[-1] * 32 // bits
    pos = np.arange(K, dtype=np.uint64) * np.uint64(bits)
    word, off = (pos // np.uint64(32)).astype(np.int64), pos % np.uint64(32)
    nxt = np.minimum(word + 1, p.shape[-1] - 1)
    both = p[..., word] | (p[..., nxt] << np.uint64(32))
    both = np.where(off + np.uint64(bits) > np.uint64(32), both, p[..., word])
    return ((both >> off) & np.uint64((1 << bits) - 1)).astype(np.uint32)


def quantize_any(w, group, bits):
    """MLX affine quantisation at any width (the formula of ref_core.quantize, float32 throughout): (q [..., K], scale, bias) with q
    unpacked."""
    w = np.asarray(w, np.float32)
    f32 = np.float32
    n_bins = f32((1 << bits) - 1)
    g = w.reshape(*w.shape[:-1], w.shape[-1] // group, group)
    w_max, w_min = g.max(axis=-1), g.min(axis=-1)
    mask = np.abs(w_min) > np.abs(w_max)
    scale = np.maximum(((w_max - w_min).astype(f32) / n_bins).astype(f32), f32(1e-7))
    scale = np.where(mask, scale, -scale).astype(f32)
    edge = np.where(mask, w_min, w_max).astype(f32)
    q0 = np.rint((edge / scale).astype(f32))
    scale = np.where(q0 != 0, (edge / np.where(q0 != 0, q0, f32(1))).astype(f32), scale).astype(f32)
    bias = np.where(q0 == 0, f32(0), edge).astype(f32)
    q = np.clip(np.rint(((g - bias[..., None]).astype(f32) / scale[..., None]).astype(f32)), 0, n_bins).astype(np.uint32)
    return q.reshape(w.shape), scale, bias


def dequantize_any(q, scale, bias, group, dt="bf16"):
    """w = q * scale + bias per element in float32 (the device's expression: a product, then a sum), rounded once to `dt`."""
    s = np.repeat(np.asarray(scale, np.float32), group, axis=-1)
    b = np.repeat(np.asarray(bias, np.float32), group, axis=-1)
    v = (q.astype(np.float32) * s).astype(np.float32) + b
    return rc.rnd(v.astype(np.float32), dt).astype(np.float32) if dt != "f32" else v.astype(np.float32)


KAT = {
    3: ([j % 8 for j in range(32)], [0x88FAC688, 0xC688FAC6, 0xFAC688FA]),
    5: ([(3 * j + 2) % 32 for j in range(32)], [0x22E5A0A2, 0x6183BABD, 0xE2B27B12, 0xAA3903ED, 0xFF3369C1]),
    6: ([(5 * j + 1) % 64 for j in range(32)], [0x9540B181, 0x3BA991F6, 0x3070BDE3, 0xA581B591, 0x3FB9D2FA, 0x71748D20]),
}


@pytest.mark.parametrize("bits", [3, 5, 6])
def test_packer_reproduces_the_known_answer_words(bits):
    q, words = KAT[bits]
    got = pack_bits(np.array([q]), bits)[0]
    assert [int(v) for v in got] == words
    np.testing.assert_array_equal(unpack_bits(got, bits), q)
    if bits == 3:   # MLX writes 3 bits as 8 elements per 3 bytes: the same little-endian bytes
        assert bytes(got.astype("<u4").tobytes()[:3]) == bytes([0x88, 0xC6, 0xFA])


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("group", [32, 64, 128])
def test_packer_equals_the_oracle_at_widths_dividing_32(bits, group):
    w = np.random.default_rng(bits * 100 + group).standard_normal((24, 512)).astype(np.float32)
    rq, rs, rb = rc.quantize(w, group, bits)
    q, s, b = quantize_any(w, group, bits)
    np.testing.assert_array_equal(s, rs)
    np.testing.assert_array_equal(b, rb)
    np.testing.assert_array_equal(pack_bits(q, bits), rq)
    np.testing.assert_array_equal(unpack_bits(rq, bits), q)


@pytest.mark.parametrize("bits", [3, 5, 6])
@pytest.mark.parametrize("K", [512, 1536])
def test_unpack_inverts_pack(bits, K):
    q = np.random.default_rng(K + bits).integers(0, 1 << bits, size=(7, K)).astype(np.uint32)
    p = pack_bits(q, bits)
    assert p.shape == (7, K * bits // 32)
    np.testing.assert_array_equal(unpack_bits(p, bits), q)
