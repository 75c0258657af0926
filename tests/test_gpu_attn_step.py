"""GPU: the step attention (csrc/attn_step.hip: q/k RMSNorm, RoPE, KV append, split-KV attention, split merge in one launch) at
kernel level against float64 (oracle/ref_decode.py), through omx_debug_attn_step on caller-owned slabs and granules -- positions
across split and bucket boundaries, the engine's split plans and explicit ones (1 to 3 gather batches), score spikes that force the
merge's rescale, and one granule buffer reused across (step, layer) tags."""
import ctypes
import zlib

import numpy as np
import pytest

from oracle import ref_decode as rd

pytestmark = pytest.mark.gpu

EPS = 1e-6
CAP = 8200
# name: (H, Hkv, D, q/k norm, dtype)
GEOMS = {
    "qwen3_8b": (32, 8, 128, True, "bf16"),
    "g8": (64, 8, 128, True, "bf16"),
    "g7": (28, 4, 128, True, "bf16"),
    "g3": (24, 8, 128, True, "bf16"),
    "g1": (8, 8, 128, True, "bf16"),
    "d64": (14, 2, 64, True, "bf16"),
    "no_qk_norm": (32, 8, 128, False, "bf16"),
    "f16": (32, 8, 128, True, "f16"),
}


@pytest.fixture(scope="module")
def lib(omx):
    from ominix_mlx_amd import engine
    assert "omx_debug_attn_step" in engine.ENGINE_SIGNATURES
    return omx.lib


def engine_tk_max(pos, cap=CAP):
    """prepare_step's context bucket: 1024-token buckets up to 8 k, 4096 beyond, capped at the cache"""
    tk = pos + 1
    gran = 1024 if tk <= 8192 else 4096
    return min(cap, -(-tk // gran) * gran)


class Slabs:
    """device K / V slabs [Hkv, cap, D], their host mirror, one granule buffer and its tag sequence, for one geometry"""

    def __init__(self, omx, lib, name, H, Hkv, D, qk_norm, dt, rng, cap=CAP):
        from ominix_mlx_amd.ops import Tensor
        self.omx, self.lib, self.T = omx, lib, Tensor
        self.H, self.Hkv, self.D, self.dt, self.cap, self.qk_norm = H, Hkv, D, dt, cap, qk_norm
        self.K = rd.rand16(rng, (Hkv, cap, D), dt, -2, 0)
        self.V = rd.rand16(rng, (Hkv, cap, D), dt, -2, 0)
        self.dK, self.dV = Tensor.from_numpy(self.K, dt), Tensor.from_numpy(self.V, dt)
        self.n_gran = H * 48 * (D + 2)
        self.gran = Tensor.from_numpy(np.zeros(self.n_gran * 2, np.uint32), "u32")   # (tag 0 is never a call's tag)
        self.seq = 1

    def call(self, qkv, q_nw, k_nw, pos, chunk=0, nsplit=0, tk_max=0, seq=None, tag_mul=1, tag_add=1):
        from ominix_mlx_amd.engine import AttnStepDbg
        T, dt = self.T, self.dt
        H, Hkv, D = self.H, self.Hkv, self.D
        rope = rd.rope_cur(pos, D)
        keep = [T.from_numpy(qkv, dt), T.from_numpy(rope, "f32")]
        if q_nw is not None:
            keep += [T.from_numpy(q_nw, dt), T.from_numpy(k_nw, dt)]
        out = T((H * D,), dt)
        a = AttnStepDbg(qkv=keep[0].ptr, k=self.dK.ptr, v=self.dV.ptr, H=H, Hkv=Hkv, D=D, cap=self.cap, scale=float(np.float32(D ** -0.5)),
                        eps=EPS, q_norm_w=keep[2].ptr if q_nw is not None else None, k_norm_w=keep[3].ptr if q_nw is not None else None,
                        rope_cur=keep[1].ptr, granules=self.gran.ptr, granules_n=self.n_gran, pos=pos,
                        seq=self.seq if seq is None else seq, tag_mul=tag_mul, tag_add=tag_add, f16=int(dt == "f16"),
                        chunk=chunk, nsplit=nsplit, tk_max=tk_max, out=out.ptr)
        if seq is None:
            self.seq += 1
        self.omx.check(self.lib.omx_debug_attn_step(ctypes.byref(a), None))
        assert a.abort_flag == 0, "a consumer gave up waiting for a split's granules"
        return out.numpy().astype(np.float64).reshape(H, D), a, rope

    def check(self, got, a, rope, qkv, q_nw, k_nw, pos):
        """slab row pos of K = the modelled rope(rmsnorm(k_raw)) up to the documented flips, of V = v_raw bit for bit, every other
        row unchanged; the output within the derived bound of float64 attention over rows [0, pos]"""
        H, Hkv, D, dt = self.H, self.Hkv, self.D, self.dt
        Kd = self.dK.numpy().reshape(Hkv, self.cap, D)
        Vd = self.dV.numpy().reshape(Hkv, self.cap, D)
        ref, bound, k_c, _ = rd.attn_step_ref(qkv, self.K, self.V, pos, H, Hkv, D, q_nw, k_nw, rope, EPS, D ** -0.5, dt, a.chunk, a.nsplit)
        rd.check_row(Kd[:, pos].astype(np.float64), k_c, "appended K row")
        v_raw = qkv[(H + Hkv) * D:].reshape(Hkv, D)
        np.testing.assert_array_equal(Vd[:, pos], v_raw, err_msg="appended V row")
        other = np.ones(self.cap, bool)
        other[pos] = False
        assert np.array_equal(Kd[:, other], self.K[:, other]) and np.array_equal(Vd[:, other], self.V[:, other]), "rows other than pos changed"
        rd.check_attn(got, ref, bound, dt)
        self.K, self.V = Kd, Vd

    def step(self, rng, pos, spike=None, **plan):
        qkv, q_nw, k_nw = self.inputs(rng)
        if spike is not None:
            qkv, k_nw = self.plant_spike(qkv, q_nw, k_nw, pos, spike, plan)
        got, a, rope = self.call(qkv, q_nw, k_nw, pos, **plan)
        self.check(got, a, rope, qkv, q_nw, k_nw, pos)
        return a

    def inputs(self, rng):
        H, Hkv, D, dt = self.H, self.Hkv, self.D, self.dt
        qkv = rd.rand16(rng, ((H + 2 * Hkv) * D,), dt, -3, 1)
        if not self.qk_norm:
            return qkv, None, None
        return qkv, rd.rand16(rng, (D,), dt, -1, 0), rd.rand16(rng, (D,), dt, -1, 0)

    def plant_spike(self, qkv, q_nw, k_nw, pos, where, plan):
        """one score of KV head 0 dominates (~40 above the rest): a cached row aligned with query head 0 in split 0 or in the last
        live split, or the appended row itself (k_raw := q_raw of head 0, k_norm_w := 4 q_norm_w)"""
        H, D, dt = self.H, self.D, self.dt
        qkv = qkv.copy()
        if where == "appended":
            qkv[H * D:H * D + D] = qkv[:D]
            return qkv, rd.rnd(4.0 * q_nw.astype(np.float64), dt).astype(np.float32)
        q_mid, _ = rd.norm_rope_candidates(qkv[:D].reshape(1, D), q_nw, EPS, rd.rope_cur(pos, D), dt)
        q = q_mid[0]
        row = rd.rnd(40.0 * (D ** 0.5) * q / (q @ q), dt).astype(np.float32)
        chunk = plan["chunk"]
        t = 0 if where == "split0" else (pos // chunk) * chunk + (pos % chunk) // 2   # last split: a row before pos
        self.K[0, t] = row
        self.dK = self.T.from_numpy(self.K, dt)
        return qkv, k_nw


def positions(chunk, nsplit, cap=CAP):
    ps = set(range(10)) | {1023, 1024, 1025, 8191, 8192, 8193, cap - 1}
    for j in (1, 2, nsplit // 2, nsplit - 1):
        ps |= {j * chunk - 1, j * chunk, j * chunk + 1}
    return sorted(p for p in ps if 0 <= p < cap)


@pytest.mark.parametrize("name", list(GEOMS))
def test_attn_step_engine_plan(omx, lib, name):
    """the engine's plan (attn_step_plan of the context bucket) at positions across splits and buckets"""
    H, Hkv, D, qk, dt = GEOMS[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sl = Slabs(omx, lib, name, H, Hkv, D, qk, dt, rng)
    a = sl.step(rng, 0, tk_max=1024)
    for pos in positions(a.chunk, a.nsplit):
        a = sl.step(rng, pos, tk_max=engine_tk_max(pos))
        assert a.chunk * a.nsplit >= pos + 1 and a.nsplit >= H // Hkv


def explicit_plans(H, Hkv, D, pos):
    """nsplit in {G, 16, 17, 32, 33, 48} where the launcher takes it, chunk the smallest whole number of wave units covering pos"""
    G, tpw = H // Hkv, 64 // (D // 8)
    for ns in sorted({G, 16, 17, 32, 33, 48}):
        if ns < G or Hkv * ns > 256:
            continue
        yield ns, tpw * -(-(pos + 1) // (ns * tpw))


@pytest.mark.parametrize("name", list(GEOMS))
def test_attn_step_explicit_plans(omx, lib, name):
    """explicit split counts: one, two and three gather batches of 16; a position in the first and in the last split"""
    H, Hkv, D, qk, dt = GEOMS[name]
    rng = np.random.default_rng(zlib.crc32(("plans/" + name).encode()))
    sl = Slabs(omx, lib, name, H, Hkv, D, qk, dt, rng)
    seen = set()
    for pos in (7, 1025, 8193, CAP - 1):
        for ns, chunk in explicit_plans(H, Hkv, D, pos):
            a = sl.step(rng, pos, chunk=chunk, nsplit=ns)
            assert (a.chunk, a.nsplit) == (chunk, ns)
            seen.add(ns)
        # a plan with room to spare: the same position with the chunk of a bucket twice as long (trailing empty splits)
        ns, chunk = next(explicit_plans(H, Hkv, D, 2 * pos + 1))
        sl.step(rng, pos, chunk=chunk, nsplit=ns)
    assert (Hkv > 5) or 48 in seen, "48 splits (three gather batches) run where Hkv <= 5"


@pytest.mark.parametrize("where", ["split0", "last_split", "appended"])
@pytest.mark.parametrize("name", ["qwen3_8b", "g7", "d64", "f16"])
def test_attn_step_score_spike(omx, lib, name, where):
    """one score dominates: the merge must rescale every other split's partial by exp(m_j - M)"""
    H, Hkv, D, qk, dt = GEOMS[name]
    rng = np.random.default_rng(zlib.crc32(f"spike/{name}/{where}".encode()))
    sl = Slabs(omx, lib, name, H, Hkv, D, qk, dt, rng)
    for pos in (37, 1500, 5000):
        a = sl.step(rng, pos, tk_max=engine_tk_max(pos))   # (the engine's plan, learnt from a plain call at the same position)
        assert pos % a.chunk != 0, "the last live split must hold rows before pos"
        sl.step(rng, pos, spike=where, chunk=a.chunk, nsplit=a.nsplit)


def test_attn_step_reused_granules(omx, lib):
    """one granule buffer, consecutive calls tagged (seq, layer) = (s, 1), (s, 2), (s + 1, 1) with tag = seq * 2 + layer, each on
    its own K / V data and at its own position and plan: every call matches its own reference"""
    H, Hkv, D, qk, dt = GEOMS["qwen3_8b"]
    rng = np.random.default_rng(2024)
    layers = [Slabs(omx, lib, "l1", H, Hkv, D, qk, dt, rng), Slabs(omx, lib, "l2", H, Hkv, D, qk, dt, rng)]
    layers[1].gran = layers[0].gran   # shared
    s = 5
    for seq, layer, pos, plan in ((s, 1, 300, dict(tk_max=1024)), (s, 2, 2000, dict(chunk=64, nsplit=32)),
                                  (s + 1, 1, 301, dict(chunk=16, nsplit=20)), (s + 1, 2, 2001, dict(tk_max=3072)),
                                  (s + 2, 1, 40, dict(chunk=4, nsplit=11))):
        sl = layers[layer - 1]
        qkv, q_nw, k_nw = sl.inputs(rng)
        got, a, rope = sl.call(qkv, q_nw, k_nw, pos, seq=seq, tag_mul=2, tag_add=layer, **plan)
        sl.check(got, a, rope, qkv, q_nw, k_nw, pos)


def test_attn_step_host_refusals(omx, lib):
    """a plan that does not cover pos + 1 and a position outside the cache are refused before any launch"""
    H, Hkv, D, qk, dt = GEOMS["qwen3_8b"]
    rng = np.random.default_rng(3)
    sl = Slabs(omx, lib, "r", H, Hkv, D, qk, dt, rng, cap=512)
    qkv, q_nw, k_nw = sl.inputs(rng)
    with pytest.raises(omx.OmxError, match="does not cover position"):
        sl.call(qkv, q_nw, k_nw, 200, chunk=4, nsplit=32)
    with pytest.raises(omx.OmxError, match="outside the cache"):
        sl.call(qkv, q_nw, k_nw, 512, tk_max=512)
