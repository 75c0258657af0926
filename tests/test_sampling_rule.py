"""CPU: the numpy restatement of the filtered-sampling rule (tests/sampling_rule.py) on hand-worked rows, and the new entry points in
the library, the headers and the binding tables."""
import ctypes
import inspect

import numpy as np

from oracle import mlx_rng as rng
from oracle import ref_core as rc
import sampling_rule as sr


def test_topk_keeps_every_tie_at_the_threshold():
    y = np.array([3.0, 1.0, 2.0, 2.0, 0.5, 2.0], np.float32)
    thr, mask = sr.topk_threshold(y, 2)          # the 2nd largest is 2.0: all three 2.0s stay
    assert thr == np.float32(2.0)
    assert mask.tolist() == [True, False, True, True, False, True]
    thr, mask = sr.topk_threshold(y, 1)
    assert thr == np.float32(3.0) and mask.tolist() == [True, False, False, False, False, False]
    for off in (0, 6, 7):                         # 0 and >= V: off
        thr, mask = sr.topk_threshold(y, off)
        assert thr == -np.inf and mask.all()


def test_topp_keeps_the_maximum_when_p_is_tiny_and_tie_groups_whole():
    y = np.log(np.array([0.5, 0.2, 0.2, 0.1], np.float64)).astype(np.float32)
    everyone = np.ones(4, bool)
    assert sr.topp_mask(y, everyone, 1e-6).tolist() == [True, False, False, False]
    # mass strictly above the 0.2 pair is 0.5: kept together for p > 0.5, dropped together for p <= 0.5
    assert sr.topp_mask(y, everyone, 0.5).tolist() == [True, False, False, False]
    assert sr.topp_mask(y, everyone, 0.51).tolist() == [True, True, True, False]
    assert sr.topp_mask(y, everyone, 0.89).tolist() == [True, True, True, False]    # above the 0.1 entry: 0.9
    assert sr.topp_mask(y, everyone, 0.95).tolist() == [True, True, True, True]
    assert sr.topp_mask(y, everyone, 1.0).all()
    # on the survivors of top-k only: Z is their mass (0.9), the mass above the pair is 0.5 = 0.5556 Z
    surv = np.array([True, True, True, False])
    assert sr.topp_mask(y, surv, 0.55).tolist() == [True, False, False, False]
    assert sr.topp_mask(y, surv, 0.56).tolist() == [True, True, True, False]
    thr, mask = sr.kept_mask(y, top_k=3, top_p=0.56)
    assert mask.tolist() == [True, True, True, False] and thr == y[1]
    assert (mask == (y >= thr)).all()


def test_penalty_sign_rule_and_order():
    x = np.array([2.0, -2.0, 0.0, 4.0, -1.0], np.float32)
    y = sr.scaled(x, 1.0, seen_ids=[0, 1, 2], repetition_penalty=2.0)
    assert y.tolist() == [1.0, -4.0, 0.0, 4.0, -1.0]                 # positive divided, non-positive multiplied, unseen untouched
    y = sr.scaled(x, 1.0, seen_ids=[0, 1], presence_penalty=1.5)
    assert y.tolist() == [0.5, -3.5, 0.0, 4.0, -1.0]
    y = sr.scaled(x, 0.5, seen_ids=[0, 1], repetition_penalty=2.0, presence_penalty=1.5)   # division, then subtraction, then 1/T
    assert y.tolist() == [-1.0, -11.0, 0.0, 8.0, -2.0]
    r = np.float32(1.35)
    y = sr.scaled(np.array([1.0], np.float32), 0.6, seen_ids=[0], repetition_penalty=1.35)
    assert y[0] == np.float32(np.float32(np.float32(1.0) / r) * np.float32(np.float32(1.0) / np.float32(0.6)))
    # temperature 0 with a penalty: the argmax of the penalised logits
    tok, _, _ = sr.sample(np.array([1.0, 3.0, 2.5], np.float32), 0.0, None, repetition_penalty=2.0, seen_ids=[1])
    assert tok == 2


def test_everything_off_is_the_plain_sampler():
    g = np.random.default_rng(5)
    x = rc.bf16_round(3.0 * g.standard_normal(4096).astype(np.float32))
    for temp, seed in [(0.7, 0), (1.0, 3), (1.5, 99)]:
        tok, thr, kept = sr.sample(x, temp, rng.key(seed))
        assert tok == int(rc.sample(x[None, :], temp, rng.key(seed))[0])
        assert thr == -np.inf and kept == x.size
    assert sr.sample(x, 0.0, None)[0] == int(rc.sample(x[None, :], 0.0, None)[0])


def test_filtered_draw_stays_inside_the_kept_set():
    g = np.random.default_rng(6)
    x = rc.bf16_round(2.0 * g.standard_normal(1000).astype(np.float32))
    y = sr.scaled(x, 0.8)
    thr, mask = sr.kept_mask(y, top_k=20, top_p=0.9)
    assert 1 <= mask.sum() <= (y >= np.sort(y)[-20]).sum() and (mask == (y >= thr)).all()
    for seed in range(50):
        assert mask[sr.draw(y, mask, rng.key(seed))]


def test_new_entry_points_are_exported_and_bound(omx):
    from ominix_mlx_amd import engine, generate
    lib = ctypes.CDLL(omx.LIB_PATH)
    for name in ("omx_sample_filtered", "omx_topk_values", "omx_qwen3_set_sampling"):
        assert hasattr(lib, name), f"{name} is not exported"
    assert "omx_sample_filtered" in omx.SIGNATURES and "omx_topk_values" in omx.SIGNATURES
    assert "omx_qwen3_set_sampling" in engine.ENGINE_SIGNATURES
    assert ctypes.sizeof(omx.Sampling) == 20                       # float, int32, float, float, float: omx_sampling
    p = omx.Sampling()
    assert (p.temperature, p.top_k, p.top_p, p.repetition_penalty, p.presence_penalty) == (0.0, 0, 1.0, 1.0, 0.0)
    keywords = {"top_k": 0, "top_p": 1.0, "repetition_penalty": 1.0, "presence_penalty": 0.0}
    for fn in (engine.Model.set_sampler, engine.Generate.__init__, generate.generate_text):
        params = inspect.signature(fn).parameters
        for name, default in keywords.items():
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default
    assert callable(omx.ops.sample_filtered) and callable(omx.ops.topk_values)
