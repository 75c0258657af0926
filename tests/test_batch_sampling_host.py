"""CPU-only: the per-slot filtered sampler of a batch (omx_qwen3_batch_set_sampling) is exported, declared and bound, and
Batch.set_sampler routes to it exactly when a filter or a penalty is on."""
import ctypes
import inspect


def test_batch_set_sampling_is_exported_and_bound(omx):
    from ominix_mlx_amd import engine
    lib = ctypes.CDLL(omx.LIB_PATH)
    assert hasattr(lib, "omx_qwen3_batch_set_sampling")
    restype, argtypes = engine.ENGINE_SIGNATURES["omx_qwen3_batch_set_sampling"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(omx.Sampling), ctypes.c_uint64]
    # the plain entry point keeps its signature
    assert engine.ENGINE_SIGNATURES["omx_qwen3_batch_set_sampler"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint64])


def test_batch_set_sampler_signature(omx):
    from ominix_mlx_amd import engine
    sig = inspect.signature(engine.Batch.set_sampler)
    names = list(sig.parameters)
    assert names == ["self", "slot", "temperature", "seed", "top_k", "top_p", "repetition_penalty", "presence_penalty"]
    for n, default in [("seed", 0), ("top_k", 0), ("top_p", 1.0), ("repetition_penalty", 1.0), ("presence_penalty", 0.0)]:
        assert sig.parameters[n].default == default
    for n in names[4:]:
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY


def test_batch_set_sampler_routes_by_its_filters(omx, monkeypatch):
    """everything off -> omx_qwen3_batch_set_sampler (the plain sampler, as Model.set_sampler); otherwise the new entry point"""
    from ominix_mlx_amd import engine
    calls = []

    class FakeLib:
        def omx_qwen3_batch_set_sampler(self, h, slot, t, seed):
            calls.append(("plain", slot, t, seed))
            return 0

        def omx_qwen3_batch_set_sampling(self, h, slot, p, seed):
            s = p._obj
            calls.append(("filtered", slot, (s.temperature, s.top_k, s.top_p, s.repetition_penalty, s.presence_penalty), seed))
            return 0

    monkeypatch.setattr(engine, "lib", FakeLib())
    b = engine.Batch.__new__(engine.Batch)
    b._h = ctypes.c_void_p()
    b.model = None
    b.set_sampler(2, 0.5, 7)
    b.set_sampler(1, 0.5, 7, top_k=0, top_p=1.0)
    b.set_sampler(3, 0.5, 9, top_k=20, top_p=0.5)
    b.set_sampler(0, 0.0, 1, presence_penalty=1.5)
    assert calls == [("plain", 2, 0.5, 7), ("plain", 1, 0.5, 7), ("filtered", 3, (0.5, 20, 0.5, 1.0, 0.0), 9),
                     ("filtered", 0, (0.0, 0, 1.0, 1.0, 1.5), 1)]
