"""The bits a decode step leaves, pinned per form of the step: the layer's kernels (csrc/gemv.hip, csrc/gemv_chain.hip, csrc/attn_step.hip)
share their arithmetic through csrc/gemv_parts.hpp and csrc/granule.hpp, and token equality across the forms rests on every call site
producing the same bits.  Each case runs one prefill at the `second_batch` start of tests/test_gpu_attn_gateup.py and 8 greedy steps under
one form and compares sha256 digests -- tokens, last-step logits and the `h` / `h2` / `act` / `qkv` buffers (omx_qwen3_debug_read) -- with
tests/golden/layer_bits.json.  That file was written ONCE by this module's write_golden() running on the library of the commit it names
(the parent of the commit that made the arithmetic one text), so a digest here never comes from the code under test.
Models: WIDE3 and WIDE3_BIAS of tests/test_gpu_layer_launch.py (the folds are gated on those widths) and a narrow model (Qwen3-1.7B's
widths, two layers) whose shapes take the plain GEMVs and the O projection inside the attention launch with four vectors per lane."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import ref_qwen3 as rq
from oracle import synth
from test_gpu_attn_gateup import _engine, starts   # noqa: F401  (starts: the module-scoped fixture)
from test_gpu_hop_issue import _env
from test_gpu_layer_launch import WIDE3, WIDE3_BIAS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_bits.json")
# hidden 2048, 16 / 8 heads of 128, intermediate 6144: H * D = 4 x 512 (attn_step_oproj_ok: two O rows per wave), no fold's gate
NARROW2 = rq.Qwen3Config(2048, 2, 6144, 16, 8, 128, 1024, 1e-6, 1e6, False)
MODELS = {"wide3": WIDE3, "wide3_bias": WIDE3_BIAS, "narrow2": NARROW2}
STEPS = 8
SWITCHES = ("OMX_ATTN_DOWN", "OMX_ATTN_GATEUP", "OMX_DOWN_QKV", "OMX_ATTN_OPROJ")
FLAG = dict(zip(SWITCHES, ("attn_down", "attn_gateup", "down_qkv", "attn_oproj")))   # a switch's entry in Model.step_forms()
# a form = the switches set to "0" (the others unset): the default, the folds taken out one by one, and all of those without the O
# projection in the attention launch
_LADDER = {"default": (), "down0": SWITCHES[:1], "down0_gateup0": SWITCHES[:2], "down0_gateup0_chain0": SWITCHES[:3]}
FORMS = dict(_LADDER, **{name + "_oproj0": off + SWITCHES[3:] for name, off in _LADDER.items()})
# what the forms share.  Tokens and logits: tests/test_gpu_layer_launch.py, test_gpu_attn_gateup.py, test_gpu_down_qkv_chain.py and
# test_gpu_qwen3.py compare the forms pairwise.  The four buffers: every form runs the same arithmetic per layer and leaves the layer on
# the buffer it entered on (O projection into the ping-pong partner, down back), so the last step's rows sit in the same places.
SHARED = ("tokens", "logits", "h", "h2", "act", "qkv")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(omx, cfg, off, start):
    """{name: sha256} of one engine's run under the form that switches `off` off"""
    sizes = {"h": cfg.hidden_size, "h2": cfg.hidden_size, "act": cfg.intermediate_size,
             "qkv": (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim}
    prompt = synth.prompt_ids(1100, cfg.vocab_size)
    envs = [_env(name, "0" if name in off else None) for name in SWITCHES]
    for e in envs:
        e.__enter__()
    try:
        m = _engine(cfg)
        first = m.prefill(prompt[:start])
        toks = np.concatenate([[first], m.decode(STEPS)]).astype(np.uint32)
        forms = m.step_forms()
        assert not any(forms[FLAG[name]] for name in off), (off, forms)   # the run was the form it is filed under
        out = {"tokens": _sha(toks), "logits": _sha(m.last_logits())}
        for name, n in sizes.items():
            raw = np.empty(n, np.uint16)
            omx.check(omx.lib.omx_qwen3_debug_read(m._h, name.encode(), raw.ctypes.data, n))
            out[name] = _sha(raw)
        m.close()
    finally:
        for e in reversed(envs):
            e.__exit__()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_names_its_source(golden):
    """The file says which commit's library wrote it, and holds every model and form of this module."""
    assert len(golden["parent_commit"]) == 40 and golden["written_by"].startswith("libomx_hip")
    assert golden["start"] > 0 and golden["steps"] == STEPS
    assert set(golden["digests"]) == set(MODELS)
    for model in MODELS:
        assert set(golden["digests"][model]) == set(FORMS), model


@pytest.mark.parametrize("model", list(MODELS))
def test_forms_proven_equal_share_their_digests(golden, model):
    """What the forms share (SHARED) has one digest per model in the file."""
    per_form = golden["digests"][model]
    for name in SHARED:
        assert len({per_form[form][name] for form in FORMS}) == 1, (model, name)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("model", list(MODELS))
def test_step_bits_match_the_parent(omx, golden, starts, model, form):
    """One small engine: prefill, 8 greedy steps, six digests against the file."""
    assert starts["second_batch"] == golden["start"], "the split plan moved: the file's start position is another one"
    got = _digests(omx, MODELS[model], FORMS[form], golden["start"])
    want = golden["digests"][model][form]
    assert got == want, {k: (got[k][:12], want[k][:12]) for k in got if got[k] != want[k]}


def write_golden(omx, start, commit):
    """Writes tests/golden/layer_bits.json from the loaded library; run on the library of commit `commit`, never on the code under test."""
    doc = {"parent_commit": commit, "written_by": os.path.basename(omx.LIB_PATH), "start": int(start), "steps": STEPS,
           "digests": {model: {form: _digests(omx, cfg, off, start) for form, off in FORMS.items()} for model, cfg in MODELS.items()}}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc
