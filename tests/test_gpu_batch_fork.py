"""Forked batch slots (engine.Batch.fork / shared; omx_qwen3_batch_fork, batch_attn_shared_kernel in csrc/engine_batch.hip): a fork is
the sequence it copies, bit for bit, whatever group the decode attention puts it in -- n completions of one prompt, one system
prompt under several suffixes, the owner trimmed, reset and refilled under its children.  The shared span is read through grouped
blocks (OMX_BATCH_SHARE_MIN=2), through the rows' own blocks (the default), and with nothing shared (OMX_BATCH_SHARE=0, in a child
process).  max_context 1 024; the prompts are chosen so that a shared span (whole 256-token chunks below the fork), a private tail
and a crossing of a chunk boundary while decoding all occur: 500 tokens share 256 and 12 steps later cross 512; 760 share 512 and
cross 768."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_core as rc
from test_gpu_batch_decode import _bound, _build, _prompt

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["default", "grouped", "grouped_by_3"])
def attention_form(request, monkeypatch):
    """The tests that decode siblings together run three times (the switches are read when a batch is created): with the library's
    default, under which no group is large enough for a grouped block (it is the slower form at every size measured) and
    siblings read their own copies; with grouped blocks from two members on, one block per group; and with at most three member
    rows per block, so that a group of eight is taken by blocks of 3, 3 and 2 rows."""
    if request.param != "default":
        monkeypatch.setenv("OMX_BATCH_SHARE_MIN", "2")
        monkeypatch.setenv("OMX_BATCH_SHARE_ROWS", "8" if request.param == "grouped" else "3")
    else:
        monkeypatch.delenv("OMX_BATCH_SHARE_MIN", raising=False)
        monkeypatch.delenv("OMX_BATCH_SHARE_ROWS", raising=False)
    return request.param


CTX = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# slot 0 prefills, 1..7 are forked from it: seven categorical siblings with their own key sequences and a greedy one
SAMPLERS = [(0.8, 100)] + [(0.8, i) for i in range(1, 7)] + [(0.0, 0)]


def _steps(b, slots, n, toks, logits):
    """n single-step decode calls over `slots`; tokens and logits appended per slot"""
    for _ in range(n):
        step = b.decode(1, slots)
        for c, s in enumerate(slots):
            toks[s].append(int(step[0, c]))
            logits[s].append(b.logits(s))


def _siblings(m, P, forked, steps=24):
    """eight slots on prompt P with SAMPLERS, 1..7 forked from slot 0 or every slot prefilled itself -> (tokens [8, 1 + steps],
    logits [8, 1 + steps, V], shared() per slot)"""
    b = m.batch(8, CTX)
    for s, (t, seed) in enumerate(SAMPLERS):
        b.set_sampler(s, t, seed)
    toks = {0: [int(b.prefill(0, P))]}
    for s in range(1, 8):
        toks[s] = [int(b.fork(0, s) if forked else b.prefill(s, P))]
    logits = {s: [b.logits(s)] for s in range(8)}
    shared = [b.shared(s) for s in range(8)]
    assert all(b.offset(s) == len(P) for s in range(8))
    _steps(b, list(range(8)), steps, toks, logits)
    assert all(b.offset(s) == len(P) + steps for s in range(8))
    b.close()
    return np.asarray([toks[s] for s in range(8)]), np.stack([np.stack(logits[s]) for s in range(8)]), shared


# ---- 1. a fork is the sequence it copies ----

def _fork_against_itself(name, plen, out=None):
    cfg, m, _ = _build(name, CTX)
    P = _prompt(plen, cfg.vocab_size, 3)
    tf, lf, shared = _siblings(m, P, forked=True)
    ti, li, _ = _siblings(m, P, forked=False)
    m.close()
    np.testing.assert_array_equal(tf, ti)
    np.testing.assert_array_equal(lf, li)
    for s in range(8):
        assert len(set(tf[s].tolist())) > 4, f"slot {s}: a degenerate stream would not show a difference"
    assert len({tuple(t) for t in tf.tolist()}) >= 6, "the siblings' samplers are meant to take them apart"
    if out:
        np.savez(out, tokens=tf, logits=lf, shared=np.asarray(shared))
    return tf, lf, shared


@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
def test_a_fork_is_the_sequence_it_copies(omx, name, tmp_path, attention_form):
    """Slot 0 prefills 500 tokens, slots 1..7 are forked from it; a second batch prefills the prompt in every slot; the same samplers;
    24 single-step calls over all eight: first tokens, tokens and logits bit for bit -- and once more with OMX_BATCH_SHARE=0 in a
    child process, whose tokens and logits are also this process's."""
    tf, lf, shared = _fork_against_itself(name, 500)
    assert shared == [(0, 256)] * 8
    if attention_form != "default":      # (the child below shares nothing, whatever the group switches say: once is enough)
        return
    out = str(tmp_path / "off.npz")
    env = dict(os.environ, OMX_BATCH_SHARE="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), name, "500", out], env=env, capture_output=True, text=True, timeout=900,
                       stdin=subprocess.DEVNULL)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    off = np.load(out)
    assert [tuple(x) for x in off["shared"].tolist()] == [(0, 0)] * 8, "OMX_BATCH_SHARE=0: forks copy and share nothing"
    np.testing.assert_array_equal(off["tokens"], tf)
    np.testing.assert_array_equal(off["logits"], lf)


# ---- 2. group size and order do not change a sibling ----

def _run_child(m, P, children, order, steps=20, neighbour=None, reset=()):
    """slot 0 prefills P, `children` are forked from it (slot 3 is A, sampler (0.8, 5)), `reset` are emptied again, `neighbour` =
    (slot, prompt) is prefilled on its own; `steps` single-step calls over `order` -> tokens and logits of A"""
    b = m.batch(8, CTX)
    for s in range(8):
        b.set_sampler(s, 0.8 if s != 6 else 0.0, 5 if s == 3 else 40 + s)
    b.prefill(0, P)
    toks, logits = {}, {}
    for s in children:
        toks[s] = [int(b.fork(0, s))]
        logits[s] = [b.logits(s)]
    for s in reset:
        b.reset(s)
    if neighbour is not None:
        b.prefill(*neighbour)
    assert b.shared(3) == (0, len(P) // 256 * 256)
    for s in order:
        toks.setdefault(s, []); logits.setdefault(s, [])
    _steps(b, list(order), steps, toks, logits)
    b.close()
    return np.asarray(toks[3]), np.stack(logits[3])


@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
@pytest.mark.parametrize("plen", [500, 760])
def test_group_size_and_order_do_not_change_a_sibling(omx, name, plen, attention_form):
    """The same forked sequence, 20 steps: among seven siblings and the owner; with one sibling; alone, all the others reset (a group
    of one); listed first; listed last; beside an unrelated neighbour that shares nothing -- bit for bit."""
    cfg, m, _ = _build(name, CTX)
    V = cfg.vocab_size
    P = _prompt(plen, V, 11)
    kids = list(range(1, 8))
    runs = {
        "seven siblings": _run_child(m, P, kids, list(range(8))),
        "one sibling": _run_child(m, P, [3, 5], [0, 3, 5]),
        "owner only": _run_child(m, P, [3], [3, 0]),
        "group of one": _run_child(m, P, kids, [3], reset=[1, 2, 4, 5, 6, 7]),
        "listed first": _run_child(m, P, kids, [3, 7, 6, 5, 4, 2, 1, 0]),
        "listed last": _run_child(m, P, kids, [0, 1, 2, 4, 5, 6, 7, 3]),
        "unrelated neighbour": _run_child(m, P, [3, 5], [1, 0, 3, 5], neighbour=(1, _prompt(700, V, 55))),
    }
    m.close()
    t0, l0 = runs["seven siblings"]
    assert len(set(t0.tolist())) > 4
    for what, (t, l) in runs.items():
        np.testing.assert_array_equal(t, t0, err_msg=what)
        np.testing.assert_array_equal(l, l0, err_msg=what)


# ---- 2b. every instantiation of the grouped block ----

@pytest.mark.parametrize("D,H,Hkv", [(128, 8, 2), (128, 4, 4), (128, 4, 2), (128, 8, 1), (64, 4, 4), (64, 4, 2), (64, 8, 2), (64, 8, 1)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("rows", ["8", "3"])
def test_every_width_of_the_grouped_block(omx, monkeypatch, D, H, Hkv, rows):
    """batch_attn_shared_kernel<D, GT> for D = 64 / 128 and GT = 1 / 2 / 4 / 8 query heads per KV head (Qwen3-8B is <128, 4>) on
    one-layer models: five slots forked from a 600-token prompt (512 shared) and decoded 12 steps through grouped blocks against five
    slots that prefill the prompt themselves and read their own slabs -- tokens and logits bit for bit."""
    from ominix_mlx_amd import engine
    monkeypatch.setenv("OMX_BATCH_SHARE_MIN", "2")
    monkeypatch.setenv("OMX_BATCH_SHARE_ROWS", rows)
    V = 2048
    m = engine.Model(hidden_size=512, num_hidden_layers=1, intermediate_size=1024, num_attention_heads=H, num_key_value_heads=Hkv,
                     head_dim=D, vocab_size=V, max_context=CTX)
    m.synth_weights()
    P = _prompt(600, V, 17)
    out = []
    for forked in (True, False):
        b = m.batch(5, CTX)
        for s in range(5):
            b.set_sampler(s, 0.8 if s else 0.0, 20 + s)
        toks = {0: [int(b.prefill(0, P))]}
        for s in range(1, 5):
            toks[s] = [int(b.fork(0, s) if forked else b.prefill(s, P))]
        if forked:
            assert [b.shared(s) for s in range(5)] == [(0, 512)] * 5
        logits = {s: [b.logits(s)] for s in range(5)}
        _steps(b, [4, 0, 1, 2, 3], 12, toks, logits)
        b.close()
        out.append((np.asarray([toks[s] for s in range(5)]), np.stack([np.stack(logits[s]) for s in range(5)])))
    m.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert len({tuple(t) for t in out[0][0].tolist()}) >= 3


# ---- 3. one system prompt under several suffixes ----

@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
def test_shared_system_prompt(omx, name, attention_form):
    """Slot 0 prefills S (300 tokens) and is forked to 1..3 without a new draw; child i then prefills its own suffix of 200 + 3 i
    tokens on top (the prompt pass reads the child's own copy).  Against slots that prefill S and the suffix themselves: 18 steps
    (the children cross token 512), bit for bit; shared() still names the owner and 256 tokens after the suffix."""
    cfg, m, _ = _build(name, CTX)
    V = cfg.vocab_size
    S = _prompt(300, V, 21)
    U = {i: _prompt(200 + 3 * i, V, 70 + i) for i in (1, 2, 3)}
    out = []
    for forked in (True, False):
        b = m.batch(4, CTX)
        for s in range(4):
            b.set_sampler(s, 0.0 if s == 2 else 0.8, 30 + s)
        toks = {0: [int(b.prefill(0, S))]}
        for i in (1, 2, 3):
            if forked:
                assert b.fork(0, i, resample=False) == toks[0][0], "without a new draw the child's pending token is the owner's"
                assert b.offset(i) == 300
            else:
                b.prefill(i, S)
            b.set_sampler(i, 0.0 if i == 2 else 0.8, 30 + i)     # (a prefill of S has drawn once, a fork without a new draw has not)
            toks[i] = [int(b.prefill(i, U[i]))]
            assert b.offset(i) == 300 + len(U[i])
        if forked:
            assert [b.shared(i) for i in range(4)] == [(0, 256)] * 4
        logits = {s: [b.logits(s)] for s in range(4)}
        _steps(b, [0, 1, 2, 3], 18, toks, logits)
        b.close()
        out.append((np.asarray([toks[s] for s in range(4)]), np.stack([np.stack(logits[s]) for s in range(4)])))
    m.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert all(len(set(t.tolist())) > 4 for t in out[0][0])


# ---- 4. the owner's life cycle under its children ----

def _life(m, P, other, disturb):
    b = m.batch(4, CTX)
    for s in range(4):
        b.set_sampler(s, 0.8 if s != 2 else 0.0, 60 + s)
    toks = {0: [int(b.prefill(0, P))]}
    for s in (1, 2, 3):
        toks[s] = [int(b.fork(0, s))]
    logits = {s: [b.logits(s)] for s in range(4)}
    seen = [[b.shared(s) for s in range(4)]]
    _steps(b, [0, 1, 2, 3], 6, toks, logits)
    if disturb:
        b.trim(0, b.offset(0) - 400, int(P[400]))          # (a) the owner falls back below what it shares
    seen.append([b.shared(s) for s in range(4)])
    _steps(b, [0, 1, 2, 3], 6, toks, logits)
    if disturb:
        b.reset(0)                                          # (b) ... and is given to another prompt
        b.prefill(0, other)
    seen.append([b.shared(s) for s in range(4)])
    _steps(b, [0, 1, 2, 3], 8, toks, logits)
    b.close()
    return {s: (np.asarray(toks[s]), np.stack(logits[s])) for s in (1, 2, 3)}, seen


@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
def test_the_owner_is_trimmed_reset_and_refilled_under_its_children(omx, name, attention_form):
    """760 tokens (512 shared), three children.  After 6 steps the owner is trimmed to 400 tokens: every shared_len drops to 256;
    after 6 more (the children cross 768) it is reset and prefilled with another prompt: the children share nothing.  Their
    tokens and logits over the 20 steps are those of a run in which the owner is left alone."""
    cfg, m, _ = _build(name, CTX)
    V = cfg.vocab_size
    P, other = _prompt(760, V, 31), _prompt(333, V, 32)
    calm, seen_calm = _life(m, P, other, disturb=False)
    rough, seen = _life(m, P, other, disturb=True)
    m.close()
    assert seen_calm == [[(0, 512)] * 4] * 3
    assert seen[0] == [(0, 512)] * 4 and seen[1] == [(0, 256)] * 4
    assert [n for _, n in seen[2]] == [0, 0, 0, 0]
    for s in (1, 2, 3):
        np.testing.assert_array_equal(rough[s][0], calm[s][0])
        np.testing.assert_array_equal(rough[s][1], calm[s][1])
        assert len(set(calm[s][0].tolist())) > 4


@pytest.mark.parametrize("name", ["narrow", "wide", "narrow_q4"])
def test_a_child_trimmed_into_its_shared_span(omx, name, attention_form):
    """A child of a 760-token prompt and an independent slot with the same sampler: both decode 4 steps, are trimmed back to 300 tokens
    and go on for 16 steps (across 512 would need more; the trim itself crosses 512 and 768 downwards) -- bit for bit, and the child
    shares 256 tokens from then on while its sibling keeps 512."""
    cfg, m, _ = _build(name, CTX)
    V = cfg.vocab_size
    P = _prompt(760, V, 41)
    b = m.batch(4, CTX)
    for s, seed in enumerate([1, 9, 2, 9]):
        b.set_sampler(s, 0.8, seed)
    b.prefill(0, P)
    toks = {1: [int(b.fork(0, 1))], 2: [int(b.fork(0, 2))], 3: [int(b.prefill(3, P))], 0: []}
    logits = {1: [b.logits(1)], 3: [b.logits(3)], 0: [], 2: []}
    _steps(b, [0, 1, 2, 3], 4, toks, logits)
    for s in (1, 3):
        b.trim(s, b.offset(s) - 300, int(P[300]))
    assert b.offset(1) == b.offset(3) == 300
    assert [b.shared(s) for s in range(4)] == [(0, 512), (0, 256), (0, 512), (3, 0)]
    _steps(b, [0, 1, 2, 3], 16, toks, logits)
    b.close(); m.close()
    np.testing.assert_array_equal(np.asarray(toks[1]), np.asarray(toks[3]))
    np.testing.assert_array_equal(np.stack(logits[1]), np.stack(logits[3]))
    assert len(set(toks[1])) > 4


# ---- 5. against the oracle ----

def test_forked_slots_match_the_oracle_teacher_forced(omx, attention_form):
    """narrow: slot 0 prefills S (500 tokens, 256 shared) and is forked to 1..3 without a new draw; child i prefills its own suffix of
    2 + i tokens; then 14 positions per slot (the last of its prompt and 13 steps, across token 512), the oracle's token of THAT
    slot's sequence forced after every step.  The bound and the rule of test_ragged_batch_matches_the_oracle_teacher_forced:
    logits within 1.5 bound, the engine's token the oracle's unless the oracle's margin is <= 2 bound, and at most half of the 56
    positions such near-ties (the oracle alone: 22)."""
    cfg, m, oracle = _build("narrow", CTX)
    V, n_pos = cfg.vocab_size, 14
    S = _prompt(500, V, 3)
    U = {i: _prompt(2 + i, V, 80 + i) for i in (1, 2, 3)}
    seqs = [S] + [np.concatenate([S, U[i]]) for i in (1, 2, 3)]
    refs = [oracle.generate(p, n_pos, return_logits=True) for p in seqs]
    b = m.batch(4, CTX)
    got = [[int(b.prefill(0, S))]]
    for i in (1, 2, 3):
        b.fork(0, i, resample=False)
        got.append([int(b.prefill(i, U[i]))])
    assert [b.shared(i) for i in range(4)] == [(0, 256)] * 4
    logits = [[b.logits(s)] for s in range(4)]
    for i in range(1, n_pos):
        for s in range(4):
            b.trim(s, 0, int(refs[s][0][i - 1]))
        step = b.decode(1)
        for s in range(4):
            got[s].append(int(step[0, s]))
            logits[s].append(b.logits(s))
    near, worst = 0, 0.0
    for s in range(4):
        assert b.offset(s) == len(seqs[s]) + n_pos - 1
        ref_tokens, ref_logits = refs[s]
        bound = _bound(cfg, ref_logits)
        margins = rc.argmax_margin(ref_logits)
        for i in range(n_pos):
            err = float(np.abs(logits[s][i] - ref_logits[i]).max())
            worst = max(worst, err / bound)
            print(f"slot {s} pos {i}: err {err:.4f} bound {bound:.4f} margin {margins[i]:.4f} token {got[s][i]} ref {int(ref_tokens[i])}")
            assert err <= 1.5 * bound, f"slot {s} position {i}: logits off by {err:.4f} (1.5 x bound = {1.5 * bound:.4f})"
            assert got[s][i] == int(ref_tokens[i]) or margins[i] <= 2 * bound, f"slot {s} position {i}: token {got[s][i]} vs {int(ref_tokens[i])}"
            near += int(margins[i] <= 2 * bound)
    print(f"worst error {worst:.3f} x bound, {near} of {4 * n_pos} positions are near-ties of the oracle")
    assert near <= 4 * n_pos // 2
    b.close(); m.close()


# ---- 6. refusals and bookkeeping ----

def test_fork_refusals_and_bookkeeping(omx):
    cfg, m, _ = _build("narrow", CTX)
    V = cfg.vocab_size
    P = _prompt(300, V, 9)
    b = m.batch(3, CTX)
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_fork: source slot 0 has not been prefilled"):
        b.fork(0, 1)
    b.prefill(0, P)
    with pytest.raises(omx.OmxError, match="omx_qwen3_batch_fork: source and destination are the same slot 0"):
        b.fork(0, 0)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_fork: destination slot 3 out of range \(0\.\.2\)"):
        b.fork(0, 3)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_fork: source slot -1 out of range"):
        b.fork(-1, 1)
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_shared: slot 7 out of range"):
        b.shared(7)
    b.prefill(1, P[:10])
    with pytest.raises(omx.OmxError, match=r"omx_qwen3_batch_fork: destination slot 1 is not empty \(reset it first\)"):
        b.fork(0, 1)
    assert b.offset(1) == 10 and b.shared(1) == (1, 0) and b.shared(0) == (0, 0), "a refused fork changes nothing"
    b.reset(1)
    first = b.fork(0, 1)
    assert b.offset(1) == b.offset(0) == 300
    assert first == int(np.argmax(b.logits(0))), "a greedy fork draws the owner's greedy token"
    np.testing.assert_array_equal(b.logits(1), b.logits(0))
    assert b.shared(0) == (0, 256) and b.shared(1) == (0, 256) and b.shared(2) == (2, 0)
    # one level deep: a fork of the fork shares the root's span with the root
    b.decode(3, [0, 1])
    b.fork(1, 2, resample=False)
    assert b.offset(2) == 303 and b.shared(2) == (0, 256)
    t = b.decode(4, [0, 1, 2])
    np.testing.assert_array_equal(t[:, 1], t[:, 2])            # greedy twins
    np.testing.assert_array_equal(b.logits(1), b.logits(2))
    b.reset(0)
    assert b.shared(1)[1] == 0 and b.shared(2)[1] == 0 and b.shared(0) == (0, 0)
    b.close()

    # the model's own sequence with forks at work in between: bit for bit the undisturbed run
    Q = _prompt(48, V, 9)
    want = np.concatenate([[m.prefill(Q)], m.decode(16)])
    m.reset()
    got = np.concatenate([[m.prefill(Q)], m.decode(8)])
    b = m.batch(4, CTX)
    b.prefill(0, _prompt(520, V, 5))
    for s in (1, 2, 3):
        b.set_sampler(s, 0.9, s)
        b.fork(0, s)
    b.decode(5)
    b.reset(2)
    b.decode(3, [0, 1, 3])
    got = np.concatenate([got, m.decode(8)])
    np.testing.assert_array_equal(got, want)
    assert m.offset() == 48 + 16 and b.offset(0) == 528 and b.offset(2) == 0
    b.close(); m.close()


if __name__ == "__main__":   # the child of test_a_fork_is_the_sequence_it_copies: variant, prompt length, output file
    import omx_import
    omx_import.load_package()
    _fork_against_itself(sys.argv[1], int(sys.argv[2]), sys.argv[3])
