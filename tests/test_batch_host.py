"""CPU-only: generate.generate_batch (many prompts over the slots of an engine.Batch) against a fake Batch -- a deterministic
next-token function per sequence -- for the scheduling cases: more prompts than slots, EOS in the middle of a chunk, EOS as the
first token, max_new_tokens hit exactly at a chunk edge."""
import numpy as np
import pytest

V = 1000
EOS = 7


def _next(history):
    """next token of a sequence = f(last token, length): a walk that reaches EOS where the test prompts below make it"""
    last, n = history[-1], len(history)
    if last % 100 == 99:                      # ... 99 -> EOS
        return EOS
    return (last + 1) % V if last != EOS else (EOS + n) % V    # (past EOS the walk goes on: those tokens must never be returned)


class FakeBatch:
    """engine.Batch's interface on the host; records every call and asserts the contract generate_batch has to keep."""

    def __init__(self, n_slots):
        self.n_slots = n_slots
        self.hist = {}                        # slot -> token history (prompt + generated), present = prefilled
        self.calls = []
        self.dirty = set()                    # slots used and not reset since

    def prefill(self, slot, prompt):
        assert 0 <= slot < self.n_slots
        assert slot not in self.dirty, f"slot {slot} reused without a reset"
        assert len(prompt) >= 1
        self.hist[slot] = [int(t) for t in prompt]
        self.dirty.add(slot)
        tok = _next(self.hist[slot])
        self.hist[slot].append(tok)
        self.calls.append(("prefill", slot, len(prompt)))
        return tok

    def decode(self, n, slots=None):
        slots = list(range(self.n_slots)) if slots is None else [int(s) for s in slots]
        assert n >= 1 and len(slots) >= 1
        assert len(set(slots)) == len(slots), f"decode with duplicate slots {slots}"
        for s in slots:
            assert s in self.hist, f"decode of slot {s} that is not prefilled"
        out = np.zeros((n, len(slots)), np.uint32)
        for i in range(n):
            for c, s in enumerate(slots):
                tok = _next(self.hist[s])
                self.hist[s].append(tok)
                out[i, c] = tok
        self.calls.append(("decode", tuple(slots), n))
        return out

    def reset(self, slot):
        assert slot in self.dirty
        self.hist.pop(slot, None)
        self.dirty.discard(slot)
        self.calls.append(("reset", slot))


def _want(prompt, max_new, stop=True):
    h, out = [int(t) for t in prompt], []
    while len(out) < max_new:
        tok = _next(h)
        h.append(tok)
        out.append(tok)
        if stop and tok == EOS:
            break
    return out


# chunk 4, max_new_tokens 8:
PROMPTS = [
    [10, 11, 12],        # runs to max_new_tokens
    [5, 96],             # 97 98 99 EOS: EOS is the 4th token = 3rd of the first chunk (mid-chunk)
    [3, 99],             # EOS as the FIRST token
    [500],               # one-token prompt, runs to max_new_tokens
    [1, 2, 3, 4, 94],    # 95 .. 99 EOS: EOS is the 6th token
    [42, 98],            # 99 EOS: EOS is the first DECODED token
    [700, 701],          # waits for a slot
]


@pytest.mark.parametrize("n_slots", [1, 2, 3, 8])
def test_generate_batch_schedules_prompts_over_slots(omx, n_slots):
    from ominix_mlx_amd import generate
    fake = FakeBatch(n_slots)
    outs = generate.generate_batch(fake, PROMPTS, 8, eos_ids=[EOS], chunk=4)
    assert outs == [_want(p, 8) for p in PROMPTS]                       # prompt order, nothing past EOS, nothing past max_new_tokens
    assert [len(o) for o in outs] == [8, 4, 1, 8, 6, 2, 8]
    for o in outs:
        assert EOS not in o[:-1]
    assert not fake.dirty, "every slot is reset when its sequence retires"
    assert sum(1 for c in fake.calls if c[0] == "prefill") == len(PROMPTS)
    assert sum(1 for c in fake.calls if c[0] == "reset") == len(PROMPTS)
    if n_slots < len(PROMPTS):
        assert any(c[0] == "prefill" for c in fake.calls[fake.calls.index(next(c for c in fake.calls if c[0] == "decode")):]), \
            "with more prompts than slots a prompt is prefilled after decoding has begun"


def test_max_new_tokens_exactly_at_a_chunk_edge(omx):
    """first token + 2 chunks of 4 = 9 = max_new_tokens: the last decode call is a whole chunk and nothing is decoded after it"""
    from ominix_mlx_amd import generate
    fake = FakeBatch(2)
    outs = generate.generate_batch(fake, [[10], [200]], 9, eos_ids=[EOS], chunk=4)
    assert outs == [_want([10], 9), _want([200], 9)] and all(len(o) == 9 for o in outs)
    decodes = [c for c in fake.calls if c[0] == "decode"]
    assert decodes == [("decode", (0, 1), 4), ("decode", (0, 1), 4)]


def test_without_eos_every_sequence_runs_to_max_new_tokens(omx):
    from ominix_mlx_amd import generate
    fake = FakeBatch(3)
    outs = generate.generate_batch(fake, PROMPTS, 5, chunk=16)
    assert outs == [_want(p, 5, stop=False) for p in PROMPTS]
    assert all(len(o) == 5 for o in outs)


def test_empty_prompt_and_bad_arguments_are_refused(omx):
    from ominix_mlx_amd import generate
    with pytest.raises(ValueError, match="empty"):
        generate.generate_batch(FakeBatch(2), [[1], []], 4)
    with pytest.raises(ValueError, match="positive"):
        generate.generate_batch(FakeBatch(2), [[1]], 0)
