"""CPU-only: generate.generate_batch(n = ...) -- n completions of every prompt through one prefill and n - 1 forks -- against a fake
Batch with `fork`.  A sibling's next token is a function of its history AND its slot, as siblings that draw from the same logits
with their own samplers differ: more prompts than slot groups, EOS inside a chunk for one sibling only, the output order, and
n > n_slots.  n = 1 makes no `fork` call and exactly the calls it made before `n` existed."""
import numpy as np
import pytest

from test_batch_host import EOS, V, FakeBatch, PROMPTS, _next, _want


class ForkingBatch(FakeBatch):
    """FakeBatch plus `fork`: slot s adds `salt[s]` to every token it draws (its "sampler"); the salts are multiples of 100, so a
    walk reaches its x99 -> EOS step at the same place whatever the slot, unless the salt is made to miss it."""

    def __init__(self, n_slots, salts=None):
        super().__init__(n_slots)
        self.salt = list(salts) if salts is not None else [0] * n_slots

    def _draw(self, slot):
        tok = _next(self.hist[slot])
        if tok != EOS:
            tok = (tok + self.salt[slot]) % V
        self.hist[slot].append(tok)
        return tok

    def prefill(self, slot, prompt):
        assert 0 <= slot < self.n_slots and slot not in self.dirty and len(prompt) >= 1
        self.hist[slot] = [int(t) for t in prompt]
        self.dirty.add(slot)
        self.calls.append(("prefill", slot, len(prompt)))
        return self._draw(slot)

    def fork(self, src, dst, resample=True):
        assert src != dst and 0 <= dst < self.n_slots
        assert src in self.hist, f"fork of slot {src} that is not prefilled"
        assert dst not in self.dirty, f"fork onto slot {dst} without a reset"
        assert resample is True
        self.hist[dst] = self.hist[src][:-1]          # src's tokens without src's own draw: dst draws its own
        self.dirty.add(dst)
        self.calls.append(("fork", src, dst))
        return self._draw(dst)

    def decode(self, n, slots=None):
        slots = list(range(self.n_slots)) if slots is None else [int(s) for s in slots]
        assert n >= 1 and len(slots) >= 1 and len(set(slots)) == len(slots)
        out = np.zeros((n, len(slots)), np.uint32)
        for i in range(n):
            for c, s in enumerate(slots):
                assert s in self.hist, f"decode of slot {s} that is not prefilled"
                out[i, c] = self._draw(s)
        self.calls.append(("decode", tuple(slots), n))
        return out


def _want_salted(prompt, salt, max_new):
    h, out = [int(t) for t in prompt], []
    while len(out) < max_new:
        tok = _next(h)
        if tok != EOS:
            tok = (tok + salt) % V
        h.append(tok)
        out.append(tok)
        if tok == EOS:
            break
    return out


def test_three_completions_per_prompt(omx):
    """8 slots, n = 3: two groups at a time, seven prompts wait their turn.  Slot s salts its draws with 100 * (s % 3) + (s == 1):
    slot 1's walk is shifted by one and never reaches a x99 token, so in the first group EOS comes for two siblings of a prompt and not
    for the third (the exact calls of that case: the next test)."""
    from ominix_mlx_amd import generate
    salts = [100 * (s % 3) + (s == 1) for s in range(8)]
    fake = ForkingBatch(8, salts)
    outs = generate.generate_batch(fake, PROMPTS, 8, eos_ids=[EOS], chunk=4, n=3)
    assert len(outs) == 3 * len(PROMPTS)
    prefills = [c for c in fake.calls if c[0] == "prefill"]
    forks = [c for c in fake.calls if c[0] == "fork"]
    assert len(prefills) == len(PROMPTS) and len(forks) == 2 * len(PROMPTS), "one prefill and n - 1 forks per prompt"
    # which slots a prompt ran in: its prefill's slot and the destinations of the forks from it, in call order
    groups = []
    for c in fake.calls:
        if c[0] == "prefill":
            groups.append([c[1]])
        elif c[0] == "fork":
            assert c[1] == groups[-1][0], "siblings are forked from the prompt's own slot"
            groups[-1].append(c[2])
    assert all(len(g) == 3 for g in groups)
    for p, (prompt, slots) in enumerate(zip(PROMPTS, groups)):          # prompt-major, sibling k in the k-th slot of its group
        for k, s in enumerate(slots):
            assert outs[p * 3 + k] == _want_salted(prompt, salts[s], 8), f"prompt {p} sibling {k} (slot {s})"
            assert EOS not in outs[p * 3 + k][:-1] and len(outs[p * 3 + k]) <= 8
    some_split = [p for p in range(len(PROMPTS)) if len({len(outs[p * 3 + k]) for k in range(3)}) > 1]
    assert some_split, "no prompt whose siblings retire at different lengths: the case is not covered"
    assert any(o[-1] == EOS and len(o) > 1 for o in outs), "no sibling met EOS while decoding"
    assert not fake.dirty, "every slot is reset by the time its prompt's last sibling has retired"
    assert sum(1 for c in fake.calls if c[0] == "reset") == 3 * len(PROMPTS)
    first_decode = next(i for i, c in enumerate(fake.calls) if c[0] == "decode")
    assert any(c[0] == "prefill" for c in fake.calls[first_decode:]), "with more prompts than slot groups a prompt starts after decoding has begun"


def test_a_retired_sibling_is_not_decoded_and_its_slot_is_held(omx):
    """2 completions in 2 slots of one prompt whose slot-0 sibling reaches EOS with its 4th token (mid-chunk) and whose slot-1
    sibling (salt 1) never does: slot 0, the owner, leaves the decode calls and is held until its fork retires; the fork's slot is
    reset first."""
    from ominix_mlx_amd import generate
    fake = ForkingBatch(2, [0, 1])
    outs = generate.generate_batch(fake, [[5, 96]], 8, eos_ids=[EOS], chunk=4, n=2)
    assert outs[0] == [97, 98, 99, EOS]
    assert outs[1] == _want_salted([5, 96], 1, 8) and len(outs[1]) == 8 and EOS not in outs[1]
    assert fake.calls == [("prefill", 0, 2), ("fork", 0, 1), ("decode", (0, 1), 4), ("decode", (1,), 3), ("reset", 1), ("reset", 0)]


def test_a_forked_slot_is_free_as_soon_as_it_retires(omx):
    """3 slots, n = 2, two prompts.  The first prompt's FORK (slot 1, salt 0) reaches EOS with its 4th token while its owner (slot 0,
    salt 1) runs on: slot 1 is reset at once, and with the spare slot 2 the second prompt starts while the first's owner is still
    decoding.  before_sibling is called for every sibling, in order, before its prefill / fork."""
    from ominix_mlx_amd import generate
    fake = ForkingBatch(3, [1, 0, 0])
    seen = []
    outs = generate.generate_batch(fake, [[5, 96], [10, 11]], 8, eos_ids=[EOS], chunk=4, n=2,
                                   before_sibling=lambda p, k, slot: seen.append((p, k, slot, len(fake.calls))))
    assert outs[1] == [97, 98, 99, EOS] and len(outs[0]) == 8 and EOS not in outs[0]
    assert outs[2] == _want_salted([10, 11], 0, 8) and outs[3] == _want_salted([10, 11], 0, 8)
    c = fake.calls
    assert c[:4] == [("prefill", 0, 2), ("fork", 0, 1), ("decode", (0, 1), 4), ("reset", 1)]
    assert c[4:6] == [("prefill", 2, 2), ("fork", 2, 1)], "the second prompt starts in the spare slot and the freed one"
    assert c.index(("reset", 0)) > 5 and not fake.dirty
    assert [(p, k, slot) for p, k, slot, _ in seen] == [(0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 1, 1)]
    assert [at for *_, at in seen] == [0, 1, 4, 5], "each hook runs right before its sibling's prefill / fork"


def test_n_equal_one_makes_no_fork_call_and_the_calls_of_before(omx):
    from ominix_mlx_amd import generate
    a, b = ForkingBatch(3), FakeBatch(3)
    assert generate.generate_batch(a, PROMPTS, 8, eos_ids=[EOS], chunk=4, n=1) == generate.generate_batch(b, PROMPTS, 8, eos_ids=[EOS], chunk=4)
    assert a.calls == b.calls and not any(c[0] == "fork" for c in a.calls)
    assert generate.generate_batch(FakeBatch(2), PROMPTS, 8, eos_ids=[EOS], chunk=4, n=1) == [_want(p, 8) for p in PROMPTS]


def test_more_completions_than_slots_is_refused(omx):
    from ominix_mlx_amd import generate
    with pytest.raises(ValueError, match="n = 4"):
        generate.generate_batch(ForkingBatch(3), [[1, 2]], 4, n=4)
    with pytest.raises(ValueError, match="n = 0"):
        generate.generate_batch(ForkingBatch(3), [[1, 2]], 4, n=0)
    assert len(generate.generate_batch(ForkingBatch(3), [[1, 2]], 4, n=3)) == 3
