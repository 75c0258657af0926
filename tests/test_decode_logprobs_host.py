"""CPU-only: the host side of the per-token log-probabilities -- generate.generate_batch(return_logprobs=, best_of=) against a fake
Batch whose siblings have known tokens and log-probabilities (order best first, ties to the lower index, truncation at EOS with the
tokens, n <= best_of <= n_slots enforced), and generate.generate_text(logprobs=) / engine.Generate(logprobs=) against a fake model."""
import numpy as np
import pytest

EOS = 7
# log-probability of every token of sibling k; sibling 1 stops after three tokens (EOS), what its slot decodes past that is -64
LP = {0: -0.5, 1: -0.25, 2: -0.125, 3: -0.25}


def _tok(p, k, t):
    return EOS if (k == 1 and t == 2) else 100 * (p + 1) + 10 * k + t % 10


def _lp(p, k, t):
    return -64.0 if (k == 1 and t > 2) else LP[k]


class FakeBatch:
    """engine.Batch's interface on the host: sibling k of prompt p (told through before_sibling) emits _tok / _lp of its position"""

    def __init__(self, n_slots):
        self.n_slots, self.logprobs_top = n_slots, None
        self.who, self.pos, self.last = {}, {}, {}
        self.calls = []

    def tag(self, p, k, slot):
        self.who[slot] = (p, k)

    def set_logprobs(self, top_n=None):
        self.logprobs_top = top_n
        self.calls.append(("set_logprobs", top_n))

    def _emit(self, slot):
        p, k = self.who[slot]
        t = self.pos[slot]
        self.pos[slot] = t + 1
        self.last[slot] = np.float32(_lp(p, k, t))
        return _tok(p, k, t)

    def prefill(self, slot, prompt):
        assert slot not in self.pos, f"slot {slot} reused without a reset"
        self.pos[slot] = 0
        return self._emit(slot)

    def fork(self, src, dst, resample=True):
        assert resample and src in self.pos and dst not in self.pos
        self.pos[dst] = 0
        return self._emit(dst)

    def last_logprobs(self, slot):
        assert self.logprobs_top is not None
        return self.last[slot]

    def decode(self, n, slots=None, return_logprobs=False):
        slots = [int(s) for s in slots]
        toks, lps = np.zeros((n, len(slots)), np.uint32), np.zeros((n, len(slots)), np.float32)
        for i in range(n):
            for c, s in enumerate(slots):
                toks[i, c] = self._emit(s)
                lps[i, c] = self.last[s]
        if not return_logprobs:
            return toks
        assert self.logprobs_top is not None
        return toks, lps

    def reset(self, slot):
        del self.pos[slot], self.who[slot]


def _want(p, k, max_new):
    toks, lps = [], []
    for t in range(max_new):
        toks.append(_tok(p, k, t)); lps.append(_lp(p, k, t))
        if toks[-1] == EOS:
            break
    return toks, lps


def test_best_of_returns_the_best_first_with_ties_to_the_lower_index(omx):
    """two prompts, 4 siblings each over 4 slots, the best 3 kept: mean log-probabilities -0.125 (sibling 2), -0.25 (sibling 1, over
    the three tokens it keeps: the -64 its slot decoded past EOS would sink it) and -0.25 (sibling 3): 2, then 1 before 3"""
    from ominix_mlx_amd import generate
    fake = FakeBatch(4)
    outs, lps = generate.generate_batch(fake, [[1, 2], [3]], 6, eos_ids=[EOS], chunk=4, n=3, best_of=4, before_sibling=fake.tag,
                                        return_logprobs=True)
    assert ("set_logprobs", 0) in fake.calls
    assert len(outs) == len(lps) == 6
    for p in range(2):
        for rank, k in enumerate([2, 1, 3]):
            toks, want_lp = _want(p, k, 6)
            assert outs[p * 3 + rank] == toks
            assert lps[p * 3 + rank] == want_lp
    assert len(outs[1]) == 3 and outs[1][-1] == EOS            # truncated at EOS, the log-probabilities with the tokens
    # without return_logprobs: the same completions alone
    fake = FakeBatch(4)
    assert generate.generate_batch(fake, [[1, 2], [3]], 6, eos_ids=[EOS], chunk=4, n=3, best_of=4, before_sibling=fake.tag) == outs
    # best_of = n: nobody is dropped, the order is still best first
    fake = FakeBatch(4)
    outs4 = generate.generate_batch(fake, [[5]], 6, eos_ids=[EOS], chunk=4, n=4, best_of=4, before_sibling=fake.tag)
    assert outs4 == [_want(0, k, 6)[0] for k in (2, 1, 3, 0)]


def test_return_logprobs_keeps_prompt_major_order_and_an_on_setting(omx):
    """n = 2 without best_of: siblings 0, 1 of every prompt in order, a log-probability per kept token; a batch whose logprobs are
    already on (with alternatives) keeps its setting"""
    from ominix_mlx_amd import generate
    fake = FakeBatch(4)
    fake.set_logprobs(5)
    outs, lps = generate.generate_batch(fake, [[1], [2], [3]], 5, eos_ids=[EOS], chunk=2, n=2, before_sibling=fake.tag, return_logprobs=True)
    assert fake.calls == [("set_logprobs", 5)]
    assert [(o, l) for o, l in zip(outs, lps)] == [_want(p, k, 5) for p in range(3) for k in range(2)]
    assert all(len(o) == len(l) for o, l in zip(outs, lps))


def test_best_of_must_lie_between_n_and_the_slots(omx):
    from ominix_mlx_amd import generate
    for n, m in ((3, 2), (2, 5), (1, 0)):
        with pytest.raises(ValueError, match=f"best_of = {m} must be in n = {n}..4"):
            generate.generate_batch(FakeBatch(4), [[1]], 4, n=n, best_of=m)


class FakeModel:
    """engine.Model's interface as Generate drives it: token t of the stream is 50 + t with log-probability -(t + 1) / 8 and two
    alternatives"""

    def __init__(self):
        self.logprobs_top, self.t, self.calls = None, 0, []

    def set_sampler(self, temp, seed=0, **filters):
        self.calls.append(("set_sampler", temp, seed))

    def set_logprobs(self, top_n=None):
        self.logprobs_top = top_n
        self.calls.append(("set_logprobs", top_n))

    def _row(self, t):
        top = self.logprobs_top or 0
        return np.float32(-(t + 1) / 8), np.arange(50 + t, 50 + t + top, dtype=np.uint32), np.float32(-(t + 1) / 8) - np.arange(top, dtype=np.float32)

    def prefill(self, prompt):
        self.t = 1
        return 50

    def last_logprobs(self):
        row = self._row(self.t - 1)
        return row if self.logprobs_top else row[0]

    def decode(self, n, return_logprobs=False):
        ts = range(self.t, self.t + n)
        self.t += n
        toks = np.array([50 + t for t in ts], np.uint32)
        if not return_logprobs:
            return toks
        assert self.logprobs_top is not None
        rows = [self._row(t) for t in ts]
        lp = np.array([r[0] for r in rows], np.float32)
        return (toks, lp, np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])) if self.logprobs_top else (toks, lp)


class FakeTokenizer:
    def decode(self, ids, skip_special_tokens=True):
        return "".join(f"<{int(i)}>" for i in ids)


@pytest.mark.parametrize("k", [None, 0, 2])
def test_generate_text_passes_logprobs_through(omx, k):
    from ominix_mlx_amd import generate
    m = FakeModel()
    out = generate.generate_text(m, FakeTokenizer(), "", temperature=0.0, max_tokens=7, flush_every=3, prompt_ids=[1, 2, 3], logprobs=k)
    assert out["tokens"] == [50 + t for t in range(7)] and out["text"] == "".join(f"<{50 + t}>" for t in range(7))
    if k is None:
        assert "logprobs" not in out and "top_logprobs" not in out and ("set_logprobs", None) not in m.calls
        return
    assert ("set_logprobs", k) in m.calls
    assert out["logprobs"] == [-(t + 1) / 8 for t in range(7)]
    assert out["top_logprobs"] == [[(50 + t + j, -(t + 1) / 8 - j) for j in range(k)] for t in range(7)]
