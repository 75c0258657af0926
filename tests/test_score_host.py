"""generate.perplexity, the strided evaluation over model.reset / model.score, on a fake model that records its calls (no GPU): every
target is counted exactly once, each from the window that reaches it first, and ppl = exp(nll / tokens)."""
import math

import numpy as np
import pytest


class FakeModel:
    """score(tokens, next_token)[i] = -(2^-t + 8 c) for the target at text position t with c tokens of context in this window: what
    perplexity summed tells which targets it took, and from which window.  Token ids are their own positions in the text."""

    def __init__(self):
        self.calls = []
        self.fresh = False

    def reset(self):
        self.fresh = True

    def score(self, tokens, next_token=None, return_greedy=False):
        assert self.fresh, "perplexity scores every window from an empty cache"
        assert not return_greedy
        self.fresh = False
        tokens = [int(t) for t in tokens]
        self.calls.append((tokens, next_token))
        targets = tokens[1:] + ([] if next_token is None else [int(next_token)])
        return np.array([-(2.0 ** -t + 8.0 * (i + 1)) for i, t in enumerate(targets)], dtype=np.float32)


@pytest.mark.parametrize("n,ctx,stride", [(10, 4, 2), (9, 4, 4), (3, 8, None)])
def test_every_target_is_counted_exactly_once(omx, n, ctx, stride):
    from ominix_mlx_amd import generate
    m = FakeModel()
    res = generate.perplexity(m, list(range(n)), ctx=ctx, stride=stride)
    step = ctx if stride is None else stride
    # the windows: ids[b : b + ctx] at multiples of the stride until every target is covered, the token behind a window its last target
    want_calls, covered, b = [], 0, 0
    while covered < n - 1:
        end = min(b + ctx, n)
        want_calls.append((list(range(b, end)), end if end < n else None))
        covered = min(end, n - 1)
        b += step
    assert m.calls == want_calls
    # target t is taken from the FIRST window that reaches it; there it has t - b tokens of context
    want_nll = 0.0
    for t in range(1, n):
        b = next(c[0][0] for c in want_calls if c[0][0] < t <= (c[0][-1] if c[1] is None else c[1]))
        want_nll += 2.0 ** -t + 8.0 * (t - b)
    assert res["tokens"] == n - 1
    assert res["nll"] == pytest.approx(want_nll, rel=1e-6)
    # the binary fractions 2^-t identify the counted targets one by one: each of 1 .. n - 1 exactly once
    assert res["nll"] % 8.0 == pytest.approx(sum(2.0 ** -t for t in range(1, n)), abs=1e-4)
    assert res["ppl"] == pytest.approx(math.exp(res["nll"] / res["tokens"]))


def test_ppl_is_exp_of_the_mean_nll(omx):
    from ominix_mlx_amd import generate

    class Flat(FakeModel):
        def score(self, tokens, next_token=None, return_greedy=False):
            self.fresh = False
            return np.full(len(tokens) - (next_token is None), -1.25, dtype=np.float32)

    res = generate.perplexity(Flat(), list(range(11)), ctx=4, stride=3)
    assert res["tokens"] == 10 and res["nll"] == pytest.approx(12.5) and res["ppl"] == pytest.approx(math.exp(1.25))


def test_refusals(omx):
    from ominix_mlx_amd import generate
    for ids in ([], [5]):
        with pytest.raises(ValueError, match="at least 2 tokens"):
            generate.perplexity(FakeModel(), ids)
    with pytest.raises(ValueError, match="stride"):
        generate.perplexity(FakeModel(), [1, 2, 3], ctx=4, stride=5)
    with pytest.raises(ValueError, match="stride"):
        generate.perplexity(FakeModel(), [1, 2, 3], ctx=4, stride=0)
