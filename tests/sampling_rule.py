"""The filtered-sampling rule (include/omx.h, omx_sample_filtered) restated in numpy, shared by tests/test_sampling_rule.py (CPU) and
tests/test_gpu_sampling.py (GPU).  Every step up to the thresholds is one IEEE float32 operation per element, in the order

    1. x = f32(logit)                                   4. y = x * f32(1/T)
    2. seen, r != 1:  x = x > 0 ? x / r : x * r         5. top-k: keep y >= k-th largest y (ties at the threshold all kept)
    3. seen, q != 0:  x = x - q                         6. top-p on the survivors: keep v iff mass{survivors with y > y_v} < p * Z
                                                        7. token = first argmax over the kept set of y + gumbel(word v of a V-word draw)

The masses of step 6 are float64 here (`mass64`): the device sums exp(y - max) exactly in fixed point, its only error is expf's, and
the GPU tests hold it between this rule at p - delta and at p + delta."""
import numpy as np

from oracle import mlx_rng


def scaled(logits, temperature, seen_ids=(), repetition_penalty=1.0, presence_penalty=0.0) -> np.ndarray:
    """Steps 1-4 for one row: float32 y.  temperature 0 returns x after steps 2-3 (the greedy branch takes its argmax)."""
    x = np.array(logits, dtype=np.float32).copy()
    ids = np.asarray(list(seen_ids), dtype=np.int64)
    if ids.size:
        r, q = np.float32(repetition_penalty), np.float32(presence_penalty)
        if r != np.float32(1.0):
            s = x[ids]
            x[ids] = np.where(s > 0, (s / r).astype(np.float32), (s * r).astype(np.float32))
        if q != np.float32(0.0):
            x[ids] = (x[ids] - q).astype(np.float32)
    if temperature == 0.0:
        return x
    inv = np.float32(np.float32(1.0) / np.float32(temperature))
    return (x * inv).astype(np.float32)


def topk_threshold(y, top_k):
    """Step 5: (threshold, kept mask).  top_k == 0 or >= V: off (-inf, everything)."""
    y = np.asarray(y, np.float32)
    if top_k <= 0 or top_k >= y.size:
        return np.float32(-np.inf), np.ones(y.shape, bool)
    thr = np.partition(y, y.size - top_k)[y.size - top_k]
    return np.float32(thr), y >= thr


def topp_mask(y, survivors, top_p):
    """Step 6 in float64: among `survivors`, keep v iff the mass of survivors strictly greater than y_v is < top_p * Z."""
    y = np.asarray(y, np.float32)
    if top_p >= 1.0:
        return survivors.copy()
    ys = y[survivors].astype(np.float64)
    vals, inv = np.unique(ys, return_inverse=True)            # ascending distinct values: a tie group shares its fate
    mass = np.bincount(inv, weights=np.exp(ys - ys.max()), minlength=vals.size)
    z = mass.sum()
    above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])   # mass strictly above each distinct value
    keep_val = above < np.float64(top_p) * z
    out = np.zeros(y.shape, bool)
    out[np.flatnonzero(survivors)] = keep_val[inv]
    return out


def kept_mask(y, top_k=0, top_p=1.0):
    """Steps 5-6: (final threshold on y, kept mask); the kept set is exactly {y >= threshold}."""
    thr, mask = topk_threshold(y, top_k)
    mask = topp_mask(y, mask, top_p)
    if top_p < 1.0:
        thr = np.float32(np.asarray(y, np.float32)[mask].min())
    return thr, mask


def draw(y, mask, key, row=0, rows=1) -> int:
    """Step 7: first argmax over `mask` of y + gumbel, the noise of entry v being word row*V + v of a rows*V-word draw from `key`."""
    y = np.asarray(y, np.float32)
    g = mlx_rng.gumbel((rows, y.size), key)[row]
    return int(np.argmax(np.where(mask, (y + g).astype(np.float32), np.float32(-np.inf))))


def sample(logits, temperature, key, *, top_k=0, top_p=1.0, repetition_penalty=1.0, presence_penalty=0.0, seen_ids=()):
    """The whole rule for one row: (token, threshold, kept count)."""
    y = scaled(logits, temperature, seen_ids, repetition_penalty, presence_penalty)
    if temperature == 0.0:
        return int(np.argmax(y)), np.float32(-np.inf), y.size
    thr, mask = kept_mask(y, top_k, top_p)
    return draw(y, mask, key), thr, int(mask.sum())
