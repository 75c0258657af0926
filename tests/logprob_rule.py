"""Host arithmetic the log-probability tests hold the device to: a float64 log-softmax over exactly representable inputs (bf16
logits widened), nothing of the device's chunking in it."""
import numpy as np

NO_TARGET = 0xFFFFFFFF
CHUNK = 1024


def logsumexp64(x):
    """log sum exp over the last axis, float64"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def logprob64(x, targets):
    """(log p(target) per row, lse per row) in float64; a NO_TARGET row's log-probability is 0"""
    x = np.asarray(x, dtype=np.float64)
    lse = logsumexp64(x)
    t = np.asarray(targets, dtype=np.int64)
    has = t != NO_TARGET
    lp = np.zeros(x.shape[0], dtype=np.float64)
    rows = np.nonzero(has)[0]
    lp[rows] = x[rows, t[rows]] - lse[rows]
    return lp, lse


def bf16_round(x):
    """float32 values rounded to the nearest bf16 (ties to even), still float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7FFF)
    return (((u + r) >> np.uint64(16)) << np.uint64(16)).astype(np.uint32).view(np.float32).reshape(np.shape(x))
