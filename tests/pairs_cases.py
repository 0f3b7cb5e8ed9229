"""Offer sequences for the L-BFGS pair store, shared by tests/test_pairs_rule.py (CPU) and tests/test_gpu_pairs.py.

The (x, g) generator is that of tests/test_gpu_lbfgs.py:_storage -- an SPD curvature model H = Mq Mq' + I/2 applied
matrix-free, g = -H x -- with steps whose ``hv`` is negated mixed in: such a pair has dg.dx < 0 and is skipped.
Every sequence is 3 (memory + 1) + 2 offers long."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
ROOT_EPS = float(np.sqrt(EPS))
G_EXTRA = 3                      # the loop passes gradients of length n + 2 mi + me: g is longer than n


def signs(memory, pattern):
    """+1: a pair of positive curvature, -1: a negated one.
    "accepts": two single skips among accepts -- the store fills and drops 2 memory + 2 times;
    "reset":   accept, skip, accept, then memory + 1 skips in a row (reset of a non-empty store), then regrowth past full;
    "empty":   memory + 1 skips on the EMPTY store (no reset), then accepts past full."""
    total = 3 * (memory + 1) + 2
    if pattern == "accepts":
        s = [1] * total
        s[2] = s[2 * memory + 3] = -1
    elif pattern == "reset":
        s = [1, -1, 1] + [-1] * (memory + 1)
        s += [1] * (total - len(s))
    elif pattern == "empty":
        s = [-1] * (memory + 1)
        s += [1] * (total - len(s))
    else:
        raise ValueError(pattern)
    assert len(s) == total
    return s


def offers(n, memory, pattern, seed):
    """[(x_old, x_new, g_old, g_new)] -- g_* of length n + G_EXTRA."""
    rng = np.random.default_rng(seed)
    Mq = rng.standard_normal((n, 32)) / np.sqrt(32.0)
    hv = lambda v: Mq @ (Mq.T @ v) + 0.5 * v           # noqa: E731
    x_old = rng.standard_normal(n)
    out = []
    for sg in signs(memory, pattern):
        x_new = x_old + rng.standard_normal(n) / np.sqrt(n)
        tail = rng.standard_normal((2, G_EXTRA))
        g_old = np.concatenate([-sg * hv(x_old), tail[0]])
        g_new = np.concatenate([-sg * hv(x_new), tail[1]])
        out.append((x_old, x_new, g_old, g_new))
        x_old = x_new
    return out


def seed_of(n, memory, constrained, pattern):
    return 1000003 * n + 101 * memory + 7 * ("accepts", "reset", "empty").index(pattern) + int(constrained)
