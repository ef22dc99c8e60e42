"""The inputs the tests of include/world_class_parallel.h share (a helper, not a test module): the ragged batch of seven pairs of
tests/test_gpu_parallel.py, its hand-written paths, masks and rows, and the planted pair of speakers of the chain test."""
import numpy as np

DIMS, DIM_BEGIN = 5, 1
# (a, b): five aligned pairs, the pair whose path is written by hand (a staircase with K = cap), the pair with a NaN row (K = 0)
PAIRS = [(1, 1), (1, 9), (63, 65), (64, 64), (257, 130), (40, 30), (12, 10)]
HAND, BAD = 5, 6
GARBAGE = -7          # what stands in a path entry nobody wrote


def lengths():
    return [a for a, _ in PAIRS], [b for _, b in PAIRS]


def offsets():
    A, B, P, fa, fb, p = [], [], [], 0, 0, 0
    for a, b in PAIRS:
        A.append(fa), B.append(fb), P.append(p)
        fa, fb, p = fa + a, fb + b, p + a + b - 1
    return A, B, P, fa, fb, p


def staircase(a, b):
    """a + b - 1 cells from (0, 0) to (a - 1, b - 1) that step in one index at a time, in turns while both can"""
    cells, i, j, turn = [(0, 0)], 0, 0, 0
    while (i, j) != (a - 1, b - 1):
        if i < a - 1 and (turn == 0 or j == b - 1):
            i += 1
        else:
            j += 1
        turn ^= 1
        cells.append((i, j))
    assert len(cells) == a + b - 1
    return np.array(cells, dtype=np.int32)


def features(seed=3):
    """the alignment's features [frames, DIMS] of both sides: B is A's trajectory on a bent time axis plus noise; the last pair's A
    holds a NaN row"""
    rng = np.random.default_rng(seed)
    fa, fb = [], []
    for a, b in PAIRS:
        n = 4 * max(a, b) + 8
        base = np.cumsum(rng.normal(size=(n, DIMS)), axis=0) * 0.3
        ta = np.linspace(0.0, n - 1.0, a) if a > 1 else np.array([0.0])
        tb = (np.linspace(0.0, 1.0, b) ** 1.3) * (n - 1.0) if b > 1 else np.array([0.0])
        pick = lambda t: np.stack([np.interp(t, np.arange(n), base[:, c]) for c in range(DIMS)], axis=1)
        fa.append(pick(ta))
        fb.append(pick(tb) + 0.05 * rng.normal(size=(b, DIMS)))
    fa[BAD][3, 2] = np.nan
    return np.concatenate(fa), np.concatenate(fb)


def with_hand_paths(path_length, path):
    """the alignment's outputs with the hand-written pair's staircase in place (K = cap)"""
    _, _, P, _, _, _ = offsets()
    a, b = PAIRS[HAND]
    path_length, path = np.array(path_length, dtype=np.int32), np.array(path, dtype=np.int32).reshape(-1, 2)
    path[P[HAND]:P[HAND] + a + b - 1] = staircase(a, b)
    path_length[HAND] = a + b - 1
    return path_length, path


def rule_paths(feat_a, feat_b):
    """what the device's alignment writes, from tests/align_rule.py: path lengths, and the packed path with GARBAGE behind K"""
    import align_rule as al
    A, B, P, _, _, total = offsets()
    path_length, path, cost = np.zeros(len(PAIRS), dtype=np.int32), np.full((total, 2), GARBAGE, dtype=np.int32), np.zeros(len(PAIRS))
    for u, (a, b) in enumerate(PAIRS):
        r = al.align(feat_a[A[u]:A[u] + a], feat_b[B[u]:B[u] + b], DIM_BEGIN, DIMS)
        k = len(r["path"])
        path_length[u], cost[u] = k, r["cost"]
        path[P[u]:P[u] + k] = r["path"]
    return path_length, path, cost


def spoiled(path_length, path):
    """a path a caller wrote badly: K = -1, K = cap + 1, an entry with i = a and one with j = -1 (in pairs that are otherwise fine)"""
    _, _, P, _, _, _ = offsets()
    path_length, path = path_length.copy(), path.copy()
    path_length[1] = -1
    path_length[2] = PAIRS[2][0] + PAIRS[2][1]
    path[P[3] + 5, 0] = PAIRS[3][0]
    path[P[4] + 9, 1] = -1
    path[P[4] + 11] = (2 ** 31 - 1, -2 ** 31)
    return path_length, path


def masks(seed=5):
    """a mask per side with zeros of several byte values' complement: bytes are 0 or anything else"""
    _, _, _, fa, fb, _ = offsets()
    rng = np.random.default_rng(seed)
    ma = (rng.random(fa) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=fa).astype(np.uint8)
    mb = (rng.random(fb) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=fb).astype(np.uint8)
    return ma, mb


def rows(frames, ld, dtype, seed):
    """rows to gather from: every element its own value, with a -0.0, an inf and a NaN among them"""
    x = np.random.default_rng(seed).normal(size=(frames, ld)) * 1e3
    x[0, 0], x[frames // 2, ld - 1], x[frames - 1, ld // 2] = -0.0, np.inf, np.nan
    return x.astype(dtype)


def long_staircase(seed=8):
    """(a, b) = (700, 700), cap = 1 399, K = cap: rows whose distances along the staircase span 12 orders of magnitude"""
    a = b = 700
    rng = np.random.default_rng(seed)
    xa = rng.normal(size=(a, 3))
    xb = xa + rng.normal(size=(b, 3)) * 10.0 ** rng.uniform(-6.0, 6.0, size=(b, 1))
    return a, b, xa, xb, staircase(a, b)


# ---- the planted pair of speakers of the chain test ---------------------------------------------------------------------------------
ND, ORDERS, N_MIX = 6, 2, 4
CHAIN_A = (90, 60, 120)


def planted_speakers(seed=31):
    """three utterances of speaker A (coded envelopes [n, ND] with silence at both ends, f0) and of speaker B: A's rows on a bent
    time axis, sent through a fixed affine map, plus small noise.  -> dict of lengths, f0 and sp per side, and the map"""
    rng = np.random.default_rng(seed)
    M = np.eye(ND) * 0.6 + 0.25 * rng.normal(size=(ND, ND))
    M[0, :], M[:, 0] = 0.0, 0.0
    M[0, 0] = 1.0                      # c0 keeps its level: silence stays silence
    shift = np.concatenate([[0.0], 2.0 + rng.normal(size=ND - 1)])
    a_lengths, b_lengths, sp_a, sp_b = [], [], [], []
    for n in CHAIN_A:
        m = int(round(n * rng.uniform(0.8, 1.2)))
        m = min(max(m, 60), 120)
        base = np.cumsum(rng.normal(size=(n, ND)), axis=0) * 0.4
        base[:, 0] = -4.0 + 0.3 * rng.normal(size=n)
        base[:6, 0] -= 12.0            # silence: 12 units of c0 are about 52 dB
        base[-6:, 0] -= 12.0
        t = (np.linspace(0.0, 1.0, m) ** 1.2) * (n - 1.0)
        warped = np.stack([np.interp(t, np.arange(n), base[:, c]) for c in range(ND)], axis=1)
        a_lengths.append(n), b_lengths.append(m)
        sp_a.append(base)
        sp_b.append(warped @ M.T + shift + 0.02 * rng.normal(size=(m, ND)))
    return dict(a_lengths=a_lengths, b_lengths=b_lengths, sp_a=np.concatenate(sp_a), sp_b=np.concatenate(sp_b),
                f0_a=np.full(sum(a_lengths), 120.0), f0_b=np.full(sum(b_lengths), 200.0), M=M, shift=shift)
