"""Host restatement (NumPy only, no GPU import) of the project's random streams: Random123 Philox4x32-10 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC 2011) with counter {lo, hi, 0, 0} and key {seed_lo, seed_hi}, and the element mapping include/gmk.h
documents: element i of stream (seed, offset) is component i % 4 of counter (offset + i // 4) mod 2^64.

`philox4x32_10` is checked against the published Random123 known-answer vectors in tests/test_host_philox.py; the device streams and every
in-kernel consumer are checked against this file in tests/test_gpu_philox.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
ROUNDS = 10
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """-> 4 uint32 arrays.  Counter words and key words: ints or integer arrays below 2^32 (broadcast together).  uint64 arithmetic, masked to
    32 bits: a 32 x 32 bit product fits 64 bits exactly."""
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(ROUNDS):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(seed, offset, nq):
    """The 4 nq words of counters offset .. offset + nq - 1 (mod 2^64) of stream `seed`, flattened: element i is component i % 4 of counter
    offset + i // 4.  seed, offset: Python ints in [0, 2^64)."""
    seed, offset, nq = int(seed), int(offset), int(nq)
    assert 0 <= seed <= MASK64 and 0 <= offset <= MASK64 and nq >= 0
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset) + np.arange(nq, dtype=np.uint64)          # uint64 addition wraps modulo 2^64
    out = philox4x32_10(ctr & np.uint64(MASK32), ctr >> np.uint64(32), 0, 0, seed & MASK32, seed >> 32)
    return np.stack(out, axis=1).reshape(-1)


def _nq(n):
    return (int(n) + 3) // 4


def _u24(w):
    """The 24-bit integer behind u01: the word's top 24 bits."""
    return (w >> np.uint32(8)).astype(np.int64)


def uniform(seed, offset, n):
    """float32 [n] in [0, 1): (w >> 8) 2^-24, exact (every value lies on the 24-bit grid)."""
    return (_u24(words(seed, offset, _nq(n))[:n]).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def normal(seed, offset, n):
    """float64 [n]: Box-Muller on the word pairs (w0, w1) and (w2, w3) of each counter: u1 = 1 - u01(w_even) in (0, 1], u2 = u01(w_odd),
    (sqrt(-2 ln u1) cos 2 pi u2, sqrt(-2 ln u1) sin 2 pi u2)."""
    w = _u24(words(seed, offset, _nq(n))).reshape(-1, 2)
    u1 = 1.0 - w[:, 0].astype(np.float64) * 2.0 ** -24
    u2 = w[:, 1].astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.stack((rad * np.cos(ang), rad * np.sin(ang)), axis=1).reshape(-1)[:n]


def rademacher(seed, offset, n):
    """float32 [n]: +1 where the uniform is >= 1/2, else -1."""
    return np.where(uniform(seed, offset, n) >= np.float32(0.5), np.float32(1.0), np.float32(-1.0))


def keep_mask(seed, offset, n, p):
    """bool [n]: the elements nn.Dropout(p) keeps, u >= float32(p)."""
    return uniform(seed, offset, n) >= np.float32(p)


def label_drop_mask(seed, offset, n, p):
    """bool [n]: the labels classifier-free training drops, u < float32(p)."""
    return uniform(seed, offset, n) < np.float32(p)
