"""The arena digest (include/gmk.h, gmk_arena_digest) restated as a loop over Python integers: the reference of ops.arena_digest (HIP) and of
checkpoint.digest_host (numpy).

    digest = sum_i mix(w_i + (i + 1) * 0x9E3779B97F4A7C15)  mod 2^64,      w_i: the i-th 4-byte little-endian word of the buffer, i from 0
    mix    = splitmix64's finaliser"""
import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15

# words -> digest, computed with this loop and with an independent numpy restatement
KNOWN = [([0], 0xe220a8397b1dcdaf), ([0, 0], 0x509946a41cd733a3), ([1, 2, 3], 0xedbe5ca3654f5804)]
KNOWN_ARANGE_1000_F32 = 0xc5b134e9adb17b4d          # np.arange(1000, dtype=float32)


def mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def digest_words(words):
    total = 0
    for i, w in enumerate(words):
        total += mix((int(w) + (i + 1) * GOLDEN) & MASK)
    return total & MASK


def prefix_digests(words, lengths):
    """{n: digest_words(words[:n])} for every n in `lengths`, in ONE pass over the words (the same loop, read off where a prefix ends)."""
    want, out, total = set(lengths), {}, 0
    assert want and min(want) >= 1 and max(want) <= len(words)
    term = 0
    for i, w in enumerate(words[:max(want)], 1):           # `mix` written out: this loop runs over millions of words
        term += GOLDEN
        x = (w + term) & MASK
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & MASK
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & MASK
        total += x ^ (x >> 31)
        if i in want:
            out[i] = total & MASK
    return out


def words_of(array):
    """The 4-byte little-endian words of a numpy array's bytes (C order), as Python integers."""
    raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
    assert raw.size and raw.size % 4 == 0
    return raw.view("<u4").tolist()


def digest(array):
    return digest_words(words_of(array))
