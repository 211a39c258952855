"""CPU tests (no GPU) of the random streams' contract: the host restatement (tests/philox_ref.py) against the published Random123 known-answer
vectors of philox4x32-10, its counter / key layout (2^64 wrap, carry into the high counter word, the seed's high half in k1), the counter
ranges `PhiloxStream` reserves, and the seed / offset check of the wrappers that take a stream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref  # noqa: E402

# Random123 kat_vectors, philox4x32 10 rounds: (counter; key) -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_reference_reproduces_the_random123_known_answer_vectors():
    for ctr, key, want in KAT:
        got = philox_ref.philox4x32_10(*ctr, *key)
        assert all(g.dtype == np.uint32 for g in got)
        assert tuple(int(g) for g in got) == want, [hex(int(g)) for g in got]
    # vectorised: the three at once, as arrays
    cols = [np.array([k[0][i] for k in KAT]) for i in range(4)] + [np.array([k[1][i] for k in KAT]) for i in range(2)]
    got = np.stack(philox_ref.philox4x32_10(*cols), axis=1)
    assert got.tolist() == [list(k[2]) for k in KAT]


def _one(c_lo, c_hi, k0, k1):
    return [int(v) for v in philox_ref.philox4x32_10(c_lo, c_hi, 0, 0, k0, k1)]


def test_words_layout_carry_wrap_and_key_halves():
    # element i = component i % 4 of counter offset + i // 4; the first known-answer vector is (seed 0, offset 0)
    w = philox_ref.words(0, 0, 3)
    assert w.dtype == np.uint32 and w.shape == (12,)
    assert w[:4].tolist() == list(KAT[0][2])
    assert w[4:8].tolist() == _one(1, 0, 0, 0) and w[8:].tolist() == _one(2, 0, 0, 0)
    # the carry from the low into the high counter word inside one call
    w = philox_ref.words(7, (1 << 32) - 2, 4)
    assert w.reshape(4, 4).tolist() == [_one(0xfffffffe, 0, 7, 0), _one(0xffffffff, 0, 7, 0), _one(0, 1, 7, 0), _one(1, 1, 7, 0)]
    assert w[8:12].tolist() != _one(0, 0, 7, 0)                                     # the high word is used
    # the wrap at 2^64
    w = philox_ref.words(7, (1 << 64) - 2, 4)
    assert w.reshape(4, 4).tolist() == [_one(0xfffffffe, 0xffffffff, 7, 0), _one(0xffffffff, 0xffffffff, 7, 0), _one(0, 0, 7, 0), _one(1, 0, 7, 0)]
    assert w[8:].tolist() == philox_ref.words(7, 0, 2).tolist()
    # the seed's low half is k0, its high half k1
    seed = (0x299f31d0 << 32) | 0xa4093822
    assert philox_ref.words(seed, (5 << 32) | 9, 1).tolist() == _one(9, 5, 0xa4093822, 0x299f31d0)
    assert philox_ref.words(1 << 32, 0, 1).tolist() == _one(0, 0, 0, 1) != philox_ref.words(1, 0, 1).tolist()
    # the second known-answer vector has c2 = c3 = ffffffff, which no stream reaches: the streams keep c2 = c3 = 0
    assert philox_ref.words((1 << 64) - 1, (1 << 64) - 1, 1).tolist() == _one(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)


def test_derived_draws():
    seed, off = (1 << 63) + 12345, (1 << 40) + 7
    for n in (1, 2, 3, 4, 5, 13):
        w = philox_ref.words(seed, off, (n + 3) // 4)[:n]
        u = philox_ref.uniform(seed, off, n)
        assert u.dtype == np.float32 and u.shape == (n,)
        assert u.tolist() == [(int(v) >> 8) / 2 ** 24 for v in w]                    # exact: 24-bit grid
        z = philox_ref.normal(seed, off, n)
        assert z.dtype == np.float64 and z.shape == (n,)
        assert np.array_equal(philox_ref.rademacher(seed, off, n), np.where(u >= 0.5, 1.0, -1.0).astype(np.float32))
        assert np.array_equal(philox_ref.keep_mask(seed, off, n, 0.25), u >= np.float32(0.25))
        assert np.array_equal(philox_ref.label_drop_mask(seed, off, n, 0.1), u < np.float32(0.1))
    # Box-Muller by hand on the first counter: pairs (w0, w1), (w2, w3); cos first
    w = [int(v) >> 8 for v in philox_ref.words(seed, off, 1)]
    want = []
    for a, b in ((w[0], w[1]), (w[2], w[3])):
        rad = np.sqrt(-2.0 * np.log(1.0 - a / 2 ** 24))
        want += [rad * np.cos(2 * np.pi * b / 2 ** 24), rad * np.sin(2 * np.pi * b / 2 ** 24)]
    assert np.allclose(philox_ref.normal(seed, off, 4), want, rtol=0, atol=1e-14)
    # u1 = 1 - u lies in (0, 1]: a zero word gives radius 0, never log 0
    assert np.isfinite(philox_ref.normal(0, 0, 4099)).all()


def test_philox_stream_reserves_adjacent_disjoint_counter_ranges(monkeypatch):
    """Each draw of n values takes ceil(n / 4) counters, starting where the one before ended - through the public draws (the wrappers
    replaced by recorders) and through `_take` itself."""
    from generative_models_amd.diffusion import gaussian_diffusion as gd
    calls = []
    monkeypatch.setattr(gd.ops, "rng_normal", lambda shape, seed, offset, device: calls.append(("normal", shape, seed, offset)))
    monkeypatch.setattr(gd.ops, "rng_uniform", lambda shape, seed, offset, device: calls.append(("uniform", shape, seed, offset)))
    seed = (1 << 63) + 5
    rng = gd.PhiloxStream(seed)
    shapes = [(1,), (3,), (4,), (5,), (3, 784), (1, 1), (2, 1, 28, 28)]
    sizes = [int(np.prod(s)) for s in shapes]
    assert sizes[:5] == [1, 3, 4, 5, 784 * 3]
    for k, s in enumerate(shapes):
        (rng.normal if k % 2 else rng.uniform)(s, "cpu")
    assert [c[0] for c in calls] == ["uniform", "normal"] * 3 + ["uniform"]
    assert [c[1] for c in calls] == shapes and all(c[2] == seed for c in calls)
    start = 0
    for c, n in zip(calls, sizes):
        assert c[3] == start                          # adjacent: begins where the previous range ended; disjoint: the ranges tile [0, total)
        start += -(-n // 4)
    assert rng.counter == start == 1 + 1 + 1 + 2 + 588 + 1 + 392
    assert rng._take(784 * 3) == start and rng._take(1) == start + 588 and rng.counter == start + 589
    assert gd.PhiloxStream(-1).seed == (1 << 64) - 1 and gd.PhiloxStream((1 << 64) + 3).seed == 3      # seeds are reduced modulo 2^64


def test_stream_wrappers_reject_seeds_and_offsets_outside_64_bits():
    """ctypes would wrap a negative or oversize int into c_uint64 silently - another stream than the one asked for.  The check comes before
    any tensor is looked at, so CPU arguments do."""
    from generative_models_amd import ops
    x = torch.zeros((3, 5))
    y = torch.zeros((6,), dtype=torch.int64)
    z = torch.zeros((3, 1, 4, 4))
    m = torch.ones((3, 16), dtype=torch.uint8)
    calls = {"rng_normal": lambda s, o: ops.rng_normal((4,), s, o, "cpu"),
             "rng_uniform": lambda s, o: ops.rng_uniform((4,), s, o, "cpu"),
             "rng_rademacher": lambda s, o: ops.rng_rademacher((4,), s, o, "cpu"),
             "dequantize": lambda s, o: ops.dequantize(x, 0.5, s, o),
             "label_drop": lambda s, o: ops.label_drop(y, 0.1, s, o),
             "inpaint_merge": lambda s, o: ops.inpaint_merge(z, z, m, 0.8, 0.6, 0.5, 0.7, False, False, -1.0, 1.0, s, o)}
    for name, call in calls.items():
        for seed, off in ((-1, 0), (1 << 64, 0), (0, -1), (0, 1 << 64), (-(1 << 63), 5), (7, (1 << 64) + 5)):
            with pytest.raises(ValueError, match="unsigned 64-bit"):
                call(seed, off)
    # the largest legal values pass the check: what stops these calls is the next one (no device tensor here)
    top = (1 << 64) - 1
    for name in ("dequantize", "label_drop", "inpaint_merge"):
        with pytest.raises(ValueError, match="device tensor"):
            calls[name](top, top)
    assert ops.check_stream(np.int64(5), torch.tensor(7)) == (5, 7) and ops.check_stream(top, top) == (top, top)
