"""numpy float32 restatement of gmk_loss_profile and gmk_u_importance, operation for operation, and a float64 inverse CDF (test infrastructure;
written from the definitions in include/gmk.h, not from the kernels).

Every arithmetic step below is ONE operation on np.float32 operands, which numpy rounds correctly - the kernels' __fadd_rn / __fmul_rn /
__fdiv_rn / sqrt in the same order - so the results agree bit for bit.

State: fp32 [5][64] - row 0 W (decayed sample count), rows 1, 2 (S1, S2) of value channel 0, rows 3, 4 of value channel 1.
"""
import numpy as np

BINS = 64
F = np.float32
ONE_BELOW = F(1.0 - 2.0 ** -24)
INV = F(2.0 ** -6)


def loss_profile(state, u, v0, v1, decay):
    """-> the new state (a copy).  Sample b: bin min(int(fmul(u, 64)), 63), skipped when u is outside [0, 1) or a value is not finite; per bin in
    ascending b: n, a_c = sequential sum of v_c from 0, q_c = sequential sum of fmul(v_c, v_c); a bin with n > 0 takes
    W = fadd(fmul(decay, W), n), S1_c = fadd(fmul(decay, S1_c), a_c), S2_c likewise; other bins, and rows 3, 4 without v1, keep their bits."""
    state = np.array(state, dtype=F).reshape(5, BINS).copy()
    u, v0 = np.asarray(u, dtype=F).reshape(-1), np.asarray(v0, dtype=F).reshape(-1)
    v1 = None if v1 is None else np.asarray(v1, dtype=F).reshape(-1)
    decay = F(decay)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = (u >= F(0)) & (u < F(1)) & np.isfinite(v0)
        if v1 is not None:
            keep &= np.isfinite(v1)
        bins = np.minimum((u * F(64)).astype(np.int64, copy=False), BINS - 1)
        n = np.zeros(BINS, dtype=np.int64)
        acc = np.zeros((4, BINS), dtype=F)                 # a0, q0, a1, q1
        for b in np.nonzero(keep)[0]:
            k = bins[b]
            n[k] += 1
            acc[0, k] = acc[0, k] + v0[b]
            acc[1, k] = acc[1, k] + v0[b] * v0[b]
            if v1 is not None:
                acc[2, k] = acc[2, k] + v1[b]
                acc[3, k] = acc[3, k] + v1[b] * v1[b]
        hit = n > 0
        state[0, hit] = decay * state[0, hit] + n[hit].astype(F)
        for row in range(1, 5 if v1 is not None else 3):
            state[row, hit] = decay * state[row, hit] + acc[row - 1, hit]
    assert state.dtype == F
    return state


def table(state, warm, floor):
    """-> (p [64], c [65], w [64], ready) in fp32, formed in bin order as the kernel does."""
    state = np.asarray(state, dtype=F).reshape(5, BINS)
    W, S2 = state[0], state[2]
    warm, floor = F(warm), F(floor)
    p = np.full(BINS, INV, dtype=F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ready = bool((W >= warm).all())
        if ready:
            r = np.sqrt(S2 / W)
            R = F(0)
            for k in range(BINS):
                R = R + r[k]
            if np.isfinite(R) and R > 0:
                p = (r / R) * (F(1) - floor) + floor / F(64)
        c = np.zeros(BINS + 1, dtype=F)
        for k in range(BINS):
            c[k + 1] = c[k] + p[k]
        w = c[BINS] / (F(64) * p)
    assert p.dtype == c.dtype == w.dtype == F
    return p, c, w, ready


def u_importance(state, u0, warm, floor):
    """-> (u [B], w [B], p [64], w_table [64]) in fp32: t = fmul(u0, C), k = the largest index with c_k <= t, f = min(fdiv(fsub(t, c_k), p_k),
    1 - 2^-24), u = min(fmul(fadd(k, f), 2^-6), nextafter((k + 1) 2^-6, 0)), w = w_k.  (fmin: a NaN quotient yields the bound, as fminf does.)"""
    p, c, w, _ = table(state, warm, floor)
    u0 = np.asarray(u0, dtype=F).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = u0 * c[BINS]
        k = np.clip(np.searchsorted(c[:BINS], t, side="right") - 1, 0, BINS - 1)
        f = np.fmin((t - c[k]) / p[k], ONE_BELOW)
        below = np.nextafter(((k + 1).astype(F) * INV).astype(F), F(0))
        u = np.fmin((k.astype(F) + f) * INV, below)
    assert t.dtype == f.dtype == below.dtype == u.dtype == F
    return u, w[k], p, w


def inverse_cdf64(p, c, u0):
    """The float64 inverse CDF of the SAME fp32 table: t = u0 C, k with c_k <= t < c_{k+1}, u = (k + (t - c_k) / p_k) / 64, all in float64."""
    p, c, u0 = np.asarray(p, dtype=np.float64), np.asarray(c, dtype=np.float64), np.asarray(u0, dtype=np.float64)
    t = u0 * c[BINS]
    k = np.clip(np.searchsorted(c[:BINS], t, side="right") - 1, 0, BINS - 1)
    return (k + (t - c[k]) / p[k]) / 64.0, k


def steep_state(rate, count=8.0):
    """A ready state whose r_k = sqrt(S2 / W) = exp(rate (k / 63 - 1/2)): rate 14 spans e^-7 ... e^7 (across e^14), rate 28 e^-14 ... e^14;
    a negative rate falls."""
    k = np.arange(BINS, dtype=np.float64)
    r = np.exp(rate * (k / (BINS - 1) - 0.5))
    state = np.zeros((5, BINS), dtype=F)
    state[0] = F(count)
    state[1] = (count * r).astype(F)
    state[2] = (count * r * r).astype(F)
    state[3] = F(count)
    state[4] = F(count)
    return state


def stratified(u0, B):
    """gmk_u_stratified's rule (tests/loss_weight_ref.u_stratified), restated here so this file stands alone."""
    u0 = F(u0)
    s = np.arange(B, dtype=F) / F(B)
    cc = F(1.0) - s
    return np.where(u0 >= cc, u0 - cc, np.minimum(u0 + s, ONE_BELOW))
