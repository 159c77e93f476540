"""NumPy restatement of the pitch-range arithmetic (csrc/pitch_auto.hip; include/alive_vc.h "Pitch range"): the CPU yardstick of
alive_pitch_stats2_groups, alive_pitch_range_groups, alive_pitch_follow2_rows and alive_pitch_transform_rows_centred.

Unlike tools/pitch_ref.py, whose sums run in NumPy's order, this file reproduces the kernels' summation order -- thread tid of a row takes
frames tid, tid + 256, ..., then the 256-wide tree (strides 128, 64, ..., 1), then the rows of a group in index order -- and every fp64
operation of the kernels is one of + - * / sqrt, rounded on its own.  So sums, states and outputs agree with the device bit for bit;
the one libm call left is log2 in float64 rounded to float32 (pitch_ref.pitch), where NumPy's and the device's last float64 bit almost
never reaches the float32 result.  exp2 in the transform is NumPy's 2^x: compare transformed f0 to a couple of float32 ulps, or bit for
bit where both round alike.
"""
import numpy as np

from pitch_ref import pitch, voiced  # noqa: F401  (re-exported: the same "pitch" and "voiced")

F32 = np.float32


def row_sums(f0_row, scale=None):
    """(sum p, count, sum p^2) of one row's voiced pitch in the kernels' order: float64, int, float64.  scale: f0 * float32(scale)
    first (what mode 1 forms before the shift)"""
    f = np.asarray(f0_row, dtype=F32).reshape(-1)
    if scale is not None:
        f = f * F32(scale)
    p = pitch(f)
    v = voiced(p)
    pd = np.where(v, p, F32(0.0)).astype(np.float64)            # (an unvoiced frame adds nothing: x + 0.0 is x)
    k = -(-f.shape[0] // 256)
    lanes = np.zeros((k, 256), dtype=np.float64)
    lanes.reshape(-1)[:f.shape[0]] = pd
    s, q = np.zeros(256), np.zeros(256)
    for j in range(k):                                          # thread tid: frames tid, tid + 256, ... one after the other
        s = s + lanes[j]
        q = q + lanes[j] * lanes[j]
    o = 128
    while o > 0:                                                # the tree
        s[:o] = s[:o] + s[o:2 * o]
        q[:o] = q[:o] + q[o:2 * o]
        o >>= 1
    return float(s[0]), int(v.sum()), float(q[0])


def stats2_groups(f0, first, t_lo=0, t_hi=None):
    """f0 [N, T], first [G + 1] -> float64 [G, 3]: (sum, count, sum of squares) over frames [t_lo, t_hi) of rows first[g] ..
    first[g + 1] - 1, bitwise alive_pitch_stats2_groups; empty and all-unvoiced groups give zeros"""
    f0 = np.asarray(f0, dtype=F32)
    f0 = f0.reshape(f0.shape[0], -1)
    t_hi = f0.shape[1] if t_hi is None else t_hi
    out = np.zeros((len(first) - 1, 3), dtype=np.float64)
    for g in range(len(first) - 1):
        s = c = q = 0.0
        for r in range(max(first[g], 0), min(first[g + 1], f0.shape[0])):
            rs, rc, rq = row_sums(f0[r, t_lo:t_hi])
            s, c, q = s + rs, c + float(rc), q + rq
        out[g] = (s, c, q)
    return out


def range_factor(v, sd, range_max):
    """clamp(sd / sqrt(v), 1 / range_max, range_max) in float64; 1 when v <= 0, sd <= 0 or either is not finite"""
    v, sd, range_max = np.float64(v), np.float64(sd), np.float64(range_max)
    if not (v > 0.0) or not (sd > 0.0) or np.isinf(v) or np.isinf(sd):
        return np.float64(1.0)
    r = sd / np.sqrt(v)
    lo = np.float64(1.0) / range_max
    r = lo if r < lo else r
    return range_max if r > range_max else r


def mean_var(s, c, q):
    """(m, v) = (s / c, q / c - m * m) in float64, each operation rounded, as the kernels form them"""
    s, c, q = np.float64(s), np.float64(c), np.float64(q)
    m = s / c
    return m, q / c - m * m


def range_groups(stats3, first, inton, range_on, target_sd, range_max=2.0):
    """alive_pitch_range_groups: -> (inton_out float32 [N], centre_out float32 [N], centre_on_out int32 [N]), N = first[-1]"""
    n = int(first[-1])
    i_out, c_out, on_out = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32), np.zeros(n, dtype=np.int32)
    for g, (s, c, q) in enumerate(np.asarray(stats3, dtype=np.float64)):
        i, ce, on = F32(inton[g]), F32(0.0), 0
        if range_on[g] and c > 0:
            m, v = mean_var(s, c, q)
            i = F32(np.float64(i) * range_factor(v, np.float64(target_sd[g]), range_max))
            ce, on = F32(m), 1
        rows = slice(max(first[g], 0), min(first[g + 1], n))
        i_out[rows], c_out[rows], on_out[rows] = i, ce, on
    return i_out, c_out, on_out


def follow2_rows(state3, f0, f0_rate, offset, auto_on, target, inton, range_on, target_sd, emit, decay, prior, range_max=2.0):
    """one streaming update, alive_pitch_follow2_rows: state3 float64 [N, 3] = (S, W, Q), f0 [N, T] ->
    (new state, shift float32 [N], inton_out float32 [N], centre float32 [N], centre_on int32 [N])"""
    f0 = np.asarray(f0, dtype=F32)
    f0 = f0.reshape(f0.shape[0], -1)
    n = f0.shape[0]
    state = np.array(state3, dtype=np.float64)
    offset = np.asarray(offset, dtype=F32)
    decay, prior = np.float64(decay), np.float64(prior)
    shift, i_out = offset.copy(), np.ones(n, dtype=F32)
    c_out, on_out = np.zeros(n, dtype=F32), np.zeros(n, dtype=np.int32)
    for r in range(n):
        i0 = F32(inton[r])
        if not (auto_on[r] or range_on[r] or i0 != F32(1.0)):
            continue
        S, W, Q = state[r]
        if emit[r]:
            rs, rc, rq = row_sums(f0[r], f0_rate[r])
            S = decay * S + rs
            W = decay * W + np.float64(rc)
            Q = decay * Q + rq
            state[r] = (S, W, Q)
        if W != 0:
            a = W / (W + prior)
            m = S / W
            rr = range_factor(Q / W - m * m, np.float64(target_sd[r]), range_max) if range_on[r] else np.float64(1.0)
            ie = np.float64(i0) * rr
            i_out[r] = F32(np.float64(1.0) + a * (ie - np.float64(1.0)))
            c_out[r] = F32(m)
            if auto_on[r]:
                shift[r] = offset[r] + F32(a * (np.float64(F32(target[r])) - m))
        on_out[r] = int(i_out[r] != F32(1.0))
    return state, shift, i_out, c_out, on_out


def transform_rows_centred(f0, mode, f0_rate, shift, inton, centre, centre_on):
    """alive_pitch_transform_rows_centred on f0 [N, T] -> float32 [N, T].  centre_on == 0: alive_pitch_transform_rows' arithmetic
    (mode 0: around the row's own voiced mean; mode 1: p + shift); else p = c + (p - c) * inton + shift in either mode"""
    f0 = np.asarray(f0, dtype=F32)
    f0 = f0.reshape(f0.shape[0], -1)
    out = np.empty_like(f0)
    with np.errstate(all="ignore"):
        for r in range(f0.shape[0]):
            rate, sh, it = F32(f0_rate[r]), F32(shift[r]), F32(inton[r])
            x = f0[r] * rate if mode == 1 else f0[r]
            p = pitch(x)
            if centre_on[r]:
                c = F32(centre[r])
                p = c + (p - c) * it + sh
            elif mode == 0:
                s, cnt, _ = row_sums(f0[r])
                c = F32(np.float64(s) / np.float64(cnt))
                p = c + (p - c) * it + sh
            else:
                p = p + sh
            e = (p + F32(9.0)) / F32(12.0)
            y = F32(440.0) * np.exp2(e.astype(np.float64)).astype(F32)
            y = np.where(np.isfinite(y), y, F32(0.0)).astype(F32)
            out[r] = y * rate if mode == 0 else y
    return out
