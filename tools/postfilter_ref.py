"""NumPy restatement of the adaptive formant post filter (csrc/postfilter.hip; include/alive_vc.h "Post filter"): the CPU yardstick of
alive_postfilter_waves, as tools/envelope_ref.py is the envelope follow's.  It also holds the host builders of the two tables the call
takes (window_table, lag_table): module/multistream.py repeats them and a host test pins the two equal.

Per row of n samples, frames of `hop` samples, F = ceil(n / hop), a = (double)alpha[row], b = a * ratio.  Per frame f:
    q[i]      the int16 grid: clamp(rintf(32768 y[i]), +-32767) in float32, NaN -> 0, 0 outside [0, n)
    s[i]      q[f hop - (window - hop) / 2 + i] * win[i], i < window            (integers)
    R[k]      sum_i s[i] s[i + k], k = 0 .. order                                (exact integers: below 2^53)
    r[k]      (double)R[k] * lag[k];  r[0] = r[0] * 1.0001
    Levinson-Durbin, m = 1 .. order:  acc = r[m], then acc = acc + A[j] * r[m - j] for j = 1 .. m - 1 ascending;  k = -acc / err
    (err starts at r[0]);  A'[j] = A[j] + k * A[m - j] (j < m), A'[m] = k;  err = err * (1 - k * k)
    den[j]    A[j] * a^j, num[j] = A[j] * b^j (A[0] = 1; the powers by repeated multiplication: p = p * a)
    h0[k]     (num[k] if k <= order else 0) - acc, acc = 0.0 then acc = acc + den[j] * h0[k - j] for j = 1 .. min(k, order), k < TAPS
    t         tilt * (c1 / c0), c0 = sum_k h0[k]^2, c1 = sum_k h0[k] h0[k + 1], both ascending from 0.0
    h[k]      h0[k] - t * h0[k - 1] (h[0] = h0[0])
    U(f, i)   sum_k h[k] * (double)y[i - k], k ascending from 0.0, y = 0 before the row's start
    g[f]      clamp(sqrt((Ein + e) / (Eout + e)), g_lo, g_hi) if the quotient and its denominator are finite, else 1: Ein = sum y^2 and Eout = sum U(f, .)^2 over
              the frame's own samples in the order of ordered_sums (envelope.hip's frame_sum), e = floor_ms * count
A frame is the identity (h = delta, so g = 1) when R[0] <= 0, a k is non-finite or |k| >= 1, or err stops being > 0.
    out[i]    (float)(g[0] U(0, i)) for i < hop / 2; (float)(g[F-1] U(F-1, i)) for i >= hop / 2 + (F - 1) hop; otherwise
              (float)(Z0 + (Z1 - Z0) * w), Z0 = g[f] U(f, i), Z1 = g[f+1] U(f+1, i), f = (i - hop / 2) // hop,
              w = (double)((i - hop / 2) - f hop) / (double)hop
Everything is float64 with every operation rounded on its own (only + - * / and sqrt), so NumPy and the device agree bit for bit.
A row whose alpha (as a float32) is not in (0, 0.85], or whose n <= 0, is copied bit for bit, and so are the samples at or beyond n.
"""
import numpy as np

TAPS, MAX_ORDER, TILE = 128, 32, 16             # ALIVE_POSTFILTER_TAPS / _MAX_ORDER / _TILE (include/alive_vc.h)
MAX_ALPHA = 0.85
HOP, WINDOW, ORDER, RATIO, TILT, FLOOR_DB, RANGE_DB = 320, 640, 16, 0.625, 0.5, -100.0, 12.0


def window_table(window=WINDOW):
    """int16 [window]: a Hamming window on the half-sample grid in units of 1/64: rint(64 (0.54 - 0.46 cos(2 pi (i + 0.5) / window)))"""
    i = np.arange(int(window), dtype=np.float64)
    return np.rint(64.0 * (0.54 - 0.46 * np.cos(2.0 * np.pi * (i + 0.5) / float(window)))).astype(np.int16)


def lag_table(order=ORDER):
    """float64 [order + 1]: the 60 Hz Gaussian lag window at 16 kHz: exp(-0.5 (2 pi 60 k / 16000)^2)"""
    k = np.arange(int(order) + 1, dtype=np.float64)
    return np.exp(-0.5 * (2.0 * np.pi * 60.0 * k / 16000.0) ** 2)


def constants(floor_db=FLOOR_DB, range_db=RANGE_DB):
    """(e, g_lo, g_hi) as the host forms them, in float64"""
    return float(10.0 ** (float(floor_db) / 10.0)), float(10.0 ** (-float(range_db) / 20.0)), float(10.0 ** (float(range_db) / 20.0))


def filters(alpha, n):
    a = np.float32(alpha)
    return bool(a > 0 and a <= np.float32(MAX_ALPHA) and n > 0)


def quantise(y, n):
    """float32 [>= n] -> int64 [n] on the int16 grid"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(y[:n], dtype=np.float32) * np.float32(32768.0)
        q = np.minimum(np.maximum(np.rint(v), np.float32(-32767.0)), np.float32(32767.0))
    return np.where(np.isnan(v), np.float32(0.0), q).astype(np.int64)


def autocorrelation(y, n, hop=HOP, window=WINDOW, order=ORDER, win=None):
    """-> R int64 [F, order + 1], exact"""
    win = (window_table(window) if win is None else np.asarray(win)).astype(np.int64)
    F = -(-n // hop)
    half = (window - hop) // 2
    q = np.zeros(half + F * hop + window, dtype=np.int64)
    q[half:half + n] = quantise(y, n)
    s = q[np.arange(F)[:, None] * hop + np.arange(window)[None, :]] * win[None, :]
    R = np.empty((F, order + 1), dtype=np.int64)
    for k in range(order + 1):
        R[:, k] = np.sum(s[:, :window - k] * s[:, k:], axis=1)
    return R


def levinson(R, lag, order):
    """R int64 [F, order + 1] -> (A float64 [F, order + 1] with A[:, 0] = 1, identity bool [F])"""
    F = R.shape[0]
    r = R.astype(np.float64) * np.asarray(lag, dtype=np.float64)[None, :]
    r[:, 0] = r[:, 0] * np.float64(1.0001)
    A = np.zeros((F, order + 1), dtype=np.float64)
    A[:, 0] = 1.0
    ident = ~(r[:, 0] > 0.0)
    err = np.where(ident, 1.0, r[:, 0])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for m in range(1, order + 1):
            acc = r[:, m].copy()
            for j in range(1, m):
                acc = acc + A[:, j] * r[:, m - j]
            k = -acc / err
            ident = ident | ~np.isfinite(k) | ~(np.abs(k) < 1.0)
            k = np.where(ident, 0.0, k)
            new = A.copy()
            for j in range(1, m):
                new[:, j] = A[:, j] + k * A[:, m - j]
            new[:, m] = k
            A = new
            err = err * (1.0 - k * k)
            ident = ident | ~(err > 0.0)
            err = np.where(ident, 1.0, err)
    return A, ident


def impulse_responses(A, ident, alpha, ratio=RATIO, tilt=TILT, taps=TAPS):
    """A [F, order + 1] -> h float64 [F, taps]: num / den with the tilt compensation; delta for an identity frame"""
    F, order = A.shape[0], A.shape[1] - 1
    a = np.float64(np.float32(alpha))
    b = a * np.float64(ratio)
    den, num = A.copy(), A.copy()
    pa = pb = np.float64(1.0)
    for j in range(1, order + 1):
        pa, pb = pa * a, pb * b
        den[:, j] = A[:, j] * pa
        num[:, j] = A[:, j] * pb
    h0 = np.zeros((F, taps), dtype=np.float64)
    for k in range(taps):
        acc = np.zeros(F, dtype=np.float64)
        for j in range(1, min(k, order) + 1):
            acc = acc + den[:, j] * h0[:, k - j]
        h0[:, k] = (num[:, k] if k <= order else 0.0) - acc
    c0, c1 = np.zeros(F, dtype=np.float64), np.zeros(F, dtype=np.float64)
    for k in range(taps):
        c0 = c0 + h0[:, k] * h0[:, k]
    for k in range(taps - 1):
        c1 = c1 + h0[:, k] * h0[:, k + 1]
    t = np.float64(tilt) * (c1 / c0)
    h = h0.copy()
    h[:, 1:] = h0[:, 1:] - t[:, None] * h0[:, :-1]
    h[ident] = 0.0
    h[ident, 0] = 1.0
    return h


def ordered_sums(sq):
    """sq float64 [F, hop] (0.0 where a frame has no sample) -> float64 [F]: envelope.hip's frame_sum order: 256 accumulators,
    accumulator a adds sq[a + 256 j] for ascending j from 0.0; s[l] = (acc[4l] + acc[4l + 1]) + (acc[4l + 2] + acc[4l + 3]); then
    s[l] = s[l] + s[l + o] for l < o, o = 32, 16, .., 1"""
    F, hop = sq.shape
    steps = -(-hop // 256)
    pad = np.zeros((F, steps * 256), dtype=np.float64)
    pad[:, :hop] = sq
    acc = np.zeros((F, 256), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(steps):
            acc = acc + pad[:, 256 * j:256 * (j + 1)]
        a = acc.reshape(F, 64, 4)
        s = (a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])
        o = 32
        while o:
            s = s[:, :o] + s[:, o:2 * o]
            o >>= 1
    return s[:, 0]


def filter_row(y, n, alpha, hop=HOP, window=WINDOW, order=ORDER, ratio=RATIO, tilt=TILT, e=None, g_lo=None, g_hi=None, win=None,
               lag=None, taps=TAPS, dtype=np.float32):
    """one row of n > 0 samples at a filtering alpha -> (out float32 [n], g float64 [F], identity bool [F], h float64 [F, taps]).
    dtype=np.float64 leaves out the last rounding (for measurements)"""
    d = constants()
    e, g_lo, g_hi = (d[0] if e is None else e), (d[1] if g_lo is None else g_lo), (d[2] if g_hi is None else g_hi)
    lag = lag_table(order) if lag is None else lag
    y = np.asarray(y[:n], dtype=np.float32)
    F, c = -(-n // hop), hop // 2
    A, ident = levinson(autocorrelation(y, n, hop, window, order, win), lag, order)
    h = impulse_responses(A, ident, alpha, ratio, tilt, taps)
    # U[f, j]: sample i = f hop - c + j, j < 2 hop (the frame's own samples and half a frame on each side)
    yd = np.zeros(taps + c + F * hop + c, dtype=np.float64)
    yd[taps + c:taps + c + n] = y.astype(np.float64)
    base = taps + np.arange(F)[:, None] * hop + np.arange(2 * hop)[None, :]             # (index of sample i in yd)
    U = np.zeros((F, 2 * hop), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(taps):
            U = U + h[:, k:k + 1] * yd[base - k]
        own = np.arange(F)[:, None] * hop + np.arange(hop)[None, :]
        live = own < n
        yo = yd[taps + c + np.minimum(own, n - 1)]
        Ein = ordered_sums(np.where(live, yo * yo, 0.0))
        Uo = U[:, c:c + hop]
        Eout = ordered_sums(np.where(live, Uo * Uo, 0.0))
        ee = np.float64(e) * live.sum(axis=1).astype(np.float64)
        q = (Ein + ee) / (Eout + ee)
        g = np.where(np.isfinite(q) & np.isfinite(Eout + ee), np.minimum(np.maximum(np.sqrt(q), np.float64(g_lo)), np.float64(g_hi)), np.float64(1.0))
        i = np.arange(n, dtype=np.int64)
        f = np.clip((i - c) // hop, 0, max(F - 2, 0))
        nxt = np.minimum(f + 1, F - 1)
        w = ((i - c) - f * hop).astype(np.float64) / np.float64(hop)
        Z0 = g[f] * U[f, np.clip(i - (f * hop - c), 0, 2 * hop - 1)]
        Z1 = g[nxt] * U[nxt, np.clip(i - (nxt * hop - c), 0, 2 * hop - 1)]
        z = Z0 + (Z1 - Z0) * w
        z = np.where(i < c, g[0] * U[0, np.minimum(i + c, 2 * hop - 1)], z)
        last = c + (F - 1) * hop
        z = np.where(i >= last, g[F - 1] * U[F - 1, np.clip(i - ((F - 1) * hop - c), 0, 2 * hop - 1)], z)
        out = z.astype(dtype)
    return out, g, ident, h


def postfilter_waves(y, lens=None, alpha=0.8, hop=HOP, window=WINDOW, order=ORDER, ratio=RATIO, tilt=TILT, floor_db=FLOOR_DB,
                     range_db=RANGE_DB, e=None, g_lo=None, g_hi=None, taps=TAPS):
    """alive_postfilter_waves: y float32 [N, ld], lens int [N] or None (ld), alpha a float or one per row -> (out float32 [N, ld],
    g: per row the float64 frame gains, None for a copied row, minmax float32 [N, 2]).  e / g_lo / g_hi override floor_db / range_db"""
    y = np.asarray(y, dtype=np.float32)
    N, ld = y.shape
    d = constants(floor_db, range_db)
    e, g_lo, g_hi = (d[0] if e is None else e), (d[1] if g_lo is None else g_lo), (d[2] if g_hi is None else g_hi)
    alphas = list(alpha) if np.ndim(alpha) else [alpha] * N
    lens = [ld] * N if lens is None else [int(v) for v in lens]
    win, lag = window_table(window), lag_table(order)
    out = y.copy()
    gains = [None] * N
    minmax = np.ones((N, 2), dtype=np.float32)
    for r in range(N):
        n = min(max(lens[r], 0), ld)
        if not filters(alphas[r], n):
            continue
        out[r, :n], g, _, _ = filter_row(y[r], n, alphas[r], hop, window, order, ratio, tilt, e, g_lo, g_hi, win, lag, taps)
        gains[r] = g
        minmax[r] = np.float32(g.min()), np.float32(g.max())
    return out, gains, minmax


def post_filter(y, alpha=0.8, **kw):
    """one row: y float32 [n] -> out float32 [n]"""
    return postfilter_waves(np.asarray(y, np.float32)[None], None, alpha, **kw)[0][0]


def gain_db(minmax):
    """20 log10 of the smallest and the largest frame gain per row: (0.0, 0.0) for a copied row"""
    return [(float(20.0 * np.log10(np.float64(lo))), float(20.0 * np.log10(np.float64(hi)))) for lo, hi in np.asarray(minmax)]
