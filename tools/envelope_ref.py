"""NumPy restatement of the envelope follow (csrc/envelope.hip; include/alive_vc.h "Envelope follow"): the CPU yardstick of
alive_envelope_waves, as tools/limit_ref.py is the limiter's.

The converted wave y takes on the loudness contour of the source x that lies beside it sample for sample.  Everything is float64 with
every operation rounded on its own (only + - * / and sqrt, so NumPy and the device agree bit for bit), except the last step, which
rounds to float32 once.  Per row, with frames of `hop` samples (even), n samples, F = ceil(n / hop), radius R, amount m, floor e (a mean
square, 10^(floor_db / 10)) and the range [g_lo, g_hi] = 10^(-+range_db / 20):
    Sx[f], Sy[f]  sums of squares over [f hop, min((f + 1) hop, n)) in the order of frame_sums
    Px, Py        sums of Sx[t] / Sy[t] over t = a .. b ascending from 0.0, a = max(f - R, 0), b = min(f + R, F - 1)
    Cn            (double)(min((b + 1) hop, n) - a hop)
    q             (Px / Cn + e) / (Py / Cn + e);   rc = min(max(sqrt(q), g_lo), g_hi) if q is finite, else 1.0
    G[f]          1.0 + (double)m * (rc - 1.0)
    g[i]          G[0] for i < hop / 2; G[F - 1] for i >= hop / 2 + (F - 1) hop; otherwise G[f] + (G[f + 1] - G[f]) * w with
                  f = (i - hop / 2) // hop and w = (double)((i - hop / 2) - f hop) / (double)hop
    out[i]        (float)((double)y[i] * g[i])
A row whose amount is not in (0, 1] or whose n <= 0 is copied bit for bit, and so are the samples at or beyond n.  A NaN in either
signal, or an inf in x, makes q non-finite in the frames within R of it: they stay at G = 1 and no other frame changes.
"""
import numpy as np

TILE, MAX_RADIUS = 16, 4                        # ALIVE_ENVELOPE_TILE, ALIVE_ENVELOPE_MAX_RADIUS (include/alive_vc.h)
HOP, RADIUS, FLOOR_DB, RANGE_DB = 320, 1, -60.0, 12.0


def constants(floor_db=FLOOR_DB, range_db=RANGE_DB):
    """(e, g_lo, g_hi) as the host forms them, in float64"""
    return float(10.0 ** (float(floor_db) / 10.0)), float(10.0 ** (-float(range_db) / 20.0)), float(10.0 ** (float(range_db) / 20.0))


def frame_sums(v, n, hop):
    """v float32 [>= n] -> S float64 [F]: per frame the sum of squares in the kernel's order: 256 accumulators, accumulator a adds
    v[f hop + a + 256 j]^2 for ascending j from 0.0 (a missing sample adds +0.0); s[l] = (acc[4l] + acc[4l + 1]) + (acc[4l + 2] +
    acc[4l + 3]); then s[l] = s[l] + s[l + o] for l < o, o = 32, 16, .., 1"""
    F = -(-n // hop)
    steps = -(-hop // 256)
    sq = np.zeros((F, steps * 256), dtype=np.float64)
    d = np.asarray(v[:n], dtype=np.float32).astype(np.float64)
    flat = np.zeros(F * hop, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        flat[:n] = d * d
    sq[:, :hop] = flat.reshape(F, hop)
    acc = np.zeros((F, 256), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(steps):
            acc = acc + sq[:, 256 * j:256 * (j + 1)]
        a = acc.reshape(F, 64, 4)
        s = (a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])
        o = 32
        while o:
            s = s[:, :o] + s[:, o:2 * o]
            o >>= 1
    return s[:, 0]


def frame_gains(x, y, n, amount, hop=HOP, radius=RADIUS, e=None, g_lo=None, g_hi=None):
    """-> G float64 [F], the frame gains of one row of n > 0 samples"""
    d = constants()
    e, g_lo, g_hi = (d[0] if e is None else e), (d[1] if g_lo is None else g_lo), (d[2] if g_hi is None else g_hi)
    Sx, Sy = frame_sums(x, n, hop), frame_sums(y, n, hop)
    F, R = Sx.shape[0], int(radius)
    G = np.empty(F, dtype=np.float64)
    m = np.float64(np.float32(amount))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for f in range(F):
            a, b = max(f - R, 0), min(f + R, F - 1)
            px = py = np.float64(0.0)
            for t in range(a, b + 1):
                px = px + Sx[t]
                py = py + Sy[t]
            cn = np.float64(min((b + 1) * hop, n) - a * hop)
            q = (px / cn + np.float64(e)) / (py / cn + np.float64(e))
            rc = min(max(np.sqrt(q), np.float64(g_lo)), np.float64(g_hi)) if np.isfinite(q) else np.float64(1.0)
            G[f] = np.float64(1.0) + m * (rc - np.float64(1.0))
    return G


def sample_gains(G, n, hop):
    """G float64 [F] -> g float64 [n]: constant over the first and the last half frame, linear between the frame centres"""
    F, c = G.shape[0], hop // 2
    i = np.arange(n, dtype=np.int64)
    f = np.clip((i - c) // hop, 0, max(F - 2, 0))
    w = ((i - c) - f * hop).astype(np.float64) / np.float64(hop)
    nxt = np.minimum(f + 1, F - 1)
    g = G[f] + (G[nxt] - G[f]) * w
    g = np.where(i < c, G[0], g)
    return np.where(i >= c + (F - 1) * hop, G[F - 1], g)


def follows(amount, n):
    a = np.float32(amount)
    return bool(a > 0 and a <= 1 and n > 0)


def envelope_waves(y, x, lens=None, amount=1.0, hop=HOP, radius=RADIUS, floor_db=FLOOR_DB, range_db=RANGE_DB, e=None, g_lo=None,
                   g_hi=None):
    """alive_envelope_waves: y float32 [N, ld_y], x float32 [N, ld_x], lens int [N] or None (ld_y), amount a float or one per row ->
    (out float32 [N, ld_y], G: per row the float64 frame gains, None for a copied row, minmax float32 [N, 2]).  e / g_lo / g_hi
    override what floor_db / range_db give"""
    y, x = np.asarray(y, dtype=np.float32), np.asarray(x, dtype=np.float32)
    N, ld_y = y.shape
    ld_x = x.shape[1]
    d = constants(floor_db, range_db)
    e, g_lo, g_hi = (d[0] if e is None else e), (d[1] if g_lo is None else g_lo), (d[2] if g_hi is None else g_hi)
    amounts = list(amount) if np.ndim(amount) else [amount] * N
    lens = [ld_y] * N if lens is None else [int(v) for v in lens]
    out = y.copy()
    gains = [None] * N
    minmax = np.ones((N, 2), dtype=np.float32)
    for r in range(N):
        n = min(max(lens[r], 0), ld_y, ld_x)
        if not follows(amounts[r], n):
            continue
        G = frame_gains(x[r], y[r], n, amounts[r], hop, radius, e, g_lo, g_hi)
        with np.errstate(invalid="ignore", over="ignore"):
            out[r, :n] = (y[r, :n].astype(np.float64) * sample_gains(G, n, hop)).astype(np.float32)
        gains[r] = G
        minmax[r] = np.float32(G.min()), np.float32(G.max())
    return out, gains, minmax


def follow(y, x, amount=1.0, **kw):
    """one row: y, x float32 [n] -> out float32 [n]"""
    return envelope_waves(np.asarray(y, np.float32)[None], np.asarray(x, np.float32)[None], None, amount, **kw)[0][0]


def gain_db(minmax):
    """20 log10 of the smallest and the largest frame gain per row: (0.0, 0.0) for a row that does not follow"""
    return [(float(20.0 * np.log10(np.float64(lo))), float(20.0 * np.log10(np.float64(hi)))) for lo, hi in np.asarray(minmax)]
