"""NumPy restatement of the loudness kernels (csrc/loudness.hip; include/alive_vc.h "Loudness"): the CPU yardstick of
alive_loudness_measure_waves, alive_loudness_apply_waves and alive_loudness_rows, as tools/limit_ref.py is the limiter's.

Programme loudness after ITU-R BS.1770-4 / EBU R 128 for one channel.  Everything is float64 with every operation rounded on its own, in
the kernels' order; only + - * / sqrt and compares touch the signal, and every 10^x, 2^x and tan is formed here in Python floats, as the
product's host code forms them (module/multistream.py).

K-weighting at rate fs: two biquads in transposed direct form II, the second fed the first's output (coefficients(fs)); a non-finite
sample counts as 0.0.  H = hop(fs) = (fs + 5) // 10 samples per 100-ms sub-block; q[j] the sum of the squared filter output over
sub-block j, in sample order from 0.0; block b is z[b] = (((q[b] + q[b+1]) + q[b+2]) + q[b+3]) / (4 H).

THE FILTER IN TILES (tile_q): a tile is a sub-block, H samples.  e[j] is the 4-state left by the recurrence over tile j from zero state,
AP (carry_matrix) the 4x4 matrix whose column k is the state left after H zero samples from unit state k, s[0] = 0 and
    s[j+1] = (((AP[:,0] s[j][0] + AP[:,1] s[j][1]) + AP[:,2] s[j][2]) + AP[:,3] s[j][3]) + e[j];
q[j] comes from the recurrence over tile j started from s[j].  plain_q is the end-to-end recurrence, for cross-checks: the two differ
by rounding alone.
"""
import math

import numpy as np

STATE, PARAMS = 16, 6                  # ALIVE_LOUDNESS_STATE, ALIVE_LOUDNESS_PARAMS
G_SLOT = 12                            # where the state keeps the current gain


# ------------------------------------------------------------------------------------------------ the host's numbers
def hop(fs):
    return (int(fs) + 5) // 10


def _biquad(f0, Q, fs, Vh=None):
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    a1, a2 = 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0
    if Vh is None:
        return 1.0, -2.0, 1.0, a1, a2
    Vb = Vh ** 0.4996667741545416
    return (Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, a1, a2


def coefficients(fs):
    """(b0, b1, b2, a1, a2) of the shelf, then of the high-pass: float64 [10]"""
    fs = float(fs)
    shelf = _biquad(1681.974450955533, 0.7071752369554196, fs, 10.0 ** (3.999843853973347 / 20.0))
    return np.array(shelf + _biquad(38.13547087602444, 0.5003270373238773, fs), dtype=np.float64)


def z_of(level):
    """the mean square of a loudness in LUFS: 10^((L + 0.691) / 10)"""
    return 10.0 ** ((float(level) + 0.691) / 10.0)


def lufs(z):
    """-0.691 + 10 log10(z); -inf for 0"""
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(np.asarray(z, dtype=np.float64))


def params(fs, n, target, gate=-70.0, half_life=3.0, prior=1.0, max_db=12.0, slew=6.0):
    """a session's row of alive_loudness_rows' par: (z_abs, z_t, d, P, gmax, qs) for spans of n samples at fs"""
    return np.array([z_of(gate), z_of(target), 2.0 ** (-0.1 / float(half_life)), 10.0 * float(prior), 10.0 ** (float(max_db) / 20.0),
                     10.0 ** (float(slew) * (int(n) / float(fs)) / 20.0)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the filter
def clean(y):
    y = np.asarray(y, dtype=np.float32)
    return np.where(np.isfinite(y), y.astype(np.float64), 0.0)


def run(v, c, z):
    """the recurrence over the columns of v float64 [T, n], one lane per row, from the states z float64 [T, 4] ->
    (the states after, the sums of squares of the output in column order from 0.0)"""
    z = np.array(z, dtype=np.float64)
    z1a, z2a, z1b, z2b = (z[:, i].copy() for i in range(4))
    acc = np.zeros(v.shape[0], dtype=np.float64)
    c = [np.float64(x) for x in c]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i in range(v.shape[1]):
            x = v[:, i]
            o1 = c[0] * x + z1a
            z1a = (c[1] * x - c[3] * o1) + z2a
            z2a = c[2] * x - c[4] * o1
            o2 = c[5] * o1 + z1b
            z1b = (c[6] * o1 - c[8] * o2) + z2b
            z2b = c[7] * o1 - c[9] * o2
            acc = acc + o2 * o2
    return np.stack([z1a, z2a, z1b, z2b], axis=1), acc


def carry_matrix(c, H):
    """AP float64 [4, 4]: column k is the state left after H zero samples from unit state k"""
    return run(np.zeros((4, int(H))), c, np.eye(4))[0].T.copy()


def tile_q(y, H, c, AP=None):
    """q float64 [len(y) // H] by the tiled scheme"""
    H = int(H)
    nb = len(y) // H
    if nb == 0:
        return np.zeros(0, dtype=np.float64)
    AP = carry_matrix(c, H) if AP is None else np.asarray(AP, dtype=np.float64)
    v = clean(y[:nb * H]).reshape(nb, H)
    e = run(v, c, np.zeros((nb, 4)))[0]
    s = np.zeros((nb, 4), dtype=np.float64)
    for j in range(nb - 1):
        s[j + 1] = (((AP[:, 0] * s[j, 0] + AP[:, 1] * s[j, 1]) + AP[:, 2] * s[j, 2]) + AP[:, 3] * s[j, 3]) + e[j]
    return run(v, c, s)[1]


def plain_q(y, H, c):
    """q float64 [len(y) // H] by one end-to-end recurrence in Python floats"""
    H = int(H)
    nb = len(y) // H
    v = clean(y[:nb * H]).tolist()
    b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = (float(x) for x in c)
    z1a = z2a = z1b = z2b = 0.0
    q = np.zeros(nb, dtype=np.float64)
    for j in range(nb):
        acc = 0.0
        for x in v[j * H:(j + 1) * H]:
            o1 = b0 * x + z1a
            z1a = (b1 * x - a1 * o1) + z2a
            z2a = b2 * x - a2 * o1
            o2 = d0 * o1 + z1b
            z1b = (d1 * o1 - e1 * o2) + z2b
            z2b = d2 * o1 - e2 * o2
            acc = acc + o2 * o2
        q[j] = acc
    return q


# ------------------------------------------------------------------------------------------------ offline
def blocks(q, H):
    """z float64 [max(len(q) - 3, 0)]"""
    q = np.asarray(q, dtype=np.float64)
    if len(q) < 4:
        return np.zeros(0, dtype=np.float64)
    return (((q[:-3] + q[1:-2]) + q[2:-1]) + q[3:]) / np.float64(4 * int(H))


def gate(z, z_abs):
    """the two gating passes over the blocks z -> (zI, c1, c2); zI = 0.0 where c2 == 0"""
    z_abs = float(z_abs)
    sum1, c1 = 0.0, 0
    for v in z.tolist():
        if v > z_abs:
            sum1, c1 = sum1 + v, c1 + 1
    sum2, c2 = 0.0, 0
    if c1:
        rel = 0.1 * (sum1 / float(c1))
        for v in z.tolist():
            if v > z_abs and v > rel:
                sum2, c2 = sum2 + v, c2 + 1
    return (sum2 / float(c2) if c2 else 0.0), c1, c2


def ungated(z):
    """the plain mean of the blocks (no gate), for comparisons"""
    return float(np.mean(z)) if len(z) else 0.0


def measure_waves(y, lens, hops, coefs, aps=None, z_abs=None, max_tiles=None):
    """alive_loudness_measure_waves: y float32 [N, ld], per row lens, hops, coefs [N, 10], aps [N, 4, 4] (None: formed here) ->
    (zI float64 [N], c1 int32 [N], c2 int32 [N]).  A row with hop < 1 or more than max_tiles sub-blocks is not measured"""
    y = np.asarray(y, dtype=np.float32)
    n, ld = y.shape
    z_abs = z_of(-70.0) if z_abs is None else z_abs
    zI, c1, c2 = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for r in range(n):
        ln, H = min(max(int(lens[r]), 0), ld), int(hops[r])
        if H < 1 or (max_tiles is not None and ln // H > int(max_tiles)):
            continue
        q = tile_q(y[r, :ln], H, coefs[r], None if aps is None else np.asarray(aps[r]).reshape(4, 4))
        zI[r], c1[r], c2[r] = gate(blocks(q, H), z_abs)
    return zI, c1, c2


def clamp_gain(r, gmax):
    lo = 1.0 / gmax
    r = r if r > lo else lo
    return r if r < gmax else gmax


def gain(zI, c2, z_t, gmax):
    """g = min(max(sqrt(z_t / zI), 1 / gmax), gmax); 1 where c2 == 0 or the target is a NaN"""
    if z_t != z_t or c2 <= 0:
        return 1.0
    return clamp_gain(math.sqrt(float(z_t) / float(zI)), float(gmax))


def apply_waves(y, lens, zI, c2, z_t, gmax):
    """alive_loudness_apply_waves: -> (out float32 [N, ld], gain float64 [N]); a row whose target is a NaN is copied bit for bit"""
    y = np.asarray(y, dtype=np.float32)
    out = y.copy()
    n, ld = y.shape
    g = np.ones(n, dtype=np.float64)
    for r in range(n):
        if z_t[r] != z_t[r]:
            continue
        ln = min(max(int(lens[r]), 0), ld)
        g[r] = gain(zI[r], c2[r], z_t[r], gmax)
        with np.errstate(over="ignore", invalid="ignore"):
            out[r, :ln] = (y[r, :ln].astype(np.float64) * g[r]).astype(np.float32)
    return out, g


# ------------------------------------------------------------------------------------------------ streaming
def state0(n=1):
    """the state of n new streams: zeros, the gain 1"""
    st = np.zeros((n, STATE), dtype=np.float64)
    st[:, G_SLOT] = 1.0
    return st


def target_gain(st, par):
    """step 3: where the state's running loudness wants the gain to be, before the slew"""
    z_abs, z_t, d, P, gmax, qs = (float(x) for x in par)
    Sm, W = float(st[10]), float(st[11])
    if W == 0.0:
        return 1.0
    with np.errstate(divide="ignore"):
        r = clamp_gain(math.sqrt(float(np.float64(z_t) / (np.float64(Sm) / np.float64(W)))), gmax)
        a = float(np.float64(W) / np.float64(P))
    a = a if a < 1.0 else 1.0
    return 1.0 + a * (r - 1.0)


def running_lufs(st):
    """the running loudness S / W of a state in LUFS; -inf before any block counted"""
    return float(lufs(st[10] / st[11])) if st[11] != 0.0 else -math.inf


def loudness_rows(y, span_lo, span_len, emit, on, hops, coefs, par, state):
    """alive_loudness_rows on copies: y float32 [N, ld], par float64 [N, 6], state float64 [N, 16] -> (y, state)"""
    y = np.array(y, dtype=np.float32)
    state = np.array(state, dtype=np.float64)
    n, ld = y.shape
    for r in range(n):
        if not emit[r]:
            continue
        lo, S, H = int(span_lo[r]), int(span_len[r]), int(hops[r])
        if not on[r] or H < 1 or lo < 0 or S < 1 or lo + S > ld:
            state[r] = state0()[0]
            continue
        b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = (float(x) for x in coefs[r])
        z_abs, z_t, d, P, gmax, qs = (float(x) for x in par[r])
        z1a, z2a, z1b, z2b, acc, cnt, q0, q1, q2, nsub, Sm, W, g = (float(x) for x in state[r, :13])
        Hd, H4 = float(H), float(4 * H)
        for x in clean(y[r, lo:lo + S]).tolist():
            o1 = b0 * x + z1a
            z1a = (b1 * x - a1 * o1) + z2a
            z2a = b2 * x - a2 * o1
            o2 = d0 * o1 + z1b
            z1b = (d1 * o1 - e1 * o2) + z2b
            z2b = d2 * o1 - e2 * o2
            acc = acc + o2 * o2
            cnt = cnt + 1.0
            if cnt >= Hd:
                nsub = nsub + 1.0 if nsub < 3.0 else 4.0
                zb = (((q0 + q1) + q2) + acc) / H4
                Sm, W = Sm * d, W * d
                if nsub == 4.0 and zb > z_abs and (W < P or zb * W > 0.1 * Sm):
                    Sm, W = Sm + zb, W + 1.0
                q0, q1, q2 = q1, q2, acc
                acc, cnt = 0.0, 0.0
        state[r, :12] = (z1a, z2a, z1b, z2b, acc, cnt, q0, q1, q2, nsub, Sm, W)
        G = target_gain(state[r], par[r])
        lo_g, hi_g = g / qs, g * qs
        G = G if G > lo_g else lo_g
        G = G if G < hi_g else hi_g
        state[r, G_SLOT] = G
        ramp = np.float64(g) + np.float64(G - g) * (np.arange(1, S + 1, dtype=np.float64) / np.float64(S))
        with np.errstate(over="ignore", invalid="ignore"):
            y[r, lo:lo + S] = (y[r, lo:lo + S].astype(np.float64) * ramp).astype(np.float32)
    return y, state


def stream(waves, span_lo, span_len, on, hops, coefs, par, emit=None, state=None):
    """a sequence of ticks through loudness_rows.  waves: T arrays float32 [N, ld], the full per-tick waves of a converter without
    loudness; on / par: arrays, or lists of T such (a session may retune between ticks); emit bool [N] per tick (default: all).
    Returns (the T waves, per tick the list of N emitted spans -- None for a row that does not emit --, the final state)"""
    waves = [np.asarray(w, dtype=np.float32) for w in waves]
    n = waves[0].shape[0]
    per_tick = np.ndim(on[0]) > 0
    state = state0(n) if state is None else state
    outs, spans = [], []
    for t, w in enumerate(waves):
        e = [True] * n if emit is None else emit[t]
        o, p = (on[t], par[t]) if per_tick else (on, par)
        y, state = loudness_rows(w, span_lo, span_len, e, o, hops, coefs, p, state)
        outs.append(y)
        spans.append([y[r, int(span_lo[r]):int(span_lo[r]) + int(span_len[r])].copy() if e[r] else None for r in range(n)])
    return outs, spans, state
