"""NumPy restatement of the voicing decision (csrc/voicing.hip; include/alive_vc.h "Voicing"): the CPU yardstick of
alive_voicing_rows, as tools/gate_ref.py is the gate's.

The samples are quantised to the int16 grid first, so Sxy, Sxx, Syy and the frame energy are exact int64 sums: the kernel's partition
of them (prefix sums, lanes over lags, a wave per frame) cannot show, and plain NumPy sums serve.  rho is three float64 operations,
each rounded on its own (int64 -> float64 is exact below 2^53; sqrt and the division are correctly rounded on both sides).  The
decision of a row is integer work over its frames.
"""
import numpy as np

SAMPLE_RATE = 16000
HOP = 320
DEFAULTS = dict(on=0.6, off=0.45, floor_db=-60.0, lo=50, hi=500, window_ms=40, bridge=1, min_run=2)
MAX_WINDOW, MAX_LAG = 4096, 1600                # ALIVE_VOICING_MAX_WINDOW, ALIVE_VOICING_MAX_LAG


def lags(lo=DEFAULTS["lo"], hi=DEFAULTS["hi"], sample_rate=SAMPLE_RATE):
    """the lag range [ceil(rate / hi), floor(rate / lo)] of the pitch range lo .. hi Hz (integers or floats)"""
    return int(np.ceil(sample_rate / float(hi))), int(np.floor(sample_rate / float(lo)))


def window(window_ms=DEFAULTS["window_ms"], sample_rate=SAMPLE_RATE):
    """W, the samples of a correlation window of window_ms milliseconds"""
    return int(round(float(window_ms) * sample_rate / 1000.0))


def floor_e(floor_db=DEFAULTS["floor_db"], hop=HOP):
    """the silence floor as an energy of a frame of q: 10^(dB / 10) * hop * 2^30 in float64 (dBFS of the mean square)"""
    return 10.0 ** (float(floor_db) / 10.0) * float(hop) * float(2 ** 30)


def quantise(x, length=None):
    """x float32 [n] -> int64 [n]: clamp(rint(x * 32768), -32768, 32767), NaN -> 0, 0 from `length` on"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(32768.0)
        q = np.clip(np.rint(v), np.float32(-32768.0), np.float32(32767.0))
    q = np.where(np.isnan(v), np.float32(0.0), q).astype(np.int64)
    if length is not None:
        q[int(length):] = 0
    return q


def scores(x, T, length=None, hop=HOP, lag_lo=32, lag_hi=320, W=640, floor=None):
    """steps 1 - 3 on one row.  x float32 [ld], T frames -> (r float64 [T], lag int32 [T], silent bool [T]); floor: floor_e (None:
    the default's)"""
    floor = floor_e(hop=hop) if floor is None else float(floor)
    q = quantise(x, length)
    lo_ext = max((W + lag_hi) // 2, hop // 2)
    hi_ext = max((W + lag_hi + 1) // 2, hop - hop // 2)
    need = hop * (T - 1) + hop // 2 + hi_ext
    z = np.zeros(lo_ext + max(need, q.size), dtype=np.int64)          # z[lo_ext + i] = q[i], zero on either side
    z[lo_ext:lo_ext + q.size] = q
    sq = np.concatenate([[0], np.cumsum(z * z)])                     # sq[k] = sum of z[j]^2 over j < k
    t = np.arange(T, dtype=np.int64)
    c = hop * t + hop // 2 + lo_ext
    r = np.zeros(T, dtype=np.float64)
    lag = np.full(T, lag_lo, dtype=np.int32)
    for tau in range(lag_lo, lag_hi + 1):
        xy = np.concatenate([[0], np.cumsum(z[:z.size - tau] * z[tau:])])
        s = c - (W + tau) // 2
        sxy = xy[s + W] - xy[s]
        sxx = sq[s + W] - sq[s]
        syy = sq[s + tau + W] - sq[s + tau]
        ok = (sxy > 0) & (sxx > 0) & (syy > 0)
        den = np.sqrt(np.where(ok, sxx, 1).astype(np.float64) * np.where(ok, syy, 1).astype(np.float64))
        rho = np.where(ok, sxy.astype(np.float64) / den, 0.0)
        better = rho > r                                             # ascending tau: the first of equals stays
        r = np.where(better, rho, r)
        lag = np.where(better, tau, lag).astype(np.int32)
    e0 = hop * t + lo_ext
    energy = sq[e0 + hop] - sq[e0]
    return r, lag, energy.astype(np.float64) < floor


def decide(r, silent, thr_on=DEFAULTS["on"], thr_off=DEFAULTS["off"], bridge=DEFAULTS["bridge"], min_run=DEFAULTS["min_run"]):
    """step 4 on one row: r float64 [T], silent bool [T] -> voiced bool [T]"""
    T = len(r)
    v = np.zeros(T, dtype=bool)
    s = False
    for t in range(T):                                               # (a) hysteresis
        if silent[t]:
            s = False
        elif r[t] >= thr_on:
            s = True
        elif r[t] < thr_off:
            s = False
        v[t] = s
    for a, b in _runs(v, False):                                     # (b) bridge: the runs of (a), [a, b)
        if a >= 1 and b <= T - 1 and b - a <= bridge and not np.any(silent[a:b]):
            v[a:b] = True
    for a, b in _runs(v, True):                                      # (c) minimum run: the runs after (b)
        if a >= 1 and b <= T - 1 and b - a < min_run:
            v[a:b] = False
    return v


def _runs(v, value):
    """the maximal runs [a, b) of `value` in v, found before any of them is changed"""
    out, a = [], None
    for t, e in enumerate(list(v) + [not value]):
        if e == value and a is None:
            a = t
        elif e != value and a is not None:
            out.append((a, t))
            a = None
    return out


def voicing_rows(x, f0, length=None, hop=HOP, lag_lo=32, lag_hi=320, W=640, min_run=DEFAULTS["min_run"], bridge=DEFAULTS["bridge"],
                 on=None, thr_on=DEFAULTS["on"], thr_off=DEFAULTS["off"], floor=None):
    """alive_voicing_rows on copies: x float32 [N, ld], f0 float32 [N, T] -> dict(f0, r [N, T] float64, lag, voiced [N, T] int32,
    changed [N] int32).  on / thr_on / thr_off / floor: scalars or one per row; a row that is off keeps its f0 and leaves zeros in the
    other outputs (the kernel leaves them untouched)."""
    x = np.asarray(x, dtype=np.float32)
    f0 = np.array(f0, dtype=np.float32)
    n, T = f0.shape
    per_row = lambda v, d: np.broadcast_to(np.asarray(d if v is None else v), (n,))
    on, thr_on, thr_off = per_row(on, 1), per_row(thr_on, None), per_row(thr_off, None)
    floor = per_row(floor, floor_e(hop=hop))
    out = dict(f0=f0, r=np.zeros((n, T)), lag=np.zeros((n, T), np.int32), voiced=np.zeros((n, T), np.int32),
               changed=np.zeros(n, np.int32))
    for i in range(n):
        if not on[i]:
            continue
        r, lag, silent = scores(x[i], T, length, hop, lag_lo, lag_hi, W, floor[i])
        v = decide(r, silent, thr_on[i], thr_off[i], bridge, min_run)
        out["changed"][i] = int(np.count_nonzero(~v & (f0[i] != 0)))          # (a NaN is not zero)
        f0[i][~v] = np.float32(0.0)
        out["r"][i], out["lag"][i], out["voiced"][i] = r, lag, v
    return out
