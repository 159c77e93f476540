"""NumPy restatement of the output limiter (csrc/limit.hip; include/alive_vc.h "Limiter"): the CPU yardstick of alive_limit_rows and
alive_limit_waves, as tools/seam_ref.py is the seam's.

Everything is float32 with every operation rounded on its own, except the mean of the window minima, which is summed in float64 in
ascending order from 0.0 and divided by (double)L before it is rounded to float32 once.  With ceiling c, lookahead L >= 1 and hold
H >= 0 (P = L - 1 + H), for stream index i of the emitted signal y:
    a[j]   = c / fmax(|y[j]|, c)                        the required gain: exactly 1 where |y[j]| <= c, 1 for a NaN, 0 for an inf
    m[k]   = min a[k - H .. k + L - 1]
    g[i]   = (float)(sum_{k = i - L + 1 .. i} (double)m[k] / (double)L)
    out[i] = fmin(fmax(y[i] * g[i], -c), c)
Every window that enters g[i] contains i, so g[i] <= a[i] and |out[i]| <= c whatever the neighbours are.
`stream` runs a sequence of full per-tick waves through limit_rows and cuts the emitted spans: what a limiting converter must emit,
made from the waves of a converter that does not limit.
"""
import numpy as np

CEIL_MAX = np.float32(32767.0 / 32768.0)


def required(y, c):
    """the required gains a = c / fmax(|y|, c), float32"""
    y, c = np.asarray(y, dtype=np.float32), np.float32(c)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (c / np.fmax(np.abs(y), c)).astype(np.float32)


def gains(a, look, hold, n):
    """a float32 [P + n + L - 1]: the required gains of stream indices -P .. n + L - 2 -> g float32 [n], the gains of indices 0 .. n - 1"""
    a = np.asarray(a, dtype=np.float32)
    L, H = int(look), int(hold)
    assert L >= 1 and H >= 0 and a.shape[0] == L - 1 + H + n + L - 1
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    m = np.lib.stride_tricks.sliding_window_view(a, L + H).min(axis=1)           # m[k], k = -(L - 1) .. n - 1
    acc = np.zeros(n, dtype=np.float64)
    for k in range(L):                                                           # ascending k, from 0.0, in float64
        acc = acc + m[k:k + n].astype(np.float64)
    return (acc / np.float64(L)).astype(np.float32)


def apply(y, g, c):
    """out = fmin(fmax(y * g, -c), c) in float32: a NaN product (a NaN sample, or inf * 0) comes out as -c"""
    y, g, c = np.asarray(y, dtype=np.float32), np.asarray(g, dtype=np.float32), np.float32(c)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.fmin(np.fmax(y * g, -c), c).astype(np.float32)


def ceil_ok(c):
    return bool(np.float32(c) > 0 and np.float32(c) <= np.float32(1.0))


def fits(lo, span, sh, look, hold, ld, ld_hist):
    """whether a row's span [lo, lo + span), its lookahead [lo + sh, lo + sh + L - 1) and its history fit"""
    return (look >= 1 and hold >= 0 and lo >= 0 and 0 <= span <= sh and look <= sh and lo + sh + look - 1 <= ld
            and look - 1 + hold <= ld_hist)


def limit_rows(y, span_lo, span_len, shift, look, hold, ceil, emit, hist):
    """alive_limit_rows on copies: y float32 [N, ld], hist float32 [N, ld_hist] -> (y, hist, gmin float32 [N]; nan where the kernel
    leaves gmin alone).  Per row: emit == 0 leaves everything; look == 0, a ceiling outside (0, 1] or regions that do not fit leave y
    and set hist = 1, gmin = 1; else the span is limited with the past from hist, the present y[lo + i] and the future y[lo + shift + j],
    j < L - 1, and hist becomes the last ld_hist of (hist, a[span])"""
    y = np.array(y, dtype=np.float32)
    hist = np.array(hist, dtype=np.float32)
    n, ld = y.shape
    ld_hist = hist.shape[1]
    gmin = np.full(n, np.nan, dtype=np.float32)
    for r in range(n):
        if not emit[r]:
            continue
        lo, S, sh, L, H, c = int(span_lo[r]), int(span_len[r]), int(shift[r]), int(look[r]), int(hold[r]), np.float32(ceil[r])
        if L == 0 or not ceil_ok(c) or not fits(lo, S, sh, L, H, ld, ld_hist):
            hist[r] = 1.0
            gmin[r] = 1.0
            continue
        P = L - 1 + H
        a_span = required(y[r, lo:lo + S], c)
        a = np.concatenate([hist[r, ld_hist - P:], a_span, required(y[r, lo + sh:lo + sh + L - 1], c)])
        g = gains(a, L, H, S)
        y[r, lo:lo + S] = apply(y[r, lo:lo + S], g, c)
        hist[r] = np.concatenate([hist[r], a_span])[-ld_hist:]
        gmin[r] = np.min(g) if S else 1.0
    return y, hist, gmin


def limit_waves(y, lens, look, hold, ceil):
    """alive_limit_waves: y float32 [N, ld], lens int [N] -> (out, gmin float32 [N]): row n's first lens[n] samples limited as one
    signal with a = 1 outside it, the rest copied; a row whose ceiling is outside (0, 1] is copied whole (gmin 1)"""
    y = np.asarray(y, dtype=np.float32)
    out = y.copy()
    n, ld = y.shape
    L, H = int(look), int(hold)
    P = L - 1 + H
    gmin = np.ones(n, dtype=np.float32)
    for r in range(n):
        ln, c = min(max(int(lens[r]), 0), ld), np.float32(ceil[r])
        if ln == 0 or not ceil_ok(c):
            continue
        a = np.concatenate([np.ones(P, np.float32), required(y[r, :ln], c), np.ones(L - 1, np.float32)])
        g = gains(a, L, H, ln)
        out[r, :ln] = apply(y[r, :ln], g, c)
        gmin[r] = np.min(g)
    return out, gmin


def gain_db(gmin):
    """20 log10(gmin) per row; 0.0 for an untouched row, -inf for a gain of 0"""
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.asarray(gmin, dtype=np.float64))


def stream(waves, span_lo, span_len, shift, look, hold, ceil, emit=None, ld_hist=None, hist=None):
    """a sequence of ticks through limit_rows.  waves: T arrays float32 [N, ld], the full per-tick waves of a converter without a
    limiter; span_lo / span_len / shift int [N]; look / hold int [N] and ceil float [N], or lists of T such (a session may retune
    between ticks); emit bool [N] per tick (default: all).  Returns (limited, spans, gmins, hist): the T limited waves, per tick the
    list of N emitted spans (None for a row that does not emit), the T gmin arrays and the final history.  hist continues an earlier
    run (default: all 1.0, ld_hist wide)"""
    waves = [np.asarray(w, dtype=np.float32) for w in waves]
    n = waves[0].shape[0]
    per_tick = np.ndim(look[0]) > 0
    if hist is None:
        hist = np.ones((n, int(ld_hist)), dtype=np.float32)
    limited, spans, gmins = [], [], []
    for t, w in enumerate(waves):
        e = [True] * n if emit is None else emit[t]
        lk, hd, cl = (look[t], hold[t], ceil[t]) if per_tick else (look, hold, ceil)
        y, hist, gm = limit_rows(w, span_lo, span_len, shift, lk, hd, cl, e, hist)
        limited.append(y)
        spans.append([y[r, int(span_lo[r]):int(span_lo[r]) + int(span_len[r])].copy() if e[r] else None for r in range(n)])
        gmins.append(gm)
    return limited, spans, gmins, hist
