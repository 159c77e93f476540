"""NumPy restatement of the seam crossfade (csrc/seam.hip; include/alive_vc.h "Seam crossfade"): the CPU yardstick of alive_seam_rows,
as tools/gate_ref.py is the gate's.

The fade is float32 with every operation rounded on its own: w = (i + 1) / (Xe + 1), y = t + (c - t) * w.  The seam statistic is
summed in float64 in the kernel's own order (256 strided partial sums, then a pairwise tree), so it can be compared bitwise.
`stream` runs a sequence of full per-tick waves through seam_rows and cuts the emitted spans: what a crossfading converter must
emit, made from the waves of a converter that does not crossfade.
"""
import numpy as np


def ordered_sum(v):
    """v float64 [L] -> its sum in alive_seam_rows' order: partial sum tid takes v[tid], v[tid + 256], ... in turn, then
    acc[i] += acc[i + o] for o = 128, 64, ..., 1"""
    v = np.asarray(v, dtype=np.float64)
    v = np.concatenate([v, np.zeros(-v.shape[0] % 256)]).reshape(-1, 256)        # (+ 0.0 leaves a non-negative sum as it is)
    acc = np.zeros(256, dtype=np.float64)
    for j in range(v.shape[0]):
        acc = acc + v[j]
    o = 128
    while o > 0:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o >>= 1
    return acc[0]


def weights(xe):
    """the float32 weights of a fade over xe samples: (i + 1) / (xe + 1), i in [0, xe): never 0, never 1"""
    return np.arange(1, xe + 1, dtype=np.float32) / np.float32(xe + 1)


def fits(lo, sh, x, ld, ld_tail):
    """whether a row's two regions [lo, lo + x) and [lo + sh, lo + sh + x) lie in a row of ld samples, apart, and x in the tail"""
    return lo >= 0 and 0 <= x <= ld_tail and x <= sh and lo + sh + x <= ld


def seam_rows(y, span_lo, shift, xlen, emit, tail, stored, g0=None, g1=None):
    """alive_seam_rows on copies: y float32 [N, ld], tail float32 [N, ld_tail], stored int [N] -> (y, tail, stored, stats float64
    [N, 2]).  Per row: emit == 0 leaves everything; xlen == 0 or regions that do not fit leave y and set stored = 0; else
    Xe = min(xlen, max(stored, 0)), stats = (sum (c - t)^2, sum c^2) of the unfaded head over i < Xe, the head faded from the tail,
    the new tail y[lo + shift : lo + shift + xlen], stored = xlen -- 0 where g0 and g1 are given and both 0 for the row"""
    y = np.array(y, dtype=np.float32)
    tail = np.array(tail, dtype=np.float32)
    stored = np.array(stored, dtype=np.int32)
    n, ld = y.shape
    ld_tail = tail.shape[1]
    stats = np.zeros((n, 2), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(n):
            if not emit[r]:
                continue
            lo, sh, x = int(span_lo[r]), int(shift[r]), int(xlen[r])
            if x == 0 or not fits(lo, sh, x, ld, ld_tail):
                stored[r] = 0
                continue
            xe = min(x, max(int(stored[r]), 0))
            t, c = tail[r, :xe].copy(), y[r, lo:lo + xe].copy()
            d = c.astype(np.float64) - t.astype(np.float64)
            v = c.astype(np.float64)
            stats[r] = ordered_sum(d * d), ordered_sum(v * v)
            y[r, lo:lo + xe] = t + (c - t) * weights(xe)
            tail[r, :x] = y[r, lo + sh:lo + sh + x]
            stored[r] = 0 if (g0 is not None and g0[r] == 0 and g1[r] == 0) else x
    return y, tail, stored, stats


def seam_db(stats):
    """stats float64 [N, 2] -> 10 log10(d2 / e2) per row, nan for a row that did not fade (or whose head was all zero)"""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(stats[:, 0] / stats[:, 1])
    return np.where(stats[:, 1] > 0, db, np.nan)


def stream(waves, span_lo, span_len, shift, xlen, emit=None, ld_tail=None, tail=None, stored=None, gains=None):
    """a sequence of ticks through seam_rows.  waves: T arrays float32 [N, ld], the full per-tick waves of a converter without
    crossfade; span_lo / span_len / shift int [N]; xlen int [N], or a list of T such (a session may retune between ticks); emit bool
    [N] per tick (default: all); gains: per tick None or (g0, g1).  Returns (faded, spans, stats, tail, stored): the T faded waves,
    per tick the list of N emitted spans y[n, lo : lo + len] (None for a row that does not emit), the T stats arrays and the
    final state.  tail / stored continue an earlier run (default: nothing stored)"""
    waves = [np.asarray(w, dtype=np.float32) for w in waves]
    n = waves[0].shape[0]
    per_tick = np.ndim(xlen[0]) > 0
    if tail is None:
        width = int(ld_tail) if ld_tail is not None else max(1, int(np.max(xlen)))
        tail, stored = np.zeros((n, width), dtype=np.float32), np.zeros(n, dtype=np.int32)
    faded, spans, stats = [], [], []
    for t, w in enumerate(waves):
        e = [True] * n if emit is None else emit[t]
        g = (None, None) if gains is None or gains[t] is None else gains[t]
        y, tail, stored, st = seam_rows(w, span_lo, shift, xlen[t] if per_tick else xlen, e, tail, stored, *g)
        faded.append(y)
        spans.append([y[r, int(span_lo[r]):int(span_lo[r]) + int(span_len[r])].copy() if e[r] else None for r in range(n)])
        stats.append(st)
    return faded, spans, stats, tail, stored
