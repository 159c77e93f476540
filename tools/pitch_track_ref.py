"""NumPy restatement of the pitch tracker (csrc/f0_track.hip; include/alive_vc.h "Pitch tracking"): the CPU yardstick of
alive_f0_track_rows, as tools/envelope_ref.py is the envelope follow's.

A Viterbi path over the f0 estimator's class scores instead of the per-frame argmax.  The states i = 0 .. S - 1 stand for the classes
lo .. hi (1 <= lo <= hi <= 4095, S = hi - lo + 1 <= 4000); everything is float64 with every operation rounded on its own (only + - *
abs and compares, so NumPy and the device agree bit for bit).  Tables, built once on the host and shared with the device:
    s[i]            12 log2(lo + i)
    blo[i], bhi[i]  the first and last state j with |s[i] - s[j]| <= band (semitones)
Per row, with weight w >= 0 (cost per semitone moved inside the band) and jump k >= 0 (flat cost of any other move), both in the units
of the scores:
    x[t][i]   (double) of logits[lo + i][t] with NaN -> -FLT_MAX, else clamped to +-FLT_MAX
    e[t][i]   x[t][i] - max_j x[t][j]                                         the frame's scores below its best one: <= 0, the best 0
    D[0][i]   e[0][i]
    t >= 1:   g = max_j D[t - 1][j] - k                                       gi: the lowest j attaining the max
              a = max_{j = blo[i] .. bhi[i]} (D[t - 1][j] - w |s[i] - s[j]|)    ai: the lowest j attaining it
              (m, back[t][i]) = (a, ai) if a >= g else (g, gi);   D[t][i] = e[t][i] + m
    p[T - 1] = the lowest i attaining max D[T - 1];  p[t - 1] = back[t][p[t]];  f0[t] = (float)(lo + p[t])
T = 1 is the argmax over [lo, hi]; w = k = 0 is the per-frame argmax over [lo, hi], the lowest class on ties; class 0 is not a state, so
a tracked contour never holds 0.  The path does not depend on a constant added to a frame's scores; taking the frame's best score off
keeps D within the reach of fp64 whatever the scores are: a frame that is all NaN (or all equal) is e = 0, a frame of no information,
and the path passes through it as the moves' costs say, where D = -FLT_MAX + m would round every m away and lose the path for good.
"""
import numpy as np

MAX_STATES = 4000                               # ALIVE_F0_TRACK_MAX_STATES (include/alive_vc.h)
LO, HI, BAND, WEIGHT, JUMP = 50, 1100, 2.0, 1.0, 12.0
FLT_MAX = float(np.finfo(np.float32).max)


def tables(lo=LO, hi=HI, band=BAND):
    """(s float64 [S], blo int32 [S], bhi int32 [S]) as module/common.py::pitch_track_tables forms them"""
    lo, hi, band = int(lo), int(hi), float(band)
    if not (1 <= lo <= hi <= 4095) or hi - lo + 1 > MAX_STATES or not (np.isfinite(band) and band >= 0.0):
        raise ValueError(f"pitch track: needs 1 <= lo <= hi <= 4095, at most {MAX_STATES} states and a finite band >= 0")
    s = 12.0 * np.log2(np.arange(lo, hi + 1, dtype=np.float64))
    S = s.size
    blo, bhi = np.empty(S, dtype=np.int32), np.empty(S, dtype=np.int32)
    for i0 in range(0, S, 256):
        near = np.abs(s[i0:i0 + 256, None] - s[None, :]) <= band
        blo[i0:i0 + 256] = near.argmax(axis=1)
        bhi[i0:i0 + 256] = S - 1 - near[:, ::-1].argmax(axis=1)
    return s, blo, bhi


def scores(logits, lo, S):
    """logits float32 [C, T] -> e float64 [T, S]"""
    x = np.asarray(logits, dtype=np.float32)[lo:lo + S].T
    x = np.where(np.isnan(x), np.float32(-FLT_MAX), np.clip(x, np.float32(-FLT_MAX), np.float32(FLT_MAX)))
    return x.astype(np.float64)


def centred(e):
    """e float64 [T, S] -> each frame's scores minus the frame's best one"""
    return e - e.max(axis=1, keepdims=True)


class Tracker:
    """the tables of one (lo, hi, band) and the gather that turns a score column into every state's band candidates"""

    def __init__(self, lo=LO, hi=HI, band=BAND):
        self.lo, self.hi, self.band = int(lo), int(hi), float(band)
        self.s, self.blo, self.bhi = tables(lo, hi, band)
        self.S = self.s.size
        width = int((self.bhi - self.blo).max()) + 1
        j = self.blo[:, None].astype(np.int64) + np.arange(width)[None, :]
        self.inside = j <= self.bhi[:, None]
        self.j = np.where(self.inside, j, 0)
        self.dist = np.abs(self.s[:, None] - self.s[self.j])

    def path(self, logits, weight=WEIGHT, jump=JUMP):
        """logits float32 [C, T] -> the states p int64 [T]"""
        w, k = float(weight), float(jump)
        if not (np.isfinite(w) and np.isfinite(k) and w >= 0.0 and k >= 0.0):
            raise ValueError("pitch track: weight and jump must be finite and >= 0")
        e = centred(scores(logits, self.lo, self.S))
        T = e.shape[0]
        back = np.zeros((T, self.S), dtype=np.int64)
        cost = w * self.dist
        D = e[0].copy()
        for t in range(1, T):
            gi = int(D.argmax())                            # (argmax: the lowest index of the maximum)
            g = D[gi] - k
            cand = np.where(self.inside, D[self.j] - cost, -np.inf)
            ak = cand.argmax(axis=1)
            a = cand[np.arange(self.S), ak]
            band = a >= g
            back[t] = np.where(band, self.blo + ak, gi)
            D = e[t] + np.where(band, a, g)
        p = np.empty(T, dtype=np.int64)
        p[T - 1] = int(D.argmax())
        for t in range(T - 1, 0, -1):
            p[t - 1] = back[t][p[t]]
        return p

    def track(self, logits, weight=WEIGHT, jump=JUMP):
        """logits float32 [C, T] -> f0 float32 [T]: the tracked classes"""
        return (self.lo + self.path(logits, weight, jump)).astype(np.float32)


def track(logits, lo=LO, hi=HI, band=BAND, weight=WEIGHT, jump=JUMP):
    return Tracker(lo, hi, band).track(logits, weight, jump)


def track_rows(logits, f0, tracker, on=None, weight=WEIGHT, jump=JUMP):
    """alive_f0_track_rows: logits [N, C, T], f0 float32 [N, T] (what the rows hold on entry) -> (f0 [N, T], changed int32 [N]); a row
    that is off keeps its f0 and its `changed` (0 here)"""
    logits, out = np.asarray(logits, dtype=np.float32), np.array(f0, dtype=np.float32)
    N = logits.shape[0]
    on = np.ones(N, dtype=np.int32) if on is None else np.asarray(on)
    weight, jump = np.broadcast_to(np.asarray(weight, dtype=np.float64), (N,)), np.broadcast_to(np.asarray(jump, dtype=np.float64), (N,))
    changed = np.zeros(N, dtype=np.int32)
    for n in range(N):
        if on[n]:
            new = tracker.track(logits[n], weight[n], jump[n])
            changed[n] = int((new != out[n]).sum())
            out[n] = new
    return out, changed


def brute_force(logits, tracker, weight, jump):
    """the best path by enumeration of all S^T of them (tiny S and T), scored as the recurrence scores a path: ties go to the path the
    recurrence would pick, so only paths with a unique best score are comparable"""
    import itertools
    e = centred(scores(logits, tracker.lo, tracker.S))
    T, S = e.shape
    s, band = tracker.s, tracker.band
    best, arg, ties = -np.inf, None, 0
    for p in itertools.product(range(S), repeat=T):
        v = e[0][p[0]]
        for t in range(1, T):
            d = abs(s[p[t]] - s[p[t - 1]])
            m = v - float(jump)
            if d <= band:
                m = max(m, v - float(weight) * d)
            v = e[t][p[t]] + m
        if v > best:
            best, arg, ties = v, p, 1
        elif v == best:
            ties += 1
    return np.array(arg), best, ties


def ridge_scores(centres, heights, seed=0, classes=4096):
    """the test signal: N(0, 1) noise from default_rng(seed) of shape [classes, T] plus, per frame, ridges h exp(-((c - f) / 3)^2 / 2);
    centres / heights: per frame a list of ridge centres (Hz) and heights"""
    T = len(centres)
    x = np.random.default_rng(seed).standard_normal((classes, T))
    c = np.arange(classes, dtype=np.float64)
    for t in range(T):
        for f, h in zip(centres[t], heights[t]):
            x[:, t] += h * np.exp(-0.5 * ((c - f) / 3.0) ** 2)
    return x.astype(np.float32)
