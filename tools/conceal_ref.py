"""NumPy restatement of the lost-chunk concealment (csrc/conceal.hip: alive_conceal_rows), bit for bit: the yardstick of
tests/test_host_conceal.py and tests/test_gpu_conceal.py.  Host only, no device.

Waveform substitution in the style of G.711 Appendix I, at the input edge of a sparse MultiStreamConverter: when a session's chunk is
LOST (its clock must go on, unlike a stall) the hole in its int16 ring is filled with the ring's last pitch period, repeated and -- if
the loss goes on -- faded out; the first chunk that arrives again is crossfaded in from that continuation.

Per session at rate r (samples per second), ring = the session's int16 ring in time order, rl samples, newest last:
    lag range   lag_lo = r // 400 .. lag_hi = ceil(r / 60)   (60 - 400 Hz);  window W = r // 50 (20 ms)
    hold = round(hold_ms r / 1000), fade = max(1, round(fade_ms r / 1000)), rec = min(round(recover_ms r / 1000), chunk_len)
    the ring must hold need = max(W + lag_hi, 2 lag_hi) samples (587 at 16 kHz), at most MAX_SPAN
Period: a[i] = ring[rl - W + i]; for every lag l: C(l) = sum a[i] ring[rl - W + i - l], E(l) = sum ring[rl - W + i - l]^2, exact in
int64; score = double(C) * double(C) / double(E) if C > 0 and E > 0 else 0 (each operation rounded on its own); P = the lag with the
largest score, the lowest lag on a tie (a silent ring: P = lag_lo).
Template: t[j] = ring[rl - P + j], j < P; over its last V = P // 4 samples faded into the period before it: for m = 1 .. V, j = P - V +
m - 1: t[j] = rint(a + ((b - a) * m) / (V + 1)), a = ring[rl - P + j], b = ring[rl - 2 P + j], in fp64 ((b - a) * m is an exact integer).
Taken ONCE, at the first lost chunk of a run.
Attenuation: att(k) = 0 if d <= 0, 1 if d >= fade, else double(d) / double(fade), d = hold + fade - k; k counts the run's samples.
A lost chunk: chunk[i] = rint(t[(q + i) mod P] * att(q + i)); q = min(q + cl, QMAX).
Recovery (the first real chunk c after a run, q > 0): for i < rec, s = t[(q + i) mod P] * att(q + i) unrounded, chunk[i] = rint(s +
((c[i] - s) * (i + 1)) / (rec + 1)) clamped to int16; the rest of c untouched; then the state is (0, 0).
A session with concealment off that loses a chunk gets zeros, and its state is (0, 0).
State per session: (q, P) int32 and the template int16 [lag_hi]; a row that is absent (a stall) leaves all of it standing still.
"""
import numpy as np

QMAX = 1 << 30           # ALIVE_CONCEAL_QMAX: where a run's sample count saturates (the output is zeros long before)
MAX_SPAN = 4096          # ALIVE_CONCEAL_MAX_SPAN: the most ring samples a row's search may need (they are staged in LDS)


def geometry(rate, chunk_len, hold_ms=10.0, fade_ms=50.0, recover_ms=5.0):
    """a session's constants -> dict(lag_lo, lag_hi, window, hold, fade, recover, need)"""
    r = int(rate)
    lag_lo, lag_hi, w = r // 400, -(-r // 60), r // 50
    return dict(lag_lo=lag_lo, lag_hi=lag_hi, window=w, hold=int(round(float(hold_ms) * r / 1000.0)),
                fade=max(1, int(round(float(fade_ms) * r / 1000.0))),
                recover=min(int(round(float(recover_ms) * r / 1000.0)), int(chunk_len)), need=max(w + lag_hi, 2 * lag_hi))


def scores(ring, lag_lo, lag_hi, w):
    """(C, E, score) over the lags lag_lo .. lag_hi of `ring` (its last sample the newest): int64, int64, float64"""
    x = np.asarray(ring).astype(np.int64)
    rl = x.shape[0]
    a = x[rl - w:]
    lags = np.arange(lag_lo, lag_hi + 1)
    seg = x[rl - w - lag_hi:rl - lag_lo]                      # windows start at rl - w - l: position lag_hi - l of seg
    win = np.lib.stride_tricks.sliding_window_view(seg, w)[lag_hi - lags]
    C = win @ a
    sq = np.concatenate([[0], np.cumsum(seg * seg)])
    E = sq[lag_hi - lags + w] - sq[lag_hi - lags]
    Cd, Ed = C.astype(np.float64), E.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where((C > 0) & (E > 0), (Cd * Cd) / Ed, 0.0)
    return C, E, sc


def find_period(ring, lag_lo, lag_hi, w):
    """the lag with the largest score, the lowest on a tie"""
    return int(lag_lo + np.argmax(scores(ring, lag_lo, lag_hi, w)[2]))      # (argmax: the first of equal maxima)


def template(ring, P):
    """the last period of `ring` as int16 [P], its last P // 4 samples faded into the period before"""
    x = np.asarray(ring).astype(np.int64)
    rl = x.shape[0]
    t = x[rl - P:].copy()
    V = P // 4
    if V:
        j = np.arange(P - V, P)
        m = j - (P - V) + 1
        a, b = x[rl - P + j], x[rl - 2 * P + j]
        t[j] = np.rint(a.astype(np.float64) + ((b - a) * m).astype(np.float64) / np.float64(V + 1)).astype(np.int64)
    return t.astype(np.int16)


def att(k, hold, fade):
    """the attenuation at run samples k (an int64 array) -> float64"""
    d = np.int64(hold) + np.int64(fade) - np.asarray(k, dtype=np.int64)
    return np.where(d <= 0, 0.0, np.where(d >= fade, 1.0, d.astype(np.float64) / np.float64(fade)))


def _continuation(t, q, n, hold, fade):
    """the unrounded continuation s[i] = t[(q + i) mod P] * att(q + i), i < n"""
    k = np.int64(q) + np.arange(n, dtype=np.int64)
    return np.asarray(t).astype(np.float64)[k % len(t)] * att(k, hold, fade)


def synth(t, q, n, hold, fade):
    """a lost chunk of n samples after q run samples -> int16 [n]"""
    return np.rint(_continuation(t, q, n, hold, fade)).astype(np.int16)


def recover(t, q, c, rec, hold, fade):
    """the first real chunk c after a run of q samples -> int16: its first rec samples faded in from the continuation"""
    c = np.asarray(c, dtype=np.int16)
    out = c.copy()
    rec = min(int(rec), c.shape[0])
    if rec > 0:
        s = _continuation(t, q, rec, hold, fade)
        i1 = np.arange(1, rec + 1).astype(np.float64)
        v = np.rint(s + ((c[:rec].astype(np.float64) - s) * i1) / np.float64(rec + 1))
        out[:rec] = np.clip(v, -32768.0, 32767.0).astype(np.int16)
    return out


def row_fits(rl, cl, ld, ld_chunk, ld_tmpl, g):
    """whether a row takes part: its lengths fit the strides and its ring holds what its lags need (the kernel's own test)"""
    lo, hi, w = int(g["lag_lo"]), int(g["lag_hi"]), int(g["window"])
    if not (1 <= cl <= ld_chunk and 1 <= rl <= ld and cl <= rl):
        return False
    if not (1 <= lo <= hi and w >= 1 and hi <= ld_tmpl and int(g["fade"]) >= 1 and int(g["hold"]) >= 0 and int(g["recover"]) >= 0):
        return False
    if int(g["hold"]) > QMAX or int(g["fade"]) > QMAX:
        return False
    need = max(w + hi, 2 * hi)
    return need <= rl and need <= MAX_SPAN


def conceal_rows(ring, ring_len, chunks, chunk_len, present, lost, on, lag_lo, lag_hi, window, hold, fade, recover_len, state, tmpl):
    """alive_conceal_rows over all rows, on copies: ring int16 [N, ld] (read only), chunks int16 [N, ld_chunk], present / lost / on
    [N], the six per-row constants [N], state int32 [N, 2], tmpl int16 [N, ld_tmpl] -> dict(chunks=, state=, tmpl=)"""
    ring, chunks = np.asarray(ring), np.array(chunks, dtype=np.int16, copy=True)
    state, tmpl = np.array(state, dtype=np.int32, copy=True), np.array(tmpl, dtype=np.int16, copy=True)
    for n in range(ring.shape[0]):
        rl, cl = int(ring_len[n]), int(chunk_len[n])
        g = dict(lag_lo=lag_lo[n], lag_hi=lag_hi[n], window=window[n], hold=hold[n], fade=fade[n], recover=recover_len[n])
        if not present[n] or not row_fits(rl, cl, ring.shape[1], chunks.shape[1], tmpl.shape[1], g):
            continue
        q, P = int(state[n, 0]), int(state[n, 1])
        if q < 0 or (q > 0 and not 1 <= P <= int(lag_hi[n])):
            continue                                           # (a state no run of this kernel leaves behind: the row is left alone)
        if lost[n]:
            if not on[n]:
                chunks[n, :cl] = 0
                state[n] = 0
                continue
            if q == 0:
                P = find_period(ring[n, :rl], int(lag_lo[n]), int(lag_hi[n]), int(window[n]))
                tmpl[n, :P] = template(ring[n, :rl], P)
            chunks[n, :cl] = synth(tmpl[n, :P], q, cl, int(hold[n]), int(fade[n]))
            state[n] = (min(q + cl, QMAX), P)
        elif q > 0:
            chunks[n, :cl] = recover(tmpl[n, :P], q, chunks[n, :cl], int(recover_len[n]), int(hold[n]), int(fade[n]))
            state[n] = 0
    return dict(chunks=chunks, state=state, tmpl=tmpl)


class StreamRef:
    """One session's input edge on the host: its ring in time order (zeros at first) and its concealment state.  feed(chunk) for a
    chunk that arrived, feed(None) for one that was lost -> the chunk that enters the ring (what a converter without concealment
    would have to be fed to do the same)."""

    def __init__(self, rate, chunk_len, buffersize, on=True, hold_ms=10.0, fade_ms=50.0, recover_ms=5.0):
        self.cl, self.rl, self.on = int(chunk_len), int(chunk_len) * int(buffersize), bool(on)
        self.g = geometry(rate, chunk_len, hold_ms, fade_ms, recover_ms)
        if self.rl < self.g["need"]:
            raise ValueError(f"a ring of {self.rl} samples is shorter than the {self.g['need']} the concealment needs")
        self.ring = np.zeros(self.rl, np.int16)
        self.q, self.P, self.t = 0, 0, None

    def feed(self, chunk):
        g = self.g
        if chunk is None:
            if not self.on:
                out, self.q, self.P = np.zeros(self.cl, np.int16), 0, 0
            else:
                if self.q == 0:
                    self.P = find_period(self.ring, g["lag_lo"], g["lag_hi"], g["window"])
                    self.t = template(self.ring, self.P)
                out = synth(self.t, self.q, self.cl, g["hold"], g["fade"])
                self.q = min(self.q + self.cl, QMAX)
        else:
            out = np.asarray(chunk, dtype=np.int16).reshape(-1)
            if self.q > 0:
                out = recover(self.t, self.q, out, g["recover"], g["hold"], g["fade"])
                self.q, self.P = 0, 0
        self.ring = np.concatenate([self.ring[self.cl:], out])
        return out
