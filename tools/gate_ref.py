"""NumPy restatement of the input gate (csrc/gate.hip; include/alive_vc.h "Input gate"): the CPU yardstick of alive_gate_rows and
alive_gate_apply_rows, as tools/pitch_ref.py is auto pitch's.

The level of a row is the mean square of its window in float64, summed in the kernel's own order (256 strided partial sums, then a
pairwise tree), so it can be compared bitwise; a square of a float32 is exact in float64.  The state machine is integer work.  The
ramp is float32 with every operation rounded on its own.
"""
import math

import numpy as np


def thr_ms(gate_db):
    """the threshold as a mean square: 10^(dB / 10) in float64 (dBFS of the 16 kHz ring after the input gain)"""
    return 10.0 ** (float(gate_db) / 10.0)


def hold_ticks(gate_hold, tick_seconds):
    """the ticks a gate stays open after the last loud one: ceil(hold / tick)"""
    return int(math.ceil(float(gate_hold) / float(tick_seconds)))


def mean_square(x, w_lo, w_hi):
    """x float32 [N, ld] -> float64 [N]: sum of x[n][t]^2 over [w_lo, w_hi) / (w_hi - w_lo) in alive_gate_rows' order: partial sum tid
    takes t = w_lo + tid, + 256, ... in turn, then acc[i] += acc[i + o] for o = 128, 64, ..., 1"""
    x = np.asarray(x, dtype=np.float32)
    w = x[:, w_lo:w_hi].astype(np.float64)
    sq = w * w
    n, l = sq.shape
    pad = -l % 256
    sq = np.concatenate([sq, np.zeros((n, pad))], axis=1).reshape(n, -1, 256)      # (+ 0.0 leaves a non-negative sum as it is)
    acc = np.zeros((n, 256), dtype=np.float64)
    for j in range(sq.shape[1]):
        acc = acc + sq[:, j]
    o = 128
    while o > 0:
        acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
        o >>= 1
    return acc[:, 0] / float(w_hi - w_lo)


def gate_rows(state, ms, gate_on, thr, hold, emit, seg_len, S=1, world_on=None):
    """one tick of the state machine.  state int [N, 2] = (hold_left, was_open), ms float64 [N] -> dict of the new state, g0, g1
    (float32 [N]), seg_len_eff (int32 [N * S]), follow (bool [N]), world_eff (int32 [N], None without world_on) and open (bool [N]: the
    row's gate after the tick; True for a row that is not gated).
    A row with gate_on == 0 or emit == 0: g0 = g1 = 1, seg_len_eff = seg_len, follow = emit, world_eff = world_on, state untouched.
    Else loud = ms >= thr: loud -> left = hold, open; not loud -> open = left > 0, then left = max(left - 1, 0).  g0 = was_open, g1 =
    open; skip = closed at both ends; seg_len_eff = 0 on a skipped row; world_eff = world_on and not skip; follow = open."""
    state = np.array(state, dtype=np.int32).reshape(-1, 2)
    n = state.shape[0]
    seg_len = np.asarray(seg_len, dtype=np.int32).reshape(n, S)
    out = dict(state=state, g0=np.ones(n, np.float32), g1=np.ones(n, np.float32), seg_len_eff=seg_len.copy(),
               follow=np.array([bool(e) for e in emit]), open=np.ones(n, dtype=bool),
               world_eff=None if world_on is None else np.array(world_on, dtype=np.int32))
    for r in range(n):
        if not gate_on[r] or not emit[r]:
            continue
        left, was = int(state[r, 0]), bool(state[r, 1])
        if ms[r] >= thr[r]:
            left, is_open = int(hold[r]), True
        else:
            is_open = left > 0
            left = max(left - 1, 0)
        state[r] = (left, int(is_open))
        out["g0"][r], out["g1"][r] = float(was), float(is_open)
        skip = not was and not is_open
        if skip:
            out["seg_len_eff"][r] = 0
        if world_on is not None:
            out["world_eff"][r] = int(bool(world_on[r]) and not skip)
        out["follow"][r] = is_open
        out["open"][r] = is_open
    out["seg_len_eff"] = out["seg_len_eff"].reshape(-1)
    return out


def ramp(g0, g1, span_len):
    """the float32 gains of a span: g0 + (g1 - g0) * ((i + 1) / span_len), i in [0, span_len)"""
    g0, g1 = np.float32(g0), np.float32(g1)
    t = np.arange(1, span_len + 1, dtype=np.float32) / np.float32(span_len)
    return (g0 + (g1 - g0) * t).astype(np.float32)


def apply_rows(y, span_lo, span_len, g0, g1):
    """alive_gate_apply_rows on a copy of y float32 [N, ld]: rows at (1, 1) untouched, rows at (0, 0) +0.0 over the span, the others
    multiplied by the ramp; spans clamped to the row"""
    y = np.array(y, dtype=np.float32)
    ld = y.shape[1]
    for n in range(y.shape[0]):
        if g0[n] == 1 and g1[n] == 1:
            continue
        lo, ln = int(span_lo[n]), int(span_len[n])
        if ln <= 0:
            continue
        i = np.arange(ln)
        i = i[(lo + i >= 0) & (lo + i < ld)]
        if g0[n] == 0 and g1[n] == 0:
            y[n, lo + i] = np.float32(0.0)
        else:
            y[n, lo + i] = y[n, lo + i] * ramp(g0[n], g1[n], ln)[i]
    return y
