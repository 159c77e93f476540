"""NumPy restatement of the auto-pitch arithmetic (csrc/pitch_auto.hip; include/alive_vc.h "Auto pitch"): the CPU yardstick of
alive_pitch_stats_groups, alive_pitch_shift_groups and alive_pitch_follow_rows, as tools/world_ref.py is WORLD's.

"pitch" is the reference's 12 * log2(f0 / 440) - 9 (inference.py:119) as the kernels form it: f0 / 440 in float32, log2 in float64 rounded
once to float32, the product and the difference in float32.  A frame is voiced when that value is finite (inference.py:121): 0, negative
values, NaN and inf are unvoiced.  Sums are float64 (NumPy's order, not the kernels': compare sums to ~1e-12 relative, counts exactly).
"""
import numpy as np


def pitch(f0):
    """float32 pitch of float32 f0 (any shape); unvoiced frames come out as -inf / NaN / +inf"""
    f0 = np.asarray(f0, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.log2((f0 / np.float32(440.0)).astype(np.float64)).astype(np.float32)
        return np.float32(12.0) * lg - np.float32(9.0)


def voiced(p):
    return np.isfinite(p)


def mean_pitch(f0):
    """the voiced mean pitch of f0 as a float64 (NaN when nothing is voiced): inference.py:121's mean_pitch"""
    p = pitch(f0)
    v = voiced(p)
    return float(p[v].astype(np.float64).sum() / v.sum()) if v.any() else float("nan")


def stats_groups(f0, first, t_lo=0, t_hi=None):
    """f0 [N, T], first [G + 1] -> float64 [G, 2]: (sum of voiced pitch, voiced count) over frames [t_lo, t_hi) of rows
    first[g] .. first[g + 1] - 1; empty and all-unvoiced groups give (0, 0)"""
    f0 = np.asarray(f0, dtype=np.float32)
    f0 = f0.reshape(f0.shape[0], -1)
    t_hi = f0.shape[1] if t_hi is None else t_hi
    out = np.zeros((len(first) - 1, 2), dtype=np.float64)
    for g in range(len(first) - 1):
        p = pitch(f0[first[g]:first[g + 1], t_lo:t_hi])
        v = voiced(p)
        out[g] = (p[v].astype(np.float64).sum(), float(v.sum()))
    return out


def shift_groups(stats, offset, auto_on, target):
    """the offline shift of every group, float32 [G]: offset + (target - float32(sum / count)) on an auto group with voiced frames,
    else offset"""
    offset, target = np.asarray(offset, dtype=np.float32), np.asarray(target, dtype=np.float32)
    out = offset.copy()
    for g, (s, c) in enumerate(np.asarray(stats, dtype=np.float64)):
        if auto_on[g] and c != 0:
            out[g] = offset[g] + (target[g] - np.float32(s / c))
    return out


def follow_rows(state, f0, f0_rate, offset, auto_on, target, emit, decay, prior):
    """one streaming update: state float64 [N, 2] = (S, W), f0 [N, T] -> (new state, shift float32 [N]).  A row with auto_on == 0:
    shift = offset, state untouched.  An auto row: if emit, S <- decay S + sum of voiced p_t and W <- decay W + count with
    p_t = pitch(f0 * f0_rate); then shift = offset + float32(W / (W + prior) * (target - S / W)), the automatic part 0 when W == 0."""
    f0 = np.asarray(f0, dtype=np.float32)
    f0 = f0.reshape(f0.shape[0], -1)
    state = np.array(state, dtype=np.float64)
    offset = np.asarray(offset, dtype=np.float32)
    shift = offset.copy()
    for n in range(f0.shape[0]):
        if not auto_on[n]:
            continue
        S, W = state[n]
        if emit[n]:
            p = pitch(f0[n] * np.float32(f0_rate[n]))
            v = voiced(p)
            S = decay * S + p[v].astype(np.float64).sum()
            W = decay * W + float(v.sum())
            state[n] = (S, W)
        a = np.float32(0.0) if W == 0 else np.float32(W / (W + prior) * (float(np.float32(target[n])) - S / W))
        shift[n] = offset[n] + a
    return state, shift


def decay_of(tick_seconds, half_life):
    """the per-tick decay of a half-life in seconds (None: never forget)"""
    return 1.0 if half_life is None else 2.0 ** (-tick_seconds / half_life)
