"""Float64 NumPy restatement of WORLD's DIO + StoneMask F0 estimation: the CPU reference of csrc/world_f0.hip.

Restated from the published algorithm (M. Morise, "Harvest"/"DIO" papers and the WORLD vocoder's documented defaults): pyworld
itself is not part of this project, so parity with it is UNPINNED; what this file pins is the device kernels, which follow it
operation by operation:

  * DIO's filtering is written as zero-extended linear convolutions in the time domain (WORLD multiplies spectra; the sums are
    the same up to rounding), each output a sequential sum over the taps in a fixed order, mul and add rounded separately;
  * the mean is a 256-way strided sum followed by a pairwise tree, the order of the kernel's reduction;
  * the filter taps come from `taps()`, whose cosines are Python's `math.cos`, the C library's cos the device library uses to
    build the same table (alive_world_f0_taps).
So on the same input the kernels' DIO is bitwise this file's; StoneMask evaluates its DFT bins with the device's sin/cos and
agrees to rounding.

  dio(x, fs, ...)        -> (f0, t)          pyworld.dio with f0_floor / f0_ceil / channels_in_octave / frame_period / allowed_range
  stonemask(x, f0, t, fs) -> refined f0       pyworld.stonemask
  dio_stonemask_rows(X, fs, f0_floor, f0_ceil) -> float32 [N, F]   the pair on every row of X (float32 [N, L] at fs)
  dio_stages(X, fs, ...)  -> per row what every stage of the kernels leaves behind (mean, low cut, streams, candidates, contour steps)
  stonemask_margin(x, fs, t, f0) -> how far StoneMask's frame is from taking another branch on a value it computes
"""
import math

import numpy as np

K_CUTOFF = 50.0                 # DIO's low-cut frequency
K_SAFE = 1e-12                  # WORLD's kMySafeGuardMinimum
K_MAX = 100000.0                # WORLD's kMaximumValue
K_FLOOR_STONEMASK = 40.0
LOG2 = 0.69314718055994529


def matlab_round(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def n_frames(L, fs, frame_period=5.0):
    return int(1000.0 * L / fs / frame_period) + 1


def bands(f0_floor, f0_ceil, channels_in_octave=2.0):
    nb = 1 + int(math.log(f0_ceil / f0_floor) / LOG2 * channels_in_octave)
    return [f0_floor * 2.0 ** ((i + 1) / channels_in_octave) for i in range(nb)]


def taps(fs, f0_floor, f0_ceil, channels_in_octave=2.0):
    """(low-cut taps at lags -c..c, [(h, nuttall taps [4h]) per band])"""
    c = matlab_round(fs / K_CUTOFF)
    n = 2 * c + 1
    hann = [0.5 - 0.5 * math.cos(i * 2.0 * math.pi / (n + 1)) for i in range(1, n + 1)]
    total = 0.0
    for v in hann:
        total += v
    lc = [-v / total for v in hann]
    lc[c] += 1.0
    out = []
    for b in bands(f0_floor, f0_ceil, channels_in_octave):
        h = matlab_round(fs / b / 2.0)
        m = 4 * h
        w = []
        for i in range(m):
            t = i / (m - 1.0)
            w.append(0.355768 - 0.487396 * math.cos(2.0 * math.pi * t) + 0.144232 * math.cos(4.0 * math.pi * t)
                     - 0.012604 * math.cos(6.0 * math.pi * t))
        out.append((h, np.array(w)))
    return np.array(lc), out


def _row_means(X):
    """sum of each row in the kernel's order: 256 strided partial sums, then a pairwise tree"""
    N, L = X.shape
    P = np.zeros((N, -(-L // 256) * 256))
    P[:, :L] = X
    acc = np.zeros((N, 256))
    for r in range(P.shape[1] // 256):
        acc = acc + P[:, r * 256:(r + 1) * 256]
    s = 128
    while s:
        acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
        s >>= 1
    return acc[:, 0]


def lowcut_signals(X, fs, f0_floor, f0_ceil):
    """DIO's mean and low-cut signal: float64 [N, L] -> (mean [N], yl [N, L + 1 + 2c], yl[:, n + c] the lag n in [-c, L + 1 + c))"""
    N, L = X.shape
    Ly = L + 1
    lc, _ = taps(fs, f0_floor, f0_ceil)
    c = (len(lc) - 1) // 2
    mean = _row_means(X) / Ly
    y = np.zeros((N, Ly))
    y[:, :L] = X
    y = y - mean[:, None]
    # low cut: yl[n] for n in [-c, Ly + c), stored at n + c
    yp = np.zeros((N, Ly + 4 * c))
    yp[:, 2 * c:2 * c + Ly] = y
    yl = np.zeros((N, Ly + 2 * c))
    for j in range(2 * c + 1):                # lag k = j - c: yl[n] += lc[k] * y[n - k]
        k = j - c
        yl = yl + lc[j] * yp[:, c - k:c - k + Ly + 2 * c]
    return mean, yl


def band_signals(yl, L, fs, f0_floor, f0_ceil):
    """the Nuttall low-pass of every band on the low-cut signal -> list per band of [N, L + 1]"""
    N, Ly = yl.shape[0], L + 1
    lc, bl = taps(fs, f0_floor, f0_ceil)
    c = (len(lc) - 1) // 2
    out = []
    for h, w in bl:
        pad = max(0, 2 * h - c)
        ylp = np.zeros((N, Ly + 2 * c + 2 * pad))
        ylp[:, pad:pad + Ly + 2 * c] = yl
        s = np.zeros((N, Ly))
        for j in range(4 * h):                # s[i] += w[j] * yl[i + 2h - j]
            o = 2 * h - j + c + pad
            s = s + w[j] * ylp[:, o:o + Ly]
        out.append(s)
    return out


def filtered_signals(X, fs, f0_floor, f0_ceil):
    """DIO's band signals: float64 [N, L] -> list per band of [N, L + 1]"""
    _, yl = lowcut_signals(X, fs, f0_floor, f0_ceil)
    return band_signals(yl, X.shape[1], fs, f0_floor, f0_ceil)


def _zero_crossing(s, fs):
    """ZeroCrossingEngine: negative-going crossings of s -> (interval locations, intervals)"""
    e = np.nonzero((s[:-1] > 0.0) & (s[1:] <= 0.0))[0] + 1
    if len(e) < 2:
        return np.zeros(0), np.zeros(0)
    fine = e - s[e - 1] / (s[e] - s[e - 1])
    return (fine[:-1] + fine[1:]) / 2.0 / fs, fs / (fine[1:] - fine[:-1])


def _interp1(x, y, xi):
    """WORLD's interp1 (histc indexing: linear extrapolation from the first / last segment)"""
    k = np.clip(np.searchsorted(x, xi, side="right"), 1, len(x) - 1)
    h = x[k] - x[k - 1]
    s = (xi - x[k - 1]) / h
    return y[k - 1] + s * (y[k] - y[k - 1])


def _streams(s, fs, t):
    """the four event streams of a band signal (negative / positive crossings, peaks, dips): per stream the interval count and,
    from two intervals on, interp1 of the intervals at the frame times (None below two: nothing to interpolate)"""
    neg = _zero_crossing(s, fs)
    pos = _zero_crossing(-s, fs)
    d = (-s[:-1]) - (-s[1:])
    peak = _zero_crossing(d, fs)
    dip = _zero_crossing(-d, fs)
    ni = [len(a) for a, _ in (neg, pos, peak, dip)]
    return ni, [_interp1(a, b, t) if len(a) >= 2 else None for a, b in (neg, pos, peak, dip)]


def _candidates(s, fs, boundary, f0_floor, f0_ceil, t, streams=None):
    ni, iv = _streams(s, fs, t) if streams is None else streams
    F = len(t)
    if min(ni) <= 2:
        return np.zeros(F), np.full(F, K_MAX)
    cand = (((iv[0] + iv[1]) + iv[2]) + iv[3]) / 4.0
    dv = [v - cand for v in iv]
    score = np.sqrt((((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]) + dv[3] * dv[3]) / 3.0)
    bad = (cand > boundary) | (cand < boundary / 2.0) | (cand > f0_ceil) | (cand < f0_floor)
    return np.where(bad, 0.0, cand), np.where(bad, K_MAX, score)


def _select_best(cur, past, cands, j, allowed_range):
    ref = (cur * 3.0 - past) / 2.0
    err = abs(ref - cands[0][j])
    best = cands[0][j]
    for c in cands[1:]:
        e = abs(ref - c[j])
        if e < err:
            err, best = e, c[j]
    return 0.0 if abs(1.0 - best / ref) > allowed_range else best


def voice_range(frame_period, f0_floor):
    return int(0.5 + 1000.0 / frame_period / f0_floor) * 2 + 1


def fix_f0_contour(best, cands, frame_period, f0_floor, allowed_range):
    """FixF0Contour's four steps; every frame stays 0 when there are no more frames than the voice range"""
    return fix_f0_contour_steps(best, cands, frame_period, f0_floor, allowed_range)[2]


def fix_f0_contour_steps(best, cands, frame_period, f0_floor, allowed_range):
    """(step 1, step 2, steps 3-4) of FixF0Contour; (None, None, zeros) when there are no more frames than the voice range"""
    F = len(best)
    vr = voice_range(frame_period, f0_floor)
    if F <= vr:
        return None, None, np.zeros(F)
    base = best.copy()
    base[:vr] = 0.0
    base[F - vr:] = 0.0
    s1 = np.zeros(F)
    for i in range(vr, F):
        s1[i] = base[i] if abs((base[i] - base[i - 1]) / (K_SAFE + base[i])) < allowed_range else 0.0
    s2 = s1.copy()
    ctr = (vr - 1) // 2
    for i in range(ctr, F - ctr):
        if np.any(s1[i - ctr:i + ctr + 1] == 0):
            s2[i] = 0.0
    pos_idx, neg_idx = [], []
    for i in range(1, F):
        if s2[i] == 0 and s2[i - 1] != 0:
            neg_idx.append(i - 1)
        elif s2[i - 1] == 0 and s2[i] != 0:
            pos_idx.append(i)
    s3 = s2.copy()
    for n, j0 in enumerate(neg_idx):
        limit = F - 1 if n == len(neg_idx) - 1 else neg_idx[n + 1]
        for j in range(j0, limit):
            s3[j + 1] = _select_best(s3[j], s3[j - 1], cands, j + 1, allowed_range)
            if s3[j + 1] == 0:
                break
    s4 = s3.copy()
    for n in range(len(pos_idx) - 1, -1, -1):
        limit = 1 if n == 0 else pos_idx[n - 1]
        for j in range(pos_idx[n], limit, -1):
            s4[j - 1] = _select_best(s4[j], s4[j + 1], cands, j - 1, allowed_range)
            if s4[j - 1] == 0:
                break
    return s1, s2, s4


def dio_stages(X, fs, f0_floor=20.0, f0_ceil=4096.0, frame_period=5.0, allowed_range=0.1):
    """DIO on every row of X (float64 [N, L]) with what each stage of csrc/world_f0.hip leaves behind: a dict per row of
         mean, yl [L + 1 + 2c]           the row's mean and its low-cut signal at every lag (stages 1, 2)
         ni [bands][4], iv [bands][4]    per band and stream the interval count and the F interp1 values (None where ni < 2) (stage 3)
         cand [bands][F]                 the band's candidate, 0 where refused (stage 4)
         best, s1, s2 [F]                the best band and FixF0Contour's steps 1 and 2 (s1, s2 None when F <= the voice range)
         f0 [F]                          the contour after steps 3-4"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    N, L = X.shape
    F = n_frames(L, fs, frame_period)
    t = np.arange(F) * frame_period / 1000.0
    bnd = bands(f0_floor, f0_ceil)
    mean, yl = lowcut_signals(X, fs, f0_floor, f0_ceil)
    sig = band_signals(yl, L, fs, f0_floor, f0_ceil)
    rows = []
    for r in range(N):
        cands, scores, nis, ivs = [], [], [], []
        for b, s in zip(bnd, sig):
            ni, iv = _streams(s[r], float(fs), t)
            c, sc = _candidates(s[r], float(fs), b, f0_floor, f0_ceil, t, (ni, iv))
            nis.append(ni)
            ivs.append(iv)
            cands.append(c)
            scores.append(sc / (c + K_SAFE))
        best = cands[0].copy()
        low = scores[0].copy()
        for c, sc in zip(cands[1:], scores[1:]):
            better = low > sc
            low = np.where(better, sc, low)
            best = np.where(better, c, best)
        s1, s2, f0 = fix_f0_contour_steps(best, cands, frame_period, f0_floor, allowed_range)
        rows.append(dict(mean=mean[r], yl=yl[r], ni=np.array(nis, dtype=np.int64), iv=ivs, cand=np.stack(cands), best=best, s1=s1,
                         s2=s2, f0=f0))
    return rows, t


def dio_rows(X, fs, f0_floor=20.0, f0_ceil=4096.0, frame_period=5.0, allowed_range=0.1):
    """pyworld.dio on every row of X (float64 [N, L]) -> (f0 [N, F], t [F])"""
    rows, t = dio_stages(X, fs, f0_floor, f0_ceil, frame_period, allowed_range)
    return np.stack([row["f0"] for row in rows]), t


def dio(x, fs, f0_floor=50.0, f0_ceil=800.0, frame_period=5.0, allowed_range=0.1):
    f0, t = dio_rows(np.asarray(x, dtype=np.float64)[None], fs, f0_floor, f0_ceil, frame_period, allowed_range)
    return f0[0], t


def _dft_bins(v, n, bins):
    k = np.asarray(bins, dtype=np.int64)[:, None] % n
    m = (k * np.arange(len(v))[None, :]) % n
    ang = 2.0 * np.pi * m / n
    return (v[None, :] * np.cos(ang)).sum(1), -(v[None, :] * np.sin(ang)).sum(1)


def _fix_f0(seg_main, seg_diff, n, fs, f0, harmonics):
    idx = [matlab_round(f0 * n / fs * (i + 1)) for i in range(harmonics)]
    mr, mi = _dft_bins(seg_main, n, idx)
    dr, di = _dft_bins(seg_diff, n, idx)
    num_i = mr * di - mi * dr
    pw = mr * mr + mi * mi
    num = den = 0.0
    for i in range(harmonics):
        inst = 0.0 if pw[i] == 0.0 else idx[i] * fs / n + num_i[i] / pw[i] * fs / 2.0 / math.pi
        amp = math.sqrt(pw[i])
        num += amp * inst
        den += amp * (i + 1)
    return num / den if den != 0.0 else 0.0       # a window without energy (WORLD divides 0 by 0 here): no refinement


def _refined(x, fs, t, f0, margins=None):
    """StoneMask of one frame; `margins` (a list) collects the relative margin of every decision taken on a computed value"""
    if f0 <= K_FLOOR_STONEMASK or f0 > fs / 12.0:
        return 0.0
    hw = 3.0 / f0 / 2.0
    r = matlab_round(hw * fs)
    m = r * 2 + 1
    wl = (r * 2 + 1) / fs
    n = int(2.0 ** (2.0 + int(math.log(hw * fs + K_SAFE) / LOG2)))
    base0 = (-r + 0) / fs
    bi = matlab_round((t + base0) * fs + 0.001) + np.arange(m)
    tmp = (bi - 1.0) / fs - t
    win = 0.42 + 0.5 * np.cos(2.0 * math.pi * tmp / wl) + 0.08 * np.cos(4.0 * math.pi * tmp / wl)
    dwin = np.empty(m)
    dwin[0] = -win[1] / 2.0
    dwin[1:-1] = -(win[2:] - win[:-2]) / 2.0
    dwin[-1] = win[-2] / 2.0
    seg = x[np.clip(bi - 1, 0, len(x) - 1)]
    main, diff = seg * win, seg * dwin
    tent = _fix_f0(main, diff, n, fs, f0, 2)
    if margins is not None:
        margins += [abs(tent) / f0, abs(tent - f0 * 2) / (f0 * 2)]
    if tent <= 0.0 or tent > f0 * 2:
        tent = 0.0
    else:
        if margins is not None:
            for i in range(6):
                v = tent * n / fs * (i + 1)
                margins.append(abs(v - (math.floor(v) + 0.5)) / v)
        tent = _fix_f0(main, diff, n, fs, tent, 6)
    if margins is not None:
        margins.append(abs(abs(tent - f0) - f0 * 0.2) / f0)
    return f0 if abs(tent - f0) > f0 * 0.2 else tent


def stonemask_margin(x, fs, t, f0):
    """How far StoneMask's frame at time t with DIO's f0 is from taking another branch on a value it computes, as the smallest
    relative margin of: tent <= 0 (|tent| / f0); tent > 2 f0; each of the second pass's six bins f0 n / fs (i + 1) from a
    half-integer (relative to the bin); |tent - f0| against 0.2 f0 (relative to f0).  inf for a frame the f0 gates leave unvoiced:
    those are taken on DIO's f0 itself.  An implementation whose computed values agree to well below the margin takes the same
    branches."""
    margins = []
    _refined(np.asarray(x, dtype=np.float64), float(fs), t, f0, margins)
    return min(margins) if margins else math.inf


def stonemask(x, f0, t, fs):
    x = np.asarray(x, dtype=np.float64)
    return np.array([_refined(x, float(fs), t[i], f0[i]) for i in range(len(f0))])


def dio_stonemask_rows(X, fs=8000, f0_floor=20.0, f0_ceil=4096.0, frame_period=5.0):
    """float32 [N, L] -> float32 [N, F]: what alive_world_f0 returns"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float32)).astype(np.float64)
    f0, t = dio_rows(X, fs, f0_floor, f0_ceil, frame_period)
    return np.stack([stonemask(X[r], f0[r], t, fs) for r in range(X.shape[0])]).astype(np.float32)
