"""Cases and expected bits of the exact tests of the fp32 glue kernels: dw conv + norm and channel norm (csrc/blocks.hip), argmax over
channels (blocks.hip, the act = 3 epilogue of csrc/gemm_planes.hip), the waveform edges of the Filter (csrc/filter_edge.hip), the
resampler (csrc/audio.hip), the pitch transform and gelu + FiLM in a frame range (blocks.hip).  NumPy and torch on the CPU only; the
library is not imported here.  tests/test_host_glue_cases.py proves on the CPU what the builders promise, tests/test_gpu_glue_exact.py
runs the cases on the device and asserts bit equality.

The pattern is tests/conv_cases.py's: operands on which every intermediate value is an fp32 number, so that the expected bits do not
depend on the order of a sum, on which thread owns which channel, or on whether a multiply and an add are contracted.

A. norm columns.  x, the taps w[c][7] and the biases are small integers (|x| <= 8, |w| <= 3, neighbouring taps of a channel differ,
   |b| <= 4).  One BALANCING channel (C // 2) has the taps (0, 0, 0, 1, 0, 0, 0): its x gets, per column, the residue that makes the
   column sum of y = dw(x) a multiple of C.  Mean, y - mean and the centred sum of squares are then integers below 2^24, exact in any
   order, and what is left is a chain of single correctly rounded fp32 operations on known inputs: ss / (C - 1), sqrtf, + eps,
   d / sigma, and v * g + o with g a signed power of two (v * g is exact: one rounding with or without contraction).  channel_norm
   takes y itself as its input.
B. argmax columns: a background of distinct values in (-1, 1), or one fill value, and planted channels.  Expected: torch.argmax.
C. filter edges: integers times a power of two, both fused convolutions exact; expected = the float64 F.conv1d chain.
D. resampler: impulses (every output is 0 or one entry of the bank), and a synthetic integer bank with integer x.
E. pitch rows: f0 in 440 * 2^j, shifts multiples of 12, so that every log2 / exp2 argument is an integer power.
F. gelu + FiLM: the columns of a frame range whose two interpolation frames lie inside the range."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
BUDGET = 1 << 24


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- A. dw conv + norm, channel norm ------------------------------------------------------------------------------------------------
NORM_N = 2
NORM_EPS = (1e-4, 1e-3)
NORM_T_SMALL = (1, 2, 3, 4, 7, 31, 32)            # one block per frame (T <= 32); T <= 3 clips every tap set on both sides
NORM_T_TILED = (33, 36, 63, 64, 65, 130)          # 64 columns per block: first T above the switch, a full tile, +1, a ragged third tile
NORM_C = (2, 3, 5, 40, 255, 256, 257, 512, 641)


def _pairs(ts):
    return [(NORM_C[(2 * i + k) % len(NORM_C)], t) for i, t in enumerate(ts) for k in (0, 1)]


NORM_SHAPES = _pairs(NORM_T_SMALL) + _pairs(NORM_T_TILED)       # every C on either side of the switch, every T at two values of C
PLANE_SHAPES = [(64, 5), (64, 65), (256, 33), (256, 130), (512, 7), (512, 70)]
SCALE_ROW = 3                                      # the adaptive form: scale rows [3, 3 + C), shift rows [C + 5, 2 C + 5) of 2 C + 7


def dw_int(x, w, b):
    """depthwise k7, zero pad 3, in int64: y[n][c][t] = b[c] + sum_j w[c][j] x[n][c][t + j - 3]"""
    n, c, t = x.shape
    xp = np.zeros((n, c, t + 6), np.int64)
    xp[:, :, 3:3 + t] = x
    y = np.broadcast_to(b[None, :, None], (n, c, t)).copy()
    for j in range(7):
        y += w[None, :, j, None] * xp[:, :, j:j + t]
    return y


def norm_case(c, t, n=NORM_N):
    """integer operands of one shape: x [n][c][t], w [c][7], b [c] (int64), y = dw(x) with column sums divisible by c; gain / offset [c]
    and cond [n][2 c + 7][t] (float32): gains signed powers of two, offsets multiples of 1/8"""
    r = _rng("norm", c, t)
    x = r.integers(-8, 9, (n, c, t))
    w = np.empty((c, 7), np.int64)
    w[:, 0] = r.integers(-3, 4, c)
    for j in range(1, 7):                                            # neighbouring taps differ: a shifted tap changes y
        w[:, j] = (w[:, j - 1] + 3 + r.integers(1, 7, c)) % 7 - 3
    b = r.integers(-4, 5, c)
    cb = c // 2
    w[cb] = (0, 0, 0, 1, 0, 0, 0)
    s = dw_int(x, w, b).sum(1)
    res = -((s + c // 2) % c - c // 2)                               # in (-c / 2, c / 2]
    x[:, cb, :] += res
    y = dw_int(x, w, b)
    pw = lambda shape: (F32(2.0) ** r.integers(-2, 3, shape) * r.choice([-1.0, 1.0], shape)).astype(F32)
    dy = lambda shape: (r.integers(-16, 17, shape) / 8.0).astype(F32)
    rows = 2 * c + 7
    cond = np.full((n, rows, t), 7.0, F32)                          # a row read from the wrong place is 7
    cond[:, SCALE_ROW:SCALE_ROW + c] = pw((n, c, t))
    cond[:, c + 5:2 * c + 5] = dy((n, c, t))
    return dict(c=c, t=t, n=n, x=x, w=w, b=b, y=y, cb=cb, gain=pw(c), offset=dy(c), cond=cond, rows=rows, scale_row=SCALE_ROW,
                shift_row=c + 5)


def norm_stats(y):
    """integer mean [n][1][t] and centred sum of squares of the columns of y (int64)"""
    c = y.shape[1]
    s = y.sum(1, keepdims=True)
    assert not (s % c).any()
    mean = s // c
    return mean, ((y - mean) ** 2).sum(1, keepdims=True)


def norm_expected(case, eps, adaptive):
    """the bits the kernels must give, from the integer column statistics by single fp32 operations"""
    y, c = case["y"], case["c"]
    mean, ss = norm_stats(y)
    var = ss.astype(F32) / F32(c - 1)
    sigma = np.sqrt(var) + F32(eps)
    v = (y - mean).astype(F32) / sigma
    if adaptive:
        g, o = case["cond"][:, case["scale_row"]:case["scale_row"] + c], case["cond"][:, case["shift_row"]:case["shift_row"] + c]
    else:
        g, o = case["gain"][None, :, None], case["offset"][None, :, None]
    out = v * g + o
    assert out.dtype == F32
    return out


def bf16_split3_lossless(v):
    """True where three bf16 planes (round to nearest, then the remainder, twice) add up to the fp32 value exactly"""
    v = torch.as_tensor(v, dtype=torch.float32)
    h0 = v.bfloat16().float()
    r1 = v - h0
    h1 = r1.bfloat16().float()
    r2 = r1 - h1
    h2 = r2.bfloat16().float()
    return ((h0 + h1) + h2) == v


# ---- B. argmax ----------------------------------------------------------------------------------------------------------------------
ARGMAX_C = (1, 3, 255, 256, 257, 4096)
ARGMAX_T = (8, 77)                                 # one block per frame (T <= 32) / 64 columns per block, channels over four waves
GEMM_ARGMAX_CO = (100, 4096)
BIG = 4096.0
NAN, INF = float("nan"), float("inf")
# (higher, lower) channel pairs for ties and for two NaNs; the lower index is owned by what is merged later:
#   (8, 1), (300, 9): wave c % 4 of the tiled kernel (waves are merged 0, 1, 2, 3), and different threads of the per-frame kernel's tree;
#   (8, 4): the two half-waves of a column in the GEMM epilogue (rows 8 g + 4 h + e: row 8 is half 0, which receives; row 4 is half 1);
#   (70, 5): two 64-row blocks of alive_argmax_merge
PAIRS = ((8, 1), (300, 9), (8, 4), (70, 5))


def argmax_patterns(c):
    """[(name, fill or None (= the background), [(channel, value), ...])]"""
    pats = [("max at 0", None, [(0, BIG)]), ("max at C - 1", None, [(c - 1, BIG)]), ("all equal", 1.5, []),
            ("one NaN", None, [(c // 2, NAN)]), ("all -inf", -INF, []), ("-inf but the last", -INF, [(c - 1, -3.0)]),
            ("-inf but the first", -INF, [(0, -3.0)])]
    for hi, lo in PAIRS + ((c - 1, 2),):
        if lo < hi < c:
            pats += [(f"tie {hi} {lo}", None, [(hi, BIG), (lo, BIG)]), (f"NaNs {hi} {lo}", None, [(hi, NAN), (lo, NAN)])]
    if c >= 3:
        pats += [("NaN below +inf", None, [(c // 3, NAN), (c - 1, INF)]), ("+inf below NaN", None, [(0, INF), (c - 2, NAN)])]
    return pats


def argmax_case(c, t):
    """X [n][c][t] float32 whose column n t + tt carries pattern (n t + tt) % len(patterns), and torch.argmax of it as float [n][1][t]"""
    pats = argmax_patterns(c)
    n = max(2, -(-len(pats) // t))
    r = _rng("argmax", c, t)
    x = np.empty((n, c, t), F32)
    for q in range(n * t):
        name, fill, plants = pats[q % len(pats)]
        col = (r.permutation(c).astype(F32) + F32(0.5)) / F32(c) * F32(2.0) - F32(1.0) if fill is None else np.full(c, fill, F32)
        for ch, v in plants:
            col[ch] = v
        x[q // t, :, q % t] = col
    xt = torch.from_numpy(x)
    return xt, torch.argmax(xt, dim=1, keepdim=True).float(), pats


def first_max(col):
    """the rule in plain Python: a NaN is the maximum; the first of equal candidates wins"""
    best, besti = None, -1
    for i, v in enumerate(col):
        v = float(v)
        if best is None or (v != v and best == best) or (best == best and v > best):
            best, besti = v, i
    return besti


def gemm_argmax_cases(co, ci=32, cols=5):
    """one GEMM per pattern: w [co][ci][1], x [1][ci][cols] small integers (exact in three bf16 planes, |w x| < 300 < BIG), bias [co].
    A filled pattern has zero weights and the fill as bias; a planted row has a zero weight row and its value as bias (a NaN or an inf
    cannot travel through the planes).  Expected: torch.argmax of w x + bias."""
    out = []
    for name, fill, plants in argmax_patterns(co):
        r = _rng("gemm argmax", co, name)
        w = r.integers(-3, 4, (co, ci)).astype(F32)
        x = r.integers(-3, 4, (1, ci, cols)).astype(F32)
        b = r.integers(-8, 9, co).astype(F32) / F32(4.0)
        if fill is not None:
            w[:] = 0.0
            b[:] = fill
        for ch, v in plants:
            w[ch] = 0.0
            b[ch] = v
        y = torch.from_numpy(w).double() @ torch.from_numpy(x).double()[0] + torch.from_numpy(b).double()[:, None]
        want = torch.argmax(y.float(), dim=0).float().view(1, 1, cols)
        out.append((name, torch.from_numpy(w).view(co, ci, 1), torch.from_numpy(x), torch.from_numpy(b), want, y))
    return out


# ---- C. filter edges ----------------------------------------------------------------------------------------------------------------
SOURCE_IN_LW = (2, 4, 6, 8, 510, 512, 514, 1026)   # Lh = Lw / 2 around the 256-thread block, windows shorter than the 8-sample footprint
SOURCE_OUT_LW = (1, 2, 3, 6, 7, 255, 256, 257, 513)
EDGE_N = 3


def source_in_case(lw, n=EDGE_N):
    """src in 2^-4, w_in in 2^-3, b_in in 2^-7 (x0 is a multiple of 2^-7), w_d in 2^-3, b_d in 2^-10 (d0 a multiple of 2^-10)"""
    r = _rng("source_in", lw)
    t = lambda a, k: torch.from_numpy(a.astype(np.float64) * 2.0 ** -k)
    src, w_in, b_in = t(r.integers(-15, 16, (n, 1, lw)), 4), t(r.integers(-7, 8, (8, 1, 7)), 3), t(r.integers(-64, 65, 8), 7)
    w_d, b_d = t(r.integers(-7, 8, (16, 8, 2)), 3), t(r.integers(-512, 513, 16), 10)
    x0 = F.conv1d(src, w_in, b_in, padding=3)
    ref = F.conv1d(x0, w_d, b_d, stride=2)
    bound0 = F.conv1d(src.abs(), w_in.abs(), b_in.abs(), padding=3)
    bound = F.conv1d(bound0, w_d.abs(), b_d.abs(), stride=2)            # sum of |terms|: bounds every partial sum in any order
    return dict(src=src, w_in=w_in, b_in=b_in, w_d=w_d, b_d=b_d, x0=x0, ref=ref, units0=bound0.max().item() * 2.0 ** 7,
                units=bound.max().item() * 2.0 ** 10)


def source_out_case(lw, n=EDGE_N):
    """h in 2^-5, w in 2^-4, b in 2^-9: the sum is a multiple of 2^-9"""
    r = _rng("source_out", lw)
    t = lambda a, k: torch.from_numpy(a.astype(np.float64) * 2.0 ** -k)
    h, w, b = t(r.integers(-63, 64, (n, 8, lw)), 5), t(r.integers(-15, 16, (1, 8, 7)), 4), t(r.integers(-256, 257, 1), 9)
    ref = F.conv1d(h, w, b, padding=3)
    bound = F.conv1d(h.abs(), w.abs(), b.abs(), padding=3)
    return dict(h=h, w=w, b=b, ref=ref, units=bound.max().item() * 2.0 ** 9)


# ---- D. resampler -------------------------------------------------------------------------------------------------------------------
RESAMPLE_PAIRS = ((3, 2), (2, 3), (3, 1), (441, 160), (160, 441))
DENSE_PAIRS = ((3, 2, 13), (3, 2, 700), (441, 160, 4 * 441 + 17))
LOWPASS_WIDTH, ROLLOFF = 6, 0.99
LDS_BANK_BYTES = 16 * 1024                         # a larger bank stays in global memory


def resample_width(orig, new):
    return math.ceil(LOWPASS_WIDTH * orig / (min(orig, new) * ROLLOFF))


def resample_taps(orig, new):
    return 2 * resample_width(orig, new) + orig


def resample_length(length, orig, new):
    return -(-new * length // orig)


def bank_is_lds_staged(orig, new):
    return new * resample_taps(orig, new) * 4 <= LDS_BANK_BYTES


def resample_bank64(orig, new):
    """the windowed-sinc bank [new][taps] in float64, in the operation order of the kernel's comment and code"""
    width, taps = resample_width(orig, new), resample_taps(orig, new)
    p, j = np.arange(new, dtype=np.float64)[:, None], np.arange(taps, dtype=np.float64)[None, :]
    base = float(min(orig, new)) * ROLLOFF
    t = (-p / float(new) + (j - width) / float(orig)) * base
    t = np.clip(t, -float(LOWPASS_WIDTH), float(LOWPASS_WIDTH))
    cw = np.cos(t * math.pi / float(LOWPASS_WIDTH) / 2.0)
    window = cw * cw
    t = t * math.pi
    scale = base / float(orig)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 1.0, np.sin(t) / t)
    return s * window * scale


def bank_sensitive(b64, ulps=8):
    """taps whose fp32 rounding changes when the float64 value moves by `ulps` float64 ulps either way"""
    d = ulps * np.spacing(np.abs(b64))
    return ((b64 - d).astype(F32) != b64.astype(F32)) | ((b64 + d).astype(F32) != b64.astype(F32))


def impulse_case(orig, new):
    """two rows of impulses of height 2^-1, further apart than the tap count: row 0 at 1, e + 1, L - 1, row 1 at 0, e, L - 2, where e is
    the input sample under an output block edge (index 256 k - 1 / 256 k).  new L % orig != 0: the last output reads past the row's end
    (and, for row 0, would find row 1's impulse at sample 0 there).  idx(Lout) [2][Lout]: the bank entry p taps + j behind every output
    sample, -1 where no impulse lies under its taps: y = 0.5 * (2 * 0.5) * bank entry, or 0."""
    width, taps = resample_width(orig, new), resample_taps(orig, new)
    k = 1
    while ((256 * k - 1) * orig) // new <= taps + 1:
        k += 1
    e = ((256 * k - 1) * orig) // new
    length = e + 1 + taps + 40
    while (new * length) % orig == 0 or resample_length(length, orig, new) <= 256 * k + new:
        length += 1
    pos = [[1, e + 1, length - 1], [0, e, length - 2]]
    x = np.zeros((2, length), F32)
    for b in range(2):
        assert min(np.diff(pos[b])) > taps
        x[b, pos[b]] = 0.5
    full = resample_length(length, orig, new)

    def idx(lout):
        o = np.arange(lout)
        m, p = o // new, o % new
        out = np.full((2, lout), -1, np.int64)
        for b in range(2):
            for s in pos[b]:
                j = s - (m * orig - width)
                hit = (j >= 0) & (j < taps)
                assert (out[b][hit] == -1).all()
                out[b][hit] = (p * taps + j)[hit]
        return out
    return dict(x=x, L=length, full=full, pos=pos, idx=idx, edge=256 * k, louts=(full, full - 1, full - new))


def dense_case(orig, new, length):
    """a synthetic bank of integers (|f| <= 15) times 2^-8, integer x (|x| <= 7, two rows, row 1 starts with a non-zero sample), pre 2,
    post 1/4: y[b][m new + p] = post * sum_j filt[p][j] (pre xpad[b][m orig + j]) in float64, exact in fp32"""
    width, taps = resample_width(orig, new), resample_taps(orig, new)
    r = _rng("dense", orig, new, length)
    filt = r.integers(-15, 16, (new, taps)).astype(np.float64) / 256.0
    x = r.integers(-7, 8, (2, length)).astype(np.float64)
    x[1, 0] = 5.0
    pre, post = 2.0, 0.25
    full = resample_length(length, orig, new)
    xpad = np.zeros((2, (full // new + 2) * orig + taps))
    xpad[:, width:width + length] = x * pre
    y = np.empty((2, full))
    for o in range(full):
        m, p = divmod(o, new)
        y[:, o] = post * (xpad[:, m * orig:m * orig + taps] @ filt[p])
    units = (np.abs(filt).max() * 256.0) * taps * np.abs(x * pre).max()
    return dict(filt=filt, x=x, pre=pre, post=post, y=y, full=full, L=length, units=units)


# ---- E. pitch transform -------------------------------------------------------------------------------------------------------------
PITCH_T = (1, 255, 256, 257, 450)
PITCH_PARAMS = ((1.0, 0.0, 1.0), (0.5, 12.0, 0.5), (2.0, -12.0, 2.0), (4.0, 24.0, 0.5), (1.0, -24.0, 2.0))    # f0_rate, shift, intonation
PITCH_KINDS = ("dense", "none", "one", "last stride")


def pitch_row(kind, t):
    """j [t] int with None-like -99 for an unvoiced frame: f0 = 440 * 2^j.  The voiced j are mbar - 2, mbar, mbar + 2 with mbar = -1 and
    as many of the first as of the last: their mean is mbar, and every deviation is even (an intonation of 1/2 keeps it an integer)."""
    j = np.full(t, -99)
    if kind == "dense":
        voiced = [i for i in range(t) if i % 5 != 3 or t == 1]
        s = [(1, -1, 0, 0)[i % 4] for i in range(len(voiced))]
        if sum(s) != 0:
            s[max(i for i, v in enumerate(s) if v == 1)] = 0
        j[voiced] = -1 + 2 * np.array(s)
    elif kind == "one":
        j[t // 2] = 1
    elif kind == "last stride":
        first = (t - 1) // 256 * 256
        j[first:] = pitch_row("dense", t - first)
    return j


def pitch_case(kind, t, mode, params):
    """f0 row (float32) and the expected row, computed in float64 (every step is exact)"""
    rate, shift, inton = params
    j = pitch_row(kind, t)
    voiced = j != -99
    f0 = np.where(voiced, 440.0 * 2.0 ** np.where(voiced, j, 0), 0.0)
    y = np.zeros(t)
    if voiced.any():
        p = 12.0 * j[voiced] - 9.0
        if mode == 0:
            mean = p.mean()
            e = (mean + (p - mean) * inton + shift + 9.0) / 12.0
            y[voiced] = 440.0 * 2.0 ** e * rate
        else:
            e = (12.0 * np.log2(f0[voiced] * rate / 440.0) - 9.0 + shift + 9.0) / 12.0
            y[voiced] = 440.0 * 2.0 ** e
        assert (e == np.round(e)).all() and (mode == 1 or mean == round(mean))
    return f0.astype(F32), y.astype(F32), y


# ---- F. gelu + FiLM in a frame range ------------------------------------------------------------------------------------------------
FILM_FRAMES = 16                                   # the window's frames
# the ranges [first, end): frames 3 .. 10, and ten frames from frame 3 on.  The first and the last half frame of a range interpolate
# from a frame outside it, so 7 / 8 resp. 9 / 10 of a range's samples have both frames inside
FILM_RANGES = ((3, 11), (3, 13))
FILM_SHAPES = ((256, 10), (64, 80))                # C, samples per frame: the decoder's 256-channel scale and its 64-channel scale
FILM_OFF = 3                                       # scale rows [3, 3 + C), shift rows [3 + C, 3 + 2 C) of 2 C + 7 (networks.hip: film_off, + C)


def lerp_frames(i, ratio, in_len):
    """common.h lerp_coord: the two frames of sample i.  src = fmaf(ratio, i + 0.5, -0.5): the product and the sum are exact in float64,
    so one rounding to fp32 is the fma"""
    src = F32(np.float64(F32(ratio)) * (np.float64(i) + 0.5) - 0.5)
    src = F32(0.0) if src < 0 else src
    i0 = min(int(src), in_len - 1)
    return i0, i0 + (1 if i0 < in_len - 1 else 0)


def film_range_columns(spf, rng, frames=FILM_FRAMES):
    """mask over the samples of the range: both interpolation frames lie inside the range's film columns"""
    f_lo, f_hi = rng
    length = frames * spf
    ratio = F32(frames) / F32(length)
    assert ratio == F32(f_hi - f_lo) / F32((f_hi - f_lo) * spf)         # the ranged call derives the same ratio
    ok = []
    for t in range(f_lo * spf, f_hi * spf):
        i0, i1 = lerp_frames(t, ratio, frames)
        ok.append(f_lo <= i0 and i1 <= f_hi - 1)
    return np.array(ok)


def film_case(c, spf, n=2):
    r = _rng("film", c, spf)
    length = FILM_FRAMES * spf
    h = torch.from_numpy(r.standard_normal((n, c, length)).astype(F32))
    film = torch.from_numpy(r.standard_normal((n, 2 * c + 7, FILM_FRAMES)).astype(F32))
    return h, film
