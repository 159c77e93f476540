"""The output limiter on the device (csrc/limit.hip) and through the converters and CLIs, against the NumPy restatement
tools/limit_ref.py.  Every comparison is bitwise, or equality of int16 streams.

1. alive_limit_rows alone: fifteen rows in one call, three ticks with the history carried (a filling row, an off row, L = 1 with H = 0,
   L = 2, L = 255 / 256 / 257, P equal to ld_hist, a span shorter and one longer than P, the 441 / 440 geometry, a row that never
   exceeds its ceiling, a row with a NaN and both infinities, a row whose regions do not fit, a span of more than one tile); y, hist
   and gmin between guard bands.
2. alive_limit_waves: lengths 0, 1, tile - 1, tile, tile + 1 and 3 tile + 7 in one call, peaks on and beside the tile borders and within
   L of both ends; alive_limit_rows tick by tick over windows of one signal is bitwise alive_limit_waves over the whole signal.
3. MultiStreamConverter(limiter=True): no session limiting -> bitwise the plain converter; a limiting session with crossfade and gate
   on through a silence -> every chunk is the restatement applied to the waves of a twin without a limiter, where the twin's int16
   wraps; enable_graph in the middle, retuning and on / off without re-capture; the bf16 repeat.
4. RealtimeConverter(limit_db=): bitwise a one-slot MultiStreamConverter, with and without interior reuse.
5. multistream_inference.py, inference.py -lim and batch_inference.py with a "limit_db" job."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import limit_ref as LR                                               # noqa: E402
from module import audio_io, synthetic                               # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 16                                                             # guard band, elements on each side of every output
TILE = MS.LIMIT_TILE


def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _pcm(n, seed, scale=12000):
    return (synthetic.make_waveform(n, seed)[0].numpy() * scale).astype(np.int16)


class Guarded:
    """a device array between two guard bands filled with a sentinel"""

    def __init__(self, shape, dtype, sentinel, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(*shape)
        self.sentinel = sentinel
        if init is not None:
            self.view.copy_(torch.as_tensor(np.asarray(init), dtype=dtype).view(*shape))

    def intact(self):
        s = torch.full((PAD,), self.sentinel, dtype=self.buf.dtype, device=DEV)
        return torch.equal(self.buf[:PAD], s) and torch.equal(self.buf[-PAD:], s)


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _bits_equal(a, b):
    """bit for bit (the sign of zero included), except that a NaN matches any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan]))


def _peaky(shape, seed, level=0.3, peaks=25, height=4.0):
    """noise under the ceilings with a few samples far above them, per row"""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(shape) * level).astype(np.float32)
    for r in range(shape[0]):
        at = rng.choice(shape[1], peaks, replace=False)
        y[r, at] = (rng.uniform(1.0, height, peaks) * rng.choice([-1.0, 1.0], peaks)).astype(np.float32)
    return y


# ---------------------------------------------------------------------------------------------------- 1. alive_limit_rows alone
LD, R_HIST = 2003, 300                                              # (a stride that is no multiple of 256)
#        filling off   L=1   L=2   255   256   257   P=hist S<P   S>P   441/440 quiet nonfinite nofit 2 tiles
R_LO = [100,    100,  100,  107,  50,   51,   52,   60,    300,  90,   400,    100,  100,      1765, 20]
R_SPAN = [160,  160,  160,  161,  300,  300,  300,  250,   64,   700,  440,    160,  200,      160,  1100]
R_SHIFT = [160, 160,  160,  162,  300,  300,  300,  250,   64,   700,  441,    160,  200,      160,  1100]
R_LOOK = [80,   0,    1,    2,    255,  256,  257,  101,   50,   30,   220,    80,   16,       80,   100]
R_HOLD = [160,  160,  0,    5,    0,    44,   10,   200,   150,  40,   80,     160,  10,       160,  100]
R_CEIL = [0.9,  0.9,  0.9,  0.5,  0.9,  0.8,  0.7,  0.9,   0.6,  0.9,  0.89,   0.9,  0.9,      0.9,  32767 / 32768]
R_EMIT = [0] + [1] * 14
QUIET, NONFINITE, NOFIT = 11, 12, 13
ROWS = len(R_LO)


def _rows_wave(tick):
    y = _peaky((ROWS, LD), 100 + tick)
    for r in range(ROWS):
        y[r, R_LO[r] + R_SPAN[r] // 2] = 2.5                         # every span has something to limit
    y[QUIET] = np.clip(y[QUIET], -0.9, 0.9)
    y[QUIET, 130], y[QUIET, 131] = 0.9, -0.9                         # exactly the ceiling: still untouched
    if tick == 1:
        y[NONFINITE, 150], y[NONFINITE, 200], y[NONFINITE, 260] = np.nan, np.inf, -np.inf
    return y


def test_limit_rows_against_the_restatement_over_three_ticks():
    assert R_LO[NOFIT] + R_SHIFT[NOFIT] + R_LOOK[NOFIT] - 1 == LD + 1 and R_LOOK[7] - 1 + R_HOLD[7] == R_HIST
    assert R_SPAN[14] > TILE and R_SPAN[8] < R_LOOK[8] - 1 + R_HOLD[8] and R_SPAN[9] > R_LOOK[9] - 1 + R_HOLD[9]
    i32 = torch.int32
    args = [_dev(a, i32) for a in (R_LO, R_SPAN, R_SHIFT, R_LOOK, R_HOLD)] + [_dev(R_CEIL, torch.float32), _dev(R_EMIT, torch.uint8)]
    hist = Guarded((ROWS, R_HIST), torch.float32, -9.0, np.ones((ROWS, R_HIST), np.float32))
    gmin = Guarded((ROWS,), torch.float32, -5.0, np.full(ROWS, 7.0, np.float32))
    ref_hist = np.ones((ROWS, R_HIST), np.float32)
    for tick in range(3):
        wave = _rows_wave(tick)
        y = Guarded((ROWS, LD), torch.float32, 123.0, wave)
        MS.limit_rows_(y.view, *args, hist.view, gmin.view)
        torch.cuda.synchronize()
        assert y.intact() and hist.intact() and gmin.intact()
        want_y, ref_hist, want_g = LR.limit_rows(wave, R_LO, R_SPAN, R_SHIFT, R_LOOK, R_HOLD, R_CEIL, R_EMIT, ref_hist)
        got_y, got_h, got_g = y.view.cpu().numpy(), hist.view.cpu().numpy(), gmin.view.cpu().numpy()
        for r in range(ROWS):
            assert _bits_equal(got_y[r], want_y[r]), (tick, r)
            assert _bits_equal(got_h[r], ref_hist[r]), (tick, r)
            assert got_g[r] == (7.0 if np.isnan(want_g[r]) else want_g[r]), (tick, r)
        # the rows that must not move, the bound on the rest, and nothing written outside the span
        for r in (0, 1, NOFIT, QUIET):
            assert _bits_equal(got_y[r], wave[r]), (tick, r)
        assert np.all(got_h[0] == 1.0) and np.all(got_h[1] == 1.0) and np.all(got_h[NOFIT] == 1.0) and np.all(got_h[QUIET] == 1.0)
        assert got_g[0] == 7.0 and got_g[1] == 1.0 and got_g[NOFIT] == 1.0 and got_g[QUIET] == 1.0
        for r in range(2, ROWS):
            if r in (NOFIT, QUIET):
                continue
            lo, s, c = R_LO[r], R_SPAN[r], np.float32(R_CEIL[r])
            assert np.abs(got_y[r, lo:lo + s]).max() <= c and np.isfinite(got_y[r, lo:lo + s]).all(), (tick, r)
            assert _bits_equal(got_y[r, :lo], wave[r, :lo]) and _bits_equal(got_y[r, lo + s:], wave[r, lo + s:]), (tick, r)
            assert got_g[r] < 1.0 and np.nanmax(np.abs(wave[r, lo:lo + s])) > c, (tick, r)
        if tick == 1:
            lo, c = R_LO[NONFINITE], np.float32(R_CEIL[NONFINITE])
            assert got_y[NONFINITE, [150, 200, 260]].tolist() == [-c] * 3 and got_g[NONFINITE] == 0.0
            assert not np.isfinite(wave[NONFINITE, [150, 200, 260]]).any()
    # a history that outlives a tick: row 8 emits 64 samples per tick under P = 199
    assert not np.all(ref_hist[8, -3 * 64:] == 1.0) and R_SPAN[8] * 3 < R_HIST
    # without gmin: the same y and hist
    wave = _rows_wave(5)
    h0 = np.random.default_rng(9).uniform(0.3, 1.0, (ROWS, R_HIST)).astype(np.float32)
    outs = []
    for with_gmin in (True, False):
        y, h = Guarded((ROWS, LD), torch.float32, 123.0, wave), Guarded((ROWS, R_HIST), torch.float32, -9.0, h0)
        MS.limit_rows_(y.view, *args, h.view, gmin.view if with_gmin else None)
        torch.cuda.synchronize()
        assert y.intact() and h.intact()
        outs.append((y.view.cpu().numpy(), h.view.cpu().numpy()))
    want_y, want_h, _ = LR.limit_rows(wave, R_LO, R_SPAN, R_SHIFT, R_LOOK, R_HOLD, R_CEIL, R_EMIT, h0)
    assert all(_bits_equal(a, want_y) and _bits_equal(b, want_h) for a, b in outs)


# ---------------------------------------------------------------------------------------------------- 2. alive_limit_waves
W_LD = 3 * TILE + 7
W_LENS = [0, 1, TILE - 1, TILE, TILE + 1, W_LD, 2000, W_LD]
W_CEIL = [0.9, 0.9, 0.5, 0.9, 0.8, 0.9, 0.7, 0.0]                    # (the last row has no valid ceiling: copied whole)


def _waves_case(L):
    y = _peaky((len(W_LENS), W_LD), 200 + L, peaks=10)
    for r, ln in enumerate(W_LENS):
        # on, just before and just after the tile borders; within L of both ends; just past the row's length (must not count)
        for p in (0, 1, L - 1, L, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE, ln - L, ln - 2, ln - 1, ln,
                  ln + 1):
            if 0 <= p < W_LD:
                y[r, p] = 3.0 if p % 2 else -2.5
    return y


@pytest.mark.parametrize("L,H", [(37, 50), (1, 0), (300, 700), (1025, 2047)])
def test_limit_waves_against_the_restatement(L, H):
    wave = _waves_case(L)
    n = len(W_LENS)
    y = _dev(wave, torch.float32)
    out = Guarded((n, W_LD), torch.float32, 123.0)
    gmin = Guarded((n,), torch.float32, -5.0)
    lens_d, ceil_d = _dev(W_LENS, torch.int32), _dev(W_CEIL, torch.float32)      # (kept alive until the kernel has run)
    MS.nat.check(MS.nat.lib().alive_limit_waves(out.view.data_ptr(), y.data_ptr(), n, W_LD, lens_d.data_ptr(), L, H, ceil_d.data_ptr(),
                                                gmin.view.data_ptr(), MS.nat.stream()), "alive_limit_waves")
    torch.cuda.synchronize()
    assert out.intact() and gmin.intact() and torch.equal(y.cpu(), torch.from_numpy(wave))
    want, want_g = LR.limit_waves(wave, W_LENS, L, H, W_CEIL)
    got, got_g = out.view.cpu().numpy(), gmin.view.cpu().numpy()
    for r, ln in enumerate(W_LENS):
        assert _bits_equal(got[r], want[r]), r
        assert got_g[r] == want_g[r], r
        assert _bits_equal(got[r, ln:], wave[r, ln:])
        if ln and W_CEIL[r] > 0:
            assert np.abs(got[r, :ln]).max() <= np.float32(W_CEIL[r]) and got_g[r] < 1
    assert got_g[0] == 1.0 and got_g[-1] == 1.0 and _bits_equal(got[-1], wave[-1])
    # the wrapper: the same samples, gmin optional
    again = MS.limit_waves_rows(y, lens_d, L, H, ceil_d)
    assert _bits_equal(again.cpu().numpy(), got)
    with pytest.raises(ValueError, match="overlaps"):
        MS.nat.check(MS.nat.lib().alive_limit_waves(y.data_ptr(), y.data_ptr(), n, W_LD, lens_d.data_ptr(), L, H, ceil_d.data_ptr(),
                                                    None, MS.nat.stream()), "alive_limit_waves")


def test_limit_waves_python_api():
    wave = _peaky((3, 5000), 31)
    y = _dev(wave, torch.float32)
    out, db = MS.limit_waves(y, [5000, 3000, 5000], [-1.0, -6, None], 5.0, 20.0, 16000, return_gain=True)
    want, g = LR.limit_waves(wave, [5000, 3000, 5000], 80, 320, [np.float32(10 ** -0.05), np.float32(10 ** -0.3), 0.0])
    assert _bits_equal(out.cpu().numpy(), want) and db == MS.gmin_db(g.tolist()) and db[2] == 0.0 and db[0] < 0
    one = MS.limit_waves(y[0], None, -1.0, 5.0, 20.0, 16000)
    assert one.shape == (5000,) and _bits_equal(one.cpu().numpy(), want[0]) and torch.equal(y.cpu(), torch.from_numpy(wave))
    with pytest.raises(ValueError, match=r"L - 1 \+ H is at most 3072 \(the largest limit_hold_ms that fits is 59.0208\)"):
        MS.limit_waves(y, None, -1.0, 5.0, 60.0, 48000)
    with pytest.raises(ValueError, match="limit_db=2 must be"):
        MS.limit_waves(y, None, 2)


@pytest.mark.parametrize("span,shift,L,H", [(160, 160, 80, 160), (440, 441, 220, 79), (1100, 1100, 300, 0)])
def test_limit_rows_tick_by_tick_is_bitwise_limit_waves_over_the_whole_signal(span, shift, L, H):
    ticks, lo = 7, 30
    ld, ld_hist = lo + shift + span + 5, L - 1 + H
    sig = _peaky((1, ticks * shift + ld), 300 + span, peaks=12 * ticks)[0]
    c = np.float32(0.85)
    args = [_dev([v], torch.int32) for v in (lo, span, shift, L, H)] + [_dev([c], torch.float32), _dev([1], torch.uint8)]
    hist = torch.ones(1, ld_hist, device=DEV)
    got = []
    for t in range(ticks):
        y = _dev(sig[t * shift:t * shift + ld][None].copy(), torch.float32)
        MS.limit_rows_(y, *args, hist)
        got.append(y[0, lo:lo + span].cpu().numpy())
    got = np.concatenate(got)
    last = sig[(ticks - 1) * shift:(ticks - 1) * shift + ld]
    emitted = np.concatenate([sig[t * shift + lo:t * shift + lo + span] for t in range(ticks)] + [last[lo + shift:lo + shift + L - 1]])
    whole = MS.limit_waves_rows(_dev(emitted[None], torch.float32), _dev([len(emitted)], torch.int32), L, H, _dev([c], torch.float32))
    assert _bits_equal(got, whole[0, :ticks * span].cpu().numpy()) and np.abs(got).max() <= c < np.abs(emitted).max()
    assert _bits_equal(got, LR.limit_waves(emitted[None], [len(emitted)], L, H, [c])[0][0, :ticks * span])


# ---------------------------------------------------------------------------------------------------- 3. the converter
CHUNK, BS = 160, 16
RATES = [16000, 44100, 48000]
CHUNKS = [160, 441, 480]
SPANS = [(1200, 160), (3308, 440), (3600, 480)]
SESS = [dict(voice="v0", pitch=1.0, rate=16000), dict(voice="v1", alpha=0.1, rate=44100), dict(voice="v2", f0_rate=0.9, rate=48000)]
TICKS = 46
QUIET_TICKS = range(20, 34)                                          # slot 0's input is silent there: its gate closes
EXTRA = [dict(gate_db=-40, gate_hold=0.0, crossfade_ms=5), dict(crossfade_ms=5), dict()]
LIM = [dict(limit_db=-1.0), dict(limit_db=-3.0, limit_lookahead_ms=2.0, limit_hold_ms=10.0), dict()]
LD_HIST = 2400                                                       # 50 ms at 48 kHz
RETUNE_AT, OFF_AT, ON_AT = BS + 5, BS + 9, BS + 12                  # slot 1: -6 dBFS, then off, then on again


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    return MS.VoicePool(voices)


def _tap(conv):
    """keep every tick's float waves (before float_to_pcm16)"""
    waves, run = [], conv._run

    def wrapped():
        w = run()
        waves.append(w.clone())
        return w
    conv._run = wrapped
    return waves


def _drive(conv, sess, pcm, ticks, chunks, actions=None, after=None):
    """-> per session the list of per-tick outputs (None while its ring fills)"""
    outs = [[] for _ in sess]
    for s, p in enumerate(sess):
        conv.open(s, **p)
    for tick in range(ticks):
        for a in (actions or {}).get(tick, []):
            a(conv)
        feed = {s: pcm[s][tick * c:(tick + 1) * c] for s, c in enumerate(chunks)}
        res = conv.step(feed)
        for s in range(len(sess)):
            outs[s].append(res[s])
        if after is not None and any(r is not None for r in res.values()):
            after(conv, tick)
    return outs


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
                                    for x, y in zip(a, b))


def _rate_pcm():
    pcm = [_pcm(c * TICKS, 70 + s) for s, c in enumerate(CHUNKS)]
    pcm[0] = pcm[0].copy()
    for t in QUIET_TICKS:
        pcm[0][t * CHUNK:(t + 1) * CHUNK] = 0
    return pcm


def _conv(pool, **kw):
    return MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, rates=RATES, **kw)


@pytest.fixture(scope="module")
def gains(pool):
    """the output gain per session that brings the peak of its emitted float samples to 1.5: the output gain is a linear factor in
    front of the output resample, so the twin's wave at that gain exceeds 1.0 in some emitted samples and stays under 2.0"""
    conv = _conv(pool, gate=True, crossfade=True)
    waves = _tap(conv)
    _drive(conv, [dict(p, **e) for p, e in zip(SESS, EXTRA)], _rate_pcm(), TICKS, CHUNKS)
    peak = [max(float(w[s, lo:lo + ln].abs().max()) for w in waves) for s, (lo, ln) in enumerate(SPANS)]
    assert all(p > 0 for p in peak)
    return [20.0 * np.log10(1.5 / p) for p in peak]


def _actions(graph_at=None):
    acts = {RETUNE_AT: [lambda c: c.set(1, limit_db=-6.0)], OFF_AT: [lambda c: c.set(1, limit_db=None)],
            ON_AT: [lambda c: c.set(1, limit_db=-3.0, limit_lookahead_ms=5.0)]}
    if graph_at is not None:
        acts.setdefault(graph_at, []).insert(0, lambda c: c.enable_graph())
    return acts


def _limited_run(pool, gains, graph_at=None):
    conv = _conv(pool, gate=True, crossfade=True, limiter=True)
    sess = [dict(p, gain=g, **e, **lim) for p, g, e, lim in zip(SESS, gains, EXTRA, LIM)]
    rec = dict(db=[], hist=[], captures=[])

    def after(c, tick):
        rec["db"].append(c.limit_db())
        rec["hist"].append(c.limit_hist.cpu().numpy())
        rec["captures"].append(c.captures)
    outs = _drive(conv, sess, _rate_pcm(), TICKS, CHUNKS, actions=_actions(graph_at), after=after)
    return outs, rec, conv


@pytest.fixture(scope="module")
def runs(pool, gains):
    """the twin without a limiter (gate and crossfade on, the same gains: outputs and full float waves), the limiting converter,
    eager, over the same script, and what limit_ref.stream makes of the twin's waves: computed once"""
    twin = _conv(pool, gate=True, crossfade=True)
    waves = _tap(twin)
    want = _drive(twin, [dict(p, gain=g, **e) for p, g, e in zip(SESS, gains, EXTRA)], _rate_pcm(), TICKS, CHUNKS)
    got, rec, conv = _limited_run(pool, gains)
    ticks = list(range(BS, TICKS))
    c1, c3, c6 = (min(10.0 ** (db / 20.0), 32767 / 32768) for db in (-1.0, -3.0, -6.0))
    look, hold, ceil = [], [], []
    for t in ticks:
        if t < RETUNE_AT:
            s1 = (88, 441, c3)                                       # 2 ms and 10 ms at 44.1 kHz
        elif t < OFF_AT:
            s1 = (88, 441, c6)
        elif t < ON_AT:
            s1 = (0, 0, 1.0)
        else:
            s1 = (220, 441, c3)
        look.append([80, s1[0], 0])
        hold.append([320, s1[1], 0])
        ceil.append([c1, s1[2], 1.0])
    w = [x.cpu().numpy() for x in waves]
    lo, ln = [s[0] for s in SPANS], [s[1] for s in SPANS]
    limited, _, gmins, hist = LR.stream(w, lo, ln, CHUNKS, look, hold, ceil, ld_hist=LD_HIST)
    pcm = [audio_io.float_to_pcm16(torch.from_numpy(f).to(DEV)).cpu().numpy() for f in limited]
    return dict(want=want, waves=w, got=got, rec=rec, conv=conv, ticks=ticks, limited=limited, gmins=gmins, pcm=pcm, hist=hist,
                ceil=ceil, look=look)


@pytest.mark.parametrize("graph", [False, True])
def test_a_limiter_converter_with_no_session_limiting_is_bitwise_the_plain_converter(pool, graph):
    ticks = BS + 4
    pcm = _rate_pcm()
    plain = _conv(pool)
    want = _drive(plain, SESS, pcm, ticks, CHUNKS)
    conv = _conv(pool, limiter=True)
    if graph:
        conv.enable_graph()
    got = _drive(conv, [dict(p, limit_db=None) for p in SESS], pcm, ticks, CHUNKS)
    assert all(sum(o is not None for o in g) == ticks - BS for g in got) and all(_same(g, w) for g, w in zip(got, want))
    assert conv.look.tolist() == [0, 0, 0] and conv.captures == int(graph) and conv.limit_db() == [0.0] * 3
    assert bool((conv.limit_hist == 1.0).all()) and conv.limit_hist.shape == (3, LD_HIST) and conv.limit_shift.tolist() == CHUNKS
    assert conv.span_lo.tolist() == [s[0] for s in SPANS] and conv.span_len.tolist() == [s[1] for s in SPANS]
    with pytest.raises(ValueError, match=r"slot 0: limit_db=-1 needs a converter built with MultiStreamConverter\(..., limiter=True\)"):
        plain.set(0, limit_db=-1)
    assert not hasattr(plain, "limit_hist") and plain.params[0].get("limit_db") is None
    with pytest.raises(ValueError, match="limit_db needs a converter built with"):
        plain.limit_db()
    before = {a: getattr(conv, a).clone() for a in ("look", "hold", "ceil", "pitch", "seg_len")}
    for bad in (dict(limit_db=float("nan")), dict(limit_db="x"), dict(limit_db=-1, limit_lookahead_ms=11, pitch=3.0),
                dict(limit_db=-1, limit_hold_ms=60)):
        with pytest.raises(ValueError, match="slot 1: limit_"):
            conv.set(1, **bad)
    assert all(torch.equal(getattr(conv, a), v) for a, v in before.items()) and conv.params[1]["pitch"] == 0.0


def test_every_emitted_chunk_is_the_restatement_of_the_twins_waves_and_never_wraps(runs):
    got, want, rec, conv = runs["got"], runs["want"], runs["rec"], runs["conv"]
    assert len(runs["waves"]) == TICKS - BS == len(rec["db"]) and conv.captures == 0
    wrapped, reduced = [0, 0, 0], [0, 0, 0]
    for i, t in enumerate(runs["ticks"]):
        for s, (lo, ln) in enumerate(SPANS):
            o, w = got[s][t], runs["waves"][i][s, lo:lo + ln]
            assert o.shape == (ln,) and np.array_equal(o, runs["pcm"][i][s, lo:lo + ln]), (t, s)
            c = runs["ceil"][i][s]
            assert np.abs(w).max() < 2.0
            scaled = (w * np.float32(32768.0)).astype(np.int32)      # (what alive_float_to_pcm16 forms before it keeps 16 bits)
            over = (scaled > 32767) | (scaled < -32768)
            if over.any():                                           # the case is live: the twin's int16 wraps there
                assert np.all(np.abs(w[over]) > 1.0) and np.all(np.sign(want[s][t][over].astype(np.int32)) == -np.sign(w[over])), (t, s)
                wrapped[s] += int(over.sum())
            if runs["look"][i][s] > 0:
                assert np.abs(o.astype(np.int32)).max() <= int(np.floor(np.float32(c) * 32768)), (t, s)
                reduced[s] += not np.array_equal(o, want[s][t])
            else:
                assert np.array_equal(o, want[s][t]), (t, s)
        g = runs["gmins"][i]
        assert rec["db"][i] == MS.gmin_db(g.tolist()), t
        print(f"tick {t}: limit_db {['%.2f' % v for v in rec['db'][i]]}")
    print("samples over 1.0 in the twin:", wrapped, "chunks the limiter changed:", reduced)
    assert wrapped[0] > 0 and wrapped[1] > 0 and wrapped[2] > 0 and reduced[0] > 0 and reduced[1] > 0 and reduced[2] == 0
    assert _bits_equal(conv.limit_hist.cpu().numpy(), runs["hist"])
    # the silence: the gate's zeros ask for nothing and come out as zeros, and their required gains in the history are 1.0 (the
    # lookahead lies beyond the span, where the gate's edge does not reach, so limit_db() may still report a reduction there)
    t = 35
    assert not got[0][t].any() and rec["db"][t - BS][0] <= 0.0 and np.all(rec["hist"][t - BS][0, -CHUNK:] == 1.0)
    # slot 1 while its limiter was off: the twin's chunk, and its history back at 1.0 after OFF_AT
    assert np.array_equal(got[1][OFF_AT], want[1][OFF_AT]) and np.all(rec["hist"][OFF_AT - BS][1] == 1.0)
    assert np.all(rec["hist"][-1][2] == 1.0) and any(not np.all(h[0] == 1.0) for h in rec["hist"])


def test_enable_graph_in_the_middle_and_retuning_leave_the_stream_unchanged_and_capture_once(pool, gains, runs):
    g_out, g_rec, conv = _limited_run(pool, gains, graph_at=BS + 3)
    assert all(_same(a, b) for a, b in zip(g_out, runs["got"]))
    assert all(_bits_equal(a, b) for a, b in zip(g_rec["hist"], runs["rec"]["hist"])) and g_rec["db"] == runs["rec"]["db"]
    # captured once: the retune, the switch off and the switch on never re-captured
    assert g_rec["captures"] == [0] * 3 + [1] * (TICKS - BS - 3) and conv.captures == 1
    conv.set(2, limit_db=-2.0)
    conv.set(0, limit_db=None)
    conv.step({s: np.zeros(c, np.int16) for s, c in enumerate(CHUNKS)})
    assert conv.captures == 1 and conv.look.tolist() == [0, 220, 240] and bool((conv.limit_hist[0] == 1.0).all())
    conv.close(1)
    assert conv.look.tolist() == [0, 0, 240] and bool((conv.limit_hist[1] == 1.0).all()) and conv.limit_shift.tolist() == [160, 160, 480]
    conv.open(1, "v1", rate=48000, limit_db=-1.0)
    assert conv.look.tolist() == [0, 240, 240] and conv.limit_shift.tolist() == [160, 480, 480] and conv.limit_db()[1] == 0.0


@pytest.mark.parametrize("graph", [False, True])
def test_the_bf16_repeat_restarts_from_the_history_the_tick_started_from(pool, monkeypatch, graph):
    """the repeat of a tick (after an fp16 saturation) with the switch of the process to bf16 planes stubbed out: the same tick again
    gives the same limited samples -- from the history the tick started from, not the one its first attempt left"""
    from module.realtime import RealtimeConverter
    monkeypatch.setattr(MS.ops, "switch_to_bf16", lambda *a: None)
    ticks = BS + 3
    pcm = _pcm(CHUNK * ticks, 80)
    kw = dict(chunk=CHUNK, buffersize=BS, k=4)
    conv = MS.MultiStreamConverter(*_nets(), pool, 1, limiter=True, **kw)
    conv.open(0, "v0", gain=60.0, limit_db=-1.0)
    rt = RealtimeConverter(*_nets(), pool.tokens("v0")[None], "cuda", reuse_interior=False, gain=60.0, limit_db=-1.0, **kw)
    if graph:
        conv.enable_graph()
        rt.enable_graph()
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        if t == ticks - 1:
            saved = (conv.phi.clone(), conv._seam_state(), rt._g_phi.clone() if graph else rt.phi,
                     (rt._limit_hist.clone(), rt._limit_gmin.clone()))
        out, out_rt = conv.step({0: c})[0], rt.step(c)
    after = conv.limit_hist.clone(), rt._limit_hist.clone(), conv.limit_db()[0], rt.limit_db()
    assert after[2] < 0 and after[3] < 0 and not torch.equal(saved[1][2], after[0]) and not torch.equal(saved[3][0], after[1])
    assert saved[1][0] is None
    lo, ln = conv._span(CHUNK)
    again = conv._repeat_on_bf16(saved[0], None, None, saved[1])
    assert np.array_equal(again[0, lo:lo + ln], out) and conv.limit_db()[0] == after[2] and torch.equal(conv.limit_hist, after[0])
    data = audio_io.pcm16_to_float(torch.from_numpy(np.concatenate(rt.ring)).to(DEV)).unsqueeze(0)
    again = rt._repeat_on_bf16(data, saved[2], None, None, saved[3])
    assert np.array_equal(again[lo:lo + ln], out_rt) and rt.limit_db() == after[3] and torch.equal(rt._limit_hist, after[1])


# ---------------------------------------------------------------------------------------------------- 4. RealtimeConverter
@pytest.mark.parametrize("graph", [False, True])
def test_a_limiting_realtime_converter_is_bitwise_a_one_slot_multistream(graph):
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(400, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    lim = dict(limit_db=-2.0, limit_lookahead_ms=5.0, limit_hold_ms=20.0)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, gain=60.0, reuse_interior=False, **lim, **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, limiter=True, **kw)
    ms.open(0, "lib", pitch=1.5, alpha=0.2, gain=60.0, **lim)
    plain = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, gain=60.0, reuse_interior=False, **kw)
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    ticks, differ = BS + 5, 0
    pcm = _pcm(CHUNK * ticks, 80)
    top = int(np.floor(np.float32(10 ** -0.1) * 32768))
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b, p = rt.step(c), ms.step({0: c})[0], plain.step(c)
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b) and torch.equal(rt._limit_hist, ms.limit_hist), t
            assert rt.limit_db() == ms.limit_db()[0] < 0 and np.abs(a.astype(np.int32)).max() <= top
            differ += not np.array_equal(a, p)
    assert differ == ticks - BS and rt._limit_look.tolist() == [80] and rt._limit_hold.tolist() == [320]
    # reset() and a ring unrelated to the previous one start from a history of 1.0
    assert not bool((rt._limit_hist == 1.0).all())
    ring = audio_io.pcm16_to_float(torch.from_numpy(np.concatenate(rt.ring)).to(DEV)).unsqueeze(0)
    assert rt._limit_hist.shape == (1, 800) and not bool((rt._limit_hist[0, :-CHUNK] == 1.0).all())
    rt.step_device(ring, continues=False)                            # the history holds this step's span alone
    assert bool((rt._limit_hist[0, :-CHUNK] == 1.0).all()) and not bool((rt._limit_hist[0, -CHUNK:] == 1.0).all())
    rt.step_device(ring, continues=True)
    assert not bool((rt._limit_hist[0, -2 * CHUNK:-CHUNK] == 1.0).all())
    rt.reset()
    assert bool((rt._limit_hist == 1.0).all()) and rt.limit_db() == 0.0
    with pytest.raises(ValueError, match="limit_db needs a converter built with"):
        plain.limit_db()
    with pytest.raises(ValueError, match=r"limit_lookahead_ms=11 is 176 samples"):
        RealtimeConverter(*_nets(), lib, "cuda", limit_db=-1, limit_lookahead_ms=11, **kw)


def test_a_limiting_realtime_converter_with_interior_reuse_is_bitwise_itself_without():
    """-c 960 -b 26: a ring of 78 frames advancing by 3"""
    from module.realtime import RealtimeConverter
    chunk, bs, ticks = 960, 26, 29
    lib = synthetic.make_library(400, 1)
    pcm = _pcm(chunk * ticks, 95)
    outs, dbs = {}, {}
    for reuse in (False, "auto"):
        rt = RealtimeConverter(*_nets(), lib, "cuda", chunk=chunk, buffersize=bs, k=4, alpha=0.1, gain=60.0, reuse_interior=reuse,
                               limit_db=-1.0)
        assert rt.reuse == bool(reuse) and rt._limit_look.tolist() == [80] and rt._limit_shift.tolist() == [960]
        outs[reuse], dbs[reuse] = [], []
        for t in range(ticks):
            o = rt.step(pcm[t * chunk:(t + 1) * chunk])
            if o is not None:
                outs[reuse].append(o)
                dbs[reuse].append(rt.limit_db())
    top = int(np.floor(np.float32(10 ** -0.05) * 32768))
    assert len(outs[False]) == ticks - bs and all(np.array_equal(a, b) for a, b in zip(outs[False], outs["auto"]))
    assert dbs[False] == dbs["auto"] and all(d < 0 for d in dbs[False])
    assert all(np.abs(o.astype(np.int32)).max() <= top for o in outs[False])


# ---------------------------------------------------------------------------------------------------- 5. the CLIs
def _save_nets(d):
    for name, net in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _nets()):
        torch.save(net.state_dict(), d / name)
    return ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]


def _loaded_nets(d):
    CE, PE, Dec = (n.to(DEV) for n in _nets())
    CE.load_state_dict(torch.load(d / "content_encoder.pt"))
    PE.load_state_dict(torch.load(d / "f0_estimator.pt"))
    Dec.load_state_dict(torch.load(d / "decoder.pt"))
    return CE, PE, Dec


def test_multistream_cli_with_a_limiting_session_writes_what_the_converter_emits(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    ticks = BS + 6
    wav = _pcm(CHUNK * ticks, 80).astype(np.float32) / 32767
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    base = [dict(input="in0.wav", lib="voice_library.pt", gain=60), dict(input="in1.wav", lib="voice_library.pt", gain=60)]
    json.dump([dict(base[0], limit_db=-1, limit_hold_ms=10), base[1]], open(d / "lim.json", "w"))
    json.dump(base, open(d / "plain.json", "w"))
    json.dump([base[0], dict(base[1], limit_db=None)], open(d / "null.json", "w"))
    common = nets + ["-c", str(CHUNK), "-b", str(BS)]
    msi.main(common + ["-o", str(d / "out_lim"), str(d / "lim.json")])
    msi.main(common + ["-o", str(d / "out_plain"), str(d / "plain.json")])
    msi.main(common + ["-o", str(d / "out_flag"), "-lim", "-1", "--limit-hold", "10", str(d / "null.json")])
    ss = msi.load_sessions(str(d / "lim.json"))
    assert ss[0]["limit_db"] == -1.0 and ss[0]["limit_hold_ms"] == 10.0 and "limit_db" not in ss[1]

    def read(sub):
        out = []
        for p in (d / sub / "0_in0.wav", d / sub / "1_in1.wav"):
            g, sr = audio_io.load(str(p))
            assert sr == 16000
            out.append(np.round(g[0].numpy() * 32768).astype(np.int16))
        return out
    CE, PE, Dec = _loaded_nets(d)
    vpool = MS.VoicePool()
    name = msi.voice_name(None, str(d / "voice_library.pt"))
    vpool.add(name, msi.voice_tokens(CE, None, str(d / "voice_library.pt"), DEV))
    pcms = [msi.input_pcm(s["input"], 16000, DEV) for s in ss]
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4, limiter=True)
    want_lim = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, gain=60.0, limit_db=-1.0, limit_hold_ms=10.0),
                                                   dict(voice=name, gain=60.0)])
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4)
    want_plain = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, gain=60.0), dict(voice=name, gain=60.0)])
    lim, plain, flag = read("out_lim"), read("out_plain"), read("out_flag")
    assert all(len(w) == CHUNK * (ticks - BS) for w in want_lim + want_plain)
    assert np.array_equal(lim[0], want_lim[0]) and np.array_equal(lim[1], want_lim[1])
    # a file without the key, run without the flag: what the converter built without the limiter writes, byte for byte
    assert np.array_equal(plain[0], want_plain[0]) and np.array_equal(plain[1], want_plain[1])
    assert np.array_equal(lim[1], plain[1]) and not np.array_equal(lim[0], plain[0])
    assert np.abs(lim[0].astype(np.int32)).max() <= int(np.floor(np.float32(10 ** -0.05) * 32768))
    # -lim as the default, switched off by a session's null: the same input twice, so the outputs swap roles
    assert np.array_equal(flag[0], lim[0]) and np.array_equal(flag[1], plain[1])


def test_offline_clis_with_a_limit_write_limit_waves_of_what_they_wrote_without(tmp_path):
    import batch_inference as BI
    import inference as INF
    from module.pipeline import Converter
    d = tmp_path
    nets = _save_nets(d)
    lib = synthetic.make_library(512, 5)
    torch.save({"tokens": lib}, d / "voice_library.pt")
    os.makedirs(d / "inputs")
    wav = synthetic.make_waveform(24000, 91) * 0.5                   # 1 s mono at 24 kHz
    audio_io.save(str(d / "inputs" / "utt.wav"), wav, 24000)
    base = ["-i", str(d / "inputs"), "-lib", str(d / "voice_library.pt"), "-d", "cuda", "-c", "4800", "-g", "40"] + nets
    INF.main(base + ["-o", str(d / "out_plain")])
    INF.main(base + ["-o", str(d / "out_lim"), "-lim", "-1", "--limit-lookahead", "2", "--limit-hold", "10"])
    plain, sr = audio_io.load(str(d / "out_plain" / "0_utt.wav"))
    lim, sr2 = audio_io.load(str(d / "out_lim" / "0_utt.wav"))
    assert sr == sr2 == 24000 and float(plain.abs().max()) > 1.0
    want = MS.limit_waves(plain.to(DEV), None, -1.0, 2.0, 10.0, 24000).cpu()
    assert torch.equal(lim, want) and float(lim.abs().max()) <= 10 ** -0.05 and not torch.equal(lim, plain)
    # without the flag: the bytes the API path makes (inference.py as it was)
    CE, PE, Dec = _loaded_nets(d)
    wf = audio_io.resample(audio_io.load(str(d / "inputs" / "utt.wav"))[0].to(DEV), 24000, 16000)
    wf = (wf / wf.abs().max()).mean(dim=0, keepdim=True)
    out = Converter(CE, PE, Dec, DEV).set_library(lib.to(DEV)).convert(wf, chunk=4800, k=4, alpha=0.0, pitch_shift=0, world_pitch=False,
                                                                      intonation=1.0, f0_rate=1.0, window_batch=64, trim_context=True,
                                                                      share_overlap="auto")
    assert torch.equal(plain, audio_io.resample(out, 16000, 24000, post_gain_db=40.0).cpu())
    # batch_inference.py: a job with "limit_db" beside the same job without; -lim as the default with a null
    jobs = [dict(input="inputs/utt.wav", lib="voice_library.pt", gain=40, output="b_plain.wav"),
            dict(input="inputs/utt.wav", lib="voice_library.pt", gain=40, limit_db=-3, output="b_lim.wav")]
    (d / "jobs.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs.json"), "-c", "4800"] + nets)
    b_plain, b_lim = audio_io.load(str(d / "b_plain.wav"))[0], audio_io.load(str(d / "b_lim.wav"))[0]
    assert float(b_plain.abs().max()) > 1.0
    assert torch.equal(b_lim, MS.limit_waves(b_plain.to(DEV), None, -3.0, 5.0, 20.0, 24000).cpu())
    assert float(b_lim.abs().max()) <= 10 ** -0.15
    pool = MS.VoicePool({"l": lib.to(DEV)[0]}, device=DEV)
    many = Converter(CE, PE, Dec, DEV).convert_many([wf, wf], pool, ["l", "l"], pitch_shift=[0.0, 0.0], intonation=[1.0, 1.0],
                                                    f0_rate=[1.0, 1.0], alpha=[0.0, 0.0], world_pitch=[False, False], auto_pitch=False,
                                                    chunk=4800, k=4, window_batch=64, trim_context=True)
    assert torch.equal(b_plain, audio_io.resample(many[0], 16000, 24000, post_gain_db=40.0).cpu())
    jobs = [dict(jobs[0], limit_db=None, output="c_plain.wav"), dict(jobs[0], output="c_lim.wav")]
    (d / "jobs2.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs2.json"), "-c", "4800", "-lim", "-3"] + nets)
    assert torch.equal(audio_io.load(str(d / "c_plain.wav"))[0], b_plain) and torch.equal(audio_io.load(str(d / "c_lim.wav"))[0], b_lim)
