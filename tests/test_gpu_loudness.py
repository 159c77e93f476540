"""GPU tests of loudness normalisation (csrc/loudness.hip), everything bitwise against tools/loudness_ref.py and every output between
guard bands: alive_loudness_measure_waves / alive_loudness_apply_waves in one call with mixed rates and every edge length, the Python
API, alive_loudness_rows over 18 ticks with the state carried, MultiStreamConverter(loudness=True) against a twin converter's
pre-loudness waves (beside crossfade, gate and limiter, with a mid-stream capture and retunes), the bf16 repeat, a sparse converter
with a stalled slot, and the three CLIs."""
import json
import math
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
import loudness_ref as R                                             # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import audio_io, synthetic                               # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 16                                                             # guard band, elements on each side of every output
Z_ABS = R.z_of(-70.0)


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
    i = np.int32 if a.dtype.itemsize == 4 else np.int64
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(i)[~nan], b.view(i)[~nan]))


# ---------------------------------------------------------------------------------------------------- 1. measure and apply
W_LD = 7 * 4410 + 3 + 5                                              # the 44.1 kHz row's 7 H + 3 and a tail that is copied
#          len 0  4H-1  4H    4H+1  7H+3         silent  rel gate  nonfinite  clamped  NaN target  48 kHz   short tail
W_RATE = [8000,  8000, 16000, 16000, 44100,       16000,  16000,    8000,      16000,   16000,      48000,   8000]
W_LENS = [0,     3199, 6400,  6401,  7 * 4410 + 3, 12000, W_LD,     9000,      20000,   W_LD,       28900,   W_LD + 50]
W_TGT = [-23.0, -23.0, -23.0, -23.0, -16.0,       -23.0,  -23.0,    -23.0,     -16.0,   None,       -25.0,   -23.0]
SILENT, RELGATE, NONFINITE, CLAMPED, COPIED = 5, 6, 7, 8, 9
W_ROWS = len(W_RATE)


def _waves():
    rng = np.random.default_rng(11)
    y = (0.1 * rng.standard_normal((W_ROWS, W_LD))).astype(np.float32)
    y[SILENT, :12000] = 0.0
    y[RELGATE, 14400:] *= np.float32(0.01)                           # -40 dB: above the absolute gate, under the relative one
    y[NONFINITE, [5, 1700, 4000]] = [np.nan, np.inf, -np.inf]
    y[CLAMPED] *= np.float32(0.005)
    return y


def _filters(rates):
    hops = [R.hop(r) for r in rates]
    coefs = np.stack([R.coefficients(r) for r in rates])
    aps = np.stack([R.carry_matrix(c, h).reshape(16) for c, h in zip(coefs, hops)])
    return hops, coefs, aps


def test_measure_and_apply_waves_against_the_restatement():
    y = _waves()
    hops, coefs, aps = _filters(W_RATE)
    tiles = max(min(max(v, 0), W_LD) // h for v, h in zip(W_LENS, hops))
    assert tiles == 38 and W_LENS[4] // hops[4] == 7 and W_LENS[1] // hops[1] == 3 and W_LENS[2] // hops[2] == 4
    L = nat.lib()
    nbytes = L.alive_loudness_workspace_bytes(W_ROWS, tiles)
    assert nbytes == W_ROWS * tiles * 72
    ws = Guarded((nbytes,), torch.uint8, 0xAB)
    zI = Guarded((W_ROWS,), torch.float64, -9.0)
    c1, c2 = Guarded((W_ROWS,), torch.int32, -5), Guarded((W_ROWS,), torch.int32, -5)
    yd, lens, hop = _dev(y, torch.float32), _dev(W_LENS, torch.int32), _dev(hops, torch.int32)
    coef, ap = _dev(coefs, torch.float64), _dev(aps, torch.float64)
    rc = L.alive_loudness_measure_waves(nat.ptr(yd), W_ROWS, W_LD, nat.ptr(lens), nat.ptr(hop), nat.ptr(coef), nat.ptr(ap), Z_ABS,
                                        tiles, nat.ptr(zI.view), nat.ptr(c1.view), nat.ptr(c2.view), nat.ptr(ws.view), nbytes,
                                        nat.stream())
    torch.cuda.synchronize()
    assert rc == 0 and ws.intact() and zI.intact() and c1.intact() and c2.intact() and _bits_equal(yd.cpu().numpy(), y)
    want_z, want_c1, want_c2 = R.measure_waves(y, W_LENS, hops, coefs, aps, Z_ABS, tiles)
    got_z, got_c1, got_c2 = zI.view.cpu().numpy(), c1.view.cpu().numpy(), c2.view.cpu().numpy()
    print("LUFS:", ["%.2f" % v for v in R.lufs(got_z)], "c1:", got_c1.tolist(), "c2:", got_c2.tolist())
    assert _bits_equal(got_z, want_z) and np.array_equal(got_c1, want_c1) and np.array_equal(got_c2, want_c2)
    # the cases are live
    assert got_c2[0] == 0 and got_c2[1] == 0 and got_c2[2] == 1 and got_c2[3] == 1 and got_c2[4] == 4 and got_c2[10] == 3
    assert got_c1[SILENT] == 0 and got_z[SILENT] == 0.0
    assert 0 < got_c2[RELGATE] < got_c1[RELGATE] == W_LD // 1600 - 3
    assert got_c2[NONFINITE] == 9000 // 800 - 3 and np.isfinite(got_z[NONFINITE])
    assert got_c2[11] == W_LD // 800 - 3                              # a len past the row is clamped to it
    assert abs(float(R.lufs(got_z[2])) - (-17.0)) < 1.0               # white noise at 0.1 rms: -20 dB, and the shelf lifts its top
    # against the end-to-end recurrence: rounding alone
    for r in (4, 10):
        z = R.gate(R.blocks(R.plain_q(y[r, :W_LENS[r]], hops[r], coefs[r]), hops[r]), Z_ABS)[0]
        assert abs(got_z[r] - z) <= 1e-11 * z
    # a row that has more sub-blocks than the workspace holds is not measured; the others do not change
    rc = L.alive_loudness_measure_waves(nat.ptr(yd), W_ROWS, W_LD, nat.ptr(lens), nat.ptr(hop), nat.ptr(coef), nat.ptr(ap), Z_ABS,
                                        19, nat.ptr(zI.view), nat.ptr(c1.view), nat.ptr(c2.view), nat.ptr(ws.view), nbytes, nat.stream())
    torch.cuda.synchronize()
    want19 = R.measure_waves(y, W_LENS, hops, coefs, aps, Z_ABS, 19)
    assert rc == 0 and ws.intact() and _bits_equal(zI.view.cpu().numpy(), want19[0]) and np.array_equal(c2.view.cpu().numpy(), want19[2])
    assert want19[2][11] == 0 and want19[2][RELGATE] == want_c2[RELGATE] and want19[2][4] == 4 and want19[0][4] == want_z[4]

    # apply
    z_t = np.array([math.nan if t is None else R.z_of(t) for t in W_TGT])
    gmax = 10.0 ** (12.0 / 20.0)
    out = Guarded((W_ROWS, W_LD), torch.float32, 123.0)
    gain = Guarded((W_ROWS,), torch.float64, -9.0)
    z_d, c2_d, zt_d = _dev(want_z, torch.float64), _dev(want_c2, torch.int32), _dev(z_t, torch.float64)
    rc = L.alive_loudness_apply_waves(nat.ptr(out.view), nat.ptr(yd), W_ROWS, W_LD, nat.ptr(lens), nat.ptr(z_d), nat.ptr(c2_d),
                                      nat.ptr(zt_d), gmax, nat.ptr(gain.view), nat.stream())
    torch.cuda.synchronize()
    assert rc == 0 and out.intact() and gain.intact()
    want_out, want_g = R.apply_waves(y, W_LENS, want_z, want_c2, z_t, gmax)
    got_out, got_g = out.view.cpu().numpy(), gain.view.cpu().numpy()
    assert _bits_equal(got_g, want_g)
    for r in range(W_ROWS):
        assert _bits_equal(got_out[r], want_out[r]), r
    for r in (0, 1, SILENT, COPIED):                                 # nothing to measure, silence, no target: the row as it was
        assert got_g[r] == 1.0 and _bits_equal(got_out[r], y[r]), r
    assert got_g[CLAMPED] == gmax and got_g[4] != 1.0 and 1 / gmax < got_g[4] < gmax
    for r in (2, 3, 4, 10):                                          # past the length the row is copied
        assert _bits_equal(got_out[r, W_LENS[r]:], y[r, W_LENS[r]:]) and not _bits_equal(got_out[r, :W_LENS[r]], y[r, :W_LENS[r]])
    assert np.isnan(got_out[NONFINITE, 5]) and np.isinf(got_out[NONFINITE, [1700, 4000]]).all()
    # what comes out reads the target (a stationary signal measured over the same samples)
    again = R.measure_waves(got_out, W_LENS, hops, coefs, aps, Z_ABS)
    for r in (4, 10, 11):
        assert abs(float(R.lufs(again[0][r])) - W_TGT[r]) < 0.05, r


def test_the_python_api_measures_and_normalises():
    y = _waves()
    hops, coefs, aps = _filters(W_RATE)
    want_z, want_c1, want_c2 = R.measure_waves(y, W_LENS, hops, coefs, aps, Z_ABS)
    yd = _dev(y, torch.float32)
    lens = [min(v, W_LD) for v in W_LENS]
    lufs, c1, c2 = MS.measure_loudness(yd, lens, W_RATE)
    assert c1 == want_c1.tolist() and c2 == want_c2.tolist()
    for got, z, c in zip(lufs, want_z, want_c2):
        assert got == -math.inf if not c else abs(got - float(R.lufs(z))) < 1e-9
    assert lufs[0] == lufs[SILENT] == -math.inf
    out, db = MS.normalize_loudness(yd, lens, W_TGT, W_RATE, return_gain=True)
    z_t = np.array([math.nan if t is None else R.z_of(t) for t in W_TGT])
    want_out, want_g = R.apply_waves(y, lens, want_z, want_c2, z_t, 10.0 ** 0.6)
    assert _bits_equal(out.cpu().numpy(), want_out) and db == [20.0 * math.log10(g) for g in want_g]
    assert db[CLAMPED] == 20.0 * math.log10(10.0 ** 0.6) and db[COPIED] == 0.0
    # one row, one rate, one target; the whole row by default; a smaller range
    one = MS.normalize_loudness(yd[4], None, -16.0, 44100)
    assert one.shape == (W_LD,) and _bits_equal(one.cpu().numpy()[:7 * 4410], want_out[4][:7 * 4410])
    l1, a1, b1 = MS.measure_loudness(yd[10, :28900].contiguous(), None, 48000)
    assert (l1, a1, b1) == (lufs[10], c1[10], c2[10])
    _, db3 = MS.normalize_loudness(yd[CLAMPED], None, -16.0, 16000, max_gain_db=3.0, return_gain=True)
    assert db3 == 20.0 * math.log10(10.0 ** 0.15)
    for bad, msg in ((dict(target_lufs=1.0), "lufs=1.0 must be"), (dict(target_lufs=-23.0, max_gain_db=-1), "loudness max gain"),
                     (dict(target_lufs=[-23.0] * 3), "3 target_lufs for 12 rows"), (dict(target_lufs=-23.0, rate=[16000]), "1 rates for"),
                     (dict(target_lufs=-23.0, rate=16000.5), "rate=16000.5 must be"), (dict(target_lufs=-23.0, lens=[1]), "1 lens for")):
        kw = dict(dict(lens=None, rate=16000), **bad)
        with pytest.raises(ValueError, match=msg):
            MS.normalize_loudness(yd, kw["lens"], kw["target_lufs"], kw["rate"], kw.get("max_gain_db", 12.0))
    with pytest.raises(ValueError, match="wave must be float32"):
        MS.measure_loudness(yd.double())


# ---------------------------------------------------------------------------------------------------- 2. alive_loudness_rows alone
LD = 2003                                                            # (a stride that is no multiple of 256)
#         off    filling  2 per tick  slewed  44.1 kHz  pause   no fit  nonfinite  far target
R_RATE = [16000, 16000,   8000,       16000,  44100,    16000,  16000,  16000,     16000]
R_LO = [100,     100,     50,         107,    200,      200,    1900,   100,       300]
R_SPAN = [160,   160,     1700,       1600,   1764,     1600,   160,    200,       1100]
R_EMIT = [1,     0,       1,          1,      1,        1,      1,      1,         1]
R_ON = [0,       1,       1,          1,      1,        1,      1,      1,         1]
R_TGT = [-20.0,  -20.0,   -23.0,      -5.0,   -16.0,    -20.0,  -20.0,  -23.0,     -60.0]
#        (row 5: half-life 0.3 s, prior 0.2 s, so that W passes P = 2 within three blocks and falls under it within a few more)
R_KW = [{}, {}, dict(slew=60.0), dict(slew=1.0, prior=0.1), dict(slew=30.0), dict(half_life=0.3, prior=0.2, slew=60.0), {}, {},
        dict(slew=200.0, prior=0.1, max_db=20.0)]
OFF, FILLING, TWO, SLEWED, PAUSE, NOFIT, NONFIN, FAR = 0, 1, 2, 3, 5, 6, 7, 8
ROWS, TICKS_ROWS, LOUD_TICKS = len(R_RATE), 18, 8


def _rows_wave(tick):
    rng = np.random.default_rng(300 + tick)
    y = (0.1 * rng.standard_normal((ROWS, LD))).astype(np.float32)
    if tick >= LOUD_TICKS:
        y[PAUSE] *= np.float32(0.02)                                 # -34 dB: above the absolute gate, a pause to the relative one
    if tick == 5:
        y[NONFIN, [150, 200, 260]] = [np.nan, np.inf, -np.inf]
    return y


def test_loudness_rows_against_the_restatement_over_eighteen_ticks():
    assert R_LO[NOFIT] + R_SPAN[NOFIT] == LD + 57 and R_SPAN[TWO] > 2 * R.hop(R_RATE[TWO]) and R_SPAN[TWO] > 1024
    hops, coefs, _ = _filters(R_RATE)
    par = np.stack([R.params(fs, n, t, **kw) for fs, n, t, kw in zip(R_RATE, R_SPAN, R_TGT, R_KW)])
    args = [_dev(R_LO, torch.int32), _dev(R_SPAN, torch.int32), _dev(R_EMIT, torch.uint8), _dev(R_ON, torch.uint8), _dev(hops, torch.int32),
            _dev(coefs, torch.float64), _dev(par, torch.float64)]
    start = R.state0(ROWS)
    start[OFF, 10:13] = start[NOFIT, 10:13] = start[FILLING, 10:13] = [3e-3, 5.0, 1.5]      # what a tick must reset, or leave alone
    state = Guarded((ROWS, MS.LOUDNESS_STATE), torch.float64, -9.0, start)
    ref = start.copy()
    seen = dict(two=0, slewed=0, gated=0, released=0, clamped=0)
    for tick in range(TICKS_ROWS):
        wave = _rows_wave(tick)
        y = Guarded((ROWS, LD), torch.float32, 123.0, wave)
        MS.loudness_rows_(y.view, *args, state.view)
        torch.cuda.synchronize()
        assert y.intact() and state.intact()
        before = ref
        want_y, ref = R.loudness_rows(wave, R_LO, R_SPAN, R_EMIT, R_ON, hops, coefs, par, ref)
        got_y, got_s = y.view.cpu().numpy(), state.view.cpu().numpy()
        for r in range(ROWS):
            assert _bits_equal(got_y[r], want_y[r]), (tick, r)
            assert _bits_equal(got_s[r], ref[r]), (tick, r)
        # the rows that must not move; nothing written outside the span
        for r in (OFF, FILLING, NOFIT):
            assert _bits_equal(got_y[r], wave[r]), (tick, r)
        assert _bits_equal(got_s[FILLING], start[FILLING]) and _bits_equal(got_s[OFF], R.state0(1)[0])
        assert _bits_equal(got_s[NOFIT], R.state0(1)[0])
        for r in range(ROWS):
            lo, s = R_LO[r], R_SPAN[r]
            assert _bits_equal(got_y[r, :lo], wave[r, :lo]) and _bits_equal(got_y[r, lo + s:], wave[r, lo + s:]), (tick, r)
        assert np.isfinite(got_s).all()
        # which cases were live
        g0, g1 = before[:, R.G_SLOT], ref[:, R.G_SLOT]
        seen["two"] += int(tick >= 2 and ref[TWO, 11] - before[TWO, 11] * par[TWO, 2] ** 2 > 1.5)      # two blocks counted in one tick
        seen["slewed"] += int(g1[SLEWED] == g0[SLEWED] * par[SLEWED, 5] and g1[SLEWED] > 1.0)
        if tick >= LOUD_TICKS + 3:
            grew = ref[PAUSE, 11] > before[PAUSE, 11] * par[PAUSE, 2]
            seen["released" if grew else "gated"] += 1
        seen["clamped"] += int(abs(R.target_gain(ref[FAR], par[FAR]) - 0.1) < 1e-12)
        assert np.all(g1 <= np.maximum(g0 * par[:, 5], 1.0) * (1 + 1e-15)) and np.all(g1 >= np.minimum(g0 / par[:, 5], 1.0) * (1 - 1e-15))
    print("live cases:", seen, "gains:", ["%.3f" % v for v in ref[:, R.G_SLOT]])
    assert seen["two"] >= 5 and seen["slewed"] >= 5 and seen["gated"] >= 1 and seen["released"] >= 2 and seen["clamped"] >= 5
    # the pause: while W was trusted the quiet blocks were not counted; once believed they pull the running loudness down
    assert R.running_lufs(ref[PAUSE]) < R.running_lufs(ref[FAR]) - 5.0 and R.running_lufs(ref[FAR]) > -25.0


# ---------------------------------------------------------------------------------------------------- 3. the converter
CHUNK, BS = 320, 8
RATES = [16000, 44100, 48000]
CHUNKS = [320, 882, 960]
SPANS = [(1120, 320), (3087, 882), (3360, 960)]
SESS = [dict(voice="v0", pitch=1.0, rate=16000), dict(voice="v1", alpha=0.1, rate=44100), dict(voice="v2", f0_rate=0.9, rate=48000)]
TICKS = BS + 40                                                      # 800 ms emitted: five 400-ms blocks
QUIET_TICKS = range(30, 36)                                          # slot 0's input is silent there: its gate closes
EXTRA = [dict(gate_db=-40, gate_hold=0.0, crossfade_ms=5), dict(crossfade_ms=5), dict()]
LIM = [dict(limit_db=-1.0), dict(), dict()]
LUFS = [dict(lufs=-16.0), dict(lufs=-30.0), dict()]
LOUD_KW = dict(loudness_half_life=1.0, loudness_prior=0.3, loudness_slew_db=40.0)
RETUNE_AT, OFF_AT, ON_AT = BS + 26, BS + 31, BS + 33                # slot 1: -20 LUFS, then off, then on again (from the start)
LD_HIST = 2400


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
    """the output gain per session that brings the peak of its emitted float samples to 1.5, so that the limiter beside the loudness
    gain has work to do and the levels are far above the absolute gate"""
    conv = _conv(pool, gate=True, crossfade=True)
    waves = _tap(conv)
    _drive(conv, [dict(p, **e) for p, e in zip(SESS, EXTRA)], _rate_pcm(), BS + 12, CHUNKS)
    peak = [max(float(w[s, lo:lo + ln].abs().max()) for w in waves) for s, (lo, ln) in enumerate(SPANS)]
    assert all(p > 0 for p in peak)
    return [20.0 * np.log10(1.5 / p) for p in peak]


def _actions(graph_at=None):
    acts = {RETUNE_AT: [lambda c: c.set(1, lufs=-20.0)], OFF_AT: [lambda c: c.set(1, lufs=None)], ON_AT: [lambda c: c.set(1, lufs=-30.0)]}
    if graph_at is not None:
        acts.setdefault(graph_at, []).insert(0, lambda c: c.enable_graph())
    return acts


def _loud_run(pool, gains, graph_at=None):
    conv = _conv(pool, gate=True, crossfade=True, limiter=True, loudness=True, **LOUD_KW)
    sess = [dict(p, gain=g, **e, **lim, **lu) for p, g, e, lim, lu in zip(SESS, gains, EXTRA, LIM, LUFS)]
    rec = dict(state=[], read=[], captures=[])

    def after(c, tick):
        rec["state"].append(c.loud_state.cpu().numpy())
        rec["read"].append(c.loudness())
        rec["captures"].append(c.captures)
    outs = _drive(conv, sess, _rate_pcm(), TICKS, CHUNKS, actions=_actions(graph_at), after=after)
    return outs, rec, conv


@pytest.fixture(scope="module")
def runs(pool, gains):
    """the twin without loudness and limiter (gate and crossfade on, the same gains: outputs and full float waves), the converter with
    both, eager, over the same script, and what loudness_ref.stream followed by limit_ref.stream makes of the twin's waves: computed
    once"""
    twin = _conv(pool, gate=True, crossfade=True)
    waves = _tap(twin)
    want = _drive(twin, [dict(p, gain=g, **e) for p, g, e in zip(SESS, gains, EXTRA)], _rate_pcm(), TICKS, CHUNKS)
    got, rec, conv = _loud_run(pool, gains)
    ticks = list(range(BS, TICKS))
    d, P, z_abs, gmax, slew = MS.check_loudness_stream(LOUD_KW["loudness_half_life"], LOUD_KW["loudness_prior"], -70.0, 12.0,
                                                       LOUD_KW["loudness_slew_db"])
    row = lambda s, t: np.array([z_abs, R.z_of(t), d, P, gmax, MS.loudness_slew(slew, SPANS[s][1], RATES[s])])      # noqa: E731
    on, par = [], []
    for t in ticks:
        t1 = -30.0 if t < RETUNE_AT or t >= ON_AT else -20.0
        on.append(np.array([1, 0 if OFF_AT <= t < ON_AT else 1, 0]))
        par.append(np.stack([row(0, -16.0), row(1, t1), row(2, -23.0)]))
    w = [x.cpu().numpy() for x in waves]
    lo, ln = [s[0] for s in SPANS], [s[1] for s in SPANS]
    hops, coefs, _ = _filters(RATES)
    levelled, _, state = R.stream(w, lo, ln, on, hops, coefs, par)
    c1 = min(10.0 ** (-1.0 / 20.0), 32767 / 32768)
    limited, _, gmins, _ = LR.stream(levelled, lo, ln, CHUNKS, [80, 0, 0], [320, 0, 0], [c1, 1.0, 1.0], ld_hist=LD_HIST)
    pcm = [audio_io.float_to_pcm16(torch.from_numpy(f).to(DEV)).cpu().numpy() for f in limited]
    return dict(want=want, waves=w, got=got, rec=rec, conv=conv, ticks=ticks, levelled=levelled, pcm=pcm, state=state, gmins=gmins)


@pytest.mark.parametrize("graph", [False, True])
def test_a_loudness_converter_with_no_session_using_it_is_bitwise_the_plain_converter(pool, graph):
    ticks = BS + 4
    pcm = _rate_pcm()
    plain = _conv(pool)
    want = _drive(plain, SESS, pcm, ticks, CHUNKS)
    conv = _conv(pool, loudness=True)
    if graph:
        conv.enable_graph()
    got = _drive(conv, [dict(p, lufs=None) for p in SESS], pcm, ticks, CHUNKS)
    assert all(sum(o is not None for o in g) == ticks - BS for g in got) and all(_same(g, w) for g, w in zip(got, want))
    assert conv.loud_on.tolist() == [False] * 3 and conv.captures == int(graph) and conv.loudness() == [(-math.inf, 0.0)] * 3
    assert _bits_equal(conv.loud_state.cpu().numpy(), R.state0(3)) and conv.loud_state.shape == (3, 16)
    assert conv.span_lo.tolist() == [s[0] for s in SPANS] and conv.span_len.tolist() == [s[1] for s in SPANS]
    with pytest.raises(ValueError, match=r"slot 0: lufs=-23 needs a converter built with MultiStreamConverter\(..., loudness=True\)"):
        plain.set(0, lufs=-23)
    assert not hasattr(plain, "loud_state") and not hasattr(plain, "span_lo") and plain.params[0].get("lufs") is None
    with pytest.raises(ValueError, match="loudness needs a converter built with"):
        plain.loudness()
    before = {a: getattr(conv, a).clone() for a in ("loud_on", "loud_par", "loud_coef", "pitch", "seg_len")}
    for bad in (dict(lufs=float("nan")), dict(lufs="x"), dict(lufs=1, pitch=3.0), dict(lufs=-70)):
        with pytest.raises(ValueError, match="slot 1: lufs="):
            conv.set(1, **bad)
    assert all(torch.equal(getattr(conv, a), v) for a, v in before.items()) and conv.params[1]["pitch"] == 0.0


def test_every_emitted_chunk_is_the_restatement_of_the_twins_waves(runs):
    got, want, rec, conv = runs["got"], runs["want"], runs["rec"], runs["conv"]
    assert len(runs["waves"]) == TICKS - BS == len(rec["state"]) and conv.captures == 0
    changed = [0, 0, 0]
    for i, t in enumerate(runs["ticks"]):
        for s, (lo, ln) in enumerate(SPANS):
            o = got[s][t]
            assert o.shape == (ln,) and np.array_equal(o, runs["pcm"][i][s, lo:lo + ln]), (t, s)
            changed[s] += not np.array_equal(o, want[s][t])
        if i % 8 == 7:
            print(f"tick {t}: (LUFS, gain dB) {[('%.2f' % a, '%.2f' % b) for a, b in rec['read'][i]]}")
    assert _bits_equal(conv.loud_state.cpu().numpy(), runs["state"])
    # the cases are live: both sessions were counted and moved, the limiter had work, slot 2 is the twin's
    last = rec["state"][-1]
    assert last[0, 11] > 1.0 and last[0, R.G_SLOT] != 1.0 and rec["state"][OFF_AT - 1 - BS][1, R.G_SLOT] != 1.0
    assert changed[0] > 8 and changed[1] > 8
    assert changed[2] == 0 and _bits_equal(last[2], R.state0(1)[0]) and any(g[0] < 1.0 for g in runs["gmins"])
    # slot 1 while it was off: the twin's chunk, its state back at the start; switched on again it starts over
    assert np.array_equal(got[1][OFF_AT], want[1][OFF_AT]) and _bits_equal(rec["state"][OFF_AT - BS][1], R.state0(1)[0])
    assert rec["state"][ON_AT - BS][1][5] == SPANS[1][1] and rec["state"][ON_AT - BS][1][R.G_SLOT] == 1.0
    assert rec["state"][RETUNE_AT - BS][1][11] > 0                   # a retune keeps what the session has heard
    # the read-back is the state's
    lufs, db = rec["read"][-1][0]
    assert abs(lufs - R.running_lufs(last[0])) < 1e-9 and db == 20.0 * math.log10(last[0, R.G_SLOT]) and rec["read"][-1][2] == (-math.inf, 0.0)


def test_enable_graph_in_the_middle_and_retuning_leave_the_stream_unchanged_and_capture_once(pool, gains, runs):
    g_out, g_rec, conv = _loud_run(pool, gains, graph_at=BS + 3)
    assert all(_same(a, b) for a, b in zip(g_out, runs["got"]))
    assert all(_bits_equal(a, b) for a, b in zip(g_rec["state"], runs["rec"]["state"])) and g_rec["read"] == runs["rec"]["read"]
    # captured once: the retune, the switch off and the switch on never re-captured
    assert g_rec["captures"] == [0] * 3 + [1] * (TICKS - BS - 3) and conv.captures == 1
    conv.set(2, lufs=-18.0)
    conv.set(0, lufs=None)
    conv.step({s: np.zeros(c, np.int16) for s, c in enumerate(CHUNKS)})
    assert conv.captures == 1 and conv.loud_on.tolist() == [False, True, True] and conv.loud_hop.tolist()[1:] == [4410, 4800]
    assert _bits_equal(conv.loud_state[0].cpu().numpy(), R.state0(1)[0]) and conv.loud_state[2, 5].item() == 960.0
    conv.close(1)
    assert conv.loud_on.tolist() == [False, False, True] and _bits_equal(conv.loud_state[1].cpu().numpy(), R.state0(1)[0])
    conv.open(1, "v1", rate=48000, lufs=-23.0)
    assert conv.loud_on.tolist() == [False, True, True] and conv.loud_hop.tolist()[1] == 4800 and conv.loudness()[1] == (-math.inf, 0.0)
    assert _bits_equal(conv.loud_par[1].cpu().numpy(), np.array([*R.params(48000, 960, -23.0, half_life=1.0, prior=0.3, slew=40.0)]))


@pytest.mark.parametrize("graph", [False, True])
def test_the_bf16_repeat_restarts_from_the_state_the_tick_started_from(pool, monkeypatch, graph):
    """the repeat of a tick (after an fp16 saturation) with the switch of the process to bf16 planes stubbed out: the same tick again
    gives the same samples -- from the loudness state the tick started from, not the one its first attempt left"""
    monkeypatch.setattr(MS.ops, "switch_to_bf16", lambda *a: None)
    ticks = BS + 22
    pcm = _pcm(CHUNK * ticks, 80)
    conv = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=CHUNK, buffersize=BS, k=4, loudness=True, **LOUD_KW)
    conv.open(0, "v0", gain=40.0, lufs=-30.0)
    if graph:
        conv.enable_graph()
    for t in range(ticks):
        if t == ticks - 1:
            saved = conv.phi.clone(), conv._seam_state()
        out = conv.step({0: pcm[t * CHUNK:(t + 1) * CHUNK]})[0]
    after = conv.loud_state.clone()
    assert saved[1][0] is None and saved[1][2] is None and not torch.equal(saved[1][4], after)
    assert after[0, 11].item() > 0 and after[0, R.G_SLOT].item() != 1.0 and after[0, R.G_SLOT].item() != saved[1][4][0, R.G_SLOT].item()
    lo, ln = conv._span(CHUNK)
    again = conv._repeat_on_bf16(saved[0], None, None, saved[1])
    assert np.array_equal(again[0, lo:lo + ln], out) and torch.equal(conv.loud_state, after)


def test_with_another_output_rate_the_filter_and_the_sub_block_are_the_output_rates(pool):
    """input_sr != output_sr: step() cuts chunk samples of the 48 kHz wave, and they are measured as 48 kHz audio (H = 4800)"""
    ticks = BS + 64                                                  # 64 spans of 320 samples: four sub-blocks and a bit
    pcm = _pcm(CHUNK * ticks, 85)
    kw = dict(chunk=CHUNK, buffersize=BS, k=4, input_sr=16000, output_sr=48000)
    twin = MS.MultiStreamConverter(*_nets(), pool, 1, **kw)
    waves = _tap(twin)
    want = _drive(twin, [dict(voice="v0", gain=40.0)], [pcm], ticks, [CHUNK])[0]
    conv = MS.MultiStreamConverter(*_nets(), pool, 1, loudness=True, **dict(LOUD_KW, loudness_prior=0.1), **kw)
    got = _drive(conv, [dict(voice="v0", gain=40.0, lufs=-30.0)], [pcm], ticks, [CHUNK])[0]
    lo, ln = conv._span(CHUNK)
    assert conv.loud_hop.tolist() == [4800] and (conv.span_lo.tolist(), conv.span_len.tolist()) == ([lo], [ln]) and ln == CHUNK
    par = R.params(48000, ln, -30.0, half_life=1.0, prior=0.1, slew=40.0)
    assert _bits_equal(conv.loud_par.cpu().numpy(), par[None]) and _bits_equal(conv.loud_coef.cpu().numpy(), R.coefficients(48000)[None])
    levelled, _, state = R.stream([w.cpu().numpy() for w in waves], [lo], [ln], [1], [4800], [R.coefficients(48000)], par[None])
    assert _bits_equal(conv.loud_state.cpu().numpy(), state) and state[0, 11] > 0 and state[0, R.G_SLOT] != 1.0
    changed = 0
    for i, t in enumerate(range(BS, ticks)):
        pcm16 = audio_io.float_to_pcm16(torch.from_numpy(levelled[i]).to(DEV)).cpu().numpy()
        assert np.array_equal(got[t], pcm16[0, lo:lo + ln]), t
        changed += not np.array_equal(got[t], want[t])
    assert changed >= 3


def test_a_sparse_converters_stalled_slot_stands_still_and_its_stream_depends_on_its_chunks_alone(pool):
    ticks = BS + 24
    pcm = [_pcm(CHUNK * ticks, 90 + s) for s in range(2)]
    stalls = {1: {BS + 3, BS + 4, BS + 15}}
    outs = {}
    for stalled in (False, True):
        conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, sparse=True, loudness=True, **LOUD_KW)
        for s in range(2):
            conv.open(s, f"v{s}", gain=40.0, lufs=-28.0)
        sent, got, tick = [0, 0], [[], []], 0
        while min(sent) < ticks:
            feed = {}
            for s in range(2):
                if sent[s] < ticks and not (stalled and tick in stalls.get(s, ())):
                    feed[s] = pcm[s][sent[s] * CHUNK:(sent[s] + 1) * CHUNK]
                    sent[s] += 1
            before = conv.loud_state.clone()
            res = conv.step(feed)
            for s, o in res.items():
                if o is not None:
                    got[s].append(o)
            for s in range(2):
                if s not in feed:                                    # it sat the tick out: nothing of its state moved
                    assert torch.equal(conv.loud_state[s], before[s]), (tick, s)
            tick += 1
        outs[stalled] = [np.concatenate(g) for g in got], conv.loud_state.cpu().numpy()
        assert conv.loud_state[1, 11].item() > 0 and conv.loud_state[1, R.G_SLOT].item() != 1.0
    assert all(np.array_equal(a, b) for a, b in zip(outs[False][0], outs[True][0])) and _bits_equal(outs[False][1], outs[True][1])
    assert len(outs[True][0][1]) == CHUNK * (ticks - BS)


# ---------------------------------------------------------------------------------------------------- 4. the CLIs
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


def test_multistream_cli_with_a_normalised_session_writes_what_the_converter_emits(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    ticks = BS + 30
    wav = _pcm(CHUNK * ticks, 80).astype(np.float32) / 32767
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    base = [dict(input="in0.wav", lib="voice_library.pt", gain=40), dict(input="in1.wav", lib="voice_library.pt", gain=40)]
    json.dump([dict(base[0], lufs=-30), base[1]], open(d / "loud.json", "w"))
    json.dump(base, open(d / "plain.json", "w"))
    json.dump([base[0], dict(base[1], lufs=None)], open(d / "null.json", "w"))
    common = nets + ["-c", str(CHUNK), "-b", str(BS)]
    tune = ["--loudness-half-life", "1", "--loudness-prior", "0.3", "--loudness-slew", "40"]
    msi.main(common + tune + ["-o", str(d / "out_loud"), str(d / "loud.json")])
    msi.main(common + ["-o", str(d / "out_plain"), str(d / "plain.json")])
    msi.main(common + tune + ["-o", str(d / "out_flag"), "-lufs", "-30", str(d / "null.json")])
    ss = msi.load_sessions(str(d / "loud.json"))
    assert ss[0]["lufs"] == -30.0 and "lufs" not in ss[1]

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
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4, loudness=True, **LOUD_KW)
    want_loud = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, gain=40.0, lufs=-30.0), dict(voice=name, gain=40.0)])
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4)
    want_plain = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, gain=40.0), dict(voice=name, gain=40.0)])
    loud, plain, flag = read("out_loud"), read("out_plain"), read("out_flag")
    assert all(len(w) == CHUNK * (ticks - BS) for w in want_loud + want_plain)
    assert np.array_equal(loud[0], want_loud[0]) and np.array_equal(loud[1], want_loud[1])
    # a file without the key, run without the flag: what the converter built without loudness writes, byte for byte
    assert np.array_equal(plain[0], want_plain[0]) and np.array_equal(plain[1], want_plain[1])
    assert np.array_equal(loud[1], plain[1]) and not np.array_equal(loud[0], plain[0])
    # -lufs as the default, switched off by a session's null: the same input twice, so the outputs swap roles
    assert np.array_equal(flag[0], loud[0]) and np.array_equal(flag[1], plain[1])


def test_offline_clis_with_a_target_write_normalize_loudness_of_what_they_wrote_without(tmp_path):
    import batch_inference as BI
    import inference as INF
    d = tmp_path
    nets = _save_nets(d)
    lib = synthetic.make_library(512, 5)
    torch.save({"tokens": lib}, d / "voice_library.pt")
    os.makedirs(d / "inputs")
    wav = synthetic.make_waveform(24000, 91) * 0.5                   # 1 s mono at 24 kHz
    audio_io.save(str(d / "inputs" / "utt.wav"), wav, 24000)
    base = ["-i", str(d / "inputs"), "-lib", str(d / "voice_library.pt"), "-d", "cuda", "-c", "4800", "-g", "20"] + nets
    INF.main(base + ["-o", str(d / "out_plain")])
    INF.main(base + ["-o", str(d / "out_loud"), "-lufs", "-23", "--loudness-max-db", "40"])
    INF.main(base + ["-o", str(d / "out_both"), "-lufs", "-23", "--loudness-max-db", "40", "-lim", "-12"])
    plain, sr = audio_io.load(str(d / "out_plain" / "0_utt.wav"))
    loud, sr2 = audio_io.load(str(d / "out_loud" / "0_utt.wav"))
    both = audio_io.load(str(d / "out_both" / "0_utt.wav"))[0]
    assert sr == sr2 == 24000
    want, db = MS.normalize_loudness(plain.to(DEV), None, -23.0, 24000, 40.0, return_gain=True)
    assert torch.equal(loud, want.cpu()) and not torch.equal(loud, plain) and 0 < abs(db[0]) < 40.0
    level = MS.measure_loudness(loud.to(DEV), None, 24000)[0][0]
    print("inference.py: gain %.2f dB, the output reads %.3f LUFS" % (db[0], level))
    assert abs(level + 23.0) < 0.05
    # before -lim: the limiter sees the levelled file
    assert torch.equal(both, MS.limit_waves(loud.to(DEV), None, -12.0, 5.0, 20.0, 24000).cpu())
    # batch_inference.py: a job with "lufs" beside the same job without; -lufs as the default with a null
    jobs = [dict(input="inputs/utt.wav", lib="voice_library.pt", gain=20, output="b_plain.wav"),
            dict(input="inputs/utt.wav", lib="voice_library.pt", gain=20, lufs=-16, output="b_loud.wav")]
    (d / "jobs.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs.json"), "-c", "4800", "--loudness-max-db", "40"] + nets)
    b_plain, b_loud = audio_io.load(str(d / "b_plain.wav"))[0], audio_io.load(str(d / "b_loud.wav"))[0]
    assert torch.equal(b_loud, MS.normalize_loudness(b_plain.to(DEV), None, -16.0, 24000, 40.0).cpu()) and not torch.equal(b_loud, b_plain)
    assert abs(MS.measure_loudness(b_loud.to(DEV), None, 24000)[0][0] + 16.0) < 0.05
    jobs = [dict(jobs[0], lufs=None, output="c_plain.wav"), dict(jobs[0], output="c_loud.wav")]
    (d / "jobs2.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs2.json"), "-c", "4800", "-lufs", "-16", "--loudness-max-db", "40"] + nets)
    assert torch.equal(audio_io.load(str(d / "c_plain.wav"))[0], b_plain) and torch.equal(audio_io.load(str(d / "c_loud.wav"))[0], b_loud)
