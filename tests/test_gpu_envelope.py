"""The envelope follow on the device (csrc/envelope.hip) and through the converters and CLIs, against the NumPy restatement
tools/envelope_ref.py.  Every comparison is bitwise, or equality of int16 streams.

1. alive_envelope_waves alone: one call at hop 8 (radius 0, 1 and 4) and one at hop 320, each with ld_x != ld_y and strides that are no
   multiple of 4 (rows on and off a 16-byte boundary: both load forms); lengths 0, 1, hop / 2, hop / 2 + 1, TILE hop - 1, TILE hop,
   TILE hop + 1, 3 TILE hop + 7 and one beyond the stride; amounts 0, 0.25, 1, 1.5 and NaN; a NaN in y and both infinities in x on and
   beside a tile border; a silent source; ratios beyond both ends of the range; out and gain_minmax between guard bands.
2. follow_envelope on a [3, 5 TILE 320 + 11] batch with lens.
3. MultiStreamConverter(envelope=True): all sessions at 0 -> bitwise the plain converter; following sessions at two rates with gate,
   crossfade and limiter on -> every tick's enveloped wave is the restatement of a twin's ring and decoder wave; enable_graph in the
   middle, retuning, off and on without re-capture; envelope_db(); a sparse converter with a stalled tick.
4. RealtimeConverter(envelope=A): bitwise a one-slot MultiStreamConverter, with and without interior reuse.
5. inference.py -env, batch_inference.py with an "envelope" job, multistream_inference.py with the key on one session."""
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

import envelope_ref as ER                                            # noqa: E402
from module import audio_io, synthetic                               # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 16                                                             # guard band, elements on each side of every output
TILE = MS.ENVELOPE_TILE
E, G_LO, G_HI = ER.constants()


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


# ---------------------------------------------------------------------------------------------------- 1. the kernel alone
NONFINITE, SILENT, BOTH_ENDS = 14, 15, 16


def _kernel_case(hop, ld_x_extra):
    """-> (y [N, ld_y], x [N, ld_x], lens, amounts)"""
    ld_y = 3 * TILE * hop + 7
    ld_x = ld_y + ld_x_extra
    cap = min(ld_y, ld_x)
    lens = [0, 1, hop // 2, hop // 2 + 1, TILE * hop - 1, TILE * hop, TILE * hop + 1, cap, ld_y + 100,      # (the last: clamped)
            cap, cap, cap, 2 * TILE * hop + 3, TILE * hop + hop // 2, cap, cap, cap]
    amounts = [1.0, 1.0, 0.25, 1.0, 1.0, 0.25, 1.0, 1.0, 0.25,
               0.0, 1.5, float("nan"), 0.25, 1.0, 1.0, 1.0, 1.0]
    n = len(lens)
    rng = np.random.default_rng(1000 + hop)
    t = np.arange(max(ld_y, ld_x))
    y = (rng.standard_normal((n, ld_y)) * 0.1).astype(np.float32)
    x = (rng.standard_normal((n, ld_x)) * (0.02 + 0.3 * (1 + np.sin(2 * np.pi * t[:ld_x] / (37.0 * hop))))).astype(np.float32)
    y[2, 3], y[2, 4] = 0.0, -0.0
    b = TILE * hop                                                   # a tile border
    y[NONFINITE, b] = np.nan                                         # the first sample of frame TILE
    x[NONFINITE, 2 * b - 1] = np.inf                                 # the last sample of frame 2 TILE - 1
    x[NONFINITE, 2 * b + hop] = -np.inf                              # frame 2 TILE + 1: beside the border
    x[SILENT] = 0.0
    x[BOTH_ENDS, :cap // 2] = y[BOTH_ENDS, :cap // 2] * np.float32(10.0)
    x[BOTH_ENDS, cap // 2:cap] = y[BOTH_ENDS, cap // 2:cap] * np.float32(0.01)
    return y, x, lens, amounts


def _call(out, y, x, lens, amount, hop, radius, mm):
    return MS.nat.lib().alive_envelope_waves(out.data_ptr(), y.data_ptr(), y.shape[1], x.data_ptr(), x.shape[1], y.shape[0],
                                             None if lens is None else lens.data_ptr(), amount.data_ptr(), hop, radius, E, G_LO, G_HI,
                                             None if mm is None else mm.data_ptr(), MS.nat.stream())


@pytest.mark.parametrize("hop,radius,ld_x_extra", [(8, 0, 5), (8, 1, 5), (8, 4, 5), (320, 1, -3)])
def test_the_kernel_against_the_restatement(hop, radius, ld_x_extra):
    wave, src, lens, amounts = _kernel_case(hop, ld_x_extra)
    n, ld_y = wave.shape
    assert ld_y % 4 and src.shape[1] != ld_y
    y, x = _dev(wave, torch.float32), _dev(src, torch.float32)
    out = Guarded((n, ld_y), torch.float32, 123.0)
    mm = Guarded((n, 2), torch.float32, -5.0)
    lens_d, amount_d = _dev(lens, torch.int32), _dev(amounts, torch.float32)
    assert _call(out.view, y, x, lens_d, amount_d, hop, radius, mm.view) == 0
    torch.cuda.synchronize()
    assert out.intact() and mm.intact()
    assert _bits_equal(y.cpu().numpy(), wave) and _bits_equal(x.cpu().numpy(), src)
    want, G, want_mm = ER.envelope_waves(wave, src, lens, amounts, hop=hop, radius=radius)
    got, got_mm = out.view.cpu().numpy(), mm.view.cpu().numpy()
    cap = min(ld_y, src.shape[1])
    for r in range(n):
        assert _bits_equal(got[r], want[r]), r
        assert got_mm[r].tolist() == want_mm[r].tolist(), r
        ln = min(max(lens[r], 0), cap)
        assert _bits_equal(got[r, ln:], wave[r, ln:]), r
    for r in (0, 9, 10, 11):                                         # no samples, amount 0, 1.5 and NaN: copied, (1, 1)
        assert _bits_equal(got[r], wave[r]) and got_mm[r].tolist() == [1.0, 1.0] and G[r] is None
    assert len(G[8]) == -(-cap // hop) and not _bits_equal(got[8], wave[8])          # the length beyond the stride was clamped
    # the non-finite row: exactly the frames within `radius` of the three samples at unity, the row finite but for the NaN itself
    f_touched = sorted({f for c in (TILE, 2 * TILE - 1, 2 * TILE + 1) for f in range(c - radius, c + radius + 1)})
    assert np.all(G[NONFINITE][f_touched] == 1.0) and np.sum(G[NONFINITE] == 1.0) == len(f_touched)
    assert np.isnan(got[NONFINITE, TILE * hop]) and np.isfinite(np.delete(got[NONFINITE], TILE * hop)).all()
    assert np.all(G[SILENT] == G_LO) and got_mm[SILENT].tolist() == [float(np.float32(G_LO))] * 2
    assert G[BOTH_ENDS].min() == G_LO and G[BOTH_ENDS].max() == G_HI
    assert got_mm[BOTH_ENDS].tolist() == [float(np.float32(G_LO)), float(np.float32(G_HI))]
    # without gain_minmax and without len (the whole row, clamped to the shorter stride): the same samples
    again = Guarded((n, ld_y), torch.float32, 123.0)
    assert _call(again.view, y, x, _dev([ld_y + 9] * n, torch.int32), amount_d, hop, radius, None) == 0
    none = Guarded((n, ld_y), torch.float32, 123.0)
    assert _call(none.view, y, x, None, amount_d, hop, radius, None) == 0
    torch.cuda.synchronize()
    assert again.intact() and none.intact() and _bits_equal(again.view.cpu().numpy(), none.view.cpu().numpy())
    assert _bits_equal(none.view.cpu().numpy(), ER.envelope_waves(wave, src, None, amounts, hop=hop, radius=radius)[0])
    # a row's result depends on nothing but the row: one row alone, at another place in memory
    for r in (7, 12):
        one = MS.envelope_waves_(torch.empty(1, ld_y, device=DEV), y[r:r + 1].clone(), x[r:r + 1].clone(), lens_d[r:r + 1].clone(),
                                 amount_d[r:r + 1].clone(), hop, radius, E, G_LO, G_HI)
        assert _bits_equal(one[0].cpu().numpy(), got[r]), r
    # out must not overlap y or x
    assert _call(y, y, x, lens_d, amount_d, hop, radius, None) == -1 and b"overlaps y" in MS.nat.lib().alive_last_error()
    assert _call(x, y, x, lens_d, amount_d, hop, radius, None) == -1
    assert b"overlaps x" in MS.nat.lib().alive_last_error()
    with pytest.raises(ValueError, match="overlaps"):
        MS.envelope_waves_(y, y, x, lens_d, amount_d, hop, radius, E, G_LO, G_HI)


# ---------------------------------------------------------------------------------------------------- 2. follow_envelope
def test_follow_envelope_against_the_restatement():
    ld = 5 * TILE * 320 + 11
    rng = np.random.default_rng(7)
    t = np.arange(ld + 13)
    wave = (rng.standard_normal((3, ld)) * 0.2).astype(np.float32)
    src = (rng.standard_normal((3, ld + 13)) * (0.01 + 0.2 * (1 + np.sin(2 * np.pi * t / 9000.0)))).astype(np.float32)
    lens, amounts = [ld, 12345, 7], [1.0, 0.5, 0.8]
    y, x = _dev(wave, torch.float32), _dev(src, torch.float32)
    out = MS.follow_envelope(y, x, lens, amounts)
    want = ER.envelope_waves(wave, src, lens, amounts)[0]
    assert out is not y and out.shape == y.shape and _bits_equal(out.cpu().numpy(), want) and not _bits_equal(want, wave)
    assert _bits_equal(y.cpu().numpy(), wave) and _bits_equal(x.cpu().numpy(), src)
    # one row, lens None (as many samples as both hold), the tuning values
    one = MS.follow_envelope(y[0], x[0, :20000], None, 0.6, -50.0, 6.0, 2)
    assert one.shape == (ld,)
    assert _bits_equal(one.cpu().numpy(), ER.envelope_waves(wave[:1], src[:1, :20000], None, 0.6, radius=2, floor_db=-50.0, range_db=6.0)[0][0])
    assert _bits_equal(MS.follow_envelope(y, x, None, 0.0).cpu().numpy(), wave)
    with pytest.raises(ValueError, match=r"envelope=2 must be"):
        MS.follow_envelope(y, x, None, 2)
    with pytest.raises(ValueError, match="2 amounts for 3 rows"):
        MS.follow_envelope(y, x, None, [1.0, 0.5])


# ---------------------------------------------------------------------------------------------------- 3. the converter
CHUNK, BS = 160, 16
RATES = [16000, 44100]
CHUNKS = [160, 441, 160]
SESS = [dict(voice="v0", pitch=1.0, rate=16000), dict(voice="v1", alpha=0.1, rate=44100), dict(voice="v2", f0_rate=0.9, rate=16000)]
EXTRA = [dict(gate_db=-40, gate_hold=0.0, crossfade_ms=5, limit_db=-1.0), dict(crossfade_ms=5, limit_db=-3.0), dict()]
ENV = [0.8, 0.5, 0.0]
TICKS = BS + 12
GRAPH_AT, RETUNE_AT, OFF_AT, ON_AT = BS + 3, BS + 5, BS + 7, BS + 9


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    return MS.VoicePool(voices)


def _rate_pcm():
    """inputs whose level moves: each session's chunks scaled by a slow ramp, and a silence for slot 0's gate"""
    pcm = []
    for s, c in enumerate(CHUNKS):
        p = _pcm(c * TICKS, 70 + s).astype(np.float64)
        p *= 0.15 + 0.85 * np.abs(np.sin(np.arange(len(p)) * (2 * np.pi / (c * 9.0))))
        pcm.append(p.astype(np.int16))
    pcm[0][(BS + 10) * CHUNK:(BS + 11) * CHUNK] = 0
    return pcm


def _conv(pool, **kw):
    return MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, rates=RATES, **kw)


def _drive(conv, sess, pcm, ticks, chunks, actions=None, after=None):
    outs = [[] for _ in sess]
    for s, p in enumerate(sess):
        conv.open(s, **p)
    for tick in range(ticks):
        for a in (actions or {}).get(tick, []):
            a(conv)
        res = conv.step({s: pcm[s][tick * c:(tick + 1) * c] for s, c in enumerate(chunks)})
        for s in range(len(sess)):
            outs[s].append(res[s])
        if after is not None and any(r is not None for r in res.values()):
            after(conv, tick)
    return outs


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("graph", [False, True])
def test_an_envelope_converter_with_every_session_at_zero_is_bitwise_the_plain_converter(pool, graph):
    ticks = BS + 3
    pcm = _rate_pcm()
    plain = _conv(pool)
    want = _drive(plain, SESS, pcm, ticks, CHUNKS)
    conv = _conv(pool, envelope=True)
    if graph:
        conv.enable_graph()
    got = _drive(conv, [dict(p, envelope=0.0) for p in SESS], pcm, ticks, CHUNKS)
    assert all(sum(o is not None for o in g) == ticks - BS for g in got) and all(_same(g, w) for g, w in zip(got, want))
    assert conv.env_amount.tolist() == [0.0] * 3 and conv.captures == int(graph) and conv.envelope_db() == [(0.0, 0.0)] * 3
    assert conv._env_out is not None and conv._env == (E, G_LO, G_HI, 1)
    with pytest.raises(ValueError, match=r"slot 0: envelope=0.5 needs a converter built with MultiStreamConverter\(..., envelope=True\)"):
        plain.set(0, envelope=0.5)
    assert not hasattr(plain, "env_amount") and plain.params[0].get("envelope") == 0.0
    with pytest.raises(ValueError, match="envelope_db needs a converter built with"):
        plain.envelope_db()
    before = {a: getattr(conv, a).clone() for a in ("env_amount", "pitch", "seg_len")}
    for bad in (dict(envelope=float("nan")), dict(envelope="x"), dict(envelope=1.5, pitch=3.0)):
        with pytest.raises(ValueError, match="slot 1: envelope="):
            conv.set(1, **bad)
    assert all(torch.equal(getattr(conv, a), v) for a, v in before.items()) and conv.params[1]["pitch"] == 0.0


@pytest.fixture(scope="module")
def twin(pool):
    """a converter with gate, crossfade and limiter on and no envelope, eager: per running tick its 16 kHz rings, its decoder waves
    and its outputs.  Computed once"""
    rec = dict(data=[], wave=[])
    conv = _conv(pool, gate=True, crossfade=True, limiter=True)
    dec, spectrogram = conv.dec, MS.spectrogram

    def tapped_dec(*a, **k):
        wave, phi = dec(*a, **k)
        rec["wave"].append(wave.clone())
        return wave, phi

    def tapped_spectrogram(data):
        rec["data"].append(data.clone())
        return spectrogram(data)
    conv.dec = tapped_dec
    MS.spectrogram = tapped_spectrogram
    try:
        outs = _drive(conv, [dict(p, **e) for p, e in zip(SESS, EXTRA)], _rate_pcm(), TICKS, CHUNKS)
    finally:
        MS.spectrogram = spectrogram
    assert len(rec["data"]) == len(rec["wave"]) == TICKS - BS
    return dict(outs=outs, data=[d.cpu().numpy() for d in rec["data"]], wave=[w.cpu().numpy() for w in rec["wave"]])


def _amounts(tick):
    a0 = ENV[0] if tick < RETUNE_AT else (0.3 if tick < OFF_AT else (0.0 if tick < ON_AT else 1.0))
    return [a0, ENV[1], ENV[2]]


def test_every_ticks_enveloped_wave_is_the_restatement_of_the_twins_ring_and_decoder_wave(pool, twin):
    conv = _conv(pool, gate=True, crossfade=True, limiter=True, envelope=True)
    rec = dict(env=[], db=[], captures=[], ptr=[])

    def after(c, tick):
        rec["env"].append(c._env_out.cpu().numpy())
        rec["db"].append(c.envelope_db())
        rec["captures"].append(c.captures)
        rec["ptr"].append(c._env_out.data_ptr())
    actions = {GRAPH_AT: [lambda c: c.enable_graph()], RETUNE_AT: [lambda c: c.set(0, envelope=0.3)],
               OFF_AT: [lambda c: c.set(0, envelope=0.0)], ON_AT: [lambda c: c.set(0, envelope=1.0)]}
    sess = [dict(p, envelope=a, **e) for p, a, e in zip(SESS, ENV, EXTRA)]
    outs = _drive(conv, sess, _rate_pcm(), TICKS, CHUNKS, actions=actions, after=after)
    assert len(rec["env"]) == TICKS - BS
    moved = [0, 0, 0]
    for i, tick in enumerate(range(BS, TICKS)):
        data, wave = twin["data"][i], twin["wave"][i]
        assert data.shape[1] == 2560 and wave.shape[1] == 2560
        want, G, mm = ER.envelope_waves(wave, data, None, _amounts(tick))
        assert _bits_equal(rec["env"][i], want), tick
        assert rec["db"][i] == MS.minmax_db(mm.tolist()) == ER.gain_db(mm), tick
        for s in range(3):
            moved[s] += not _bits_equal(want[s], wave[s])
            if _amounts(tick)[s] == 0:
                assert _bits_equal(rec["env"][i][s], wave[s]) and rec["db"][i][s] == (0.0, 0.0)
        print(f"tick {tick}: envelope_db {[('%.2f' % a, '%.2f' % b) for a, b in rec['db'][i]]}")
    assert moved == [TICKS - BS - (ON_AT - OFF_AT), TICKS - BS, 0]
    # the session that does not follow emits what the twin's emits; the others differ; the limiter downstream still holds
    assert _same(outs[2], twin["outs"][2]) and not _same(outs[0], twin["outs"][0]) and not _same(outs[1], twin["outs"][1])
    top = int(np.floor(np.float32(10 ** -0.05) * 32768))
    assert all(np.abs(o.astype(np.int32)).max() <= top for o in outs[0] if o is not None)
    # captured once; retuning, off and on never re-captured, and the enveloped wave stays in the buffer allocated once
    assert rec["captures"] == [0] * (GRAPH_AT - BS) + [1] * (TICKS - GRAPH_AT) and conv.captures == 1
    assert len(set(rec["ptr"])) == 1
    conv.close(1)
    assert conv.env_amount.tolist() == [1.0, 0.0, 0.0] and conv.envelope_db()[1] == (0.0, 0.0)
    conv.open(1, "v1", rate=16000, envelope=0.25)
    assert conv.env_amount.tolist() == [1.0, 0.25, 0.0] and conv.captures == 1


def test_a_sparse_converter_with_a_stalled_tick_emits_the_same_stream(pool):
    """slot 1 sits one tick out: its ring stands still, and its stream is what it is without the stall, one tick later"""
    ticks, stall = BS + 5, BS + 2
    pcm = [_pcm(CHUNK * ticks, 50 + s) for s in range(2)]

    def run(stalled):
        conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, sparse=True, envelope=True, crossfade=True)
        conv.open(0, "v0", envelope=0.6, crossfade_ms=5)
        conv.open(1, "v1", envelope=1.0, crossfade_ms=5)
        outs, at, dbs = [[], []], [0, 0], []
        for tick in range(ticks + (1 if stalled else 0)):
            feed = {}
            for s in range(2):
                if at[s] < ticks and not (stalled and s == 1 and tick == stall):
                    feed[s] = pcm[s][at[s] * CHUNK:(at[s] + 1) * CHUNK]
                    at[s] += 1
            res = conv.step(feed)
            for s, o in res.items():
                if o is not None:
                    outs[s].append(o)
            if 1 in feed and res[1] is not None:
                dbs.append(conv.envelope_db()[1])
        return outs, dbs
    a, db_a = run(False)
    b, db_b = run(True)
    assert len(a[1]) == ticks - BS and all(np.array_equal(p, q) for p, q in zip(a[1], b[1])) and len(a[1]) == len(b[1])
    assert len(a[0]) == len(b[0]) and all(np.array_equal(p, q) for p, q in zip(a[0], b[0]))
    assert db_a == db_b and all(lo != 0.0 or hi != 0.0 for lo, hi in db_a)


# ---------------------------------------------------------------------------------------------------- 4. RealtimeConverter
@pytest.mark.parametrize("graph", [False, True])
def test_a_following_realtime_converter_is_bitwise_a_one_slot_multistream(graph):
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(400, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    env = dict(envelope_floor_db=-50.0, envelope_range_db=9.0, envelope_radius=2)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, reuse_interior=False, envelope=0.7, **env,
                           **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, envelope=True, **env, **kw)
    ms.open(0, "lib", pitch=1.5, alpha=0.2, input_gain=-3.0, envelope=0.7)
    plain = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, reuse_interior=False, **kw)
    assert rt.envelope is True and plain.envelope is False and not hasattr(plain, "_env_out")
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    ticks, differ = BS + 4, 0
    pcm = _rate_pcm()[0][:CHUNK * ticks]
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b, p = rt.step(c), ms.step({0: c})[0], plain.step(c)
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b) and torch.equal(rt._env_out, ms._env_out), t
            assert ms.envelope_db()[0] != (0.0, 0.0)
            differ += not np.array_equal(a, p)
    assert differ == ticks - BS and rt._env == ms._env == MS.check_envelope(0.7, -50.0, 9.0, 2)[1:]


def test_a_following_realtime_converter_with_interior_reuse_is_bitwise_itself_without():
    """-c 960 -b 26: a ring of 78 frames advancing by 3; the envelope runs in both step forms"""
    from module.realtime import RealtimeConverter
    chunk, bs, ticks = 960, 26, 29
    lib = synthetic.make_library(400, 1)
    pcm = _pcm(chunk * ticks, 95)
    outs = {}
    for reuse in (False, "auto", None):                              # (None: the converter without the envelope)
        rt = RealtimeConverter(*_nets(), lib, "cuda", chunk=chunk, buffersize=bs, k=4, alpha=0.1, reuse_interior=bool(reuse) and reuse,
                               envelope=0.0 if reuse is None else 1.0)
        assert rt.reuse == bool(reuse)
        outs[reuse] = [o for o in (rt.step(pcm[t * chunk:(t + 1) * chunk]) for t in range(ticks)) if o is not None]
    assert len(outs[False]) == ticks - bs and all(np.array_equal(a, b) for a, b in zip(outs[False], outs["auto"]))
    assert not any(np.array_equal(a, b) for a, b in zip(outs[False], outs[None]))


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


def test_offline_clis_with_an_envelope_write_follow_envelope_of_the_conversion(tmp_path, monkeypatch):
    import batch_inference as BI
    import inference as INF
    from module.pipeline import Converter
    monkeypatch.setenv("ALIVE_KNN_STRICT", "0")                       # (inference.py --knn-strict sets it; restored after the test)
    d = tmp_path
    nets = _save_nets(d)
    lib = synthetic.make_library(512, 5)
    torch.save({"tokens": lib}, d / "voice_library.pt")
    os.makedirs(d / "inputs")
    wav = synthetic.make_waveform(24000, 91) * 0.5                   # 1 s mono at 24 kHz, its second half 20 dB down
    wav[:, 12000:] *= 0.1
    audio_io.save(str(d / "inputs" / "utt.wav"), wav, 24000)
    base = ["-i", str(d / "inputs"), "-lib", str(d / "voice_library.pt"), "-d", "cuda", "-c", "4800", "-g", "3"] + nets
    tune = ["--envelope-floor", "-50", "--envelope-range", "9", "--envelope-radius", "2"]
    INF.main(base + ["-o", str(d / "out_env"), "-env", "0.7"] + tune)
    env, sr = audio_io.load(str(d / "out_env" / "0_utt.wav"))
    # the same file through Converter.convert: follow_envelope at 16 kHz against the source the converter saw, then resample and gain
    CE, PE, Dec = _loaded_nets(d)
    wf = audio_io.resample(audio_io.load(str(d / "inputs" / "utt.wav"))[0].to(DEV), 24000, 16000)
    wf = (wf / wf.abs().max()).mean(dim=0, keepdim=True)
    out = Converter(CE, PE, Dec, DEV).set_library(lib.to(DEV)).convert(wf, chunk=4800, k=4, alpha=0.0, pitch_shift=0, world_pitch=False,
                                                                      intonation=1.0, f0_rate=1.0, window_batch=64, trim_context=True,
                                                                      share_overlap="auto")
    followed = MS.follow_envelope(out, wf, None, 0.7, -50.0, 9.0, 2)
    assert sr == 24000 and torch.equal(env, audio_io.resample(followed, 16000, 24000, post_gain_db=3.0).cpu())
    assert not torch.equal(followed, out)
    want = ER.envelope_waves(out.cpu().numpy(), wf.cpu().numpy(), None, 0.7, radius=2, floor_db=-50.0, range_db=9.0)[0]
    assert _bits_equal(followed.cpu().numpy(), want)
    # batch_inference.py: a job with "envelope" writes the file of inference.py --knn-strict -env; -env as the default with a null
    INF.main(base + ["-o", str(d / "out_strict"), "-env", "0.7", "--knn-strict"] + tune)
    INF.main(base + ["-o", str(d / "out_strict_plain"), "--knn-strict"])
    strict, plain = audio_io.load(str(d / "out_strict" / "0_utt.wav"))[0], audio_io.load(str(d / "out_strict_plain" / "0_utt.wav"))[0]
    job = dict(input="inputs/utt.wav", lib="voice_library.pt", gain=3)
    jobs = [dict(job, output="b_plain.wav"), dict(job, envelope=0.7, output="b_env.wav")]
    (d / "jobs.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs.json"), "-c", "4800"] + tune + nets)
    assert torch.equal(audio_io.load(str(d / "b_env.wav"))[0], strict) and torch.equal(audio_io.load(str(d / "b_plain.wav"))[0], plain)
    assert not torch.equal(strict, plain)
    jobs = [dict(job, envelope=None, output="c_plain.wav"), dict(job, output="c_env.wav")]
    (d / "jobs2.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs2.json"), "-c", "4800", "-env", "0.7"] + tune + nets)
    assert torch.equal(audio_io.load(str(d / "c_env.wav"))[0], strict) and torch.equal(audio_io.load(str(d / "c_plain.wav"))[0], plain)


def test_multistream_cli_with_a_following_session_leaves_the_others_unchanged(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    ticks = BS + 5
    wav = _rate_pcm()[0][:CHUNK * ticks].astype(np.float32) / 32767
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    base = [dict(input="in0.wav", lib="voice_library.pt"), dict(input="in1.wav", lib="voice_library.pt")]
    json.dump([dict(base[0], envelope=0.7), base[1]], open(d / "env.json", "w"))
    json.dump(base, open(d / "plain.json", "w"))
    json.dump([base[0], dict(base[1], envelope=None)], open(d / "null.json", "w"))
    common = nets + ["-c", str(CHUNK), "-b", str(BS)]
    msi.main(common + ["-o", str(d / "out_env"), str(d / "env.json")])
    msi.main(common + ["-o", str(d / "out_plain"), str(d / "plain.json")])
    msi.main(common + ["-o", str(d / "out_flag"), "-env", "0.7", str(d / "null.json")])
    ss = msi.load_sessions(str(d / "env.json"))
    assert ss[0]["envelope"] == 0.7 and "envelope" not in ss[1]

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
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4, envelope=True)
    want_env = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, envelope=0.7), dict(voice=name)])
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4)
    want_plain = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name), dict(voice=name)])
    env, plain, flag = read("out_env"), read("out_plain"), read("out_flag")
    assert all(len(w) == CHUNK * (ticks - BS) for w in want_env + want_plain)
    assert np.array_equal(env[0], want_env[0]) and np.array_equal(env[1], want_env[1])
    # a file without the key, run without the flag: what the converter built without the envelope writes, byte for byte
    assert np.array_equal(plain[0], want_plain[0]) and np.array_equal(plain[1], want_plain[1])
    # the session that does not follow: unchanged bytes beside one that does
    assert np.array_equal(env[1], plain[1]) and not np.array_equal(env[0], plain[0])
    # -env as the default, switched off by a session's null: the same input twice, so the outputs swap roles
    assert np.array_equal(flag[0], env[0]) and np.array_equal(flag[1], plain[1])
