"""The post filter on the device (csrc/postfilter.hip) and through the converters and CLIs, against the NumPy restatement
tools/postfilter_ref.py.  Every comparison is bitwise, or equality of int16 streams.

1. alive_postfilter_waves alone: one call at hop 8, window 16, order 4 with a stride that is no multiple of 4 (rows off a 16-byte
   boundary), lengths 0, 1, 3 (< hop / 2), 8 * 16, 8 * 16 + 1, 8 * 37 + 5 and the stride, alphas 0, NaN, 0.3, 0.5, 0.8, 0.85 and 0.85,
   plus the shortest rows at a filtering alpha, a 0.9, a NaN and an inf mid-frame and on both kinds of tile border, and an all-zero
   analysis window between loud frames; one call at hop 320, window 640, order 16 on 40 frames of make_voiced, make_waveform and noise;
   gain_minmax with and without; a row alone and stacked; out between guard bands.
2. post_filter offline on two rows of different lengths.
3. MultiStreamConverter(post_filter=True) with 3 slots at -c 160 -b 16: a session at 0 is the plain converter's, a session at 0.8 the
   restatement of the plain converter's decoder wave; toggling under enable_graph without re-capture; the envelope follow beside it
   sees the filtered wave; a sparse converter's stalled row.
4. RealtimeConverter(post_filter=0.8): bitwise a one-slot MultiStreamConverter on both step forms.
5. inference.py -pf and batch_inference.py with a "post_filter" job."""
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
import postfilter_ref as PR                                          # noqa: E402
from module import audio_io, synthetic                               # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 16                                                             # guard band, elements on each side of every output
E, G_LO, G_HI = PR.constants()


def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _pcm(n, seed, scale=12000):
    return (synthetic.make_waveform(n, seed)[0].numpy() * scale).astype(np.int16)


class Guarded:
    """a device array between two guard bands filled with a sentinel"""

    def __init__(self, shape, dtype, sentinel):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(*shape)
        self.sentinel = sentinel

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
def _call(out, y, lens, alpha, hop, window, order, mm, ratio=PR.RATIO, tilt=PR.TILT):
    win, lag = MS.postfilter_tables(window, order, DEV)
    rc = MS.nat.lib().alive_postfilter_waves(out.data_ptr(), y.data_ptr(), y.shape[1], y.shape[0],
                                             None if lens is None else lens.data_ptr(), alpha.data_ptr(), hop, window, order,
                                             win.data_ptr(), lag.data_ptr(), ratio, tilt, E, G_LO, G_HI,
                                             None if mm is None else mm.data_ptr(), MS.nat.stream())
    torch.cuda.synchronize()
    return rc


HOP8 = dict(hop=8, window=16, order=4)
NONFINITE, ZEROED = 9, 10


def _small_case():
    """-> (y [N, ld], lens, alphas) at hop 8"""
    hop = 8
    ld = hop * 43 + 3                                                # 347: no multiple of 4, so rows 1, 2, 3 (mod 4) lie off 16 bytes
    lens = [0, 1, 3, hop * 16, hop * 16 + 1, hop * 37 + 5, ld,       # each with the alpha below it
            0, 1, ld, ld, ld, hop * 15 + 4, hop * 15 + 5, ld + 50]   # (the last: clamped to the stride)
    alphas = [0.0, float("nan"), 0.3, 0.5, 0.8, 0.85, 0.85,
              0.8, 0.8, 0.8, 0.8, 0.9, 0.8, 0.8, 0.5]
    rng = np.random.default_rng(2024)
    t = np.arange(ld)
    y = (rng.standard_normal((len(lens), ld)) * 0.1 + 0.2 * np.sin(2 * np.pi * t / 11.0)[None]).astype(np.float32)
    y[2, 1], y[3, 5] = -0.0, 0.0
    y[NONFINITE, hop * 5 + 3] = np.nan                               # mid-frame
    y[NONFINITE, hop * 16] = np.inf                                  # the first sample of frame 16
    y[NONFINITE, hop * 30 + 4] = -np.inf                             # the first sample of unit 30 (a border of the kernel's tiles)
    y[ZEROED, hop * 20 - 4:hop * 21 + 4] = 0.0                       # the whole analysis window of frame 20
    return y, lens, alphas


def test_the_kernel_at_hop_8_against_the_restatement():
    wave, lens, alphas = _small_case()
    n, ld = wave.shape
    assert ld % 4
    y = _dev(wave, torch.float32)
    out, mm = Guarded((n, ld), torch.float32, 123.0), Guarded((n, 2), torch.float32, -5.0)
    lens_d, alpha_d = _dev(lens, torch.int32), _dev(alphas, torch.float32)
    assert _call(out.view, y, lens_d, alpha_d, mm=mm.view, **HOP8) == 0
    assert out.intact() and mm.intact() and _bits_equal(y.cpu().numpy(), wave)
    want, G, want_mm = PR.postfilter_waves(wave, lens, alphas, **HOP8)
    got, got_mm = out.view.cpu().numpy(), mm.view.cpu().numpy()
    for r in range(n):
        assert _bits_equal(got[r], want[r]), r
        assert got_mm[r].tolist() == want_mm[r].tolist(), r
        ln = min(max(lens[r], 0), ld)
        assert _bits_equal(got[r, ln:], wave[r, ln:]), r
    for r in (0, 1, 7, 11):                                          # alpha 0, NaN, no samples, 0.9: copied, (1, 1)
        assert _bits_equal(got[r], wave[r]) and got_mm[r].tolist() == [1.0, 1.0] and G[r] is None
    assert G[8].tolist() == [1.0] and _bits_equal(got[8], wave[8])    # one sample: h[0] = 1, so U = y and g = 1
    for r in (2, 3, 4, 5, 6, 9, 10, 12, 13, 14):
        ln = min(lens[r], ld)
        assert G[r] is not None and len(G[r]) == -(-ln // 8) and not _bits_equal(got[r, :ln], wave[r, :ln]), r
    # the non-finite row: the frames that hold a non-finite sample or the 127 behind it stay at 1 (at hop 8 that is 16 or 17 frames each)
    g = G[NONFINITE]
    for at in (8 * 5 + 3, 8 * 16, 8 * 30 + 4):
        assert np.all(g[at // 8:(at + 127) // 8 + 1] == 1.0), at
    assert np.all(g[:5] != 1.0) and np.isfinite(got[NONFINITE, :8 * 5 + 3]).all() and np.isnan(got[NONFINITE, 8 * 5 + 3])
    # the zeroed window: the identity, and the frames around it are not
    _, gz, ident, h = PR.filter_row(wave[ZEROED], ld, 0.8, e=E, g_lo=G_LO, g_hi=G_HI, **HOP8)
    assert ident.tolist() == [f == 20 for f in range(len(ident))] and gz[20] == 1.0 and h[20].tolist() == [1.0] + [0.0] * 127
    # (its neighbours' filters still ring into it, and the output moves towards the identity: at the frame's centre it is y = 0 itself)
    assert gz[19] != 1.0 and gz[21] != 1.0 and got[ZEROED, 8 * 20 + 4] == 0 and got[ZEROED, 8 * 20 - 4] != 0 and got[ZEROED, 8 * 20 + 1] != 0
    # without gain_minmax, without len: the same samples as with the stride for every length
    again, none = Guarded((n, ld), torch.float32, 123.0), Guarded((n, ld), torch.float32, 123.0)
    assert _call(again.view, y, _dev([ld + 9] * n, torch.int32), alpha_d, mm=None, **HOP8) == 0
    assert _call(none.view, y, None, alpha_d, mm=None, **HOP8) == 0
    assert again.intact() and none.intact() and _bits_equal(again.view.cpu().numpy(), none.view.cpu().numpy())
    assert _bits_equal(none.view.cpu().numpy(), PR.postfilter_waves(wave, None, alphas, **HOP8)[0])
    # a row's result is the same at N = 1, at another place in memory
    win, lag = MS.postfilter_tables(16, 4, DEV)
    for r in (4, 5, 9, 13):
        one = MS.postfilter_waves_(torch.empty(1, ld, device=DEV), y[r:r + 1].clone(), lens_d[r:r + 1].clone(), alpha_d[r:r + 1].clone(),
                                   8, 16, 4, win, lag, PR.RATIO, PR.TILT, E, G_LO, G_HI)
        assert _bits_equal(one[0].cpu().numpy(), got[r]), r
    # other ratio and tilt
    assert _call(again.view, y, lens_d, alpha_d, mm=None, ratio=0.4, tilt=0.9, **HOP8) == 0
    assert _bits_equal(again.view.cpu().numpy(), PR.postfilter_waves(wave, lens, alphas, ratio=0.4, tilt=0.9, **HOP8)[0])
    # out must not overlap y
    assert _call(y, y, lens_d, alpha_d, mm=None, **HOP8) == -1 and b"overlaps y" in MS.nat.lib().alive_last_error()
    with pytest.raises(ValueError, match="overlaps"):
        MS.postfilter_waves_(y, y, lens_d, alpha_d, 8, 16, 4, win, lag, PR.RATIO, PR.TILT, E, G_LO, G_HI)


def _speech_case():
    n = 40 * 320
    rng = np.random.default_rng(5)
    wave = np.stack([synthetic.make_voiced(n, 3)[0][0].numpy(), synthetic.make_waveform(n, 2)[0].numpy(),
                     (rng.standard_normal(n) * 0.1).astype(np.float32)])
    return wave, [n, 12345, 7000], [0.8, 0.85, 0.5]


def test_the_kernel_at_hop_320_against_the_restatement():
    wave, lens, alphas = _speech_case()
    n, ld = wave.shape
    y = _dev(wave, torch.float32)
    out, mm = Guarded((n, ld), torch.float32, 123.0), Guarded((n, 2), torch.float32, -5.0)
    assert _call(out.view, y, _dev(lens, torch.int32), _dev(alphas, torch.float32), 320, 640, 16, mm.view) == 0
    assert out.intact() and mm.intact()
    want, G, want_mm = PR.postfilter_waves(wave, lens, alphas)
    got, got_mm = out.view.cpu().numpy(), mm.view.cpu().numpy()
    for r in range(n):
        assert _bits_equal(got[r], want[r]) and got_mm[r].tolist() == want_mm[r].tolist(), r
        assert not _bits_equal(got[r, :lens[r]], wave[r, :lens[r]]) and _bits_equal(got[r, lens[r]:], wave[r, lens[r]:])
        print(f"row {r}: gains {PR.gain_db(want_mm)[r]} dB")
    assert [len(g) for g in G] == [40, 39, 22]


# ---------------------------------------------------------------------------------------------------- 2. post_filter
def test_post_filter_against_the_restatement():
    wave, _, _ = _speech_case()
    wave = wave[:2, :9 * 320 + 11]
    y = _dev(wave, torch.float32)
    lens, alphas = [wave.shape[1], 1000], [0.8, 0.5]
    out = MS.post_filter(y, lens, alphas)
    want = PR.postfilter_waves(wave, lens, alphas)[0]
    assert out is not y and out.shape == y.shape and _bits_equal(out.cpu().numpy(), want) and not _bits_equal(want, wave)
    assert _bits_equal(y.cpu().numpy(), wave)
    one = MS.post_filter(y[0], None, 0.6, 0.5, 0.3, 10, 30.0, -80.0, 6.0)              # one row, the tuning values
    assert one.shape == (wave.shape[1],)
    assert _bits_equal(one.cpu().numpy(), PR.postfilter_waves(wave[:1], None, 0.6, window=480, order=10, ratio=0.5, tilt=0.3, floor_db=-80.0,
                                                              range_db=6.0)[0][0])
    assert _bits_equal(MS.post_filter(y, None, 0.0).cpu().numpy(), wave)
    with pytest.raises(ValueError, match=r"post_filter=0.9 must be"):
        MS.post_filter(y, None, 0.9)
    with pytest.raises(ValueError, match="1 alphas for 2 rows"):
        MS.post_filter(y, None, [0.5])


# ---------------------------------------------------------------------------------------------------- 3. the converter
CHUNK, BS = 160, 16
SESS = [dict(voice="v0", pitch=1.0), dict(voice="v1", alpha=0.1), dict(voice="v2", f0_rate=0.9)]
PF = [0.0, 0.8, 0.5]
TICKS = BS + 8
GRAPH_AT, ON_AT, OFF_AT = BS + 2, BS + 4, BS + 6


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    return MS.VoicePool(voices)


def _stream_pcm():
    pcm = []
    for s in range(3):
        p = _pcm(CHUNK * TICKS, 70 + s).astype(np.float64)
        p *= 0.15 + 0.85 * np.abs(np.sin(np.arange(len(p)) * (2 * np.pi / (CHUNK * 9.0))))
        pcm.append(p.astype(np.int16))
    return pcm


def _conv(pool, **kw):
    return MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, **kw)


def _drive(conv, sess, pcm, ticks, actions=None, after=None):
    outs = [[] for _ in sess]
    for s, p in enumerate(sess):
        conv.open(s, **p)
    for tick in range(ticks):
        for a in (actions or {}).get(tick, []):
            a(conv)
        res = conv.step({s: pcm[s][tick * CHUNK:(tick + 1) * CHUNK] for s in range(len(sess))})
        for s in range(len(sess)):
            outs[s].append(res[s])
        if after is not None and any(r is not None for r in res.values()):
            after(conv, tick)
    return outs


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def twin(pool):
    """the plain converter, eager: per running tick its 16 kHz rings, its decoder waves and its outputs.  Computed once"""
    rec = dict(data=[], wave=[])
    conv = _conv(pool)
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
        outs = _drive(conv, SESS, _stream_pcm(), TICKS)
    finally:
        MS.spectrogram = spectrogram
    assert len(rec["data"]) == len(rec["wave"]) == TICKS - BS and not hasattr(conv, "pf_alpha") and conv.post_filter is False
    with pytest.raises(ValueError, match=r"slot 1: post_filter=0.8 needs a converter built with MultiStreamConverter\(..., post_filter=True\)"):
        conv.set(1, post_filter=0.8)
    with pytest.raises(ValueError, match="post_filter_db needs a converter built with"):
        conv.post_filter_db()
    return dict(outs=outs, data=[d.cpu().numpy() for d in rec["data"]], wave=[w.cpu().numpy() for w in rec["wave"]])


@pytest.mark.parametrize("graph", [False, True])
def test_a_post_filter_converter_with_every_session_at_zero_is_bitwise_the_plain_converter(pool, twin, graph):
    conv = _conv(pool, post_filter=True)
    if graph:
        conv.enable_graph()
    got = _drive(conv, [dict(p, post_filter=0.0) for p in SESS], _stream_pcm(), TICKS)
    assert all(_same(g, w) for g, w in zip(got, twin["outs"]))
    assert conv.pf_alpha.tolist() == [0.0] * 3 and conv.captures == int(graph) and conv.post_filter_db() == [(0.0, 0.0)] * 3
    assert conv._pf_out is not None


def _alphas(tick):
    return [0.8 if ON_AT <= tick else PF[0], PF[1] if tick < OFF_AT else 0.0, PF[2]]


def test_every_ticks_filtered_wave_is_the_restatement_of_the_plain_converters_decoder_wave(pool, twin):
    conv = _conv(pool, post_filter=True)
    rec = dict(pf=[], db=[], captures=[], ptr=[])

    def after(c, tick):
        rec["pf"].append(c._pf_out.cpu().numpy())
        rec["db"].append(c.post_filter_db())
        rec["captures"].append(c.captures)
        rec["ptr"].append(c._pf_out.data_ptr())
    actions = {GRAPH_AT: [lambda c: c.enable_graph()], ON_AT: [lambda c: c.set(0, post_filter=0.8)],
               OFF_AT: [lambda c: c.set(1, post_filter=None)]}
    outs = _drive(conv, [dict(p, post_filter=a) for p, a in zip(SESS, PF)], _stream_pcm(), TICKS, actions=actions, after=after)
    assert len(rec["pf"]) == TICKS - BS
    for i, tick in enumerate(range(BS, TICKS)):
        wave = twin["wave"][i]
        assert wave.shape == (3, 2560)
        want, G, mm = PR.postfilter_waves(wave, None, _alphas(tick))
        assert _bits_equal(rec["pf"][i], want), tick
        assert rec["db"][i] == MS.minmax_db(mm.tolist()), tick
        for s in range(3):
            if _alphas(tick)[s] == 0:
                assert _bits_equal(rec["pf"][i][s], wave[s]) and rec["db"][i][s] == (0.0, 0.0)
                assert np.array_equal(outs[s][tick], twin["outs"][s][tick]), (tick, s)       # a session at 0: the plain one's chunk
            else:
                assert not _bits_equal(want[s], wave[s]) and not np.array_equal(outs[s][tick], twin["outs"][s][tick]), (tick, s)
        print(f"tick {tick}: post_filter_db {[('%.2f' % a, '%.2f' % b) for a, b in rec['db'][i]]}")
    # captured once: toggling never re-captured, and the filtered wave stays in the buffer allocated once
    assert rec["captures"] == [0] * (GRAPH_AT - BS) + [1] * (TICKS - GRAPH_AT) and conv.captures == 1 and len(set(rec["ptr"])) == 1
    conv.close(2)
    assert conv.pf_alpha.tolist() == [pytest.approx(0.8), 0.0, 0.0] and conv.post_filter_db()[2] == (0.0, 0.0)
    before = conv.pf_alpha.clone()
    for bad in (dict(post_filter=float("nan")), dict(post_filter="x"), dict(post_filter=0.9, pitch=3.0)):
        with pytest.raises(ValueError, match="slot 0: post_filter="):
            conv.set(0, **bad)
    assert torch.equal(conv.pf_alpha, before) and conv.params[0]["pitch"] == 1.0


def test_the_envelope_follow_beside_it_sees_the_filtered_wave(pool, twin):
    conv = _conv(pool, post_filter=True, envelope=True)
    rec = []
    ticks = BS + 3
    env = [1.0, 0.5, 0.0]
    _drive(conv, [dict(p, post_filter=a, envelope=e) for p, a, e in zip(SESS, PF, env)], _stream_pcm(), ticks,
           after=lambda c, tick: rec.append(c._env_out.cpu().numpy()))
    assert len(rec) == ticks - BS
    for i in range(ticks - BS):
        filtered = PR.postfilter_waves(twin["wave"][i], None, PF)[0]
        assert _bits_equal(rec[i], ER.envelope_waves(filtered, twin["data"][i], None, env)[0]), i
        assert not _bits_equal(rec[i][1], ER.envelope_waves(twin["wave"][i], twin["data"][i], None, env)[0][1])


def test_a_sparse_converter_with_a_stalled_tick_emits_the_same_stream(pool):
    """slot 1 sits one tick out: its ring stands still, and its stream is what it is without the stall, one tick later"""
    ticks, stall = BS + 4, BS + 2
    pcm = [_pcm(CHUNK * ticks, 50 + s) for s in range(2)]

    def run(stalled):
        conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, sparse=True, post_filter=True)
        conv.open(0, "v0", post_filter=0.5)
        conv.open(1, "v1", post_filter=0.8)
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
            if stalled and tick == stall:
                assert res.get(1) is None
            if 1 in feed and res[1] is not None:
                dbs.append(conv.post_filter_db()[1])
        return outs, dbs
    a, db_a = run(False)
    b, db_b = run(True)
    assert len(a[1]) == ticks - BS == len(b[1]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))
    assert len(a[0]) == len(b[0]) and all(np.array_equal(p, q) for p, q in zip(a[0], b[0]))
    assert db_a == db_b and all(lo != 0.0 or hi != 0.0 for lo, hi in db_a)


# ---------------------------------------------------------------------------------------------------- 4. RealtimeConverter
@pytest.mark.parametrize("graph", [False, True])
def test_a_filtering_realtime_converter_is_bitwise_a_one_slot_multistream(graph):
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(400, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    pf = dict(post_filter_ratio=0.5, post_filter_tilt=0.4, post_filter_order=12, post_filter_window_ms=30.0)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, reuse_interior=False, post_filter=0.8, **pf,
                           **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, post_filter=True, **pf, **kw)
    ms.open(0, "lib", pitch=1.5, alpha=0.2, input_gain=-3.0, post_filter=0.8)
    plain = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, reuse_interior=False, **kw)
    assert rt.post_filter is True and plain.post_filter is False and not hasattr(plain, "_pf_out")
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    ticks, differ = BS + 3, 0
    pcm = _stream_pcm()[0][:CHUNK * ticks]
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b, p = rt.step(c), ms.step({0: c})[0], plain.step(c)
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b) and torch.equal(rt._pf_out, ms._pf_out), t
            assert ms.post_filter_db()[0] != (0.0, 0.0)
            differ += not np.array_equal(a, p)
    assert differ == ticks - BS and rt._pf == ms._pf == MS.check_post_filter(0.8, 0.5, 0.4, 12, 30.0)[1:]


def test_a_filtering_realtime_converter_with_interior_reuse_is_bitwise_itself_without():
    """-c 960 -b 26: a ring of 78 frames advancing by 3; the post filter runs in both step forms"""
    from module.realtime import RealtimeConverter
    chunk, bs, ticks = 960, 26, 28
    lib = synthetic.make_library(400, 1)
    pcm = _pcm(chunk * ticks, 95)
    outs = {}
    for reuse in (False, "auto", None):                              # (None: the converter without the post filter)
        rt = RealtimeConverter(*_nets(), lib, "cuda", chunk=chunk, buffersize=bs, k=4, alpha=0.1, reuse_interior=bool(reuse) and reuse,
                               post_filter=0.0 if reuse is None else 0.8)
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


def test_offline_clis_with_a_post_filter_write_post_filter_of_the_conversion(tmp_path, monkeypatch):
    import batch_inference as BI
    import inference as INF
    from module.pipeline import Converter
    monkeypatch.setenv("ALIVE_KNN_STRICT", "0")                       # (inference.py --knn-strict sets it; restored after the test)
    d = tmp_path
    nets = _save_nets(d)
    lib = synthetic.make_library(512, 5)
    torch.save({"tokens": lib}, d / "voice_library.pt")
    os.makedirs(d / "inputs")
    wav = synthetic.make_waveform(24000, 91) * 0.5                   # 1 s mono at 24 kHz
    audio_io.save(str(d / "inputs" / "utt.wav"), wav, 24000)
    base = ["-i", str(d / "inputs"), "-lib", str(d / "voice_library.pt"), "-d", "cuda", "-c", "4800", "-g", "3"] + nets
    tune = ["--post-filter-ratio", "0.5", "--post-filter-tilt", "0.3"]
    INF.main(base + ["-o", str(d / "out_pf"), "-pf", "0.8", "-env", "0.7"] + tune)
    INF.main(base + ["-o", str(d / "out_zero"), "-pf", "0"] + tune)
    INF.main(base + ["-o", str(d / "out_none")])
    got, sr = audio_io.load(str(d / "out_pf" / "0_utt.wav"))
    # the same file through Converter.convert: post_filter at 16 kHz, then the envelope follow, then resample and gain
    CE, PE, Dec = _loaded_nets(d)
    wf = audio_io.resample(audio_io.load(str(d / "inputs" / "utt.wav"))[0].to(DEV), 24000, 16000)
    wf = (wf / wf.abs().max()).mean(dim=0, keepdim=True)
    out = Converter(CE, PE, Dec, DEV).set_library(lib.to(DEV)).convert(wf, chunk=4800, k=4, alpha=0.0, pitch_shift=0, world_pitch=False,
                                                                      intonation=1.0, f0_rate=1.0, window_batch=64, trim_context=True,
                                                                      share_overlap="auto")
    filtered = MS.post_filter(out, None, 0.8, 0.5, 0.3)
    assert _bits_equal(filtered.cpu().numpy(), PR.postfilter_waves(out.cpu().numpy(), None, 0.8, ratio=0.5, tilt=0.3)[0])
    assert sr == 24000 and torch.equal(got, audio_io.resample(MS.follow_envelope(filtered, wf, None, 0.7), 16000, 24000, post_gain_db=3.0).cpu())
    assert not torch.equal(filtered, out)
    # at 0 and without the flag: the unfiltered conversion, byte for byte
    plain = audio_io.resample(out, 16000, 24000, post_gain_db=3.0).cpu()
    assert torch.equal(audio_io.load(str(d / "out_zero" / "0_utt.wav"))[0], plain)
    assert torch.equal(audio_io.load(str(d / "out_none" / "0_utt.wav"))[0], plain)
    assert open(d / "out_zero" / "0_utt.wav", "rb").read() == open(d / "out_none" / "0_utt.wav", "rb").read()
    # batch_inference.py: a job with "post_filter" writes the file of inference.py --knn-strict -pf, the one beside it the plain file
    INF.main(base + ["-o", str(d / "out_strict"), "-pf", "0.8", "--knn-strict"] + tune)
    INF.main(base + ["-o", str(d / "out_strict_plain"), "--knn-strict"])
    strict, splain = audio_io.load(str(d / "out_strict" / "0_utt.wav"))[0], audio_io.load(str(d / "out_strict_plain" / "0_utt.wav"))[0]
    job = dict(input="inputs/utt.wav", lib="voice_library.pt", gain=3)
    (d / "jobs.json").write_text(json.dumps([dict(job, output="b_plain.wav"), dict(job, post_filter=0.8, output="b_pf.wav")]))
    BI.main([str(d / "jobs.json"), "-c", "4800"] + tune + nets)
    assert torch.equal(audio_io.load(str(d / "b_pf.wav"))[0], strict) and torch.equal(audio_io.load(str(d / "b_plain.wav"))[0], splain)
    assert not torch.equal(strict, splain)
    (d / "jobs2.json").write_text(json.dumps([dict(job, post_filter=None, output="c_plain.wav"), dict(job, output="c_pf.wav")]))
    BI.main([str(d / "jobs2.json"), "-c", "4800", "-pf", "0.8"] + tune + nets)
    assert torch.equal(audio_io.load(str(d / "c_pf.wav"))[0], strict) and torch.equal(audio_io.load(str(d / "c_plain.wav"))[0], splain)
    # an utterance comes out the same alone as inside the corpus
    (d / "jobs3.json").write_text(json.dumps([dict(job, post_filter=0.8, output="d_pf.wav")]))
    BI.main([str(d / "jobs3.json"), "-c", "4800"] + tune + nets)
    assert torch.equal(audio_io.load(str(d / "d_pf.wav"))[0], strict)
