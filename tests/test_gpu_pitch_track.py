"""Pitch tracking on the device (csrc/f0_track.hip, alive_f0_logits) and through the estimator, the converters and the CLIs, against the
NumPy restatement tools/pitch_track_ref.py.  Every comparison is bitwise, or equality of int16 streams.

1. alive_f0_track_rows alone: C = 4096, three rows with the middle one off and its f0 between guard bands; T in {1, 2, 7, 33}; state
   ranges of 1051, 31, 1, 65 and 4000 states (one state, under and over a wave, strided states per lane group, the cap); per-row
   (weight, jump) of (1, 12), (0, 0) and (3, 0.5); seeded noise, the three ridge cases, constant scores, NaN, +inf and -inf entries;
   `changed`; on = NULL; a repeated call on the same workspace.
2. F0Estimator(seed=2): argmax_channels(logits(x)) is estimate(x) below 96 frame columns and on the plane path, in both encoder
   precisions; estimate(x, track=) is the restatement of the downloaded logits(x).
3. MultiStreamConverter(pitch_track=True): all sessions off -> the plain converter's streams; one session on -> its f0 is the
   restatement of the tick's logits and the other rows' streams are unchanged; enable_graph in the middle, then a set() that changes a
   row with no re-capture; pitch_track_changed(); a sparse converter with a stalled tick.
4. RealtimeConverter(pitch_track=True): bitwise a one-slot MultiStreamConverter over 6 steps.
5. convert(pitch_track=True) on an utterance of three windows (the fewest the windowing makes), convert_many with a mixed list, and
   the three CLIs against the API."""
import functools
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

import pitch_track_ref as PR                                         # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import common, ops, synthetic                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 16                                                             # guard band, elements on each side
C = 4096
RANGES = [(50, 1100), (60, 90), (77, 77), (60, 124), (96, 4095)]
PARAMS = [(1.0, 12.0), (0.0, 0.0), (3.0, 0.5)]


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


# ---------------------------------------------------------------------------------------------------- 1. the kernel alone
OUTLIERS, STEP, GLIDE, NOISE, CONSTANT, NONFINITE = range(6)


@functools.lru_cache(maxsize=None)
def _scores():
    """[6, 4096, 33] float32: the octave outliers, the real step, the glide, plain noise, constant scores, and noise with an all-NaN
    frame and scattered NaN, +inf and -inf entries -- computed once"""
    T = 33
    odd = (5, 17, 18)
    x = np.empty((6, C, T), dtype=np.float32)
    x[OUTLIERS] = PR.ridge_scores([[200, 400] if t in odd else [200] for t in range(T)], [[8, 14] if t in odd else [10] for t in range(T)])
    x[STEP] = PR.ridge_scores([[120] if t < 16 else [240] for t in range(T)], [[10]] * T)
    x[GLIDE] = PR.ridge_scores([[150 + 40 * t / (T - 1)] for t in range(T)], [[10]] * T)
    x[NOISE] = np.random.default_rng(7).standard_normal((C, T)).astype(np.float32)
    x[CONSTANT] = np.float32(0.25)
    x[NONFINITE] = np.random.default_rng(8).standard_normal((C, T)).astype(np.float32)
    x[NONFINITE, :, 3] = np.nan                                      # an all-NaN frame
    rng = np.random.default_rng(9)
    for v in (np.nan, np.inf, -np.inf):
        x[NONFINITE, rng.integers(1, C, 600), rng.integers(0, T, 600)] = v
    x[NONFINITE, 77, :2] = (np.inf, -np.inf)                         # the one-state range meets both
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _tracker(lo, hi):
    return PR.Tracker(lo, hi, 2.0)


def _call(logits, track, on, weight, jump, f0, changed, ws):
    n, c, t = logits.shape
    return nat.lib().alive_f0_track_rows(logits.data_ptr(), n, c, t, track.lo, track.states, track.semis.data_ptr(),
                                         track.band_lo.data_ptr(), track.band_hi.data_ptr(), None if on is None else on.data_ptr(),
                                         weight.data_ptr(), jump.data_ptr(), f0.data_ptr(), None if changed is None else changed.data_ptr(),
                                         ws.data_ptr(), nat.stream())


@pytest.mark.parametrize("T", [1, 2, 7, 33])
@pytest.mark.parametrize("lo,hi", RANGES)
def test_the_kernel_against_the_restatement(lo, hi, T):
    ref, track = _tracker(lo, hi), common.pitch_track(lo, hi, 2.0, DEV)
    assert track.states == hi - lo + 1 == ref.S
    assert np.array_equal(track.semis.cpu().numpy().view(np.int64), ref.s.view(np.int64))
    assert np.array_equal(track.band_lo.cpu().numpy(), ref.blo) and np.array_equal(track.band_hi.cpu().numpy(), ref.bhi)
    ws = torch.empty(nat.lib().alive_f0_track_workspace_bytes(3, T, track.states), dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(100 * T + lo)
    results = []
    # a masked call (the middle row off), a call with on = NULL and other parameters per row, and the first call again
    for kinds, on, rot in (((OUTLIERS, NOISE, NONFINITE), [1, 0, 1], 0), ((STEP, GLIDE, CONSTANT), None, 1),
                           ((OUTLIERS, NOISE, NONFINITE), [1, 0, 1], 0)):
        host = np.ascontiguousarray(_scores()[list(kinds), :, :T])
        weight = [PARAMS[(r + rot) % 3][0] for r in range(3)]
        jump = [PARAMS[(r + rot) % 3][1] for r in range(3)]
        before = rng.integers(lo, hi + 1, (3, T)).astype(np.float32)
        if T > 1:
            before[0, 0] = lo + ref.path(host[0], weight[0], jump[0])[0]         # one frame that the tracker leaves as it is
        logits = _dev(host, torch.float32)
        f0 = Guarded((3, T), torch.float32, -7.0, before)
        changed = Guarded((3,), torch.int32, -3)
        on_d = None if on is None else _dev(on, torch.int32)
        assert _call(logits, track, on_d, _dev(weight, torch.float64), _dev(jump, torch.float64), f0.view, changed.view, ws) == 0
        torch.cuda.synchronize()
        assert f0.intact() and changed.intact()
        assert np.array_equal(logits.cpu().numpy().view(np.int32), host.view(np.int32))
        want, want_changed = PR.track_rows(host, before, ref, on, weight, jump)
        got, got_changed = f0.view.cpu().numpy(), changed.view.cpu().numpy()
        for r in range(3):
            assert np.array_equal(got[r], want[r]), (r, kinds[r])
            if on is None or on[r]:
                assert got_changed[r] == want_changed[r], r
                assert got[r].min() >= lo and got[r].max() <= hi
            else:
                assert np.array_equal(got[r], before[r]) and got_changed[r] == -3          # an off row: untouched
        if on is None:                                               # constant scores: the lowest class everywhere
            assert np.all(got[2] == lo)
        results.append(got)
    assert np.array_equal(results[0][[0, 2]], results[2][[0, 2]])   # the same bits from a workspace another call has used
    if (lo, hi) == (50, 1100) and T == 33:                           # what the feature is for
        assert set(_scores()[OUTLIERS].argmax(axis=0)[[5, 17, 18]].tolist()) <= {399, 400, 401}
        assert results[0][0].min() >= 199 and results[0][0].max() <= 201


def test_the_kernel_refuses_bad_arguments():
    track = common.pitch_track(50, 1100, 2.0, DEV)
    L = nat.lib()
    lg, f0 = torch.zeros(1, C, 2, device=DEV), torch.zeros(1, 2, device=DEV)
    w = torch.ones(1, dtype=torch.float64, device=DEV)
    ws = torch.empty(L.alive_f0_track_workspace_bytes(1, 2, 4001), dtype=torch.uint8, device=DEV)
    tab = (track.semis.data_ptr(), track.band_lo.data_ptr(), track.band_hi.data_ptr())

    def call(c=C, t=2, lo=50, s=1051, tables=tab):
        return L.alive_f0_track_rows(lg.data_ptr(), 1, c, t, lo, s, *tables, None, w.data_ptr(), w.data_ptr(), f0.data_ptr(), None,
                                     ws.data_ptr(), nat.stream())
    for kw, msg in ((dict(s=4001), b"states"), (dict(lo=0), b"lo < 1"), (dict(lo=3046), b"outside"), (dict(t=0), b"T < 1"),
                    (dict(tables=(None, tab[1], tab[2])), b"null tables"), (dict(c=1100), b"outside")):
        assert call(**kw) == -1 and msg in L.alive_last_error(), kw
    assert call() == 0
    torch.cuda.synchronize()
    assert L.alive_f0_track_workspace_bytes(3, 7, 31) >= 3 * 7 * 31 * 2 and L.alive_f0_track_workspace_bytes(0, 7, 31) == 0


# ---------------------------------------------------------------------------------------------------- 2. the estimator
@functools.lru_cache(maxsize=None)
def _pe():
    from module.f0_estimator import F0Estimator
    return F0Estimator(seed=2).to(DEV)


def _spec(frames):
    from module.spectrogram import spectrogram
    wav = torch.cat([synthetic.make_waveform(320 * frames, 60 + r) for r in range(2)], 0)
    return spectrogram(wav.to(DEV))


@pytest.mark.parametrize("frames,mode", [(5, 1), (64, 1), (64, 2)])
def test_the_stored_logits_reduce_to_the_estimate_and_the_tracked_estimate_is_the_restatement(frames, mode):
    pe, x = _pe(), _spec(frames)
    assert tuple(x.shape) == (2, 641, frames)
    mode0 = ops.encoder_precision(0)
    try:
        ops.encoder_precision(mode)
        plain = pe.estimate(x)
        lg = pe.logits(x)
        assert tuple(lg.shape) == (2, C, frames)
        assert torch.equal(ops.argmax_channels(lg), plain)
        buf = torch.full((2, C, frames), 9.0, device=DEV)
        assert pe.logits(x, out=buf) is buf and torch.equal(buf, lg)
        track = common.pitch_track(device=DEV)
        changed = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        got = pe.estimate(x, track=track, track_weight=0.5, track_jump=3.0, changed=changed)
        want, moved = PR.track_rows(lg.cpu().numpy(), plain.cpu().numpy()[:, 0], _tracker(50, 1100), None, 0.5, 3.0)
        assert np.array_equal(got.cpu().numpy()[:, 0], want) and changed.cpu().tolist() == moved.tolist()
        on = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
        w, j = torch.tensor([9.0, 0.0], dtype=torch.float64, device=DEV), torch.tensor([9.0, 0.0], dtype=torch.float64, device=DEV)
        got = pe.estimate(x, track=track, track_on=on, track_weight=w, track_jump=j)
        assert torch.equal(got[0], plain[0])
        inside = lg[1, 50:1101].argmax(dim=0).float() + 50          # weight = jump = 0: the argmax over [lo, hi]
        assert torch.equal(got[1, 0], inside)
        assert torch.equal(pe.estimate(x), plain)                    # and without a track the call is what it was
    finally:
        ops.encoder_precision(mode0)


# ---------------------------------------------------------------------------------------------------- 3. MultiStreamConverter
from module import audio_io                                          # noqa: E402
from module import multistream as MS                                 # noqa: E402

CHUNK, BS, TICKS = 160, 16, 16 + 8                                   # -c 160 -b 16: rings of 2560 samples, 8 frames
GRAPH_AT, SET_AT = BS + 2, BS + 5
SESS = [dict(voice="v0", pitch=2.0), dict(voice="v1", alpha=0.3), dict(voice="v2", f0_rate=0.9)]
ON = dict(pitch_track=True, track_weight=0.5, track_jump=3.0)       # (the synthetic nets' scores spread over a few units)


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    return MS.VoicePool(voices)


def _stream_pcm():
    return [_pcm(CHUNK * TICKS, 70 + s) for s in range(3)]


def _conv(pool, slots=3, **kw):
    return MS.MultiStreamConverter(*_nets(), pool, slots, chunk=CHUNK, buffersize=BS, k=4, **kw)


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
    """a converter built without pitch_track, eager: its streams, and per running tick the class scores of its spectrogram
    (pe.logits) with their argmax.  Computed once"""
    specs = []
    conv = _conv(pool)
    spectrogram = MS.spectrogram

    def tapped(data):
        spec = spectrogram(data)
        specs.append(spec.clone())
        return spec
    MS.spectrogram = tapped
    try:
        outs = _drive(conv, SESS, _stream_pcm(), TICKS)
    finally:
        MS.spectrogram = spectrogram
    assert len(specs) == TICKS - BS and tuple(specs[0].shape) == (3, 641, 8)
    assert not hasattr(conv, "track_on") and conv.pitch_track is False
    logits = [conv.pe.logits(s) for s in specs]
    for s, lg in zip(specs, logits):
        assert torch.equal(ops.argmax_channels(lg), conv.pe.estimate(s))
    with pytest.raises(ValueError, match=r"slot 0: pitch_track=True needs a converter built with MultiStreamConverter\(..., pitch_track=True\)"):
        conv.set(0, pitch_track=True)
    with pytest.raises(ValueError, match="pitch_track_changed needs a converter built with"):
        conv.pitch_track_changed()
    return dict(outs=outs, logits=[lg.cpu().numpy() for lg in logits], argmax=[ops.argmax_channels(lg).cpu().numpy()[:, 0] for lg in logits])


@pytest.mark.parametrize("graph", [False, True])
def test_a_tracking_converter_with_every_session_off_is_bitwise_the_plain_converter(pool, twin, graph):
    conv = _conv(pool, pitch_track=True)
    if graph:
        conv.enable_graph()
    got = _drive(conv, [dict(p, pitch_track=False) for p in SESS], _stream_pcm(), TICKS)
    assert all(sum(o is not None for o in g) == TICKS - BS for g in got) and all(_same(g, w) for g, w in zip(got, twin["outs"]))
    assert conv.track_on.tolist() == [0, 0, 0] and conv.captures == int(graph) and conv.pitch_track_changed() == [0, 0, 0]
    assert (conv._track.lo, conv._track.hi, conv._track.band) == (50, 1100, 2.0) and len(conv._track_bufs) == 1
    before = {a: getattr(conv, a).clone() for a in ("track_on", "track_weight", "track_jump", "pitch")}
    for bad in (dict(pitch_track=1), dict(track_weight=-1.0), dict(track_jump=float("nan"), pitch=3.0), dict(track_weight="x")):
        with pytest.raises(ValueError, match="slot 1: "):
            conv.set(1, **bad)
    assert all(torch.equal(getattr(conv, a), v) for a, v in before.items()) and conv.params[1]["pitch"] == 0.0


def _want_f0(twin, i, on, weight, jump, conv):
    """the tick's transformed f0 [3, 1, 8]: the restatement of the twin's scores on the rows that are on, the argmax on the others"""
    raw, moved = PR.track_rows(twin["logits"][i], twin["argmax"][i], _tracker(50, 1100), on, weight, jump)
    f0 = torch.from_numpy(raw)[:, None].to(DEV).contiguous()
    return MS.pitch_transform_rows_(f0, 1, conv.f0_rate, conv.pitch, conv.intonation), raw, moved


def test_a_tracked_sessions_f0_is_the_restatement_of_the_ticks_scores_and_the_other_rows_are_unchanged(pool, twin):
    conv = _conv(pool, pitch_track=True)
    rec = dict(f0=[], moved=[], captures=[], ptr=[])

    def after(c, tick):
        rec["f0"].append(c.last_f0.clone())
        rec["moved"].append(c.pitch_track_changed())
        rec["captures"].append(c.captures)
        rec["ptr"].append(next(iter(c._track_bufs.values())).data_ptr())
    actions = {GRAPH_AT: [lambda c: c.enable_graph()], SET_AT: [lambda c: c.set(2, pitch_track=True, track_weight=0.0, track_jump=0.0)]}
    outs = _drive(conv, [SESS[0], dict(SESS[1], **ON), SESS[2]], _stream_pcm(), TICKS, actions=actions, after=after)
    differ = [0, 0, 0]
    for i, tick in enumerate(range(BS, TICKS)):
        late = tick >= SET_AT
        on, w, j = [0, 1, int(late)], [1.0, 0.5, 0.0 if late else 1.0], [12.0, 3.0, 0.0 if late else 12.0]
        want, raw, moved = _want_f0(twin, i, on, w, j, conv)
        assert torch.equal(rec["f0"][i], want), tick
        assert rec["moved"][i] == [0, int(moved[1]), int(moved[2])], tick
        assert raw[1].min() >= 50 and raw[1].max() <= 1100
        if late:                                                     # weight = jump = 0: the per-frame argmax over [lo, hi]
            assert np.array_equal(raw[2], twin["logits"][i][2, 50:1101].argmax(axis=0).astype(np.float32) + 50)
        for s in range(3):
            differ[s] += not np.array_equal(raw[s], twin["argmax"][i][s])
        print(f"tick {tick}: frames moved {rec['moved'][i]}")
    # the session that never tracks emits the twin's stream; the tracked one differs; the one switched on differs from there on
    assert _same(outs[0], twin["outs"][0]) and not _same(outs[1], twin["outs"][1])
    assert _same(outs[2][:SET_AT], twin["outs"][2][:SET_AT]) and not _same(outs[2][SET_AT:], twin["outs"][2][SET_AT:])
    assert differ[0] == 0 and differ[1] > 0 and differ[2] > 0
    # captured once; switching a row on never re-captured, and the scores stay in the buffer allocated once
    assert rec["captures"] == [0] * (GRAPH_AT - BS) + [1] * (TICKS - GRAPH_AT) and conv.captures == 1 and len(set(rec["ptr"])) == 1
    conv.close(1)
    assert conv.track_on.tolist() == [0, 0, 1] and conv.pitch_track_changed()[1] == 0
    assert conv.track_weight.tolist() == [1.0, 1.0, 0.0] and conv.track_jump.tolist() == [12.0, 12.0, 0.0]
    with pytest.raises(ValueError, match="slot 1: pitch_track cannot be combined with world_pitch"):
        _conv(pool, pitch_track=True, world_pitch=True).open(1, "v1", pitch_track=True, world_pitch=True)


def test_a_sparse_tracking_converter_with_a_stalled_tick_emits_the_same_stream(pool):
    """slot 1 sits one tick out: its ring stands still, and its stream is what it is without the stall, one tick later"""
    ticks, stall = BS + 5, BS + 2
    pcm = [_pcm(CHUNK * ticks, 50 + s) for s in range(2)]

    def run(stalled):
        conv = _conv(pool, 2, sparse=True, pitch_track=True)
        conv.open(0, "v0", **ON)
        conv.open(1, "v1", **ON)
        outs, at, moved = [[], []], [0, 0], []
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
                moved.append(conv.pitch_track_changed()[1])
        return outs, moved
    a, moved_a = run(False)
    b, moved_b = run(True)
    assert len(a[1]) == ticks - BS == len(b[1]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))
    assert len(a[0]) == len(b[0]) and all(np.array_equal(p, q) for p, q in zip(a[0], b[0]))
    assert moved_a == moved_b and any(moved_a)


# ---------------------------------------------------------------------------------------------------- 4. RealtimeConverter
@pytest.mark.parametrize("graph", [False, True])
def test_a_tracking_realtime_converter_is_bitwise_a_one_slot_multistream(graph):
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(400, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    track = dict(weight=0.5, jump=3.0, lo=60, hi=900, band=1.5)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, pitch_track=track, **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, pitch_track=True, track_lo=60, track_hi=900,
                                 track_band=1.5, **kw)
    ms.open(0, "lib", pitch=1.5, alpha=0.2, input_gain=-3.0, pitch_track=True, track_weight=0.5, track_jump=3.0)
    plain = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, reuse_interior=False, **kw)
    assert rt.pitch_track is True and rt.reuse is False and plain.pitch_track is False and not hasattr(plain, "_track")
    with pytest.raises(ValueError, match="interior reuse cannot be combined with pitch_track"):
        RealtimeConverter(*_nets(), lib, "cuda", reuse_interior=True, pitch_track=True, chunk=960, buffersize=26)
    with pytest.raises(ValueError, match="pitch_track cannot be combined with world_pitch"):
        RealtimeConverter(*_nets(), lib, "cuda", world_pitch=True, pitch_track=True, **kw)
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    ticks, differ = BS + 6, 0
    pcm = _pcm(CHUNK * ticks, 70)
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b, p = rt.step(c), ms.step({0: c})[0], plain.step(c)
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b) and torch.equal(rt.last_f0, ms.last_f0), t
            assert rt.pitch_track_changed() == ms.pitch_track_changed()[0]
            differ += not np.array_equal(a, p)
    assert differ == ticks - BS


# ---------------------------------------------------------------------------------------------------- 5. offline and the CLIs
OFF_CHUNK = 9600                                                     # windows of 28800 samples: 90 frames each


@pytest.fixture(scope="module")
def offline():
    from module.pipeline import Converter
    lib = synthetic.make_library(512, 5)
    return Converter(*_nets(), DEV), lib


def test_convert_with_pitch_track_decodes_the_restatement_of_every_windows_scores(offline):
    from module.pipeline import make_windows
    from module.spectrogram import spectrogram
    conv, lib = offline
    conv.set_library(lib.to(DEV))
    wf = synthetic.make_waveform(4000, 91).to(DEV)                   # three windows: the fewest the windowing makes
    seen = []
    transform = ops.pitch_transform_

    def tapped(f0, *a, **k):
        seen.append(f0.clone())
        return transform(f0, *a, **k)
    ops.pitch_transform_ = tapped
    try:
        out = conv.convert(wf, chunk=OFF_CHUNK, k=4, pitch_shift=1.0, trim_context=True, share_overlap="auto",
                           pitch_track=dict(weight=0.5, jump=3.0))
    finally:
        ops.pitch_transform_ = transform
    plain = conv.convert(wf, chunk=OFF_CHUNK, k=4, pitch_shift=1.0, trim_context=True, share_overlap="auto")
    assert tuple(out.shape) == tuple(wf.shape) and not torch.equal(out, plain)
    windows, _ = make_windows(wf, OFF_CHUNK)
    assert windows.shape[0] == 3 and len(seen) == 1 and tuple(seen[0].shape) == (3, 1, 90)
    lg = conv.pe.logits(spectrogram(windows))
    want, moved = PR.track_rows(lg.cpu().numpy(), ops.argmax_channels(lg).cpu().numpy()[:, 0], _tracker(50, 1100), None, 0.5, 3.0)
    assert np.array_equal(seen[0].cpu().numpy()[:, 0], want) and moved.min() > 0
    assert torch.equal(out, conv.convert(wf, chunk=OFF_CHUNK, k=4, pitch_shift=1.0, trim_context=False, pitch_track=dict(weight=0.5, jump=3.0)))
    with pytest.raises(ValueError, match="pitch_track cannot be combined with world_pitch"):
        conv.convert(wf, chunk=OFF_CHUNK, world_pitch=True, pitch_track=True)


def test_convert_many_with_a_mixed_list_converts_each_utterance_as_alone(offline):
    from module.common import PackedLibrary
    conv, _ = offline
    g = torch.Generator().manual_seed(5)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 260))}
    vpool = MS.VoicePool(voices)
    utts = [synthetic.make_waveform(n, 40 + i).to(DEV) for i, n in enumerate((4000, OFF_CHUNK + 777, 5000))]      # 3, 4 and 3 windows
    tracks = [True, False, {"weight": 3}]
    names = ["v0", "v1", "v0"]
    kw = dict(chunk=OFF_CHUNK, k=4, trim_context=True)
    # batches of 4 windows: a batch whose tracked windows reach the plane path alone, one whose single tracked window does not (the
    # whole batch's scores are stored then), and one with tracked windows only
    outs = conv.convert_many(utts, vpool, names, pitch_shift=[0.0, 1.0, -1.0], pitch_track=tracks, window_batch=4, **kw)
    untracked = conv.convert_many(utts, vpool, names, pitch_shift=[0.0, 1.0, -1.0], window_batch=4, **kw)
    for i, (u, t, n, p) in enumerate(zip(utts, tracks, names, (0.0, 1.0, -1.0))):
        conv.set_library(PackedLibrary(voices[n], strict=True))
        alone = conv.convert(u, pitch_shift=p, **kw, **(dict(pitch_track=t) if t else {}))
        assert torch.equal(outs[i], alone), i
        assert torch.equal(outs[i], untracked[i]) == (not t), i
    with pytest.raises(ValueError, match="lo, hi and band are call-wide"):
        conv.convert_many(utts, vpool, names, pitch_track=[True, False, {"lo": 60}], **kw)
    with pytest.raises(ValueError, match="cannot be combined with world_pitch"):
        conv.convert_many(utts, vpool, names, pitch_track=tracks, world_pitch=[True, False, False], **kw)


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


def test_offline_clis_with_pitch_track_write_what_the_api_converts(tmp_path, monkeypatch):
    import batch_inference as BI
    import inference as INF
    from module.pipeline import Converter
    monkeypatch.setenv("ALIVE_KNN_STRICT", "0")                       # (inference.py --knn-strict sets it; restored after the test)
    d = tmp_path
    nets = _save_nets(d)
    lib = synthetic.make_library(512, 5)
    torch.save({"tokens": lib}, d / "voice_library.pt")
    os.makedirs(d / "inputs")
    audio_io.save(str(d / "inputs" / "utt.wav"), synthetic.make_waveform(36000, 91) * 0.5, 24000)      # 1.5 s mono at 24 kHz
    base = ["-i", str(d / "inputs"), "-lib", str(d / "voice_library.pt"), "-d", "cuda", "-c", "9600"] + nets
    tune = ["--track-weight", "0.5", "--track-jump", "3", "--track-lo", "60", "--track-hi", "900", "--track-band", "1.5"]
    INF.main(base + ["-o", str(d / "out_pt"), "-pt"] + tune)
    got, sr = audio_io.load(str(d / "out_pt" / "0_utt.wav"))
    CE, PE, Dec = _loaded_nets(d)
    wf = audio_io.resample(audio_io.load(str(d / "inputs" / "utt.wav"))[0].to(DEV), 24000, 16000)
    wf = (wf / wf.abs().max()).mean(dim=0, keepdim=True)
    out = Converter(CE, PE, Dec, DEV).set_library(lib.to(DEV)).convert(
        wf, chunk=9600, k=4, alpha=0.0, pitch_shift=0, intonation=1.0, f0_rate=1.0, window_batch=64, trim_context=True,
        share_overlap="auto", pitch_track=dict(weight=0.5, jump=3.0, lo=60, hi=900, band=1.5))
    assert sr == 24000 and torch.equal(got, audio_io.resample(out, 16000, 24000, post_gain_db=1.0).cpu())
    with pytest.raises(SystemExit, match="-pt cannot be combined with -wpe"):
        INF.main(base + ["-o", str(d / "x"), "-pt", "-wpe", "True"])
    # batch_inference.py: a job with "pitch_track" writes the file of inference.py --knn-strict -pt; -pt as the default with a false
    INF.main(base + ["-o", str(d / "out_strict"), "-pt", "--knn-strict"] + tune)
    INF.main(base + ["-o", str(d / "out_strict_plain"), "--knn-strict"])
    strict, plain = audio_io.load(str(d / "out_strict" / "0_utt.wav"))[0], audio_io.load(str(d / "out_strict_plain" / "0_utt.wav"))[0]
    job = dict(input="inputs/utt.wav", lib="voice_library.pt")
    jobs = [dict(job, output="b_plain.wav"), dict(job, pitch_track={"weight": 0.5, "jump": 3}, output="b_pt.wav")]
    (d / "jobs.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs.json"), "-c", "9600"] + tune[4:] + nets)
    assert torch.equal(audio_io.load(str(d / "b_pt.wav"))[0], strict) and torch.equal(audio_io.load(str(d / "b_plain.wav"))[0], plain)
    assert not torch.equal(strict, plain)
    jobs = [dict(job, pitch_track=False, output="c_plain.wav"), dict(job, output="c_pt.wav")]
    (d / "jobs2.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs2.json"), "-c", "9600", "-pt"] + tune + nets)
    assert torch.equal(audio_io.load(str(d / "c_pt.wav"))[0], strict) and torch.equal(audio_io.load(str(d / "c_plain.wav"))[0], plain)


def test_multistream_cli_with_a_tracking_session_leaves_the_others_unchanged(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    ticks = BS + 5
    wav = _pcm(CHUNK * ticks, 70).astype(np.float32) / 32767
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    base = [dict(input="in0.wav", lib="voice_library.pt"), dict(input="in1.wav", lib="voice_library.pt")]
    json.dump([dict(base[0], pitch_track=True, track_weight=0.5, track_jump=3), base[1]], open(d / "pt.json", "w"))
    json.dump(base, open(d / "plain.json", "w"))
    json.dump([base[0], dict(base[1], pitch_track=False)], open(d / "off.json", "w"))
    common_ = nets + ["-c", str(CHUNK), "-b", str(BS)]
    msi.main(common_ + ["-o", str(d / "out_pt"), str(d / "pt.json")])
    msi.main(common_ + ["-o", str(d / "out_plain"), str(d / "plain.json")])
    msi.main(common_ + ["-o", str(d / "out_flag"), "-pt", "--track-weight", "0.5", "--track-jump", "3", str(d / "off.json")])
    ss = msi.load_sessions(str(d / "pt.json"))
    assert (ss[0]["pitch_track"], ss[0]["track_weight"], ss[0]["track_jump"]) == (True, 0.5, 3.0) and "pitch_track" not in ss[1]

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
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4, pitch_track=True)
    want_pt = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, pitch_track=True, track_weight=0.5, track_jump=3.0), dict(voice=name)])
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4)
    want_plain = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name), dict(voice=name)])
    pt, plain, flag = read("out_pt"), read("out_plain"), read("out_flag")
    assert all(len(w) == CHUNK * (ticks - BS) for w in want_pt + want_plain)
    assert np.array_equal(pt[0], want_pt[0]) and np.array_equal(pt[1], want_pt[1])
    # a file without the key, run without the flag: what the converter built without the tracker writes, byte for byte
    assert np.array_equal(plain[0], want_plain[0]) and np.array_equal(plain[1], want_plain[1])
    # the session that does not track: unchanged bytes beside one that does
    assert np.array_equal(pt[1], plain[1]) and not np.array_equal(pt[0], plain[0])
    # -pt as the default, switched off by a session's false: the same input twice, so the outputs swap roles
    assert np.array_equal(flag[0], pt[0]) and np.array_equal(flag[1], plain[1])
