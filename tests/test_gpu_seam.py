"""The seam crossfade on the device (csrc/seam.hip) and through the streaming converters, against the NumPy restatement
tools/seam_ref.py.  Every comparison is bitwise, or equality of int16 streams.

1. alive_seam_rows alone: six rows in one call (filling and emitting; xlen 0, 1, 255, 256, 257, 300; stored 0, less, equal, greater;
   shift = span and span + 1; a row whose regions do not fit; a NaN in one tail; with and without the gate's gains; stats NULL), every
   output between guard bands; a row alone bitwise the row in the batch.
2. MultiStreamConverter(crossfade=True) at -c 160 -b 16 with sessions at 16, 44.1 and 48 kHz: no session crossfading -> bitwise the
   converter built without it; otherwise every emitted chunk is what seam_ref.stream makes of the full waves of a twin built without
   crossfade; enable_graph in the middle, retuning without re-capture, close + open, seam_db().
3. With gate=True through speech / silence / speech: against the restatements of both.
4. RealtimeConverter(crossfade_ms=5): bitwise a one-slot MultiStreamConverter; with interior reuse bitwise itself without; reset();
   the bf16 repeat of both converters restores the tail.
5. multistream_inference.py on a sessions file with one crossfading session, and on one without the key."""
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

import gate_ref as GR                                                # noqa: E402
import seam_ref as SR                                                # noqa: E402
from module import audio_io, synthetic                               # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 16                                                             # guard band, elements on each side of every output


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
    i = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(i)[~nan], b.view(i)[~nan]))


# ---------------------------------------------------------------------------------------------------- 1. the kernel alone
LD, LD_TAIL, SPAN = 1499, 300, 300                                   # (a stride that is no multiple of 256)
XLEN = [0, 1, 255, 256, 257, 300]                                    # the loop crosses one block width


def _case(variant):
    """six rows: per variant another pairing of xlen with emit / stored / shift, and a row that does not fit"""
    rng = np.random.default_rng(40 + variant)
    y = rng.standard_normal((6, LD)).astype(np.float32)
    tail = rng.standard_normal((6, LD_TAIL)).astype(np.float32)
    lo = np.array([100 + 7 * r for r in range(6)], dtype=np.int32)
    roll = lambda a: np.roll(np.array(a), variant)                   # noqa: E731
    emit = roll([1, 1, 0, 1, 1, 1]).astype(np.uint8)
    shift = roll([SPAN, SPAN + 1, SPAN, SPAN + 1, SPAN + 1, SPAN]).astype(np.int32)
    xlen = np.array(XLEN, dtype=np.int32)
    # stored against the row's xlen: 0, less, equal, greater
    kind = roll(["equal", "zero", "less", "greater", "less", "equal"])
    stored = np.array([dict(zero=0, less=max(x // 2, 0), equal=x, greater=min(x + 40, LD_TAIL))[k] for x, k in zip(XLEN, kind)],
                      dtype=np.int32)
    bad = (3 + variant) % 6                                          # an emitting row whose second region ends one past the row
    if XLEN[bad] == 0 or not emit[bad]:
        bad = 2
    assert emit[bad] and XLEN[bad] > 0
    lo[bad] = LD - int(shift[bad]) - XLEN[bad] + 1
    # a NaN in the part of one tail that is faded from
    nan_row = [r for r in range(6) if emit[r] and r != bad and min(XLEN[r], stored[r]) > 20][0]
    tail[nan_row, 17] = np.nan
    g0 = roll([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]).astype(np.float32)
    g1 = roll([1.0, 0.0, 1.0, 0.0, 0.0, 0.0]).astype(np.float32)
    return dict(y=y, tail=tail, lo=lo, shift=shift, xlen=xlen, emit=emit, stored=stored, g0=g0, g1=g1, bad=bad, nan_row=nan_row)


def _seam_call(c, rows=slice(None), gains=False, stats=True):
    """alive_seam_rows on the rows of a case, every output between guard bands -> (y, tail, stored, stats or None)"""
    y, tail = c["y"][rows], c["tail"][rows]
    n = y.shape[0]
    out = dict(y=Guarded((n, LD), torch.float32, 123.0, y), tail=Guarded((n, LD_TAIL), torch.float32, -9.0, tail),
               stored=Guarded((n,), torch.int32, -77, c["stored"][rows]))
    if stats:
        out["stats"] = Guarded((n, 2), torch.float64, -3.0)
    MS.seam_rows_(out["y"].view, _dev(c["lo"][rows], torch.int32), _dev(c["shift"][rows], torch.int32),
                  _dev(c["xlen"][rows], torch.int32), _dev(c["emit"][rows], torch.uint8), out["tail"].view, out["stored"].view,
                  _dev(c["g0"][rows], torch.float32) if gains else None, _dev(c["g1"][rows], torch.float32) if gains else None,
                  out["stats"].view if stats else None)
    torch.cuda.synchronize()
    assert all(g.intact() for g in out.values())
    got = {k: g.view.cpu().numpy() for k, g in out.items()}
    return got["y"], got["tail"], got["stored"], got.get("stats")


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_seam_rows_against_the_restatement(variant):
    c = _case(variant)
    for gains in (False, True):
        g = (c["g0"], c["g1"]) if gains else (None, None)
        want = SR.seam_rows(c["y"], c["lo"], c["shift"], c["xlen"], c["emit"], c["tail"], c["stored"], *g)
        got = _seam_call(c, gains=gains)
        for name, a, b in zip(("y", "tail", "stored", "stats"), got, want):
            assert _bits_equal(a, b.astype(a.dtype) if name == "stored" else b), (name, gains)
        y, tail, stored, stats = got
        xe = np.minimum(c["xlen"], c["stored"])
        for r in range(6):
            lo, x = int(c["lo"][r]), int(c["xlen"][r])
            if not c["emit"][r]:                                     # a filling row: nothing moves
                assert _bits_equal(y[r], c["y"][r]) and _bits_equal(tail[r], c["tail"][r]) and stored[r] == c["stored"][r]
                assert stats[r].tolist() == [0.0, 0.0]
            elif x == 0 or r == c["bad"]:                            # off, or regions that do not fit: y stays, nothing stored
                assert _bits_equal(y[r], c["y"][r]) and _bits_equal(tail[r], c["tail"][r]) and stored[r] == 0
                assert stats[r].tolist() == [0.0, 0.0]
            else:
                skipped = gains and c["g0"][r] == 0 and c["g1"][r] == 0
                assert stored[r] == (0 if skipped else x)
                assert np.array_equal(tail[r, :x], c["y"][r, lo + c["shift"][r]:lo + c["shift"][r] + x])
                assert _bits_equal(tail[r, x:], c["tail"][r, x:])
                assert _bits_equal(y[r, :lo], c["y"][r, :lo]) and _bits_equal(y[r, lo + xe[r]:], c["y"][r, lo + xe[r]:])
                if xe[r] > 0 and r != c["nan_row"]:
                    assert stats[r, 0] > 0 and stats[r, 1] > 0 and not np.array_equal(y[r], c["y"][r])
        # the NaN of one tail comes out in one sample of that row's head, makes its d2 a NaN, and goes nowhere else
        r, lo = c["nan_row"], int(c["lo"][c["nan_row"]])
        assert np.argwhere(np.isnan(y)).tolist() == [[r, lo + 17]] and not np.isnan(tail).any()
        assert np.isnan(stats[r, 0]) and np.isfinite(stats[r, 1]) and np.isnan(stats).sum() == 1
        # without stats: the same y, tail and stored
        ns = _seam_call(c, gains=gains, stats=False)
        assert ns[3] is None and all(_bits_equal(a, b) for a, b in zip(ns[:3], got[:3]))
        # a row alone is bitwise the row in the batch
        for r in range(6):
            one = _seam_call(c, rows=slice(r, r + 1), gains=gains)
            assert all(_bits_equal(a[0], b[r]) for a, b in zip(one, got)), (r, gains)
    assert sorted(set(c["emit"].tolist())) == [0, 1] and c["emit"][c["bad"]] == 1


# ---------------------------------------------------------------------------------------------------- 2. the converter
CHUNK, BS = 160, 16
RATES = [16000, 44100, 48000]
CHUNKS = [160, 441, 480]                                             # the sessions' chunks: spans 160, 440, 480
SPANS = [(1200, 160), (3308, 440), (3600, 480)]
SESS = [dict(voice="v0", pitch=1.0, rate=16000), dict(voice="v1", alpha=0.1, rate=44100), dict(voice="v2", f0_rate=0.9, rate=48000)]
XF = [10, 5, None]                                                   # ms: 160 samples (the whole span), 220, off
REOPEN = BS + 7                                                      # the tick at which slot 0 closes and opens again
TICKS = REOPEN + BS + 2


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


def _rate_pcm(ticks):
    return [_pcm(c * ticks, 70 + s) for s, c in enumerate(CHUNKS)]


def _script_actions(sess0, graph_at=None):
    """the run's script: slot 1 retuned to a longer crossfade (9 ms: 397 samples) at tick BS + 4 and to a shorter one (2 ms: 88) at
    BS + 5, slot 0 closed and opened again at REOPEN, the graph enabled at graph_at"""
    acts = {BS + 4: [lambda c: c.set(1, crossfade_ms=9)], BS + 5: [lambda c: c.set(1, crossfade_ms=2)],
            REOPEN: [lambda c: c.close(0), lambda c: c.open(0, **sess0)]}
    if graph_at is not None:
        acts.setdefault(graph_at, []).insert(0, lambda c: c.enable_graph())
    return acts


def _xf_run(pool, graph_at=None):
    conv = MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, rates=RATES, crossfade=True)
    sess = [dict(p, crossfade_ms=ms) for p, ms in zip(SESS, XF)]
    rec = dict(db=[], stats=[], stored=[], captures=[])

    def after(c, tick):
        rec["db"].append(c.seam_db())
        rec["stats"].append(c.seam_stats.cpu().numpy())
        rec["stored"].append(c.stored.tolist())
        rec["captures"].append(c.captures)
    outs = _drive(conv, sess, _rate_pcm(TICKS), TICKS, CHUNKS, actions=_script_actions(sess[0], graph_at), after=after)
    return outs, rec, conv


@pytest.fixture(scope="module")
def runs(pool):
    """the twin built without crossfade (outputs and full float waves; slot 0 closed and reopened as in the script) and the
    crossfading converter, eager, over the same script; and what seam_ref.stream makes of the twin's waves: computed once"""
    plain = MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, rates=RATES)
    waves = _tap(plain)
    acts = {REOPEN: [lambda c: c.close(0), lambda c: c.open(0, **SESS[0])]}
    want = _drive(plain, SESS, _rate_pcm(TICKS), TICKS, CHUNKS, actions=acts)
    got, rec, conv = _xf_run(pool)
    # the restatement, tick by tick (device ticks are BS .. TICKS - 1)
    lo, ln = [s[0] for s in SPANS], [s[1] for s in SPANS]
    ticks = list(range(BS, TICKS))
    emit = [[not REOPEN <= t < REOPEN + BS, True, True] for t in ticks]
    xlen = [[160, 397 if t == BS + 4 else (88 if t >= BS + 5 else 220), 0] for t in ticks]
    w = [x.cpu().numpy() for x in waves]
    cut = REOPEN - BS
    f1, sp1, st1, tail, stored = SR.stream(w[:cut], lo, ln, CHUNKS, xlen[:cut], emit[:cut], ld_tail=480)
    stored[0] = 0                                                    # close + open: never fade from another session's tail
    f2, sp2, st2, tail, stored = SR.stream(w[cut:], lo, ln, CHUNKS, xlen[cut:], emit[cut:], tail=tail, stored=stored)
    faded, stats = f1 + f2, st1 + st2
    pcm = [audio_io.float_to_pcm16(torch.from_numpy(f).to(DEV)).cpu().numpy() for f in faded]
    return dict(want=want, waves=w, got=got, rec=rec, conv=conv, ticks=ticks, emit=emit, xlen=xlen, faded=faded, stats=stats,
                pcm=pcm, stored=stored)


@pytest.mark.parametrize("graph", [False, True])
def test_a_crossfade_converter_with_no_session_crossfading_is_bitwise_the_plain_converter(pool, runs, graph):
    ticks = BS + 4
    conv = MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, rates=RATES, crossfade=True)
    if graph:
        conv.enable_graph()
    got = _drive(conv, [dict(p, crossfade_ms=None) for p in SESS], _rate_pcm(TICKS), ticks, CHUNKS)
    assert all(sum(o is not None for o in g) == ticks - BS for g in got)
    assert all(_same(g, w[:ticks]) for g, w in zip(got, runs["want"]))
    assert conv.stored.tolist() == [0, 0, 0] == conv.xlen.tolist() and conv.captures == int(graph)
    assert all(np.isnan(v) for v in conv.seam_db()) and conv.shift.tolist() == CHUNKS
    assert conv.span_lo.tolist() == [s[0] for s in SPANS] and conv.span_len.tolist() == [s[1] for s in SPANS]
    assert conv.tail.shape == (3, 480) and conv.tail.dtype == torch.float32 and conv.seam_stats.dtype == torch.float64
    plain = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=CHUNK, buffersize=BS, k=4)
    with pytest.raises(ValueError, match=r"slot 0: crossfade_ms=5 needs a converter built with MultiStreamConverter\(..., "
                                         r"crossfade=True\)"):
        plain.open(0, "v0", crossfade_ms=5)
    assert not plain.is_open[0] and not hasattr(plain, "tail")
    with pytest.raises(ValueError, match="seam_db needs a converter built with"):
        plain.seam_db()
    before = {a: getattr(conv, a).clone() for a in ("xlen", "shift", "stored", "pitch", "seg_len")}
    for bad in (dict(crossfade_ms=float("nan")), dict(crossfade_ms="x"), dict(crossfade_ms=10, pitch=3.0), dict(crossfade_ms=0)):
        with pytest.raises(ValueError, match="slot 1: crossfade_ms="):      # (10 ms is 441 samples at 44.1 kHz: one over the span)
            conv.set(1, **bad)
    assert all(torch.equal(getattr(conv, a), v) for a, v in before.items()) and conv.params[1]["pitch"] == 0.0


def test_every_emitted_chunk_is_the_restatements_fade_of_the_twins_waves(runs):
    got, want, rec, conv = runs["got"], runs["want"], runs["rec"], runs["conv"]
    assert len(runs["waves"]) == TICKS - BS == len(rec["db"]) and conv.captures == 0
    faded_ticks = [0, 0, 0]
    for i, t in enumerate(runs["ticks"]):
        for s, (lo, ln) in enumerate(SPANS):
            o = got[s][t]
            if not runs["emit"][i][s]:
                assert o is None and want[s][t] is None
                continue
            assert o.shape == (ln,) and np.array_equal(o, runs["pcm"][i][s, lo:lo + ln]), (t, s)
            changed = not np.array_equal(o, want[s][t])
            first = t == BS or (s == 0 and t == REOPEN + BS)         # a session's first chunk has nothing to fade from
            assert not changed or (XF[s] is not None and not first), (t, s)
            faded_ticks[s] += changed
        # the seam statistic: bitwise the restatement's sums, and its dB
        assert _bits_equal(rec["stats"][i], runs["stats"][i]), t
        ref_db = SR.seam_db(runs["stats"][i])
        assert all((np.isnan(a) and np.isnan(b)) or a == b for a, b in zip(rec["db"][i], ref_db)), t
        print(f"tick {t}: seam_db {['%.1f' % v for v in rec['db'][i]]}, stored {rec['stored'][i]}")
    print("chunks that differ from the hard cut:", faded_ticks, "of", [TICKS - BS - BS - 2, TICKS - BS - 1, 0], "faded")
    assert faded_ticks[0] > 0 and faded_ticks[1] > 0 and faded_ticks[2] == 0
    # the fade is min(X, stored) long: after the longer setting the tail holds 220, then 397, then 88
    at = lambda t: rec["stored"][t - BS]                             # noqa: E731
    assert at(BS + 3) == [160, 220, 0] and at(BS + 4) == [160, 397, 0] and at(BS + 5) == [160, 88, 0]
    assert at(REOPEN) == [0, 88, 0] and at(REOPEN + BS) == [160, 88, 0] and rec["stored"][-1] == runs["stored"].tolist()
    assert np.isnan(rec["db"][REOPEN]) [0] and np.isnan(rec["db"][0]).all() and np.isnan([d[2] for d in rec["db"]]).all()
    assert all(np.isfinite(d[1]) for d in rec["db"][1:])
    # the 44.1 kHz session: span 440, shift 441
    assert conv.span_len.tolist()[1] == 440 and conv.shift.tolist()[1] == 441 and got[1][BS].shape == (440,)
    with pytest.raises(ValueError, match=r"slot 1: crossfade_ms=10 is 441 samples at 44100 Hz"):
        conv.set(1, crossfade_ms=10)


def test_enable_graph_in_the_middle_leaves_the_stream_unchanged(pool, runs):
    g_out, g_rec, conv = _xf_run(pool, graph_at=BS + 3)
    assert all(_same(a, b) for a, b in zip(g_out, runs["got"]))
    assert all(_bits_equal(a, b) for a, b in zip(g_rec["stats"], runs["rec"]["stats"])) and g_rec["stored"] == runs["rec"]["stored"]
    # captured once: the longer and the shorter crossfade, the close and the open never re-captured
    assert g_rec["captures"] == [0] * 3 + [1] * (TICKS - BS - 3) and conv.captures == 1
    conv.set(2, crossfade_ms=10)
    conv.set(0, crossfade_ms=None)
    conv.step({s: np.zeros(c, np.int16) for s, c in enumerate(CHUNKS)})
    assert conv.captures == 1 and conv.xlen.tolist() == [0, 88, 480] and conv.stored.tolist() == [0, 88, 480]
    conv.close(1)
    assert conv.xlen.tolist() == [0, 0, 480] and conv.stored.tolist() == [0, 0, 480] and conv.shift.tolist() == [160, 160, 480]


# ---------------------------------------------------------------------------------------------------- 3. with the gate
SHORT = 46
SHORT_QUIET = range(20, 34)
GATE = dict(gate_db=-40, gate_hold=0.0)


def _script(seed, ticks, quiet):
    pcm = _pcm(CHUNK * ticks, seed).copy()
    for c in quiet:
        pcm[c * CHUNK:(c + 1) * CHUNK] = 0
    return pcm


def test_a_gated_crossfading_session_through_silence_follows_both_restatements(pool):
    """slot 0 gated and crossfading over 5 ms, slot 1 crossfading over 10 ms without a gate, through speech, silence and speech: every
    chunk is the twin's wave, faded by seam_ref (with the gate's gains: a skipped tick leaves nothing to fade from), times gate_ref's
    ramp"""
    kw = dict(chunk=CHUNK, buffersize=BS, k=4)
    pcm = [_script(80, SHORT, SHORT_QUIET), _pcm(CHUNK * SHORT, 81)]
    plain = MS.MultiStreamConverter(*_nets(), pool, 2, **kw)
    waves = _tap(plain)
    want = _drive(plain, [dict(voice="v1"), dict(voice="v0")], pcm, SHORT, [CHUNK] * 2)
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, gate=True, crossfade=True, **kw)
    rec = dict(g=[], db=[], stored=[], stats=[])

    def after(c, tick):
        rec["g"].append((c.g0.cpu().numpy(), c.g1.cpu().numpy()))
        rec["db"].append(c.seam_db())
        rec["stored"].append(c.stored.tolist())
        rec["stats"].append(c.seam_stats.cpu().numpy())
    got = _drive(conv, [dict(voice="v1", crossfade_ms=5, **GATE), dict(voice="v0", crossfade_ms=10)], pcm, SHORT, [CHUNK] * 2,
                 after=after)
    story = "".join({(0, 1): ">", (1, 1): "o", (1, 0): "<", (0, 0): "c"}[(int(a[0]), int(b[0]))] for a, b in rec["g"])
    print("story:", story)
    # fade in, speech, fade out at tick 28, closed (no search) from 29, fade in at 40, speech
    assert story == ">" + "o" * 11 + "<" + "c" * 11 + ">" + "o" * 5 and all(a[1] == 1 and b[1] == 1 for a, b in rec["g"])
    lo, ln = 1200, 160
    faded, _, stats, _, stored = SR.stream([w.cpu().numpy() for w in waves], [lo] * 2, [ln] * 2, [CHUNK] * 2, [80, 160], ld_tail=160,
                                           gains=rec["g"])
    for i, t in enumerate(range(BS, SHORT)):
        g0, g1 = rec["g"][i]
        y = GR.apply_rows(faded[i], [lo] * 2, [ln] * 2, g0, g1)
        pcm16 = audio_io.float_to_pcm16(torch.from_numpy(y).to(DEV)).cpu().numpy()[:, lo:lo + ln]
        assert np.array_equal(got[0][t], pcm16[0]) and np.array_equal(got[1][t], pcm16[1]), t
        kind = story[i]
        if kind != "c":                                              # (a skipped tick decodes the source: its sums are its own)
            assert _bits_equal(rec["stats"][i], stats[i]), t
        assert got[0][t].any() == (kind != "c")
        # what is stored after the tick: nothing after a skipped one
        assert rec["stored"][i] == [0 if kind == "c" else 80, 160], t
        faded_now = not np.isnan(rec["db"][i][0])                    # (tick 29 still fades from tick 28's tail, into silence)
        assert faded_now == (kind in "o<" or t == 29), t
    # the reopening chunk (tick 40) carries no fade: it is the twin's hard cut times the gate's ramp
    i = 40 - BS
    w = waves[i][0].cpu().numpy().copy()
    w[lo:lo + ln] = w[lo:lo + ln] * GR.ramp(0, 1, ln)
    assert np.array_equal(got[0][40], audio_io.float_to_pcm16(torch.from_numpy(w).to(DEV)).cpu().numpy()[lo:lo + ln])
    assert np.isnan(rec["db"][i][0]) and rec["stored"][i - 1][0] == 0 and rec["stored"][i][0] == 80
    # the closing chunk (tick 28): the crossfaded head times the ramp -- neither the twin's ramp alone nor the fade alone
    i = 28 - BS
    w = waves[i][0].cpu().numpy().copy()
    w[lo:lo + ln] = w[lo:lo + ln] * GR.ramp(1, 0, ln)
    only_ramp = audio_io.float_to_pcm16(torch.from_numpy(w).to(DEV)).cpu().numpy()[lo:lo + ln]
    only_fade = audio_io.float_to_pcm16(torch.from_numpy(faded[i][0]).to(DEV)).cpu().numpy()[lo:lo + ln]
    assert not np.array_equal(got[0][28], only_ramp) and not np.array_equal(got[0][28], only_fade)
    assert np.array_equal(got[0][28][80:], only_ramp[80:])                # past the 5 ms head: the ramp alone
    # open ticks after the head are the ungated, hard-cut twin
    assert np.array_equal(got[0][45][80:], want[0][45][80:]) and not np.array_equal(got[0][45][:80], want[0][45][:80])
    assert stored.tolist() == [80, 160]


# ---------------------------------------------------------------------------------------------------- 4. RealtimeConverter
@pytest.mark.parametrize("graph", [False, True])
def test_a_crossfading_realtime_converter_is_bitwise_a_one_slot_multistream(graph):
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(400, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, reuse_interior=False, crossfade_ms=5, **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, crossfade=True, **kw)
    ms.open(0, "lib", pitch=1.5, alpha=0.2, crossfade_ms=5)
    plain = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, reuse_interior=False, **kw)
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    ticks, differ = BS + 5, 0
    pcm = _pcm(CHUNK * ticks, 80)
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b, p = rt.step(c), ms.step({0: c})[0], plain.step(c)
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b), t
            assert rt._seam_stored.tolist() == ms.stored.tolist() == [80] and torch.equal(rt._seam_tail[:, :80], ms.tail[:, :80])
            da, db = rt.seam_db(), ms.seam_db()[0]
            assert (np.isnan(da) and np.isnan(db) and t == BS) or (da == db and np.isfinite(da) and t > BS)
            assert (t > BS or np.array_equal(a, p)) and np.array_equal(a[80:], p[80:])       # only the 5 ms head moves
            differ += not np.array_equal(a, p)
    assert differ > 0
    # reset() drops the tail: the next stream's first chunk is not faded
    rt.reset()
    plain.reset()
    assert rt._seam_stored.tolist() == [0]
    for t in range(BS + 1):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, p = rt.step(c), plain.step(c)
    assert np.array_equal(a, p) and np.isnan(rt.seam_db()) and rt._seam_stored.tolist() == [80]
    # a ring unrelated to the previous one (continues=False) drops it too
    ring = audio_io.pcm16_to_float(torch.from_numpy(np.concatenate(rt.ring)).to(DEV)).unsqueeze(0)
    rt.step_device(ring, continues=False)
    assert np.isnan(rt.seam_db()) and rt._seam_stored.tolist() == [80]
    rt.step_device(ring, continues=True)
    assert np.isfinite(rt.seam_db())
    with pytest.raises(ValueError, match="seam_db needs a converter built with"):
        plain.seam_db()
    with pytest.raises(ValueError, match=r"crossfade_ms=11 is 176 samples"):
        RealtimeConverter(*_nets(), lib, "cuda", crossfade_ms=11, **kw)


def test_a_crossfading_realtime_converter_with_interior_reuse_is_bitwise_itself_without():
    """-c 960 -b 26: a ring of 78 frames advancing by 3"""
    from module.realtime import RealtimeConverter
    chunk, bs, ticks = 960, 26, 31
    lib = synthetic.make_library(400, 1)
    pcm = _pcm(chunk * ticks, 95)
    outs, dbs = {}, {}
    for reuse in (False, "auto"):
        rt = RealtimeConverter(*_nets(), lib, "cuda", chunk=chunk, buffersize=bs, k=4, alpha=0.1, reuse_interior=reuse, crossfade_ms=5)
        assert rt.reuse == bool(reuse) and rt._seam_x.tolist() == [80] and rt._seam_shift.tolist() == [960]
        outs[reuse], dbs[reuse] = [], []
        for t in range(ticks):
            o = rt.step(pcm[t * chunk:(t + 1) * chunk])
            if o is not None:
                outs[reuse].append(o)
                dbs[reuse].append(rt.seam_db())
    assert len(outs[False]) == ticks - bs
    assert all(np.array_equal(a, b) for a, b in zip(outs[False], outs["auto"]))
    assert np.isnan(dbs[False][0]) and np.isnan(dbs["auto"][0]) and dbs[False][1:] == dbs["auto"][1:]
    assert all(np.isfinite(d) for d in dbs[False][1:])


@pytest.mark.parametrize("graph", [False, True])
def test_the_bf16_repeat_starts_from_the_tail_the_tick_started_from(pool, monkeypatch, graph):
    """the repeat of a tick (after an fp16 saturation) with the switch of the process to bf16 planes stubbed out: the same tick again
    gives the same crossfaded samples -- faded from the tail the tick started from, not from the one its first attempt saved"""
    from module.realtime import RealtimeConverter
    monkeypatch.setattr(MS.ops, "switch_to_bf16", lambda *a: None)
    ticks = BS + 3
    pcm = _pcm(CHUNK * ticks, 80)
    conv = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=CHUNK, buffersize=BS, k=4, crossfade=True)
    conv.open(0, "v0", crossfade_ms=5)
    rt = RealtimeConverter(*_nets(), pool.tokens("v0")[None], "cuda", chunk=CHUNK, buffersize=BS, k=4, reuse_interior=False,
                           crossfade_ms=5)
    if graph:
        conv.enable_graph()
        rt.enable_graph()
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        if t == ticks - 1:
            saved = (conv.phi.clone(), conv._seam_state(), rt._g_phi.clone() if graph else rt.phi,
                     (rt._seam_tail.clone(), rt._seam_stored.clone()))
        out, out_rt = conv.step({0: c})[0], rt.step(c)
    after = conv._seam_state(), (rt._seam_tail.clone(), rt._seam_stored.clone()), conv.seam_db()[0], rt.seam_db()
    assert saved[1][1].tolist() == [80] == saved[3][1].tolist() and np.isfinite(after[2]) and np.isfinite(after[3])      # the tick did fade
    assert not torch.equal(saved[1][0], after[0][0]) and not torch.equal(saved[3][0], after[1][0])
    lo, ln = conv._span(CHUNK)
    again = conv._repeat_on_bf16(saved[0], None, None, saved[1])
    assert np.array_equal(again[0, lo:lo + ln], out) and conv.seam_db()[0] == after[2]
    assert torch.equal(conv.tail, after[0][0]) and conv.stored.tolist() == [80]
    data = audio_io.pcm16_to_float(torch.from_numpy(np.concatenate(rt.ring)).to(DEV)).unsqueeze(0)
    again = rt._repeat_on_bf16(data, saved[2], None, saved[3])
    assert np.array_equal(again[lo:lo + ln], out_rt) and rt.seam_db() == after[3]
    assert torch.equal(rt._seam_tail, after[1][0]) and rt._seam_stored.tolist() == [80]


# ---------------------------------------------------------------------------------------------------- 5. the CLI
def test_multistream_cli_with_a_crossfading_session_writes_what_the_converter_emits(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    for name, net in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _nets()):
        torch.save(net.state_dict(), d / name)
    nets = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    ticks = BS + 6
    wav = _pcm(CHUNK * ticks, 80).astype(np.float32) / 32767
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    base = [dict(input="in0.wav", lib="voice_library.pt"), dict(input="in1.wav", lib="voice_library.pt")]
    json.dump([dict(base[0], crossfade_ms=5), base[1]], open(d / "xf.json", "w"))
    json.dump(base, open(d / "plain.json", "w"))
    json.dump([base[0], dict(base[1], crossfade_ms=None)], open(d / "null.json", "w"))
    common = nets + ["-c", str(CHUNK), "-b", str(BS)]
    msi.main(common + ["-o", str(d / "out_xf"), str(d / "xf.json")])
    msi.main(common + ["-o", str(d / "out_plain"), str(d / "plain.json")])
    msi.main(common + ["-o", str(d / "out_flag"), "--crossfade", "5", str(d / "null.json")])
    ss = msi.load_sessions(str(d / "xf.json"))
    assert ss[0]["crossfade_ms"] == 5.0 and "crossfade_ms" not in ss[1]

    def read(sub):
        out = []
        for p in (d / sub / "0_in0.wav", d / sub / "1_in1.wav"):
            g, sr = audio_io.load(str(p))
            assert sr == 16000
            out.append(np.round(g[0].numpy() * 32768).astype(np.int16))
        return out
    CE, PE, Dec = (n.to(DEV) for n in _nets())
    CE.load_state_dict(torch.load(d / "content_encoder.pt"))
    PE.load_state_dict(torch.load(d / "f0_estimator.pt"))
    Dec.load_state_dict(torch.load(d / "decoder.pt"))
    vpool = MS.VoicePool()
    name = msi.voice_name(None, str(d / "voice_library.pt"))
    vpool.add(name, msi.voice_tokens(CE, None, str(d / "voice_library.pt"), DEV))
    pcms = [msi.input_pcm(s["input"], 16000, DEV) for s in ss]
    # the API runs: a crossfade=True converter with session 0 at 5 ms, and the converter as it was always built
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4, crossfade=True)
    want_xf = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, crossfade_ms=5.0), dict(voice=name)])
    conv = MS.MultiStreamConverter(CE, PE, Dec, vpool, 2, chunk=CHUNK, buffersize=BS, k=4)
    want_plain = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name), dict(voice=name)])
    xf, plain, flag = read("out_xf"), read("out_plain"), read("out_flag")
    assert all(len(w) == CHUNK * (ticks - BS) for w in want_xf + want_plain)
    assert np.array_equal(xf[0], want_xf[0]) and np.array_equal(xf[1], want_xf[1])
    # a file without the key, run without the flag: what the converter built without crossfade writes, byte for byte
    assert np.array_equal(plain[0], want_plain[0]) and np.array_equal(plain[1], want_plain[1])
    assert np.array_equal(xf[1], plain[1]) and not np.array_equal(xf[0], plain[0])
    assert np.array_equal(xf[0][:CHUNK], plain[0][:CHUNK])            # the first chunk has nothing to fade from
    # --crossfade as the default, switched off by a session's null: the same input twice, so the outputs swap roles
    assert np.array_equal(flag[0], xf[0]) and np.array_equal(flag[1], plain[1])
