"""The input gate on the device (csrc/gate.hip) and through the streaming converters, against the NumPy restatement tools/gate_ref.py.

1. alive_gate_rows: the level bitwise the restatement's ordered sum (and within 1e-12 of NumPy's mean), a row alone bitwise the row in a
   batch, the >= edge, a scripted hold sequence, rows that are off or filling, a NULL WORLD mask, guard bands.
2. alive_gate_apply_rows: bitwise the float32 formula for the four (g0, g1), spans at both ends and clamped, NaN handling, guard bands.
3. MultiStreamConverter(gate=True) at -c 160 -b 16 (ring 2560, 8 frames, window [1200, 1520)): no gated session -> bitwise the
   converter built without it; a gated session through speech / silence / low noise / speech against the restatement and the ungated
   twin; enable_graph in the middle of a hold; blend and per-session k; a 48 kHz session; auto pitch frozen while closed; a WORLD
   session out of WORLD's row mask while closed.
4. RealtimeConverter(gate_db=): bitwise a gated one-slot MultiStreamConverter; with interior reuse bitwise itself without; the bf16
   repeat of both converters restores the gate state.
5. multistream_inference.py on a sessions file with one gated session."""
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
            self.view.copy_(torch.as_tensor(init, dtype=dtype).view(*shape))

    def intact(self):
        s = torch.full((PAD,), self.sentinel, dtype=self.buf.dtype, device=DEV)
        return torch.equal(self.buf[:PAD], s) and torch.equal(self.buf[-PAD:], s)


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _gate_call(x, w_lo, w_hi, gate_on, thr, hold, emit, seg_len, S, state, world_on):
    """alive_gate_rows with every output between guard bands -> dict of host arrays (state: the updated one)"""
    n = x.shape[0]
    out = dict(state=Guarded((n, 2), torch.int32, -77, state), g0=Guarded((n,), torch.float32, 55.0),
               g1=Guarded((n,), torch.float32, 55.0), seg_len_eff=Guarded((n * S,), torch.int32, -77),
               follow=Guarded((n,), torch.uint8, 9), ms=Guarded((n,), torch.float64, -3.0))
    if world_on is not None:
        out["world_eff"] = Guarded((n,), torch.int32, -77)
    MS.gate_rows(x, w_lo, w_hi, _dev(gate_on, torch.int32), _dev(thr, torch.float64), _dev(hold, torch.int32),
                 _dev(emit, torch.uint8), None if world_on is None else _dev(world_on, torch.int32), S, _dev(seg_len, torch.int32),
                 out["state"].view, out["g0"].view, out["g1"].view, out["seg_len_eff"].view, out["follow"].view,
                 out["world_eff"].view if world_on is not None else None, out["ms"].view)
    torch.cuda.synchronize()
    assert all(g.intact() for g in out.values())
    return {k: g.view.cpu().numpy() for k, g in out.items()}


def _check_against_ref(got, ref, world):
    assert np.array_equal(got["state"], ref["state"])
    assert np.array_equal(got["g0"], ref["g0"]) and np.array_equal(got["g1"], ref["g1"])
    assert np.array_equal(got["seg_len_eff"], ref["seg_len_eff"])
    assert np.array_equal(got["follow"].astype(bool), ref["follow"])
    if world:
        assert np.array_equal(got["world_eff"], ref["world_eff"])


# ---------------------------------------------------------------------------------------------------- 1. the decision kernel
@pytest.mark.parametrize("N,S", [(1, 1), (1, 4), (3, 1), (3, 4), (1024, 1), (1024, 4)])
def test_gate_rows_against_the_restatement(N, S):
    rng = np.random.default_rng(100 * N + S)
    ld = 2563                                                            # (an odd stride)
    x = (rng.standard_normal((N, ld)) * 10.0 ** rng.uniform(-4, 0, size=(N, 1))).astype(np.float32)
    gate_on = (rng.uniform(size=N) < 0.8).astype(np.int32)
    emit = (rng.uniform(size=N) < 0.8).astype(np.uint8)
    if N >= 3:
        gate_on[:3], emit[:3] = (1, 0, 1), (1, 1, 0)
    else:
        gate_on[0] = emit[0] = 1
    thr = np.full(N, GR.thr_ms(-40))
    hold = rng.integers(0, 5, size=N).astype(np.int32)
    state = np.stack([rng.integers(0, 5, size=N), rng.integers(0, 2, size=N)], axis=1).astype(np.int32)
    state[:, 0] = np.minimum(state[:, 0], hold)
    seg_len = rng.integers(1, 900, size=N * S).astype(np.int32)
    world_on = rng.integers(0, 2, size=N).astype(np.int32)
    xd = torch.from_numpy(x).to(DEV)
    for w_lo, w_hi in ((1200, 1520), (5, 1000), (0, ld), (2562, 2563)):
        ms_ref = GR.mean_square(x, w_lo, w_hi)
        plain = (x[:, w_lo:w_hi].astype(np.float64) ** 2).mean(axis=1)
        ref = GR.gate_rows(state, ms_ref, gate_on, thr, hold, emit, seg_len, S, world_on)
        got = _gate_call(xd, w_lo, w_hi, gate_on, thr, hold, emit, seg_len, S, state, world_on)
        live = (gate_on != 0) & (emit != 0)
        rel = np.abs(got["ms"][live] - plain[live]) / plain[live]
        print(f"N={N} S={S} window [{w_lo}, {w_hi}): {int(live.sum())} live rows, ms max rel. error vs NumPy's mean {rel.max():.2e}, "
              f"open {int(ref['open'][live].sum())}")
        assert np.all(rel <= 1e-12)
        assert np.array_equal(got["ms"][live], ms_ref[live]) and np.all(got["ms"][~live] == 0.0)      # the ordered sum, bit for bit
        _check_against_ref(got, ref, True)
        # rows that are off or filling: everything passes, the state is the one that went in
        off = ~live
        assert np.array_equal(got["state"][off], state[off]) and np.all(got["g0"][off] == 1) and np.all(got["g1"][off] == 1)
        assert np.array_equal(got["seg_len_eff"].reshape(N, S)[off], seg_len.reshape(N, S)[off])
        assert np.array_equal(got["follow"][off], emit[off]) and np.array_equal(got["world_eff"][off], world_on[off])
        if (w_lo, w_hi) == (1200, 1520):
            assert N < 1024 or 0 < int(ref["open"][live].sum()) < int(live.sum())                        # both outcomes occur
            for r in sorted({0, N // 2, N - 1}):                         # a row alone is bitwise the row in the batch
                sl = slice(r, r + 1)
                one = _gate_call(xd[sl].contiguous(), w_lo, w_hi, gate_on[sl], thr[sl], hold[sl], emit[sl],
                                 seg_len[r * S:(r + 1) * S], S, state[sl], world_on[sl])
                assert one["ms"][0] == got["ms"][r] and np.array_equal(one["state"][0], got["state"][r])
                assert (one["g0"][0], one["g1"][0]) == (got["g0"][r], got["g1"][r])
                assert np.array_equal(one["seg_len_eff"], got["seg_len_eff"][r * S:(r + 1) * S])
            # a NULL WORLD mask: the same decisions, nothing else written
            nw = _gate_call(xd, w_lo, w_hi, gate_on, thr, hold, emit, seg_len, S, state, None)
            _check_against_ref(nw, ref, False)


def test_gate_rows_opens_at_exactly_the_threshold():
    """a constant 0.5 ring: every square and every partial sum is exact, ms == 0.25, and `>=` opens at thr_ms == 0.25"""
    x = torch.full((3, 2560), 0.5, device=DEV)
    thr = [0.25, np.nextafter(0.25, 1.0), np.nextafter(0.25, 0.0)]
    got = _gate_call(x, 1200, 1520, [1, 1, 1], thr, [0, 0, 0], [1, 1, 1], [5, 6, 7], 1, np.zeros((3, 2)), None)
    assert got["ms"].tolist() == [0.25, 0.25, 0.25]
    assert got["g1"].tolist() == [1.0, 0.0, 1.0] and got["g0"].tolist() == [0.0, 0.0, 0.0]
    assert got["seg_len_eff"].tolist() == [5, 0, 7] and got["state"].tolist() == [[0, 1], [0, 0], [0, 1]]


def test_gate_rows_follows_a_scripted_sequence_tick_by_tick():
    """12 ticks, hold 3: row 0 gated, row 1 gated but filling on ticks 4-5, row 2 not gated; the state lives on the device"""
    script = [0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0]
    N, S, ld = 3, 2, 400
    state = Guarded((N, 2), torch.int32, -77, np.zeros((N, 2)))
    outs = dict(g0=Guarded((N,), torch.float32, 55.0), g1=Guarded((N,), torch.float32, 55.0),
                seg=Guarded((N * S,), torch.int32, -77), follow=Guarded((N,), torch.uint8, 9), weff=Guarded((N,), torch.int32, -77))
    gate_on, thr, hold, seg_len, world_on = [1, 1, 0], [GR.thr_ms(-40)] * 3, [3, 3, 3], [10, 0, 20, 30, 40, 0], [1, 0, 1]
    ref_state, opens = np.zeros((N, 2), dtype=np.int32), []
    for t, loud in enumerate(script):
        x = np.full((N, ld), 0.1 if loud else 0.001, dtype=np.float32)              # -20 dB and -60 dB: 20 dB either side of -40
        emit = [1, 0 if t in (4, 5) else 1, 1]
        MS.gate_rows(torch.from_numpy(x).to(DEV), 100, 260, _dev(gate_on, torch.int32), _dev(thr, torch.float64),
                     _dev(hold, torch.int32), _dev(emit, torch.uint8), _dev(world_on, torch.int32), S, _dev(seg_len, torch.int32),
                     state.view, outs["g0"].view, outs["g1"].view, outs["seg"].view, outs["follow"].view, outs["weff"].view)
        ref = GR.gate_rows(ref_state, GR.mean_square(x, 100, 260), gate_on, thr, hold, emit, seg_len, S, world_on)
        ref_state = ref["state"]
        assert np.array_equal(state.view.cpu().numpy(), ref_state), t
        assert np.array_equal(outs["g0"].view.cpu().numpy(), ref["g0"]) and np.array_equal(outs["g1"].view.cpu().numpy(), ref["g1"]), t
        assert np.array_equal(outs["seg"].view.cpu().numpy(), ref["seg_len_eff"]), t
        assert np.array_equal(outs["follow"].view.cpu().numpy().astype(bool), ref["follow"]), t
        assert np.array_equal(outs["weff"].view.cpu().numpy(), ref["world_eff"]), t
        opens.append(bool(ref_state[0, 1]))
    assert opens == [False, True, True, True, True, True, False, False, True, True, True, True]
    assert state.intact() and all(g.intact() for g in outs.values())
    assert ref_state[2].tolist() == [0, 0]                                           # the row without a gate never had a state


# ---------------------------------------------------------------------------------------------------- 2. the output edge
def test_gate_apply_rows_is_bitwise_the_float32_formula():
    ld = 1000
    spans = [(0, 441), (ld - 441, 441), (ld - 100, 441), (5, 1), (ld - 1, 1), (300, 441), (-7, 20), (17, 0)]
    gains = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)]
    rows = [(lo, ln, a, b) for lo, ln in spans for a, b in gains]
    N = len(rows)
    rng = np.random.default_rng(5)
    y = rng.standard_normal((N, ld)).astype(np.float32)
    for n, (lo, ln, a, b) in enumerate(rows):
        if a == b:                                                       # a NaN in the span of every (1, 1) and (0, 0) row
            y[n, min(max(lo, 0) + ln // 2, ld - 1)] = np.nan
    buf = Guarded((N, ld), torch.float32, 123.0, y)
    lo, ln, g0, g1 = (np.array(c) for c in zip(*rows))
    want = GR.apply_rows(y, lo, ln, g0, g1)
    MS.gate_apply_rows_(buf.view, _dev(lo, torch.int32), _dev(ln, torch.int32), _dev(g0, torch.float32), _dev(g1, torch.float32))
    torch.cuda.synchronize()
    got = buf.view.cpu().numpy()
    assert buf.intact()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))       # bit for bit, NaNs and the sign of zero included
    for n, (lo_, ln_, a, b) in enumerate(rows):
        i0, i1 = max(lo_, 0), min(lo_ + ln_, ld)
        if (a, b) == (1.0, 1.0):
            assert np.array_equal(got[n].view(np.int32), y[n].view(np.int32)) and (ln_ == 0 or np.isnan(got[n]).any())
        elif (a, b) == (0.0, 0.0) and ln_ > 0:
            assert np.all(got[n, i0:i1].view(np.int32) == 0) and not np.isnan(got[n]).any()
        if ln_ > 0:                                                      # outside the span: never written
            assert np.array_equal(got[n, :i0], y[n, :i0]) and np.array_equal(got[n, i1:], y[n, i1:])
    # the ramp's last sample is g1 itself
    up = rows.index((0, 441, 0.0, 1.0))
    assert got[up, 440] == y[up, 440] and got[up, 0] == y[up, 0] * (np.float32(1.0) / np.float32(441.0))


# ---------------------------------------------------------------------------------------------------- 3. the converter
CHUNK, BS = 160, 16
TICKS = 60
W_LO, W_HI = 1200, 1520
GATE = dict(gate_db=-40, gate_hold=0.03)


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    p = MS.VoicePool(voices)
    for i, hz in enumerate((150.0, 700.0, 3000.0)):
        p.set_register(f"v{i}", hz=hz)
    return p


def _script(seed, ticks, quiet, noise=()):
    """speech-like PCM at scale 12000 in chunks of CHUNK; digital silence over the chunks `quiet`, N(0, 30) noise (about 20 dB under
    -40 dBFS) over the chunks `noise`"""
    pcm = _pcm(CHUNK * ticks, seed).copy()
    rng = np.random.default_rng(seed)
    for c in quiet:
        pcm[c * CHUNK:(c + 1) * CHUNK] = 0
    for c in noise:
        pcm[c * CHUNK:(c + 1) * CHUNK] = np.round(rng.standard_normal(CHUNK) * 30.0).astype(np.int16)
    return pcm


def _tap(conv):
    """keep every tick's float waves (before float_to_pcm16)"""
    waves, run = [], conv._run

    def wrapped():
        w = run()
        waves.append(w.clone())
        return w
    conv._run = wrapped
    return waves


def _drive(conv, sess, pcm, ticks, chunks=None, actions=None, after=None):
    """-> per session the list of per-tick outputs (None while its ring fills)"""
    chunks = chunks or [CHUNK] * len(sess)
    outs = [[] for _ in sess]
    for s, p in enumerate(sess):
        conv.open(s, **p)
    for tick in range(ticks):
        for a in (actions or {}).get(tick, []):
            a(conv)
        feed = {s: pcm[s][tick * c:(tick + 1) * c] for s, c in enumerate(chunks)}
        for s, o in conv.step(feed).items():
            outs[s].append(o)
        if after is not None and tick >= BS:
            after(conv, tick)
    return outs


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
                                    for x, y in zip(a, b))


def _expected_flags(conv, slot, log, ref_state):
    """after an emitting tick: the restatement on the host copy of the slot's ring (at 16 kHz and gain 0 the device ring is
    ring / 32768 exactly) -> appends (g0, g1, open, margin in dB) to log"""
    x = conv.ring[slot:slot + 1, :CHUNK * BS].astype(np.float32) / np.float32(32768.0)
    ms = GR.mean_square(x, W_LO, W_HI)
    thr = GR.thr_ms(GATE["gate_db"])
    r = GR.gate_rows(ref_state[0], ms, [1], [thr], [GR.hold_ticks(GATE["gate_hold"], CHUNK / 16000)], [1], [1])
    ref_state[0] = r["state"]
    margin = abs(10.0 * np.log10(max(ms[0], 1e-30) / thr))
    log.append((float(r["g0"][0]), float(r["g1"][0]), bool(r["open"][0]), margin))


SESS = [dict(voice="v0", pitch=1.0), dict(voice="v1", alpha=0.1), dict(voice="v2", f0_rate=0.9)]
QUIET, NOISE = range(28, 40), range(40, 48)


def _script_pcm():
    return [_pcm(CHUNK * TICKS, 70), _script(71, TICKS, QUIET, NOISE), _pcm(CHUNK * TICKS, 72)]


def _gated_run(pool, graph_at=None):
    """slot 1 gated, through the script -> (outputs, per-tick records, the converter)"""
    conv = MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, gate=True)
    rec = dict(open=[], seg=[], state=[], ref=[], ref_state=[np.zeros((1, 2), dtype=np.int32)])

    def after(c, tick):
        rec["open"].append(c.gate_open())
        rec["seg"].append(c.seg_len_eff.tolist())
        rec["state"].append(c.gate_state.tolist())
        _expected_flags(c, 1, rec["ref"], rec["ref_state"])
    acts = {} if graph_at is None else {graph_at: [lambda c: c.enable_graph()]}
    outs = _drive(conv, [SESS[0], dict(SESS[1], **GATE), SESS[2]], _script_pcm(), TICKS, actions=acts, after=after)
    return outs, rec, conv


@pytest.fixture(scope="module")
def runs(pool):
    """the ungated converter (outputs and float waves) and the gated one, eager, over the same script: computed once"""
    plain = MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4)
    waves = _tap(plain)
    want = _drive(plain, SESS, _script_pcm(), TICKS)
    got, rec, conv = _gated_run(pool)
    return dict(want=want, waves=waves, got=got, rec=rec, conv=conv)


@pytest.mark.parametrize("graph", [False, True])
def test_a_gate_converter_with_no_gated_session_is_bitwise_the_plain_converter(pool, runs, graph):
    ticks = 24
    conv = MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, gate=True)
    if graph:
        conv.enable_graph()
    got = _drive(conv, [dict(p, gate_db=None) for p in SESS], _script_pcm(), ticks)
    assert all(sum(o is not None for o in g) == ticks - BS for g in got)
    assert all(_same(g, w[:ticks]) for g, w in zip(got, runs["want"]))
    assert conv.gate_state.abs().sum().item() == 0 and conv.gate_open() == [True] * 3
    assert torch.equal(conv.seg_len_eff, conv.seg_len) and conv.g0.tolist() == [1.0] * 3 == conv.g1.tolist()
    assert conv.captures == int(graph)
    plain = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=CHUNK, buffersize=BS, k=4)
    with pytest.raises(ValueError, match=r"slot 0: gate_db=-40 needs a converter built with MultiStreamConverter\(..., gate=True\)"):
        plain.open(0, "v0", gate_db=-40)
    assert not plain.is_open[0]
    with pytest.raises(ValueError, match="gate_open needs a converter built with"):
        plain.gate_open()
    before = {a: getattr(conv, a).clone() for a in ("gate_on", "thr_ms", "hold_ticks", "gate_state", "pitch", "seg_len")}
    for bad in (dict(gate_db=float("nan")), dict(gate_db="x"), dict(gate_db=-40, gate_hold=-1), dict(gate_hold=None, pitch=3.0)):
        with pytest.raises(ValueError, match="slot 1: gate_"):
            conv.set(1, **bad)
    assert all(torch.equal(getattr(conv, a), v) for a, v in before.items()) and conv.params[1]["pitch"] == 0.0


def test_a_gated_session_follows_the_restatement_and_its_ungated_twin(runs):
    want, waves, got, rec, conv = (runs[k] for k in ("want", "waves", "got", "rec", "conv"))
    hold = GR.hold_ticks(GATE["gate_hold"], CHUNK / 16000)
    assert int(conv.hold_ticks[1]) == hold == 3 and float(conv.thr_ms[1]) == 1e-4 and conv.captures == 0
    assert conv.span_lo.tolist() == [BS * CHUNK // 2 - CHUNK // 2] * 3 and conv.span_len.tolist() == [CHUNK] * 3
    lo, ln = int(conv.span_lo[1]), int(conv.span_len[1])
    seg = conv.seg_len.tolist()
    kinds = []
    for i, tick in enumerate(range(BS, TICKS)):
        g0, g1, is_open, margin = rec["ref"][i]
        print(f"tick {tick}: g0 {g0:.0f} g1 {g1:.0f}, level {margin:.1f} dB from the threshold, device open {rec['open'][i][1]}")
        assert margin >= 6.0, (tick, margin)                             # (the script keeps rounding out of every decision)
        assert rec["open"][i] == [True, is_open, True], tick
        assert rec["state"][i][1][1] == int(is_open) and rec["state"][i][0] == [0, 0] == rec["state"][i][2]
        o = got[1][tick]
        if (g0, g1) == (1.0, 1.0):                                       # steady open: the ungated converter, bit for bit
            kinds.append("open")
            assert np.array_equal(o, want[1][tick]) and rec["seg"][i] == seg, tick
        elif (g0, g1) == (0.0, 0.0):                                     # closed: silence, and no search
            kinds.append("closed")
            assert o.dtype == np.int16 and not o.any() and rec["seg"][i] == [seg[0], 0, seg[2]], tick
        else:                                                            # an edge: the ungated float wave times the ramp, then PCM
            kinds.append("in" if g1 else "out")
            w = waves[i][1].cpu().numpy().copy()
            w[lo:lo + ln] = w[lo:lo + ln] * GR.ramp(g0, g1, ln)
            pcm = audio_io.float_to_pcm16(torch.from_numpy(w).to(DEV)).cpu().numpy()[lo:lo + ln]
            assert np.array_equal(o, pcm) and rec["seg"][i] == seg and not np.array_equal(o, want[1][tick]), tick
        assert np.array_equal(got[0][tick], want[0][tick]) and np.array_equal(got[2][tick], want[2][tick]), tick
    assert all(o is None for g in got for o in g[:BS])
    # the script's story: fade in, speech, three held ticks, fade out, closed through silence and low noise, fade in, speech
    story = "".join(dict(open="o", closed="c", out="<", **{"in": ">"})[k] for k in kinds)
    print("story:", story)
    assert story == ">" + "o" * 22 + "<" + "c" * 14 + ">" + "o" * 5
    assert len(waves) == TICKS - BS


def test_enable_graph_in_the_middle_of_a_hold_is_bitwise_the_eager_run(pool, runs):
    got, rec = runs["got"], runs["rec"]
    at = BS + 21                                                         # the second held tick: hold_left is 2 going in
    assert rec["state"][at - 1 - BS][1] == [2, 1]
    g_out, g_rec, conv = _gated_run(pool, graph_at=at)
    assert conv.captures == 1
    assert all(_same(a, b) for a, b in zip(g_out, got))
    assert g_rec["open"] == rec["open"] and g_rec["seg"] == rec["seg"] and g_rec["state"] == rec["state"]
    # toggling and retuning between ticks never re-capture
    conv.set(1, gate_db=-30, gate_hold=0.0)
    conv.set(0, gate_db=-50)
    conv.set(1, gate_db=None)
    conv.step({s: np.zeros(CHUNK, np.int16) for s in range(3)})
    assert conv.captures == 1 and conv.gate_on.tolist() == [1, 0, 0] and conv.gate_open()[1] is True


SHORT = 46
SHORT_QUIET = range(20, 34)


@pytest.mark.parametrize("blend,k_max", [(2, None), (1, 8), (2, 8)])
def test_every_list_row_of_a_gated_slot_goes_to_zero_and_comes_back(pool, blend, k_max):
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, blend=blend, k_max=k_max, gate=True)
    voice = {"v1": 2, "v2": 1} if blend == 2 else "v1"
    sess = [dict(voice=voice, gate_db=-40, gate_hold=0.0, **(dict(k=6) if k_max else {})), dict(voice="v0")]
    segs, opens = [], []

    def after(c, tick):
        segs.append(c.seg_len_eff.tolist())
        opens.append(c.gate_open()[0])
    outs = _drive(conv, sess, [_script(80, SHORT, SHORT_QUIET), _pcm(CHUNK * SHORT, 81)], SHORT, after=after)
    full = conv.seg_len.tolist()
    assert len(full) == 2 * blend and all(v > 0 for v in full[:blend])
    closed = [0] * blend + full[blend:]
    # window = chunks t - 8 (half), t - 7, t - 6 (half): loud up to tick 27, fade out at 28, closed 29 .. 39, loud again from 40
    want_open = [t <= 27 or t >= 40 for t in range(BS, SHORT)]
    assert opens == want_open
    for i, t in enumerate(range(BS, SHORT)):
        assert segs[i] == (closed if 29 <= t <= 39 else full), t
        assert outs[0][t].any() == (not 29 <= t <= 39), t
        assert outs[1][t].any()


def test_a_48k_sessions_ramp_covers_its_own_span(pool):
    kw = dict(chunk=CHUNK, buffersize=BS, k=4, rates=[16000, 48000])
    ticks = BS + 2
    pcm = [_pcm(CHUNK * ticks, 90), _pcm(3 * CHUNK * ticks, 91)]
    sess = [dict(voice="v0"), dict(voice="v1", rate=48000)]
    plain = MS.MultiStreamConverter(*_nets(), pool, 2, **kw)
    waves = _tap(plain)
    want = _drive(plain, sess, pcm, ticks, chunks=[CHUNK, 3 * CHUNK])
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, gate=True, **kw)
    got = _drive(conv, [sess[0], dict(sess[1], **GATE)], pcm, ticks, chunks=[CHUNK, 3 * CHUNK])
    assert conv.span_lo.tolist() == [1200, 3600] and conv.span_len.tolist() == [160, 480]
    w = waves[0][1].cpu().numpy().copy()                                 # the first emitting tick: the gated session fades in
    w[3600:4080] = w[3600:4080] * GR.ramp(0, 1, 480)
    pcm16 = audio_io.float_to_pcm16(torch.from_numpy(w).to(DEV)).cpu().numpy()[3600:4080]
    assert got[1][BS].shape == (480,) and np.array_equal(got[1][BS], pcm16) and not np.array_equal(got[1][BS], want[1][BS])
    assert np.array_equal(got[1][BS + 1], want[1][BS + 1])               # then open: the ungated converter
    assert all(np.array_equal(got[0][t], want[0][t]) for t in (BS, BS + 1))
    conv.close(1)
    assert conv.span_lo.tolist() == [1200, 1200] and conv.gate_on.tolist() == [0, 0]


def test_auto_pitch_register_is_frozen_while_the_gate_is_closed(pool):
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, auto_pitch=True, gate=True)
    sess = [dict(voice="v0", auto_pitch=True, gate_db=-40, gate_hold=0.0), dict(voice="v1", auto_pitch=True)]
    regs, opens = [conv.reg_state.clone()], []

    def after(c, tick):
        regs.append(c.reg_state.clone())
        opens.append(c.gate_open()[0])
    one = _script(80, SHORT, SHORT_QUIET)
    _drive(conv, sess, [one, one], SHORT, after=after)
    assert opens.count(False) == 12 and opens[0] and opens[-1]           # the fade-out tick and the eleven closed ones
    for i, is_open in enumerate(opens):
        moved = not torch.equal(regs[i + 1][0], regs[i][0])
        assert moved == is_open, (i, is_open)                            # frozen bit for bit while closed, learning while open
        assert not torch.equal(regs[i + 1][1], regs[i][1])               # the ungated twin keeps learning (from the room's silence)
    assert conv.follow.view(-1).tolist() == [True, True]
    conv.close(0)
    assert conv.gate_state[0].tolist() == [0, 0] and int(conv.gate_on[0]) == 0


def test_a_closed_gate_takes_its_session_out_of_the_world_branch(pool):
    """two WORLD sessions on the same input, slot 0 gated: its row leaves WORLD's mask on the ticks it is closed at both ends, and on
    its open ticks before that it is bitwise its ungated twin in a converter built without the gate (a skipped WORLD row's f0 is 0, so
    its oscillator phase does not advance through a closed gate: after one, the session is no longer its twin sample for sample)"""
    kw = dict(chunk=CHUNK, buffersize=BS, k=4, world_pitch=True)
    one = _script(80, SHORT, SHORT_QUIET)
    sess = [dict(voice="v1", world_pitch=True), dict(voice="v1", world_pitch=True)]
    want = _drive(MS.MultiStreamConverter(*_nets(), pool, 2, **kw), sess, [one, one], SHORT)
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, gate=True, **kw)
    masks = []
    got = _drive(conv, [dict(sess[0], gate_db=-40, gate_hold=0.0), sess[1]], [one, one], SHORT,
                 after=lambda c, tick: masks.append(c.world_eff.tolist()))
    assert conv.world_on.tolist() == [1, 1]
    for i, t in enumerate(range(BS, SHORT)):
        assert masks[i] == [0 if 29 <= t <= 39 else 1, 1], t
        assert np.array_equal(got[1][t], want[1][t]), t
        if BS < t <= 27:                                                 # open, and the phase has not yet sat through a closed gate
            assert np.array_equal(got[0][t], want[0][t]), t
        assert got[0][t].any() == (not 29 <= t <= 39), t


# ---------------------------------------------------------------------------------------------------- 4. RealtimeConverter
@pytest.mark.parametrize("graph", [False, True])
def test_a_gated_realtime_converter_is_bitwise_a_gated_one_slot_multistream(graph):
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(400, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, reuse_interior=False, **GATE, **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, gate=True, **kw)
    ms.open(0, "lib", pitch=1.5, alpha=0.2, **GATE)
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    pcm = _script(80, SHORT, SHORT_QUIET)
    kinds = set()
    for t in range(SHORT):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b = rt.step(c), ms.step({0: c})[0]
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b), t
            assert rt.gate_open() == ms.gate_open()[0]
            assert rt._gate_state.tolist() == ms.gate_state.tolist()
            kinds.add((rt.gate_open(), bool(a.any())))
    assert kinds == {(True, True), (False, True), (False, False)}       # open, the fade-out tick, closed
    with pytest.raises(ValueError, match="gate_db="):
        RealtimeConverter(*_nets(), lib, "cuda", gate_db="x", **kw)
    with pytest.raises(ValueError, match="gate_hold="):
        RealtimeConverter(*_nets(), lib, "cuda", gate_db=-40, gate_hold=-1, **kw)
    rt.reset()
    assert rt._gate_state.tolist() == [[0, 0]]


def test_a_gated_realtime_converter_with_interior_reuse_is_bitwise_itself_without():
    """-c 960 -b 26: a ring of 78 frames advancing by 3, window [12000, 13920) = chunks t - 13 (half), t - 12, t - 11 (half)"""
    from module.realtime import RealtimeConverter
    chunk, bs, ticks = 960, 26, 44
    lib = synthetic.make_library(400, 1)
    pcm = _pcm(chunk * ticks, 95).copy()
    pcm[18 * chunk:30 * chunk] = 0
    outs, flags = {}, {}
    for reuse in (False, "auto"):
        rt = RealtimeConverter(*_nets(), lib, "cuda", chunk=chunk, buffersize=bs, k=4, alpha=0.1, reuse_interior=reuse, gate_db=-40,
                               gate_hold=0.03)
        assert rt.reuse == bool(reuse) and int(rt._gate_hold[0]) == 1
        outs[reuse], flags[reuse] = [], []
        for t in range(ticks):
            o = rt.step(pcm[t * chunk:(t + 1) * chunk])
            if o is not None:
                outs[reuse].append(o)
                flags[reuse].append(rt.gate_open())
    assert len(outs[False]) == ticks - bs and flags[False] == flags["auto"]
    assert all(np.array_equal(a, b) for a, b in zip(outs[False], outs["auto"]))
    # loud up to tick 30, one held tick, closed from 32, loud again from 41
    assert flags[False] == [t <= 31 or t >= 41 for t in range(bs, ticks)]
    assert not outs[False][33 - bs].any() and outs[False][32 - bs].any() and outs[False][41 - bs].any()


def test_the_bf16_repeat_starts_from_the_gate_state_the_tick_started_from(pool, monkeypatch):
    """the repeat of a tick (after an fp16 saturation) with the switch of the process to bf16 planes stubbed out: the same tick again,
    in the middle of a hold, gives the same samples and leaves the hold where the first run left it, not one tick further"""
    from module.realtime import RealtimeConverter
    monkeypatch.setattr(MS.ops, "switch_to_bf16", lambda *a: None)
    pcm = _script(80, SHORT, SHORT_QUIET)                                # loud up to tick 27; hold 3: left 2 after 28, 1 after 29
    conv = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=CHUNK, buffersize=BS, k=4, gate=True)
    conv.open(0, "v0", **GATE)
    rt = RealtimeConverter(*_nets(), pool.tokens("v0")[None], "cuda", chunk=CHUNK, buffersize=BS, k=4, reuse_interior=False, **GATE)
    for t in range(30):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        if t == 29:
            saved = conv.phi.clone(), conv.gate_state.clone(), rt.phi, rt._gate_state.clone()
        out, out_rt = conv.step({0: c})[0], rt.step(c)
    assert saved[1].tolist() == [[2, 1]] == saved[3].tolist() and conv.gate_state.tolist() == [[1, 1]] == rt._gate_state.tolist()
    lo, ln = conv._span(CHUNK)
    again = conv._repeat_on_bf16(saved[0], None, saved[1])
    assert np.array_equal(again[0, lo:lo + ln], out) and conv.gate_state.tolist() == [[1, 1]]
    data = audio_io.pcm16_to_float(torch.from_numpy(np.concatenate(rt.ring)).to(DEV)).unsqueeze(0)
    again = rt._repeat_on_bf16(data, saved[2], saved[3])
    assert np.array_equal(again[lo:lo + ln], out_rt) and rt._gate_state.tolist() == [[1, 1]]


# ---------------------------------------------------------------------------------------------------- 5. the CLI
def test_multistream_cli_with_a_gated_session_writes_what_the_converter_emits(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    for name, net in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _nets()):
        torch.save(net.state_dict(), d / name)
    nets = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    wav = _script(80, SHORT, SHORT_QUIET).astype(np.float32) / 32767
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    sessions = [dict(input="in0.wav", lib="voice_library.pt", gate_db=-40, gate_hold=0.0), dict(input="in1.wav", lib="voice_library.pt")]
    json.dump(sessions, open(d / "sessions.json", "w"))
    msi.main(nets + ["-c", str(CHUNK), "-b", str(BS), "-o", str(d / "out"), str(d / "sessions.json")])
    ss = msi.load_sessions(str(d / "sessions.json"))
    assert (ss[0]["gate_db"], ss[0]["gate_hold"]) == (-40.0, 0.0) and "gate_db" not in ss[1]
    CE, PE, Dec = (n.to(DEV) for n in _nets())
    CE.load_state_dict(torch.load(d / "content_encoder.pt"))
    PE.load_state_dict(torch.load(d / "f0_estimator.pt"))
    Dec.load_state_dict(torch.load(d / "decoder.pt"))
    pool = MS.VoicePool()
    name = msi.voice_name(None, str(d / "voice_library.pt"))
    pool.add(name, msi.voice_tokens(CE, None, str(d / "voice_library.pt"), DEV))
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, 2, chunk=CHUNK, buffersize=BS, k=4, gate=True)
    params = [dict(voice=name, gate_db=-40.0, gate_hold=0.0), dict(voice=name)]
    want = msi.run(conv, [msi.input_pcm(s["input"], 16000, DEV) for s in ss], [0, 0], CHUNK, params)
    got = []
    for p, w in zip((d / "out" / "0_in0.wav", d / "out" / "1_in1.wav"), want):
        g, sr = audio_io.load(str(p))
        assert sr == 16000 and len(w) == CHUNK * (SHORT - BS)
        got.append(np.round(g[0].numpy() * 32768).astype(np.int16))
        assert np.array_equal(got[-1], w), p
    # the same input twice: the gated session is silent over its closed ticks, the other one is not, and open ticks agree
    closed = slice((29 - BS) * CHUNK, (40 - BS) * CHUNK)
    assert not got[0][closed].any() and got[1][closed].any()
    assert np.array_equal(got[0][CHUNK:(28 - BS) * CHUNK], got[1][CHUNK:(28 - BS) * CHUNK])
