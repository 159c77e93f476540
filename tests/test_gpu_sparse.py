"""Sparse ticks on the device: csrc/ring.hip against the NumPy restatement tools/ring_ref.py, and MultiStreamConverter(sparse=True)
against the dense converter.  Every comparison is bitwise, or equality of int16 streams.

1. alive_ring_push_rows: six geometries (and a row whose lengths do not fit) in one call over 2 b + 3 ticks under five presence
   patterns, on 16-byte strides and on odd ones, S = 1 and S = 2; ring, x and the masked row arrays between guard bands.
2. The same at N = 1024 with seeded random presence.
3. The push replayed inside a captured graph while `present` and `chunks` are rewritten between replays.
4. alive_emit_rows against alive_float_to_pcm16 of the same floats, non-finite and out-of-range values included.
5. A sparse converter whose sessions are all present every tick is the dense converter (4 slots over four rates with gate, crossfade,
   limiter, auto pitch, per-session k and a blend; a close and a reopen; one capture), once more at B = 16.
6. A session's stream does not depend on its absences, nor on the others'; the states stand where they stood.
7. The masked row arrays of a tick with absent slots; step({}) moves nothing.
8. The bf16 repeat: the same samples, the ring pushed once.
9. The CLI: "stall" and --sparse write byte-identical wavs."""
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

import ring_ref as RR                                                # noqa: E402
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

    def host(self):
        return self.view.cpu().numpy()


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------------------------------------------- 1-3. alive_ring_push_rows
GEOM = [(80, 16), (160, 16), (441, 16), (480, 16), (160, 2), (1, 5)]  # (chunk_len, buffersize) per row
NOFIT = (500, 4)                                                     # a chunk longer than the chunk stride: the row is absent


def _presence(pattern, tick, n, rng):
    return {"all": [1] * n, "none": [0] * n, "alternating": [(tick + r) % 2 for r in range(n)],
            "one": [int(r == 2) for r in range(n)], "random": [int(v) for v in rng.integers(0, 2, n)]}[pattern]


class PushCase:
    """device arrays of one push problem between guard bands, and the host mirror that ring_ref moves on"""

    def __init__(self, geom, ld, ld_chunk, ld_x, S, seed):
        n = len(geom)
        rng = np.random.default_rng(seed)
        self.n, self.S, self.ld_chunk = n, S, ld_chunk
        self.cl, self.rl = [c for c, _ in geom], [c * b for c, b in geom]
        self.ring_h = rng.integers(-32768, 32768, (n, ld)).astype(np.int16)          # (whatever was there: absent rows keep it)
        self.x_h = rng.standard_normal((n, ld_x)).astype(np.float32)
        self.seg = rng.integers(1, 1000, n * S).astype(np.int32)
        self.world = rng.integers(0, 2, n).astype(np.int32)
        self.ring = Guarded((n, ld), torch.int16, -12345, self.ring_h)
        self.x = Guarded((n, ld_x), torch.float32, 7.5, self.x_h)
        self.seg_tick = Guarded((n * S,), torch.int32, -77)
        self.world_tick = Guarded((n,), torch.int32, -77)
        self.chunks = torch.zeros(n, ld_chunk, dtype=torch.int16, device=DEV)
        self.present = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.d = dict(cl=_dev(self.cl, torch.int32), rl=_dev(self.rl, torch.int32), seg=_dev(self.seg, torch.int32),
                      world=_dev(self.world, torch.int32))

    def load(self, chunks, present):
        self.chunks.copy_(torch.from_numpy(chunks))
        self.present.copy_(torch.tensor(present, dtype=torch.uint8))

    def launch(self):
        MS.ring_push_rows_(self.ring.view, self.chunks, self.d["cl"], self.d["rl"], self.present, self.x.view, self.d["seg"],
                           self.seg_tick.view, self.S, self.d["world"], self.world_tick.view)

    def reference(self, chunks, present):
        want = RR.push_rows(self.ring_h, chunks, self.cl, self.rl, present, self.x_h, self.seg, self.S, self.world)
        self.ring_h, self.x_h = want["ring"], want["x"]
        return want

    def check(self, want, where):
        assert np.array_equal(self.ring.host(), want["ring"]), where
        assert _bits_equal(self.x.host(), want["x"]), where
        assert np.array_equal(self.seg_tick.host(), want["seg_len_tick"]) and np.array_equal(self.world_tick.host(), want["world_tick"]), where
        assert self.ring.intact() and self.x.intact() and self.seg_tick.intact() and self.world_tick.intact(), where


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("ld,ld_chunk,ld_x", [(7680, 480, 7688), (7683, 481, 7681)], ids=["vector", "scalar"])
def test_push_rows_against_the_restatement_until_every_ring_has_turned_over_twice(ld, ld_chunk, ld_x, S):
    geom = GEOM + [NOFIT]
    for p, pattern in enumerate(["all", "none", "alternating", "one", "random"]):
        case = PushCase(geom, ld, ld_chunk, ld_x, S, 40 + p)
        rng = np.random.default_rng(50 + p)
        for tick in range(2 * 16 + 3):
            present = _presence(pattern, tick, len(geom), rng)
            chunks = rng.integers(-32768, 32768, (len(geom), ld_chunk)).astype(np.int16)
            before = case.ring_h.copy(), case.x_h.copy()
            want = case.reference(chunks, present)
            case.load(chunks, present)
            case.launch()
            case.check(want, (pattern, tick))
            for r, (rl, pr) in enumerate(zip(case.rl, present)):     # (what the restatement itself must say)
                if pr and r < len(GEOM):
                    assert not want["x"][r, rl:].any() and np.array_equal(want["ring"][r, rl:], before[0][r, rl:])
                else:
                    assert np.array_equal(want["ring"][r], before[0][r]) and _bits_equal(want["x"][r], before[1][r])
            assert want["seg_len_tick"].reshape(-1, S)[-1].tolist() == [0] * S and want["world_tick"][-1] == 0


def test_push_rows_at_1024_rows_with_random_presence():
    geom = [GEOM[r % len(GEOM)] for r in range(1024)]
    case = PushCase(geom, 7680, 480, 7680, 1, 60)
    rng = np.random.default_rng(61)
    for tick in range(3):
        present = _presence("random", tick, 1024, rng)
        chunks = rng.integers(-32768, 32768, (1024, 480)).astype(np.int16)
        want = case.reference(chunks, present)
        case.load(chunks, present)
        case.launch()
        case.check(want, tick)
        assert 300 < sum(present) < 724


def test_push_rows_replayed_in_a_captured_graph_while_presence_and_chunks_change():
    eager, graphed = PushCase(GEOM, 7680, 480, 7688, 2, 70), PushCase(GEOM, 7680, 480, 7688, 2, 70)
    rng = np.random.default_rng(71)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # (present is all zero: the warm-up launch moves nothing)
        graphed.launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.launch()
    want = None
    for tick in range(20):
        present = _presence("random" if tick % 5 else "all", tick, len(GEOM), rng)
        chunks = rng.integers(-32768, 32768, (len(GEOM), 480)).astype(np.int16)
        want = eager.reference(chunks, present)
        graphed.reference(chunks, present)
        for c in (eager, graphed):
            c.load(chunks, present)
        eager.launch()
        g.replay()
        eager.check(want, tick)
        graphed.check(want, tick)
    assert want is not None


# ---------------------------------------------------------------------------------------------------- 4. alive_emit_rows
@pytest.mark.parametrize("ld_out", [440, 443, 2100], ids=["vector", "scalar", "two-blocks"])
def test_emit_rows_is_float_to_pcm16_of_the_spans_and_zero_elsewhere(ld_out):
    ld = 3800
    rng = np.random.default_rng(80)
    wave = (rng.standard_normal((6, ld)) * 0.4).astype(np.float32)
    special = np.array([1.0, -1.0, 1.5, -3.0, 1e10, -1e10, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 32767.5 / 32768, -0.0], np.float32)
    for r in range(6):
        for lo in (1200, 3308):
            wave[r, lo + 3:lo + 3 + len(special)] = special
            wave[r, lo + 100 + r:lo + 100 + r + len(special)] = special[::-1]
    lo = [1200, 3308, 1200, 3308, 3700, -1]                           # rows 4 and 5: spans that leave the wave
    ln = [160, 440, 160, 440, 160, 160]
    take = [1, 1, 0, 1, 1, 1]
    if ld_out == 2100:
        lo[3], ln[3] = 1, 2100                                        # a span of more than one block of the grid
    w = _dev(wave, torch.float32)
    out = Guarded((6, ld_out), torch.int16, -999)
    MS.emit_rows_(w, _dev(lo, torch.int32), _dev(ln, torch.int32), torch.tensor(take, dtype=torch.uint8, device=DEV), out.view)
    flat = audio_io.float_to_pcm16(w).cpu().numpy()
    want = np.zeros((6, ld_out), np.int16)
    for r in (0, 1, 3):
        want[r, :ln[r]] = flat[r, lo[r]:lo[r] + ln[r]]
    got = out.host()
    assert np.array_equal(got, want) and out.intact() and want[0].any() and want[1].any() and want[3].any()
    finite = np.isfinite(wave) & (np.abs(wave) < 60000)               # where the restatement is defined: the same int16
    ref = RR.emit_rows(np.where(finite, wave, 0), lo, ln, take, ld_out)
    mask = RR.emit_rows(np.where(finite, np.float32(1.0 / 32768), np.float32(0)), lo, ln, take, ld_out) == 1
    assert np.array_equal(got[mask], ref[mask]) and mask.sum() > 500
    bools = torch.tensor(take, dtype=torch.bool, device=DEV)          # the converter's flags are bools: one byte each too
    out2 = Guarded((6, ld_out), torch.int16, -999)
    MS.emit_rows_(w, _dev(lo, torch.int32), _dev(ln, torch.int32), bools, out2.view)
    assert np.array_equal(out2.host(), want)


# ---------------------------------------------------------------------------------------------------- 5-8. the converter
CHUNK, BS = 160, 16
RATES = (8000, 16000, 44100, 48000)
CHUNKS = [80, 160, 441, 480]
ITEMS = 40                                                           # ticks of a session's own clock
QUIET = range(20, 28)                                                # slot 0's input is silent there: its gate closes and reopens
REOPEN_AT = 20                                                       # slot 2 spends this tick of its clock closed, then starts again
SESS = [dict(voice="v0", pitch=1.0, rate=8000, gate_db=-40, gate_hold=0.0, crossfade_ms=5),
        dict(voice={"v1": 2, "v2": 1}, f0_rate=0.9, rate=16000, auto_pitch=True, k=8, gain=60.0, limit_db=-1.0),
        dict(voice="v2", alpha=0.1, rate=44100, k=2, crossfade_ms=5, gain=60.0, limit_db=-3.0, limit_lookahead_ms=2.0),
        dict(voice="v0", alpha=0.2, f0_rate=1.1, rate=48000)]
STATE = ("phi", "reg_state", "gate_state", "stored", "tail", "limit_hist", "limit_gmin")


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    p = MS.VoicePool(voices)
    for name, hz in (("v0", 120.0), ("v1", 210.0), ("v2", 165.0)):
        p.set_register(name, hz=hz)
    return p


def _conv(pool, slots=4, **kw):
    return MS.MultiStreamConverter(*_nets(), pool, slots, chunk=CHUNK, buffersize=BS, k=4, rates=RATES, gate=True, crossfade=True,
                                   limiter=True, auto_pitch=True, k_max=8, blend=2, **kw)


def _inputs(slots=4):
    pcm = [_pcm(CHUNKS[s % 4] * ITEMS, 70 + s) for s in range(slots)]
    for s in range(0, slots, 4):
        pcm[s] = pcm[s].copy()
        pcm[s][QUIET.start * CHUNKS[0]:QUIET.stop * CHUNKS[0]] = 0
    return pcm


def _scripts(slots=4, items=ITEMS):
    """per session what it does on each tick of its own clock: supply chunk j, or (None) spend the tick closed"""
    out = [list(range(items)) for _ in range(slots)]
    for s in range(2, slots, 4):
        out[s] = list(range(REOPEN_AT)) + [None] + list(range(REOPEN_AT, items - 1))
    return out


def _drive(conv, pcm, scripts, stalls=None, graph_at=None):
    """run every session through its script; stalls[s] = {position: ticks it sits out before that position}.  Returns per session
    the emitted chunks by position, and per position what gate_open() / limit_db() said of it after the tick"""
    n = len(scripts)
    pos, wait = [0] * n, [dict(st) for st in (stalls or [{}] * n)]
    outs = [dict() for _ in range(n)]
    said = [dict() for _ in range(n)]
    tick = fed = 0
    while any(p < len(sc) for p, sc in zip(pos, scripts)):
        if graph_at == tick:
            conv.enable_graph()
        feed, at = {}, {}
        for s in range(n):
            if pos[s] >= len(scripts[s]):
                continue
            if wait[s].get(pos[s], 0) > 0:
                wait[s][pos[s]] -= 1
                continue
            item, c = scripts[s][pos[s]], CHUNKS[s % 4]
            at[s] = pos[s]
            pos[s] += 1
            if item is None:
                conv.close(s)
                continue
            if not conv.is_open[s]:
                conv.open(s, **SESS[s % 4])
            feed[s] = pcm[s][item * c:(item + 1) * c]
        res = conv.step(feed)
        assert set(res) == set(feed)
        fed += bool(feed)
        if any(o is not None for o in res.values()):
            gate, lim = conv.gate_open(), conv.limit_db()
            for s, o in res.items():
                if o is not None:
                    outs[s][at[s]] = o
                    said[s][at[s]] = (gate[s], lim[s])
        tick += 1
    return outs, said, tick, fed


def _same_streams(a, b):
    return all(sorted(x) == sorted(y) and all(np.array_equal(x[j], y[j]) for j in x) for x, y in zip(a, b))


def _state(conv):
    return {a: getattr(conv, a).clone() for a in STATE}


@pytest.fixture(scope="module")
def dense(pool):
    """the dense converter over the script, every session present every tick: computed once"""
    conv = _conv(pool)
    outs, said, ticks, _ = _drive(conv, _inputs(), _scripts())
    assert ticks == ITEMS and [len(o) for o in outs] == [ITEMS - BS, ITEMS - BS, ITEMS - BS - (BS + 1), ITEMS - BS]
    assert [o[BS].shape[0] for o in outs] == [80, 160, 440, 480]
    return dict(outs=outs, said=said, state=_state(conv), conv=conv)


@pytest.fixture(scope="module")
def live(dense):
    """where the script's cases are live in the dense run: the position at which slot 0's gate reopens after its silence, and one
    at which slot 1's limiter turned the chunk down"""
    gate = {j: g for j, (g, _) in dense["said"][0].items()}
    closed = [j for j in sorted(gate) if not gate[j]]
    assert closed and closed[0] > BS and gate[BS] is True
    reopen = min(j for j in gate if j > closed[-1])
    assert gate[reopen] is True and gate[reopen - 1] is False
    peaks = [j for j, (_, db) in sorted(dense["said"][1].items()) if db < 0 and j > BS + 1]
    assert peaks and any(db < 0 for _, db in dense["said"][2].values())
    return dict(reopen=reopen, peak=peaks[0])


@pytest.mark.parametrize("graph", [False, True])
def test_sparse_with_every_session_present_is_the_dense_converter(pool, dense, graph):
    conv = _conv(pool, sparse=True)
    outs, said, ticks, _ = _drive(conv, _inputs(), _scripts(), graph_at=3 if graph else None)
    assert ticks == ITEMS and _same_streams(outs, dense["outs"]) and said == dense["said"]
    assert conv.captures == int(graph) and conv.pushes == ITEMS and conv.ring is None
    for a, v in dense["state"].items():
        assert torch.equal(getattr(conv, a), v), a
    # the device rings in time order are the dense converter's host rings, and the float input is their conversion
    assert np.array_equal(conv.rings(), dense["conv"].ring) and conv.rings().dtype == np.int16
    assert torch.equal(conv._in, audio_io.pcm16_to_float(torch.from_numpy(dense["conv"].ring).to(DEV)))
    with pytest.raises(ValueError, match="a chunk for slot 2, which is not open"):
        conv.close(2).step({2: np.zeros(441, np.int16)})
    with pytest.raises(ValueError, match=r"slot 1: chunk of 161 samples, expected 160"):
        conv.step({1: np.zeros(161, np.int16)})
    assert not conv.rings()[2].any() and not bool(conv._in[2].any())


@pytest.mark.parametrize("graph", [False, True])
def test_sparse_at_sixteen_slots_is_the_dense_converter(pool, graph):
    """128 frame columns: the batch kernels and the fp16 guard"""
    items = BS + 5
    pcm, scripts = _inputs(16), [list(range(items)) for _ in range(16)]
    want = _drive(_conv(pool, 16), pcm, scripts)[0]
    conv = _conv(pool, 16, sparse=True)
    assert MS.fp16_guarded(conv.B * conv.frames)
    got = _drive(conv, pcm, scripts, graph_at=0 if graph else None)[0]
    assert _same_streams(got, want) and all(len(o) == 5 for o in got) and conv.captures == int(graph)


def _stalls(live, seed):
    """two consecutive ticks, one while filling, one on the tick slot 0's gate would reopen, one right after a limiter peak of slot
    1 -- and seeded ones on top; slot 3 never sits a tick out"""
    rng = np.random.default_rng(seed)
    st = [{18: 2, live["reopen"]: 1}, {5: 1, live["peak"] + 1: 1}, {3: 1, REOPEN_AT + 1: 1, 30: 2}, {}]
    for s in range(3):
        for j in rng.choice(ITEMS, 4, replace=False):
            st[s][int(j)] = st[s].get(int(j), 0) + 1
    return st


@pytest.mark.parametrize("graph", [False, True])
def test_a_sessions_stream_does_not_depend_on_its_absences_or_on_the_others(pool, dense, live, graph):
    conv = _conv(pool, sparse=True)
    stalls = _stalls(live, 90)
    outs, said, ticks, fed = _drive(conv, _inputs(), _scripts(), stalls, graph_at=2 if graph else None)
    assert ticks > ITEMS + 4 and conv.captures == int(graph) and conv.pushes == fed >= ITEMS
    assert _same_streams(outs, dense["outs"])
    assert said == dense["said"]                                     # (the gate and the limiter said the same of every chunk)
    # every session is at the same point of its own clock as in the dense run, slot 3 for several ticks already: the states
    for a, v in dense["state"].items():
        assert torch.equal(getattr(conv, a), v), a
    assert np.array_equal(conv.rings(), dense["conv"].ring)
    # another pattern for the others: the session that never sits out is byte-identical again
    other = _conv(pool, sparse=True)
    outs2 = _drive(other, _inputs(), _scripts(), [{7: 3}, {20: 1, 21: 1}, {}, {}], graph_at=2 if graph else None)[0]
    assert _same_streams(outs2[3:], dense["outs"][3:]) and _same_streams(outs2, dense["outs"])


def test_absent_rows_are_masked_for_the_tick_and_an_empty_step_moves_nothing(pool):
    conv = _conv(pool, sparse=True)
    pcm = _inputs()
    for s in range(4):
        conv.open(s, **SESS[s])
    feed = lambda t, slots: {s: pcm[s][t * CHUNKS[s]:(t + 1) * CHUNKS[s]] for s in slots}      # noqa: E731
    for t in range(BS + 2):
        conv.step(feed(t, range(4)))
    seg = conv.seg_len.tolist()
    assert conv.seg_len_tick.tolist() == seg and seg[0] > 0 and seg[2] > 0 and seg[3] > 0 and seg[1] == 0      # (S = 2: rows 2 s, 2 s + 1)
    keep = ("seg_len_tick", "seg_len_eff", "ring_dev", "_in", "present", "emit") + STATE
    before = {a: getattr(conv, a).clone() for a in keep}
    assert conv.step({}) == {} and conv.pushes == BS + 2
    for a, v in before.items():
        assert torch.equal(getattr(conv, a), v), a
    res = conv.step(feed(BS + 2, (0, 3)))                            # slots 1 and 2 sit this tick out
    assert sorted(res) == [0, 3] and res[0].shape == (80,) and res[3].shape == (480,)
    want = [v if i // 2 in (0, 3) else 0 for i, v in enumerate(seg)]
    assert conv.seg_len_tick.tolist() == want and conv.seg_len.tolist() == seg
    assert conv.seg_len_eff.tolist() == want                         # (slot 0's gate is open on this loud input)
    assert conv.present.tolist() == [True, False, False, True] and conv.emit.view(-1).tolist() == [True, False, False, True]
    for a in STATE:                                                  # the absent rows stood still, the present ones moved
        now = getattr(conv, a)
        assert torch.equal(now[1:3], before[a][1:3]), a
    assert not torch.equal(conv.tail[0], before["tail"][0])
    assert np.array_equal(conv.rings()[1:3], before["ring_dev"][1:3, :conv.ld_in].cpu().numpy())
    assert not np.array_equal(conv.rings()[0], before["ring_dev"][0, :conv.ld_in].cpu().numpy())
    # a filling slot that is present on a tick where nobody emits still has its chunk pushed
    fresh = _conv(pool, sparse=True)
    fresh.open(1, **SESS[1])
    assert fresh.step({1: pcm[1][:160]}) == {1: None} and fresh.pushes == 1
    rl = 160 * BS                                                    # (slot 1's ring at 16 kHz; the rows are as wide as the 48 kHz ones)
    assert np.array_equal(fresh.rings()[1, rl - 160:rl], pcm[1][:160]) and not fresh.rings()[1, :rl - 160].any()
    assert not fresh.rings()[1, rl:].any() and fresh.rings().shape == (4, 480 * BS)


@pytest.mark.parametrize("graph", [False, True])
def test_the_bf16_repeat_gives_the_same_samples_and_pushes_the_ring_once(pool, monkeypatch, graph):
    """the repeat of a tick (after an fp16 saturation) with the switch of the process to bf16 planes stubbed out, first called as
    test_gpu_limit.py calls it, then through step() itself with the saturation counter stubbed to report one"""
    monkeypatch.setattr(MS.ops, "switch_to_bf16", lambda *a: None)
    ticks = BS + 4
    pcm = _pcm(CHUNK * (ticks + 1), 80)
    kw = dict(chunk=CHUNK, buffersize=BS, k=4, limiter=True, crossfade=True, sparse=True)
    conv, twin = (MS.MultiStreamConverter(*_nets(), pool, 2, **kw) for _ in range(2))
    for c in (conv, twin):
        c.open(0, "v0", gain=60.0, limit_db=-1.0, crossfade_ms=5)
        if graph:
            c.enable_graph()
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        if t == ticks - 1:
            saved = conv.phi.clone(), conv._seam_state()
        out, out2 = conv.step({0: c})[0], twin.step({0: c})[0]
        assert (out is None) == (out2 is None) == (t < BS) and (out is None or np.array_equal(out, out2))
    after = conv.limit_hist.clone(), conv.tail.clone(), conv.rings().copy(), conv.pushes
    assert conv.limit_db()[0] < 0 and not torch.equal(saved[1][2], after[0])
    lo, ln = conv._span(CHUNK)
    again = conv._repeat_on_bf16(saved[0], None, None, saved[1])
    assert again.shape == (2, conv._wave_len(16000)) and np.array_equal(again[0, lo:lo + ln], out)
    assert torch.equal(conv.limit_hist, after[0]) and torch.equal(conv.tail, after[1])
    assert conv.pushes == after[3] == ticks and np.array_equal(conv.rings(), after[2])
    # through step(): the guard on, the counter reporting a saturation once -- the tick runs twice, the ring moves once
    calls = []
    monkeypatch.setattr(MS, "fp16_guarded", lambda n: True)
    monkeypatch.setattr(MS.ops, "f16_saturations", lambda reset=False: calls.append(1) or 1)
    c = pcm[ticks * CHUNK:(ticks + 1) * CHUNK]
    got = conv.step({0: c})[0]
    monkeypatch.setattr(MS.ops, "f16_saturations", lambda reset=False: 0)
    want = twin.step({0: c})[0]
    assert calls == [1] and np.array_equal(got, want) and conv.pushes == twin.pushes == ticks + 1
    assert np.array_equal(conv.rings(), twin.rings()) and torch.equal(conv.limit_hist, twin.limit_hist)
    assert torch.equal(conv.phi, twin.phi) and torch.equal(conv.tail, twin.tail) and conv.captures == (3 if graph else 0)


# ---------------------------------------------------------------------------------------------------- 9. the CLI
def _save_nets(d):
    for name, net in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _nets()):
        torch.save(net.state_dict(), d / name)
    return ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]


@pytest.mark.parametrize("graph", [False, True])
def test_cli_writes_the_same_wavs_with_stalls_and_under_the_flag(tmp_path, graph):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    ticks = BS + 6
    for i in range(3):
        wav = _pcm(CHUNK * ticks, 80 + i).astype(np.float32) / 32767
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    base = [dict(input="in0.wav", lib="voice_library.pt", gain=60, limit_db=-1), dict(input="in1.wav", lib="voice_library.pt", start=2),
            dict(input="in2.wav", lib="voice_library.pt", pitch=2, crossfade_ms=5)]
    json.dump(base, open(d / "plain.json", "w"))
    json.dump([dict(base[0], stall=[3, 4, BS + 1, 90]), dict(base[1], stall=[0, 2, BS + 3]), base[2]], open(d / "stall.json", "w"))
    common = nets + ["-c", str(CHUNK), "-b", str(BS)] + ([] if graph else ["--no-graph"])
    built = []
    real = msi.MultiStreamConverter
    msi.MultiStreamConverter = lambda *a, **k: built.append(real(*a, **k)) or built[-1]
    try:
        msi.main(common + ["-o", str(d / "out_plain"), str(d / "plain.json")])
        msi.main(common + ["-o", str(d / "out_stall"), str(d / "stall.json")])
        msi.main(common + ["-o", str(d / "out_flag"), "--sparse", str(d / "plain.json")])
    finally:
        msi.MultiStreamConverter = real
    assert [c.sparse for c in built] == [False, True, True] and built[1].pushes > built[2].pushes == ticks + 2
    names = ["0_in0.wav", "1_in1.wav", "2_in2.wav"]
    plain = [open(d / "out_plain" / n, "rb").read() for n in names]
    assert all(len(p) > 44 + 2 * CHUNK * 5 for p in plain) and len(set(plain)) == 3
    assert [open(d / "out_stall" / n, "rb").read() for n in names] == plain
    assert [open(d / "out_flag" / n, "rb").read() for n in names] == plain
