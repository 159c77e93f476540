"""Lost-chunk concealment on the device: csrc/conceal.hip against the NumPy restatement tools/conceal_ref.py, and
MultiStreamConverter(sparse=True, conceal=True) against a converter without concealment that is fed, as real chunks, the stream the
restatement predicts.  Every comparison is bitwise, or equality of int16 streams.

3. alive_conceal_rows (and the push behind it), one call per tick over all rows: seven geometries (one whose ring is too short) x
   eight signals under seven loss patterns over 30 ticks, on 16-byte strides and on odd ones; ring, chunk buffer, state and template
   between guard bands after every tick.
4. The same at N = 1024 with seeded random presence, loss and switches.
5. Conceal and push replayed inside one captured graph while present, lost and the chunks are rewritten between replays.
6. The converter with losses is the converter without concealment fed the predicted stream (outputs and rings, every tick), plain,
   with gate, crossfade, limiter and envelope on, and under enable_graph with one capture.
7. A conceal=True converter without losses is the conceal=False sparse converter and never launches the kernel.
8. A session's stream does not depend on the others' losses; conceal=False is a chunk of zeros; set(conceal=) takes effect on the next
   loss without a re-capture.
9. The bf16 repeat: the same samples, the ring pushed and concealed once.
10. The CLI: "lose" keeps the lengths and writes what the predicted input writes; "lose": [] and --conceal write what a plain run writes."""
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

import conceal_ref as CR                                             # noqa: E402
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


# ---------------------------------------------------------------------------------------------------- 3-5. alive_conceal_rows
GEOM = [(8000, 80, 16), (16000, 160, 16), (16000, 160, 4), (44100, 441, 16), (48000, 480, 16), (16000, 960, 8)]
SHORT = (16000, 160, 3)                                              # a ring of 480 < 587 samples: the row is left alone
SIGNALS = ("h_lo", "h_mid", "h_hi", "h_frac", "noise", "silence", "square", "wave")
TICKS = 30


def _harmonic(period, n, seed, amp=6000.0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = sum(a * np.sin(2 * np.pi * h * t / period + rng.uniform(0, 6.28)) for h, a in ((1, 1.0), (2, 0.5), (3, 0.25)))
    return np.rint(x * amp).astype(np.int16)


def _signal(kind, rate, n, seed):
    g = CR.geometry(rate, 1)
    if kind == "h_lo":
        return _harmonic(g["lag_lo"], n, seed)
    if kind == "h_mid":
        return _harmonic((g["lag_lo"] + g["lag_hi"]) // 2, n, seed)
    if kind == "h_hi":
        return _harmonic(g["lag_hi"], n, seed)
    if kind == "h_frac":
        return _harmonic(rate / 123.4, n, seed)                      # a period that is no whole number of samples
    if kind == "noise":
        return np.random.default_rng(seed).integers(-8000, 8000, n).astype(np.int16)
    if kind == "silence":
        return np.zeros(n, np.int16)
    if kind == "square":                                             # full scale, both ends of int16
        return np.where((np.arange(n) // (rate // 300)) % 2 == 0, 32767, -32768).astype(np.int16)
    return _pcm(n, seed)


PATTERNS = {                                                         # per pattern: (lost ticks, absent ticks, rows with on == 0)
    "single": ({20}, set(), None),
    "three": ({20, 21, 22}, set(), None),
    "ten": (set(range(18, 28)), set(), None),                        # 100 ms: decays to zeros
    "loss-good-loss": ({20, 22}, set(), None),
    "tick0": ({0, 1, 9}, set(), None),                               # on an empty ring, and on one still filling
    "stalls": ({20, 22, 24}, {19, 21, 23, 26}, None),                # absences inside a run: the state stands still
    "off": ({20, 21, 25}, set(), 2),                                 # every second row does not conceal: zeros
}


class ConcealCase:
    """device arrays of one conceal + push problem between guard bands, and the host mirror that conceal_ref moves on"""

    def __init__(self, rows, ld, ld_chunk, ld_tmpl, seed, ticks=TICKS, prefill=False):
        n = len(rows)
        self.n, self.rows, self.ld_chunk = n, rows, ld_chunk
        self.rng = np.random.default_rng(seed)
        self.cl = [c for _, c, _, _ in rows]
        self.rl = [c * b for _, c, b, _ in rows]
        geo = [CR.geometry(r, c) for r, c, _, _ in rows]
        self.consts = np.array([[g[a] for g in geo] for a in ("lag_lo", "lag_hi", "window", "hold", "fade", "recover")], np.int32)
        self.sig = [_signal(kind, r, c * (ticks + b + 1), seed + i) for i, (r, c, b, kind) in enumerate(rows)]
        self.pos = [0] * n
        self.ring_h = np.zeros((n, ld), np.int16)
        if prefill:                                                  # rings that have been running for a while
            for i in range(n):
                self.ring_h[i, :self.rl[i]] = self.sig[i][:self.rl[i]]
                self.pos[i] = self.rl[i]
        self.state_h = np.zeros((n, 2), np.int32)
        self.tmpl_h = self.rng.integers(-99, 99, (n, ld_tmpl)).astype(np.int16)
        self.ring = Guarded((n, ld), torch.int16, -12345, self.ring_h)
        self.chunks = Guarded((n, ld_chunk), torch.int16, -4321)
        self.state = Guarded((n, 2), torch.int32, -77, self.state_h)
        self.tmpl = Guarded((n, ld_tmpl), torch.int16, -555, self.tmpl_h)
        self.x = torch.zeros(n, ld, dtype=torch.float32, device=DEV)
        self.flags = torch.zeros(3, n, dtype=torch.uint8, device=DEV)      # present, lost, on
        i32 = dict(dtype=torch.int32, device=DEV)
        self.d = dict(cl=torch.tensor(self.cl, **i32), rl=torch.tensor(self.rl, **i32), consts=torch.tensor(self.consts, **i32))

    def prepare(self, present, lost, on):
        """this tick's chunk buffer (the next samples of a row that takes part, garbage on a lost one) and what the restatement
        makes of it: the concealed chunk buffer, the state, the template and the pushed rings"""
        chunks = self.rng.integers(-32768, 32768, (self.n, self.ld_chunk)).astype(np.int16)
        for i in range(self.n):
            if present[i]:
                if not lost[i]:
                    chunks[i, :self.cl[i]] = self.sig[i][self.pos[i]:self.pos[i] + self.cl[i]]
                self.pos[i] += self.cl[i]                            # (a lost chunk is consumed and dropped)
        c = self.consts
        want = CR.conceal_rows(self.ring_h, self.rl, chunks, self.cl, present, lost, on, c[0], c[1], c[2], c[3], c[4], c[5],
                               self.state_h, self.tmpl_h)
        ring = self.ring_h.copy()
        for i in range(self.n):
            if present[i]:
                cl, rl = self.cl[i], self.rl[i]
                ring[i, :rl] = np.concatenate([self.ring_h[i, cl:rl], want["chunks"][i, :cl]])
        want["ring"] = ring
        self.ring_h, self.state_h, self.tmpl_h = ring, want["state"], want["tmpl"]
        self._load = chunks, np.array([present, lost, on], np.uint8)
        return want

    def load(self):
        self.chunks.view.copy_(torch.from_numpy(self._load[0]))
        self.flags.copy_(torch.from_numpy(self._load[1]))

    def launch(self):
        MS.conceal_rows_(self.ring.view, self.d["rl"], self.chunks.view, self.d["cl"], self.flags[0], self.flags[1], self.flags[2],
                         self.d["consts"], self.state.view, self.tmpl.view)
        MS.ring_push_rows_(self.ring.view, self.chunks.view, self.d["cl"], self.d["rl"], self.flags[0], self.x)

    def check(self, want, where):
        assert np.array_equal(self.chunks.host(), want["chunks"]), where
        assert np.array_equal(self.state.host(), want["state"]), where
        assert np.array_equal(self.tmpl.host(), want["tmpl"]), where
        assert np.array_equal(self.ring.host(), want["ring"]), where
        assert self.chunks.intact() and self.state.intact() and self.tmpl.intact() and self.ring.intact(), where


def _rows():
    return [g + (kind,) for kind in SIGNALS for g in GEOM + [SHORT]]


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("ld,ld_chunk,ld_tmpl", [(7680, 960, 800), (7683, 961, 801)], ids=["vector", "scalar"])
def test_conceal_rows_against_the_restatement_after_every_tick(ld, ld_chunk, ld_tmpl, pattern):
    rows = _rows()
    n = len(rows)
    lost_at, absent_at, off = PATTERNS[pattern]
    case = ConcealCase(rows, ld, ld_chunk, ld_tmpl, 100 + list(PATTERNS).index(pattern))
    on = [0 if off and r % off else 1 for r in range(n)]
    short = [r for r in range(n) if rows[r][:3] == SHORT]
    seen_run = seen_zero_tail = False
    for tick in range(TICKS):
        present = [0 if tick in absent_at else 1] * n
        lost = [1 if tick in lost_at and present[r] else 0 for r in range(n)]
        before = case.state_h.copy()
        want = case.prepare(present, lost, on)
        case.load()
        case.launch()
        case.check(want, (pattern, tick))
        chunks = case._load[0]
        for r in short:                                              # the row whose ring is too short: untouched, state and all
            assert np.array_equal(want["chunks"][r], chunks[r]) and want["state"][r].tolist() == [0, 0]
        if tick in absent_at:
            assert np.array_equal(want["state"], before) and np.array_equal(want["chunks"], chunks)
        if tick in lost_at:                                          # (what the restatement itself must say)
            live = [r for r in range(n) if r not in short]
            assert all(want["state"][r, 0] == before[r, 0] + case.cl[r] for r in live if on[r])
            assert all(not want["chunks"][r, :case.cl[r]].any() and want["state"][r].tolist() == [0, 0] for r in live if not on[r])
            seen_run = True
            if pattern == "ten" and tick == 27:
                seen_zero_tail = all(not want["chunks"][r, :case.cl[r]].any() for r in live)
    assert seen_run and (pattern != "ten" or seen_zero_tail)
    assert not case.state_h[:, 0].any()                              # every run has ended: the last ticks were real chunks


def test_the_harmonic_rows_find_their_own_period_on_the_device():
    rows = [g + (kind,) for kind in ("h_lo", "h_mid", "h_hi") for g in GEOM]
    case = ConcealCase(rows, 7680, 960, 800, 7, prefill=True)
    n = len(rows)
    want = case.prepare([1] * n, [1] * n, [1] * n)
    case.load()
    case.launch()
    case.check(want, "periods")
    for r, (rate, cl, b, kind) in enumerate(rows):
        g = CR.geometry(rate, cl)
        period = {"h_lo": g["lag_lo"], "h_mid": (g["lag_lo"] + g["lag_hi"]) // 2, "h_hi": g["lag_hi"]}[kind]
        assert want["state"][r].tolist() == [cl, period], (rows[r], want["state"][r])


def test_conceal_rows_at_1024_rows_with_random_presence_and_loss():
    base = _rows()
    rows = [base[r % len(base)] for r in range(1024)]
    case = ConcealCase(rows, 7680, 960, 800, 60, ticks=8, prefill=True)
    rng = np.random.default_rng(61)
    runs = 0
    for tick in range(6):
        present = (rng.random(1024) < 0.8).astype(int).tolist()
        lost = ((rng.random(1024) < 0.4) & np.array(present, bool)).astype(int).tolist()
        on = (rng.random(1024) < 0.9).astype(int).tolist()
        want = case.prepare(present, lost, on)
        case.load()
        case.launch()
        case.check(want, tick)
        runs = max(runs, int((want["state"][:, 0] > 0).sum()))
    assert runs > 150


def test_conceal_and_push_replayed_in_a_captured_graph_while_the_flags_and_chunks_change():
    rows = _rows()[:21]
    n = len(rows)
    eager, graphed = (ConcealCase(rows, 7680, 960, 800, 70, prefill=True) for _ in range(2))
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
    for tick in range(14):
        present = (rng.random(n) < 0.85).astype(int).tolist()
        lost = ((rng.random(n) < 0.4) & np.array(present, bool)).astype(int).tolist()
        on = (rng.random(n) < 0.9).astype(int).tolist()
        want = eager.prepare(present, lost, on)
        want2 = graphed.prepare(present, lost, on)
        assert np.array_equal(want["chunks"], want2["chunks"])
        for c in (eager, graphed):
            c.load()
        eager.launch()
        g.replay()
        eager.check(want, tick)
        graphed.check(want2, tick)
    assert want is not None


# ---------------------------------------------------------------------------------------------------- 6-9. the converter
CHUNK, BS = 160, 16
RATES = (8000, 16000, 44100, 48000)
CHUNKS = [80, 160, 441, 480]
ITEMS = 36
VOICES = ("v0", "v1", "v2", "v0")
PLAIN = [dict(pitch=1.0), dict(f0_rate=0.9), dict(alpha=0.1), dict(alpha=0.2, f0_rate=1.1)]
FEATURES = [dict(pitch=1.0, gate_db=-40, gate_hold=0.0, crossfade_ms=5, envelope=0.7),
            dict(f0_rate=0.9, gain=60.0, limit_db=-1.0, envelope=1.0),
            dict(alpha=0.1, crossfade_ms=5, gain=60.0, limit_db=-3.0, limit_lookahead_ms=2.0),
            dict(alpha=0.2, f0_rate=1.1, gate_db=-50)]
# per slot {tick of the run: "lost" | "absent"}; everything else is a real chunk
LOSSES = [{20: "lost", 21: "lost"},
          {5: "lost", 22: "lost", 23: "lost", 24: "lost", 25: "lost", 26: "lost", 27: "lost", 28: "lost"},
          {18: "lost", 20: "lost"},
          {0: "lost", 19: "absent", 22: "lost", 23: "absent", 24: "lost", 30: "absent"}]


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    return MS.VoicePool(voices)


@pytest.fixture(scope="module")
def pcm():
    return [_pcm(CHUNKS[s] * ITEMS, 70 + s) for s in range(4)]


def _conv(pool, conceal, features=False, **kw):
    extra = dict(gate=True, crossfade=True, limiter=True, envelope=True) if features else {}
    return MS.MultiStreamConverter(*_nets(), pool, 4, chunk=CHUNK, buffersize=BS, k=4, rates=RATES, sparse=True,
                                   **(dict(conceal=True) if conceal else {}), **extra, **kw)


def _ab(pool, pcm, script, sess, features=False, graph=False, off=(), toggles=()):
    """converter A (conceal, losses) beside converter B (no conceal, fed what conceal_ref predicts), tick by tick: equal results and
    rings after every tick.  off: slots opened with conceal=False; toggles: (tick, slot, value) for A.set(slot, conceal=value) before
    that tick.  Returns (A, B, the per-slot output lists); A must have launched the kernel on the ticks with a lost or a recovering
    slot and on no other"""
    A, B = _conv(pool, True, features), _conv(pool, False, features)
    refs = [CR.StreamRef(RATES[s], CHUNKS[s], BS, on=s not in off) for s in range(4)]
    for s in range(4):
        A.open(s, VOICES[s], rate=RATES[s], **sess[s], **(dict(conceal=False) if s in off else {}))
        B.open(s, VOICES[s], rate=RATES[s], **sess[s])
    if graph:
        A.enable_graph()
        B.enable_graph()
    pos, outs, launches = [0] * 4, [[] for _ in range(4)], 0
    for tick in range(ITEMS):
        for at, slot, value in toggles:
            if at == tick:
                A.set(slot, conceal=value)
                refs[slot].on = value
        feed, lost, feed_b, busy = {}, [], {}, False
        for s in range(4):
            what = script[s].get(tick, "real")
            if what == "absent":
                continue
            c = pcm[s][pos[s] * CHUNKS[s]:(pos[s] + 1) * CHUNKS[s]]
            pos[s] += 1
            busy = busy or what == "lost" or refs[s].q > 0
            if what == "lost":
                lost.append(s)
                feed_b[s] = refs[s].feed(None)
            else:
                feed[s] = c
                feed_b[s] = refs[s].feed(c)
        launches += busy
        ra, rb = A.step(feed, lost=lost), B.step(feed_b)
        assert A.conceals == launches, tick
        assert set(ra) == set(rb) == set(feed_b), tick
        for s in ra:
            assert (ra[s] is None) == (rb[s] is None) and (ra[s] is None or np.array_equal(ra[s], rb[s])), (tick, s)
            if ra[s] is not None:
                outs[s].append(ra[s])
        rings = A.rings()
        assert np.array_equal(rings, B.rings()), tick
        state = A.conceal_state()
        for s in range(4):
            assert np.array_equal(rings[s, :refs[s].rl], refs[s].ring), (tick, s)
            assert state[s] == ((refs[s].q, refs[s].P) if refs[s].q > 0 else (0, 0)), (tick, s)
    assert A.count == B.count and A.pushes == B.pushes and torch.equal(A.phi, B.phi)
    return A, B, outs


@pytest.fixture(scope="module")
def baseline(pool, pcm):
    """the conceal=False sparse converter over the inputs without any loss (slot 3 keeps its absences): computed once"""
    conv = _conv(pool, False)
    for s in range(4):
        conv.open(s, VOICES[s], rate=RATES[s], **PLAIN[s])
    pos, outs, rings = [0] * 4, [[] for _ in range(4)], []
    for tick in range(ITEMS):
        feed = {}
        for s in range(4):
            if LOSSES[s].get(tick) == "absent":
                continue
            feed[s] = pcm[s][pos[s] * CHUNKS[s]:(pos[s] + 1) * CHUNKS[s]]
            pos[s] += 1
        for s, o in conv.step(feed).items():
            if o is not None:
                outs[s].append(o)
        rings.append(conv.rings().copy())
    return dict(outs=outs, rings=rings)


@pytest.mark.parametrize("mode", ["plain", "features", "graph"])
def test_a_converter_with_losses_is_one_without_concealment_fed_the_predicted_stream(pool, pcm, mode):
    A, B, outs = _ab(pool, pcm, LOSSES, FEATURES if mode == "features" else PLAIN, features=mode == "features", graph=mode == "graph")
    assert A.captures == B.captures == int(mode == "graph")
    assert 15 < A.conceals < A.pushes == ITEMS
    assert [len(o) for o in outs] == [ITEMS - BS, ITEMS - BS, ITEMS - BS, ITEMS - 3 - BS]
    assert not B.conceal and not hasattr(B, "conceal_tmpl")


def test_without_losses_a_concealing_converter_is_the_plain_sparse_one(pool, pcm, baseline):
    conv = _conv(pool, True)
    for s in range(4):
        conv.open(s, VOICES[s], rate=RATES[s], **PLAIN[s])
    conv.enable_graph()
    pos, outs = [0] * 4, [[] for _ in range(4)]
    for tick in range(ITEMS):
        feed = {}
        for s in range(4):
            if LOSSES[s].get(tick) == "absent":
                continue
            feed[s] = pcm[s][pos[s] * CHUNKS[s]:(pos[s] + 1) * CHUNKS[s]]
            pos[s] += 1
        for s, o in conv.step(feed).items():
            if o is not None:
                outs[s].append(o)
        assert np.array_equal(conv.rings(), baseline["rings"][tick]), tick
    assert all(len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(outs, baseline["outs"]))
    assert conv.conceals == 0 and conv.captures == 1 and conv.conceal_state() == [(0, 0)] * 4
    assert not bool(conv._conceal_state.any())
    plain = _conv(pool, False)
    assert not hasattr(plain, "conceal_tmpl") and plain._flags.shape == (2, 4) and conv._flags.shape == (3, 4)
    with pytest.raises(ValueError, match=r"lost=\) needs a converter built with"):
        plain.open(0, "v0").step({}, lost=[0])
    with pytest.raises(ValueError, match="slot 1 is named in both chunks and lost"):
        conv.step({1: pcm[1][:160]}, lost=[1])
    with pytest.raises(ValueError, match="a lost chunk for slot 2, which is not open"):
        conv.close(2).step({}, lost=[2])


def test_isolation_the_switch_and_its_toggle(pool, pcm, baseline):
    """slot 3 loses nothing here: its stream is the baseline's whatever the others lose; slot 2 does not conceal: zeros; slot 0's
    switch goes off after its first run and on again later: the next loss after each set follows it, with one capture throughout"""
    script = [{18: "lost", 22: "lost", 23: "lost", 30: "lost"}, LOSSES[1], LOSSES[2], {t: w for t, w in LOSSES[3].items() if w == "absent"}]
    A, B, outs = _ab(pool, pcm, script, PLAIN, graph=True, off=(2,), toggles=[(21, 0, False), (28, 0, True)])
    assert A.captures == 1 and A.conceal_on.tolist() == [True, True, False, True]
    A.set(0, conceal=False)
    assert A.conceal_on.tolist() == [False, True, False, True]
    assert len(outs[3]) == len(baseline["outs"][3]) and all(np.array_equal(x, y) for x, y in zip(outs[3], baseline["outs"][3]))
    assert any(not np.array_equal(x, y) for x, y in zip(outs[0], baseline["outs"][0]))
    A.set(0, conceal=True)
    assert A.conceal_on.tolist() == [True, True, False, True] and A.captures == 1
    # a session that does not conceal is one that was fed zeros: its ring holds them where the chunks were lost
    zero = CR.StreamRef(RATES[2], CHUNKS[2], BS, on=False)
    for tick in range(ITEMS):
        zero.feed(None if LOSSES[2].get(tick) == "lost" else pcm[2][tick * 441:(tick + 1) * 441])
    assert np.array_equal(A.rings()[2, :zero.rl], zero.ring)
    # close and open clear a run
    A.step({}, lost=[1])
    assert A.conceal_state()[1][0] == 160 and A._conceal_run[1]
    A.close(1)
    assert A.conceal_state()[1] == (0, 0) and not A._conceal_run[1] and not bool(A._conceal_state[1].any())
    A.open(1, "v1", rate=16000)
    A.step({}, lost=[1])
    A.open(1, "v1", rate=16000)
    assert not bool(A._conceal_state[1].any()) and not A._conceal_run[1]
    with pytest.raises(ValueError, match=r"slot 1: conceal must be a bool or None"):
        A.set(1, conceal=1)


@pytest.mark.parametrize("graph", [False, True])
def test_the_bf16_repeat_gives_the_same_samples_and_conceals_once(pool, monkeypatch, graph):
    monkeypatch.setattr(MS.ops, "switch_to_bf16", lambda *a: None)
    ticks = BS + 6
    pcm = _pcm(CHUNK * (ticks + 1), 80)
    kw = dict(chunk=CHUNK, buffersize=BS, k=4, limiter=True, crossfade=True, sparse=True, conceal=True)
    conv, twin = (MS.MultiStreamConverter(*_nets(), pool, 2, **kw) for _ in range(2))
    for c in (conv, twin):
        c.open(0, "v0", gain=60.0, limit_db=-1.0, crossfade_ms=5)
        if graph:
            c.enable_graph()
    lose = {BS + 2, BS + 3}
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        kw = dict(lost=[0]) if t in lose else {}
        feed = {} if t in lose else {0: c}
        out, out2 = conv.step(feed, **kw)[0], twin.step(feed, **kw)[0]
        assert (out is None) == (out2 is None) == (t < BS) and (out is None or np.array_equal(out, out2))
    assert conv.conceals == twin.conceals == 3 and conv.conceal_state() == [(0, 0)] * 2
    # through step(): the guard on, the counter reporting a saturation once -- the tick runs twice, the ring is concealed and pushed once
    calls = []
    monkeypatch.setattr(MS, "fp16_guarded", lambda n: True)
    monkeypatch.setattr(MS.ops, "f16_saturations", lambda reset=False: calls.append(1) or 1)
    got = conv.step({}, lost=[0])[0]
    monkeypatch.setattr(MS.ops, "f16_saturations", lambda reset=False: 0)
    want = twin.step({}, lost=[0])[0]
    assert calls == [1] and np.array_equal(got, want) and conv.pushes == twin.pushes == ticks + 1
    assert conv.conceals == twin.conceals == 4 and conv.conceal_state() == twin.conceal_state() and conv.conceal_state()[0][0] == CHUNK
    assert np.array_equal(conv.rings(), twin.rings()) and torch.equal(conv.limit_hist, twin.limit_hist)
    assert torch.equal(conv.conceal_tmpl, twin.conceal_tmpl) and torch.equal(conv.phi, twin.phi) and torch.equal(conv.tail, twin.tail)
    assert conv.captures == (2 if graph else 0)


# ---------------------------------------------------------------------------------------------------- 10. the CLI
def _save_nets(d):
    for name, net in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _nets()):
        torch.save(net.state_dict(), d / name)
    return ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]


def test_cli_lose_keeps_the_lengths_and_writes_what_the_predicted_input_writes(tmp_path, monkeypatch):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    ticks = BS + 8
    for i in range(3):
        wav = _pcm(CHUNK * ticks, 80 + i).astype(np.float32) / 32767
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(wav)[None], 16000)
    base = [dict(input="in0.wav", lib="voice_library.pt", gain=60, limit_db=-1), dict(input="in1.wav", lib="voice_library.pt", start=2),
            dict(input="in2.wav", lib="voice_library.pt", pitch=2, crossfade_ms=5)]
    loses = [[BS - 3, BS - 2, 90], [3, BS], [BS - 4, BS - 3]]       # (early enough to reach the emitted centre of the ring)
    json.dump(base, open(d / "plain.json", "w"))
    json.dump([dict(base[0], lose=loses[0]), dict(base[1], lose=loses[1], stall=[5]), dict(base[2], lose=loses[2], conceal=False)],
              open(d / "lose.json", "w"))
    json.dump([dict(base[0], lose=[]), base[1], base[2]], open(d / "empty.json", "w"))
    json.dump([base[0], dict(base[1], stall=[5]), base[2]], open(d / "pred.json", "w"))
    # the input the restatement predicts: session i's chunk j is lost at the tick at which it would be supplied
    real = msi.input_pcm
    pcms = [real(str(d / f"in{i}.wav"), 16000, DEV) for i in range(3)]
    supply = [msi.supply_ticks(0, ticks), msi.supply_ticks(2, ticks, (5,)), msi.supply_ticks(0, ticks)]
    pred = {}
    for i in range(3):
        ref = CR.StreamRef(16000, CHUNK, BS, on=i != 2)
        out = [ref.feed(None if t in loses[i] else pcms[i][j * CHUNK:(j + 1) * CHUNK]) for j, t in enumerate(supply[i])]
        pred[str(d / f"in{i}.wav")] = np.concatenate(out)
        assert not np.array_equal(pred[str(d / f"in{i}.wav")], pcms[i])
    common = nets + ["-c", str(CHUNK), "-b", str(BS)]
    built = []
    ctor = msi.MultiStreamConverter
    monkeypatch.setattr(msi, "MultiStreamConverter", lambda *a, **k: built.append(ctor(*a, **k)) or built[-1])
    msi.main(common + ["-o", str(d / "out_plain"), str(d / "plain.json")])
    msi.main(common + ["-o", str(d / "out_lose"), str(d / "lose.json")])
    msi.main(common + ["-o", str(d / "out_empty"), str(d / "empty.json")])
    msi.main(common + ["-o", str(d / "out_flag"), "--conceal", str(d / "plain.json")])
    monkeypatch.setattr(msi, "input_pcm", lambda path, sr, dev: pred[path])
    msi.main(common + ["-o", str(d / "out_pred"), str(d / "pred.json")])
    assert [(c.sparse, c.conceal) for c in built] == [(False, False), (True, True), (True, True), (True, True), (True, False)]
    assert built[1].conceals == 8 and built[2].conceals == built[3].conceals == 0 and built[1].captures == 1
    names = ["0_in0.wav", "1_in1.wav", "2_in2.wav"]
    read = lambda sub: [open(d / sub / n, "rb").read() for n in names]      # noqa: E731
    plain, lose = read("out_plain"), read("out_lose")
    assert all(len(p) > 44 + 2 * CHUNK * 5 for p in plain) and [len(p) for p in lose] == [len(p) for p in plain]
    assert all(a != b for a, b in zip(lose, plain))
    assert lose == read("out_pred")
    assert read("out_empty") == plain and read("out_flag") == plain
