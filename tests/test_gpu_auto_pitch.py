"""Auto pitch on the device (csrc/pitch_auto.hip) and through the batched paths, against the NumPy restatement tools/pitch_ref.py.

1. alive_pitch_stats_groups: counts exact, sums to 1e-12 (fp64 in another order), bitwise reproducible, a group bitwise on its own.
2. alive_pitch_follow_rows: rows off and rows not emitting untouched, auto rows over five calls against the recurrence.
3. MultiStreamConverter(auto_pitch=True): no auto session -> bitwise the converter built without it; a session on auto against the
   recurrence run on its plain twin's f0; graph replay bitwise eager through switches, one capture, enable_graph keeps the state.
4. convert_many(auto_pitch=): an utterance alone bitwise in a corpus; the shift is the one the stats give; off is the present path.
5. VoicePool registers on the device side: measured at enrolment, merged, kept through compact / remove; auto without one refused."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pitch_ref as PR                                               # noqa: E402
from module import synthetic                                         # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _pcm(n, seed, scale=12000):
    return (synthetic.make_waveform(n, seed)[0].numpy() * scale).astype(np.int16)


def _i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device=DEV)


def _f32(a):
    return torch.tensor(list(a), dtype=torch.float32, device=DEV)


def _f0(N, T, seed):
    """f0 with voiced values over the pitch range and every kind of unvoiced frame: 0, NaN, +inf, negatives"""
    rng = np.random.default_rng(seed)
    f0 = rng.uniform(30.0, 4000.0, size=(N, T)).astype(np.float32)
    flat = f0.reshape(-1)
    for j, bad in enumerate((0.0, np.nan, np.inf, -220.0, -0.0)):
        flat[j + 1::11] = bad
    return f0


# ---------------------------------------------------------------------------------------------------- 1. the stats kernel
STATS_CASES = [
    # (N, T, first, row to silence (all-unvoiced group) or None, (t_lo, t_hi) sub-range)
    (1, 1, [0, 1], None, (0, 0)),
    (1, 1, [0, 0, 1], 0, (1, 1)),
    (5, 7, [0, 2, 2, 5], None, (2, 6)),
    (5, 7, [0, 2, 3, 5], 2, (0, 1)),
    (3, 300, [0, 1, 1, 3], None, (255, 257)),         # more frames than the block's 256 threads
    (3, 300, [0, 1, 2, 3], 1, (7, 290)),
]


@pytest.mark.parametrize("N,T,first,silent,sub", STATS_CASES)
def test_stats_kernel_against_numpy(N, T, first, silent, sub):
    f0 = _f0(N, T, 10 * N + T)
    if N * T == 1:
        f0[0, 0] = 311.0
    if silent is not None:
        f0[silent] = np.array([0.0, np.nan, np.inf, -5.0] * T, dtype=np.float32)[:T]
    dev = torch.from_numpy(f0).to(DEV).view(N, 1, T)
    G = len(first) - 1
    for lo, hi in ((0, T), sub):
        ref = PR.stats_groups(f0, first, lo, hi)
        got = MS.pitch_stats_groups(dev, _i32(first), lo, hi)
        again = MS.pitch_stats_groups(dev, _i32(first), lo, hi)
        assert got.shape == (G, 2) and got.dtype == torch.float64
        assert torch.equal(got, again)                                       # bitwise reproducible
        g_ = got.cpu().numpy()
        print(f"stats ({N}, {T}) first {first} frames [{lo}, {hi}): device {g_.tolist()} numpy {ref.tolist()}")
        assert np.array_equal(g_[:, 1], ref[:, 1])                           # counts are exact
        assert np.all(np.abs(g_[:, 0] - ref[:, 0]) <= 1e-12 * np.abs(ref[:, 0]))
        for g in range(G):
            if first[g] == first[g + 1] or (silent is not None and first[g] == silent and first[g + 1] == silent + 1) or lo == hi:
                assert g_[g].tolist() == [0.0, 0.0], g                       # empty, all-unvoiced, no frames
            alone = MS.pitch_stats_groups(dev, _i32([first[g], first[g + 1]]), lo, hi)
            assert torch.equal(alone[0], got[g]), g                          # the other groups do not matter


def test_one_row_group_mean_is_the_transforms_mean():
    """(float)(sum / count) of a one-row group is bitwise the mean pitch_kernel's mode 0 uses: intonation 0 collapses every voiced
    frame of the transform onto 440 * 2^((mean + 9) / 12)"""
    f0 = _f0(2, 300, 3)
    dev = torch.from_numpy(f0).to(DEV).view(2, 1, 300)
    st = MS.pitch_stats_groups(dev, _i32([0, 1, 2])).cpu().numpy()
    flat = MS.pitch_transform_rows_(dev.clone(), 0, _f32([1, 1]), _f32([0, 0]), _f32([0, 0])).cpu().numpy()[:, 0]
    for n in range(2):
        v = PR.voiced(PR.pitch(f0[n]))
        mean = np.float32(st[n, 0] / st[n, 1])
        want = np.float32(440.0) * np.float32(2.0 ** np.float64((mean + np.float32(9.0)) / np.float32(12.0)))
        assert st[n, 1] == v.sum() > 100 and np.all(flat[n][v] == flat[n][v][0]) and np.all(flat[n][~v] == 0.0)
        assert abs(float(flat[n][v][0]) - float(want)) <= 2 * float(np.spacing(want))      # (exp2 is the device's, 2^x NumPy's)


def test_shift_groups_kernel_is_the_restated_arithmetic():
    stats = torch.tensor([[-100.0, 7.0], [0.0, 0.0], [55.5, 3.0], [-9.0, 1.0]], dtype=torch.float64, device=DEV)
    first, offset, on, target = [0, 3, 3, 4, 9], [0.5, -1.0, 2.0, 0.25], [1, 1, 0, 1], [-20.0, 3.0, 4.0, 2.5]
    got = MS.pitch_shift_groups(stats, _i32(first), 9, _f32(offset), _i32(on), _f32(target)).cpu().numpy()
    ref = PR.shift_groups(stats.cpu().numpy(), offset, on, target)
    want = np.repeat(ref, np.diff(first))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert want[3] == np.float32(2.0) and want[4] == np.float32(0.25) + (np.float32(2.5) - np.float32(-9.0))


# ---------------------------------------------------------------------------------------------------- 2. the follow kernel
def test_follow_kernel_against_the_recurrence():
    N, T, decay, prior = 6, 300, 0.97, 40.0
    rng = np.random.default_rng(8)
    auto = [1, 0, 1, 1, 0, 1]
    emit = [1, 1, 0, 1, 0, 1]
    rate = [1.0, 0.5, 0.8, 0.7, 1.0, 1.25]
    offset = [0.0, 1.7, -2.0, 0.3, 5.0, -0.6]
    target = [-30.0, 0.0, -12.5, 4.0, 0.0, 63.9]
    state0 = rng.uniform(-50.0, 50.0, size=(N, 2))
    state0[:, 1] = np.abs(state0[:, 1])
    state0[3] = 0.0                                                          # a fresh session
    state = torch.from_numpy(state0.copy()).to(DEV)
    shift = torch.full((N,), 99.0, device=DEV)
    ref_state = state0.copy()
    args = (_f32(rate), _f32(offset), _i32(auto), _f32(target), torch.tensor(emit, dtype=torch.bool, device=DEV).view(N, 1))
    worst = 0.0
    for call in range(5):
        f0 = _f0(N, T, 20 + call)
        MS.pitch_follow_rows_(torch.from_numpy(f0).to(DEV).view(N, 1, T), *args, decay, prior, state, shift)
        ref_state, ref_shift = PR.follow_rows(ref_state, f0, rate, offset, auto, target, emit, decay, prior)
        got_state, got_shift = state.cpu().numpy(), shift.cpu().numpy()
        for n in range(N):
            if not auto[n]:                                                  # off: the offset bit for bit, the state untouched
                assert got_shift[n] == np.float32(offset[n]) and np.array_equal(got_state[n], state0[n]), (call, n)
            elif not emit[n]:                                                # filling: the state stays
                assert np.array_equal(got_state[n], state0[n]), (call, n)
        assert np.array_equal(got_state[:, 1], ref_state[:, 1]) or np.allclose(got_state[:, 1], ref_state[:, 1], rtol=1e-14, atol=0)
        assert np.allclose(got_state[:, 0], ref_state[:, 0], rtol=1e-12, atol=0)
        err = float(np.abs(got_shift.astype(np.float64) - ref_shift.astype(np.float64)).max())
        worst = max(worst, err)
        print(f"follow call {call}: shifts {got_shift.tolist()} max |device - numpy| {err:.3e}")
        # four float32 ulps at magnitude 64, the bound of the pitch range
        assert err <= 3.1e-5, (call, err)
    assert np.abs(ref_shift[0]) > 1.0 and np.abs(ref_shift[5]) > 1.0         # the automatic part is at work


def test_follow_kernel_prior_zero_on_an_unvoiced_row_is_exactly_the_offset():
    f0 = torch.tensor([[0.0, float("nan"), float("inf"), -3.0, 0.0]] * 2, device=DEV).view(2, 1, 5)
    state = torch.zeros(2, 2, dtype=torch.float64, device=DEV)
    shift = torch.full((2,), 99.0, device=DEV)
    for _ in range(2):
        MS.pitch_follow_rows_(f0, _f32([1, 1]), _f32([0.37, -1.25]), _i32([1, 1]), _f32([-9.0, 12.0]),
                              torch.ones(2, 1, dtype=torch.bool, device=DEV), 0.9, 0.0, state, shift)
        assert shift.tolist() == _f32([0.37, -1.25]).tolist() and state.abs().sum().item() == 0.0


# ---------------------------------------------------------------------------------------------------- 3. streaming
CHUNK, BS = 960, 8
HZ = {"v0": 150.0, "v1": 700.0, "v2": 3000.0}


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 700, 450, 64))}
    p = MS.VoicePool(voices)
    for name, hz in HZ.items():
        p.set_register(name, hz=hz)
    return p                                                                 # v3 carries no register


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _drive(conv, sess, pcm, ticks, actions=None, after=None):
    outs = [[] for _ in sess]
    for tick in range(ticks):
        if tick == 0:
            for s, p in enumerate(sess):
                conv.open(s, **p)
        for a in (actions or {}).get(tick, []):
            a(conv)
        feed = {s: pcm[s][tick * CHUNK:(tick + 1) * CHUNK] for s in range(len(sess))}
        for s, o in conv.step(feed).items():
            if o is not None:
                outs[s].append(o)
        if after is not None and tick >= BS:
            after(conv, tick)
    return outs


def test_a_converter_with_no_auto_session_is_bitwise_the_plain_converter(pool):
    sess = [dict(voice="v0", pitch=2.0, f0_rate=0.8), dict(voice="v3", pitch=-1.5, alpha=0.2)]
    pcm = [_pcm(CHUNK * 12, 40 + s) for s in range(2)]
    plain = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4)
    want = _drive(plain, sess, pcm, 12)
    auto = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, auto_pitch=True)
    got = _drive(auto, [dict(p, auto_pitch=False) for p in sess], pcm, 12)
    assert all(len(o) == 12 - BS for o in got) and all(_same(a, b) for a, b in zip(got, want))
    assert auto.reg_state.abs().sum().item() == 0.0 and auto.shift_eff.tolist() == [2.0, -1.5]
    with pytest.raises(ValueError, match="slot 0: auto_pitch=True needs a converter built with"):
        plain.set(0, auto_pitch=True)
    with pytest.raises(ValueError, match="auto_pitch must be a bool"):
        auto.set(0, auto_pitch=1)


def test_a_session_on_auto_follows_the_recurrence_of_its_twins_f0(pool):
    """slot 0 on auto (offset 0.5) and slot 1 plain at pitch 0 get the same chunks, voice and f0_rate: the twin's f0 is the source's
    (rate applied, shift 0), so the NumPy recurrence over its pitch gives the shift slot 0 must carry on that tick"""
    ticks = BS + 8
    one = _pcm(CHUNK * ticks, 51)
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, auto_pitch=True)
    decay, prior = 2.0 ** (-(CHUNK / 16000) / 10.0), 0.5 * 50 * BS
    assert (conv.auto_decay, conv.auto_prior) == (decay, prior)
    target = np.float32(PR.pitch(np.float32(HZ["v0"])))
    seen = dict(state=np.zeros((1, 2)), shifts=[], voiced=0, frames=0)

    def check(c, tick):
        f0 = c.last_f0.cpu().numpy()[:, 0]
        twin = f0[1]
        v = PR.voiced(PR.pitch(twin))
        seen["voiced"] += int(v.sum())
        seen["frames"] += v.size
        seen["state"], shift = PR.follow_rows(seen["state"], twin[None], [1.0], [0.5], [1], [target], [1], decay, prior)
        want = twin.astype(np.float64) * 2.0 ** (float(shift[0]) / 12.0)
        rel = np.abs(f0[0][v] - want[v]) / want[v]
        print(f"tick {tick}: shift {float(shift[0]):+.5f} semitones (device {float(c.shift_eff[0]):+.5f}), voiced {int(v.sum())}/"
              f"{v.size}, max relative f0 error {rel.max():.2e}")
        assert np.all(rel <= 1e-5) and np.all(f0[0][~v] == 0.0)
        assert float(c.shift_eff[1]) == 0.0
        seen["shifts"].append(float(shift[0]))
    _drive(conv, [dict(voice="v0", pitch=0.5, f0_rate=0.8, auto_pitch=True), dict(voice="v0", pitch=0.0, f0_rate=0.8)], [one, one],
           ticks, after=check)
    assert len(seen["shifts"]) == ticks - BS and 2 * seen["voiced"] >= seen["frames"]          # at least half the frames voiced
    auto_part = [s - 0.5 for s in seen["shifts"]]
    assert abs(auto_part[0]) > 0.1 and abs(auto_part[-1]) > 2 * abs(auto_part[0])        # at work, and growing with the evidence
    S, W = conv.reg_state[0].tolist()                        # (the host inverted the twin's transform: ~1e-6 semitones a frame)
    assert W == seen["state"][0, 1] and abs(S - seen["state"][0, 0]) <= 1e-6 * abs(S)
    assert conv.reg_state[1].abs().sum().item() == 0.0
    conv.close(0)
    assert conv.reg_state[0].abs().sum().item() == 0.0 and int(conv.auto_on[0]) == 0


def test_graph_replay_is_bitwise_eager_through_switches_of_auto_pitch(pool):
    ticks = BS + 11
    pcm = [_pcm(CHUNK * ticks, 60 + s) for s in range(3)]
    sess = [dict(voice="v0", pitch=1.0), dict(voice={"v1": 2, "v2": 1}, f0_rate=0.9, auto_pitch=True), dict(voice="v3", alpha=0.1)]
    acts = {BS + 2: [lambda c: c.set(0, auto_pitch=True)], BS + 5: [lambda c: c.set(0, voice="v2")],
            BS + 8: [lambda c: c.set(0, auto_pitch=False), lambda c: c.set(1, pitch=-0.5)]}
    states = {}

    def make():
        return MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, blend=2, auto_pitch=True)

    def record(key):
        return lambda c, tick: states.setdefault(key, []).append((c.reg_state.clone(), c.shift_eff.clone()))
    graph = make().enable_graph()
    got = _drive(graph, sess, pcm, ticks, acts, record("graph"))
    assert graph.captures == 1
    want = _drive(make(), sess, pcm, ticks, acts, record("eager"))
    assert all(len(o) == ticks - BS for o in got) and all(_same(a, b) for a, b in zip(got, want))
    for (gs, gh), (es, eh) in zip(states["graph"], states["eager"]):
        assert torch.equal(gs, es) and torch.equal(gh, eh)
    # the switches did something: slot 0's automatic part is on between the switches only, and the new voice moved its shift
    sh0 = [float(h[0]) for _, h in states["graph"]]
    assert sh0[0] == sh0[1] == 1.0 and sh0[-1] == 1.0 and all(s != 1.0 for s in sh0[2:8])
    assert (sh0[5] - sh0[4]) > 5.0                                           # v0 (150 Hz) -> v2 (3000 Hz): 52 semitones up, shrunk
    w = MS.blend_spec({"v1": 2, "v2": 1})[1]
    want_t = np.float32(w[0] * pool.register("v1") + w[1] * pool.register("v2"))
    assert float(graph.target[1]) == float(want_t)
    # enable_graph mid-session: capture_step runs the step three times, the running registers come back bit for bit
    before = graph.reg_state.clone()
    assert before[1].abs().sum().item() > 0
    graph.enable_graph()
    assert torch.equal(graph.reg_state, before) and graph.captures == 2


# ---------------------------------------------------------------------------------------------------- 4. convert_many
MANY_CHUNK = 3200


@pytest.fixture(scope="module")
def rig():
    from module.pipeline import Converter
    conv = Converter(*_nets(), DEV)
    g = torch.Generator(device=DEV).manual_seed(43)
    tokens = {"a": torch.randn(1, 768, 600, device=DEV, generator=g), "b": synthetic.make_library(512, 5).to(DEV),
              "bare": synthetic.make_library(100, 6).to(DEV)}
    pool_ = MS.VoicePool(tokens, device=DEV, registers={"a": (PR.pitch(np.float32(900.0)) * 4.0, 4.0)})
    pool_.set_register("b", hz=300.0)
    utts = [synthetic.make_waveform(n, 310 + i).to(DEV) for i, n in enumerate((2 * MANY_CHUNK, 3 * MANY_CHUNK + 700, MANY_CHUNK))]
    return conv, pool_, [u / u.abs().max() for u in utts]


def _measured(conv, u):
    """the utterance's own (sum, count): the raw f0 of its windows' centre thirds through the stats call, read back"""
    from module.pipeline import make_windows
    from module.spectrogram import spectrogram
    windows, _ = make_windows(u.reshape(1, -1), MANY_CHUNK)
    f0 = conv.pe.estimate(spectrogram(windows))
    return MS.pitch_stats_groups(f0, _i32([0, windows.shape[0]]), MANY_CHUNK // 320, 2 * MANY_CHUNK // 320)[0].tolist()


def test_convert_many_auto_utterance_is_bitwise_alone_and_in_a_corpus(rig):
    conv, pool_, utts = rig
    kw = dict(chunk=MANY_CHUNK, k=4, trim_context=True)
    alone = conv.convert_many(utts[:1], pool_, ["a"], pitch_shift=0.5, auto_pitch=True, **kw)[0]
    corpus = conv.convert_many(utts, pool_, ["a", {"a": 1, "b": 3}, "bare"], pitch_shift=[0.5, -1.0, 2.0], alpha=[0.0, 0.1, 0.0],
                               auto_pitch=[True, True, False], **kw)
    assert alone.shape == (1, 2 * MANY_CHUNK) and torch.equal(alone, corpus[0])
    # the shift is the one the stats give: bitwise the plain path at offset + (target - mean), formed in float32 on the host
    for i, voice, offset in ((0, "a", 0.5), (1, {"a": 1, "b": 3}, -1.0)):
        s, c = _measured(conv, utts[i])
        assert c > 0
        target = np.float32(pool_.blend_register(*MS.blend_spec(voice)))
        shift = np.float32(offset) + (target - np.float32(s / c))
        assert abs(float(shift) - offset) > 1.0
        plain = conv.convert_many([utts[i]], pool_, [voice], pitch_shift=float(shift), alpha=[0.0, 0.1][i], **kw)[0]
        assert torch.equal(plain, corpus[i]), i
    off = conv.convert_many([utts[2]], pool_, ["bare"], pitch_shift=2.0, **kw)[0]
    assert torch.equal(off, corpus[2])                                       # a plain utterance beside auto ones: as alone
    with pytest.raises(ValueError, match="voice 'bare' has no register"):
        conv.convert_many(utts[:1], pool_, [{"a": 1, "bare": 1}], auto_pitch=True, **kw)
    with pytest.raises(ValueError, match="auto_pitch: expected bools"):
        conv.convert_many(utts[:1], pool_, ["a"], auto_pitch=1, **kw)


def test_convert_many_with_the_voices_register_at_the_utterances_own_mean_is_the_plain_path(rig):
    conv, pool_, utts = rig
    kw = dict(chunk=MANY_CHUNK, k=4, trim_context=True)
    was = pool_.registers["a"]
    try:
        pool_.set_register("a", register=_measured(conv, utts[0]))
        auto = conv.convert_many(utts[:1], pool_, ["a"], pitch_shift=-1.5, auto_pitch=True, **kw)[0]
    finally:
        pool_.set_register("a", register=was)
    plain = conv.convert_many(utts[:1], pool_, ["a"], pitch_shift=-1.5, **kw)[0]
    assert torch.equal(auto, plain)


@pytest.mark.parametrize("trim", [True, False])
def test_convert_many_with_auto_pitch_off_is_the_present_path(rig, trim):
    conv, pool_, utts = rig
    kw = dict(pitch_shift=[0.5, -1.0, 2.0], chunk=MANY_CHUNK, k=4, trim_context=trim)
    voices = ["a", "b", "bare"]
    today = conv.convert_many(utts, pool_, voices, **kw)
    off = conv.convert_many(utts, pool_, voices, auto_pitch=[False] * 3, **kw)
    assert all(torch.equal(a, b) for a, b in zip(today, off))
    on = conv.convert_many(utts, pool_, voices, auto_pitch=[False, True, False], **kw)
    assert torch.equal(on[0], today[0]) and torch.equal(on[2], today[2]) and not torch.equal(on[1], today[1])


# ---------------------------------------------------------------------------------------------------- 5. the pool
def test_registers_are_measured_at_enrolment_and_survive_the_pools_operations():
    from module import audio_io
    from module.spectrogram import spectrogram
    CE, PE, _ = (n.to(DEV) for n in _nets())
    wav, sr = synthetic.make_waveform(24000 * 2, 60).repeat(2, 1) * torch.tensor([[0.5], [0.25]]), 24000
    plain = MS.VoicePool(capacity=2000)
    m = MS.enrol_voice(plain, "v", CE, wav, sr)
    assert plain.register("v") is None
    pool_ = MS.VoicePool(capacity=2000)
    assert MS.enrol_voice(pool_, "v", CE, wav, sr, max_frames=17, f0_estimator=PE) == m          # add, then extends
    assert torch.equal(pool_.rows[:m], plain.rows[:m]) and torch.equal(pool_.norms[:m], plain.norms[:m])
    wf = audio_io.resample(wav.to(DEV), sr, 16000)
    wf = wf / wf.abs().max()
    f0 = PE.estimate(spectrogram(wf[:1]))
    ref = PR.stats_groups(f0.cpu().numpy()[:, 0], [0, 1])[0]
    s, c = pool_.registers["v"]
    assert c == ref[1] > 50 and abs(s - ref[0]) <= 1e-12 * abs(ref[0])
    assert abs(pool_.register("v") - PR.mean_pitch(f0.cpu().numpy())) < 1e-9
    parts, reg = MS.voice_parts(CE, wav, sr, device=DEV, f0_estimator=PE)
    assert reg == (s, c) and MS.voice_parts(CE, None, None, lib=torch.ones(768, 3, device=DEV), device=DEV, f0_estimator=PE)[1] is None
    # merged on extend, kept through another voice's removal, compact and a move; gone with its own voice
    pool_.add("w", torch.randn(768, 40, device=DEV), register=(-30.0, 3.0))
    pool_.extend("v", torch.randn(768, 25, device=DEV), register=(10.0, 4.0))                    # (w lies behind v: v moves)
    assert pool_.registers["v"] == (s + 10.0, c + 4.0) and pool_.segment("v")[0] > 0
    pool_.add("x", torch.randn(768, 10, device=DEV))
    pool_.remove("x")
    pool_.compact()
    assert pool_.segment("w")[0] == 0 and pool_.registers == {"v": (s + 10.0, c + 4.0), "w": (-30.0, 3.0)}
    pool_.remove("w")
    pool_.add("w", torch.randn(768, 40, device=DEV))
    assert pool_.register("w") is None and pool_.registers["v"] == (s + 10.0, c + 4.0)


def test_auto_pitch_on_a_voice_without_a_register_is_refused_before_anything_changes(pool):
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, blend=2, auto_pitch=True)
    conv.open(0, "v0", pitch=1.0, auto_pitch=True)
    arrays = ("seg_lo", "seg_len", "weight", "alpha", "f0_rate", "pitch", "auto_on", "target", "reg_state", "in_post", "out_pre")
    before = {a: getattr(conv, a).clone() for a in arrays}
    with pytest.raises(ValueError, match="slot 1: auto pitch: voice 'v3' has no register"):
        conv.open(1, "v3", auto_pitch=True)
    with pytest.raises(ValueError, match="slot 0: auto pitch: voice 'v3' has no register"):
        conv.set(0, voice={"v1": 1, "v3": 1}, pitch=3.0)
    assert all(torch.equal(getattr(conv, a), before[a]) for a in arrays)
    assert not conv.is_open[1] and conv.params[0]["voice"] == "v0"
    conv.open(1, "v3")                                                       # the same voice without auto pitch is fine
    conv.set(0, voice={"v1": 1, "v2": 1})
    assert float(conv.target[0]) == float(np.float32(0.5 * pool.register("v1") + 0.5 * pool.register("v2")))
