"""Pitch range on the device (csrc/pitch_auto.hip) and through the batched paths, against the NumPy restatement tools/pitch_range_ref.py,
which reproduces the kernels' summation order and is therefore compared bit for bit.

1. alive_pitch_stats2_groups: columns 0 and 1 bitwise alive_pitch_stats_groups, all three bitwise the restatement.
2. alive_pitch_range_groups, alive_pitch_follow2_rows, alive_pitch_transform_rows_centred: bitwise the restatement; S, W and the auto
   shift bitwise the two-moment kernel run beside it; rows that are off bitwise the uncentred transform.
3. MultiStreamConverter(pitch_range=True): sessions at the defaults bitwise the plain converter, an auto_pitch session bitwise the
   auto_pitch=True converter; a session on intonation + auto_range against the recurrence run on its plain twin's f0; graph replay
   bitwise eager through switches, one capture; a stalled slot of a sparse converter stands still; RealtimeConverter(intonation=).
4. convert_many(auto_range=): alone bitwise in a corpus; off is the present path; a voice declared at the utterance's own moments.
5. The CLIs: files without the new keys write what the plain path writes."""
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

import pitch_range_ref as RR                                         # noqa: E402
import pitch_ref as PR                                               # noqa: E402
from module import audio_io                                          # noqa: E402
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


def _f64(a):
    return torch.tensor(list(a), dtype=torch.float64, device=DEV)


def _f0(N, T, seed):
    """f0 with voiced values over the pitch range and every kind of unvoiced frame: 0, NaN, +inf, negatives"""
    rng = np.random.default_rng(seed)
    f0 = rng.uniform(30.0, 4000.0, size=(N, T)).astype(np.float32)
    flat = f0.reshape(-1)
    for j, bad in enumerate((0.0, np.nan, np.inf, -220.0, -0.0)):
        flat[j + 1::11] = bad
    return f0


def _bits(a):
    """float arrays compared bit for bit (NaN included)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------- 1. the stats kernel
STATS_CASES = [
    # (N, T, first, row to silence (all-unvoiced group) or None, (t_lo, t_hi) sub-range): test_gpu_auto_pitch.py's, then T = 1, 255, 257
    (1, 1, [0, 1], None, (0, 0)),
    (1, 1, [0, 0, 1], 0, (1, 1)),
    (5, 7, [0, 2, 2, 5], None, (2, 6)),
    (5, 7, [0, 2, 3, 5], 2, (0, 1)),
    (3, 300, [0, 1, 1, 3], None, (255, 257)),
    (3, 300, [0, 1, 2, 3], 1, (7, 290)),
    (4, 1, [0, 1, 4], None, (0, 1)),
    (3, 255, [0, 2, 3], None, (1, 255)),
    (3, 257, [0, 0, 3], 1, (0, 256)),
]


@pytest.mark.parametrize("N,T,first,silent,sub", STATS_CASES)
def test_stats2_kernel_is_bitwise_the_old_kernel_and_the_restatement(N, T, first, silent, sub):
    f0 = _f0(N, T, 10 * N + T)
    if N * T == 1:
        f0[0, 0] = 311.0
    if silent is not None:
        f0[silent] = np.array([0.0, np.nan, np.inf, -5.0] * T, dtype=np.float32)[:T]
    dev = torch.from_numpy(f0).to(DEV).view(N, 1, T)
    G = len(first) - 1
    for lo, hi in ((0, T), sub):
        got = MS.pitch_stats2_groups(dev, _i32(first), lo, hi)
        old = MS.pitch_stats_groups(dev, _i32(first), lo, hi)
        ref = RR.stats2_groups(f0, first, lo, hi)
        assert got.shape == (G, 3) and got.dtype == torch.float64
        assert torch.equal(got[:, :2], old)                                  # bitwise what the two-moment kernel writes
        g_ = got.cpu().numpy()
        print(f"stats2 ({N}, {T}) first {first} frames [{lo}, {hi}): device {g_.tolist()}")
        assert np.array_equal(_bits(g_), _bits(ref))                         # all three columns, bit for bit
        for g in range(G):
            if first[g] == first[g + 1] or (silent is not None and first[g] == silent and first[g + 1] == silent + 1) or lo == hi:
                assert g_[g].tolist() == [0.0, 0.0, 0.0], g                  # empty, all-unvoiced, no frames
            alone = MS.pitch_stats2_groups(dev, _i32([first[g], first[g + 1]]), lo, hi)
            assert torch.equal(alone[0], got[g]), g                          # the other groups do not matter


# ---------------------------------------------------------------------------------------------------- 2. the three other kernels
def test_range_groups_kernel_is_bitwise_the_restatement():
    f0 = _f0(9, 300, 77)
    first = [0, 3, 3, 4, 7, 9]
    f0[3] = 0.0                                                              # group 2: nothing voiced
    f0[7:9] = 440.0                                                          # group 4: every frame at pitch -9, sums exact -> v = 0, r = 1
    stats = MS.pitch_stats2_groups(torch.from_numpy(f0).to(DEV), _i32(first))
    inton, on, sd, rmax = [1.5, 0.7, 0.3, 0.7, 1.1], [1, 1, 1, 0, 1], [1e3, 2.0, 2.0, 1e-3, 5.0], 3.0
    got = MS.pitch_range_groups(stats, _i32(first), 9, _f32(inton), _i32(on), _f64(sd), rmax)
    ref = RR.range_groups(stats.cpu().numpy(), first, inton, on, sd, rmax)
    for g_, r_ in zip(got, ref):
        assert g_.cpu().numpy().dtype == r_.dtype and np.array_equal(_bits(g_.cpu().numpy()), _bits(r_))
    it, c, con = (x.cpu().numpy() for x in got)
    assert np.all(it[:3] == np.float32(np.float64(np.float32(1.5)) * 3.0)) and np.all(con[:3] == 1)      # clamped at range_max
    assert it[3] == np.float32(0.3) and c[3] == 0.0 and con[3] == 0          # on, but nothing voiced: passed through
    assert np.all(_bits(it[4:7]) == _bits(np.float32(0.7))) and np.all(c[4:7] == 0.0) and np.all(con[4:7] == 0)      # off: bit for bit
    assert np.all(it[7:] == np.float32(1.1)) and np.all(con[7:] == 1)        # v = 0: r = 1
    assert np.all(c[7:] == np.float32(-9.0))
    # the other end of the clamp
    got = MS.pitch_range_groups(stats, _i32(first), 9, _f32(inton), _i32(on), _f64([1e-3] * 5), rmax)[0].cpu().numpy()
    assert np.all(got[:3] == np.float32(np.float64(np.float32(1.5)) * (1.0 / 3.0)))


def _state3(rng, N):
    """(S, W, Q) of a source that has been heard: mean in [-40, 20], variance in [1, 9]"""
    W = rng.uniform(5.0, 500.0, size=N)
    m = rng.uniform(-40.0, 20.0, size=N)
    return np.stack([m * W, W, W * (m * m + rng.uniform(1.0, 9.0, size=N))], axis=1)


@pytest.mark.parametrize("T,decay", [(33, 0.5), (300, 0.97)])
def test_follow2_kernel_is_bitwise_the_old_kernel_and_the_restatement(T, decay):
    """rows: 0 auto only; 1 does not follow; 2 fresh, auto range towards a huge sd (the top of the clamp); 3 auto + auto range towards
    a tiny sd (the bottom); 4 fresh, auto range, every frame equal (v = 0: r = 1 -- on every call at decay 0.5, where nothing rounds);
    5 intonation only and not emitting (its state stays, its outputs are formed from it)"""
    N, prior, rmax = 6, 40.0, 2.5
    rng = np.random.default_rng(8)
    auto, ranged = [1, 0, 0, 1, 0, 0], [0, 0, 1, 1, 1, 0]
    inton = [1.0, 1.0, 1.5, 0.8, 1.0, 0.6]
    emit = [1, 1, 1, 1, 1, 0]
    rate = [1.0, 0.5, 0.8, 0.7, 1.0, 1.25]
    offset = [0.0, 1.7, -2.0, 0.3, 5.0, -0.6]
    target = [-30.0, 0.0, -12.5, 4.0, 0.0, 63.9]
    sd = [0.0, 0.0, 1e3, 1e-3, 2.0, 0.0]
    follows = [int(a or r or np.float32(i) != 1) for a, r, i in zip(auto, ranged, inton)]
    assert follows == [1, 0, 1, 1, 1, 1]
    state0 = _state3(rng, N)
    state0[2] = state0[4] = 0.0                                              # fresh sessions
    state = torch.from_numpy(state0.copy()).to(DEV)
    old_state = torch.from_numpy(state0[:, :2].copy()).to(DEV)
    outs = (torch.full((N,), 99.0, device=DEV), torch.full((N,), 99.0, device=DEV), torch.full((N,), 99.0, device=DEV),
            torch.full((N,), 99, dtype=torch.int32, device=DEV))
    old_shift = torch.full((N,), 99.0, device=DEV)
    emit_d = torch.tensor(emit, dtype=torch.bool, device=DEV).view(N, 1)
    ref_state, seen = state0.copy(), set()
    for call in range(5):
        f0 = _f0(N, T, 20 + call)
        f0[4] = 440.0
        dev = torch.from_numpy(f0).to(DEV).view(N, 1, T)
        MS.pitch_follow2_rows_(dev, _f32(rate), _f32(offset), _i32(auto), _f32(target), _f32(inton), _i32(ranged), _f64(sd), emit_d,
                               decay, prior, rmax, state, *outs)
        # the two-moment kernel beside it, on for the rows that follow here
        MS.pitch_follow_rows_(dev, _f32(rate), _f32(offset), _i32(follows), _f32(target), emit_d, decay, prior, old_state, old_shift)
        ref_state, *ref = RR.follow2_rows(ref_state, f0, rate, offset, auto, target, inton, ranged, sd, emit, decay, prior, rmax)
        got_state = state.cpu().numpy()
        got = [o.cpu().numpy() for o in outs]
        print(f"follow2 T {T} call {call}: shift {got[0].tolist()} inton {got[1].tolist()} centre {got[2].tolist()} on {got[3].tolist()}")
        assert np.array_equal(_bits(got_state[:, :2]), _bits(old_state.cpu().numpy()))        # S, W: the old kernel's, bit for bit
        assert np.array_equal(_bits(got_state), _bits(ref_state))
        for g_, r_ in zip(got, ref):
            assert g_.dtype == r_.dtype and np.array_equal(_bits(g_), _bits(r_))
        for n in (0, 3):                                                     # an auto row's shift is the old kernel's expression
            assert _bits(got[0][n:n + 1]) == _bits(old_shift.cpu().numpy()[n:n + 1])
        # row 1 does not follow: untouched state, shift = offset bit for bit, intonation 1, no centre
        assert np.array_equal(got_state[1], state0[1])
        assert (got[0][1], got[1][1], got[2][1], got[3][1]) == (np.float32(1.7), 1.0, 0.0, 0)
        assert np.array_equal(got_state[5], state0[5]) and got[3][5] == 1 and got[0][5] == np.float32(-0.6)      # not emitting
        assert got[0][2] == np.float32(-2.0) and got[0][4] == np.float32(5.0)                 # not on auto: the offset alone
        # which range factors the rows ran at, from the restated state
        for n in (2, 3, 4):
            m, v = RR.mean_var(*ref_state[n])
            r = float(RR.range_factor(v, sd[n], rmax))
            seen.add((n, "top" if r == rmax else "bottom" if r == 1.0 / rmax else "one" if r == 1.0 else "inside"))
            if n == 4 and (call == 0 or decay == 0.5):
                assert v == 0.0 and r == 1.0 and got[1][4] == 1.0 and got[3][4] == 0          # all frames equal: r = 1, so I = 1
    assert (2, "top") in seen and (3, "bottom") in seen and (4, "one") in seen                # both ends of the clamp were reached


def test_follow2_kernel_prior_zero_on_an_unvoiced_row_is_exactly_the_offset():
    f0 = torch.tensor([[0.0, float("nan"), float("inf"), -3.0, 0.0]] * 2, device=DEV).view(2, 1, 5)
    state = torch.zeros(2, 3, dtype=torch.float64, device=DEV)
    outs = (torch.full((2,), 99.0, device=DEV), torch.full((2,), 99.0, device=DEV), torch.full((2,), 99.0, device=DEV),
            torch.full((2,), 99, dtype=torch.int32, device=DEV))
    for _ in range(2):
        MS.pitch_follow2_rows_(f0, _f32([1, 1]), _f32([0.37, -1.25]), _i32([1, 0]), _f32([-9.0, 12.0]), _f32([1.5, 0.5]), _i32([1, 1]),
                               _f64([2.0, 3.0]), torch.ones(2, 1, dtype=torch.bool, device=DEV), 0.9, 0.0, 2.0, state, *outs)
        assert outs[0].tolist() == _f32([0.37, -1.25]).tolist() and outs[1].tolist() == [1.0, 1.0] and outs[3].tolist() == [0, 0]
        assert state.abs().sum().item() == 0.0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [33, 257, 450])
def test_centred_transform_rows_off_are_the_old_transform_and_rows_on_the_restatement(mode, T):
    N = 5
    f0 = _f0(N, T, 5 + T)
    rate, shift, inton = [1.0, 0.8, 1.25, 0.5, 1.0], [0.0, 2.5, -3.0, 12.0, -0.75], [1.0, 1.5, 0.6, 0.0, 2.0]
    centre, on = [7.0, -12.5, 99.0, 3.0, -30.25], [0, 1, 0, 1, 1]
    dev = torch.from_numpy(f0).to(DEV).view(N, 1, T)
    got = MS.pitch_transform_rows_centred_(dev.clone(), mode, _f32(rate), _f32(shift), _f32(inton), _f32(centre), _i32(on)).cpu().numpy()[:, 0]
    old = MS.pitch_transform_rows_(dev.clone(), mode, _f32(rate), _f32(shift), _f32(inton)).cpu().numpy()[:, 0]
    ref = RR.transform_rows_centred(f0, mode, rate, shift, inton, centre, on)
    v = PR.voiced(PR.pitch(f0))
    for n in range(N):
        if on[n]:
            assert np.array_equal(_bits(got[n]), _bits(ref[n])), (mode, T, n)
            assert not np.array_equal(got[n], old[n])
        else:
            assert np.array_equal(_bits(got[n]), _bits(old[n])), (mode, T, n)
    assert np.all(got[~v] == 0.0) and np.all(np.isfinite(got)) and np.all(got[v] > 0.0)
    # intonation 0 around a given centre: every voiced frame at 440 * 2^((c + shift + 9) / 12), times the rate in mode 0
    assert np.all(got[3][v[3]] == got[3][v[3]][0])


# ---------------------------------------------------------------------------------------------------- 3. streaming
CHUNK, BS = 960, 8
HZ = {"v0": 150.0, "v1": 700.0, "v2": 3000.0}
ST = {"v0": 2.5, "v1": 4.0, "v2": 1.5}


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 700, 450, 64))}
    p = MS.VoicePool(voices)
    for name, hz in HZ.items():
        p.set_register(name, hz=hz, range_st=ST[name])
    return p                                                                 # v3 carries neither register nor range


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


def test_sessions_at_the_defaults_are_the_plain_converter_and_auto_sessions_the_auto_converter(pool):
    sess = [dict(voice="v0", pitch=2.0, f0_rate=0.8), dict(voice="v3", pitch=-1.5, alpha=0.2)]
    pcm = [_pcm(CHUNK * 12, 40 + s) for s in range(2)]
    kw = dict(chunk=CHUNK, buffersize=BS, k=4)
    plain = MS.MultiStreamConverter(*_nets(), pool, 2, **kw)
    want = _drive(plain, sess, pcm, 12)
    ranged = MS.MultiStreamConverter(*_nets(), pool, 2, pitch_range=True, **kw)
    got = _drive(ranged, [dict(p, intonation=1.0, auto_range=False) for p in sess], pcm, 12)
    assert all(len(o) == 12 - BS for o in got) and all(_same(a, b) for a, b in zip(got, want))
    assert ranged.reg_state.shape == (2, 3) and ranged.reg_state.abs().sum().item() == 0.0
    assert ranged.shift_eff.tolist() == [2.0, -1.5] and ranged.inton_eff.tolist() == [1.0, 1.0] and ranged.centre_on.tolist() == [0, 0]
    assert ranged.pitch_range_state() == [(None, None, 1.0)] * 2
    # an auto_pitch session works here without auto_pitch=True being passed, bitwise as in an auto_pitch=True converter
    sess[0]["auto_pitch"] = True
    auto = MS.MultiStreamConverter(*_nets(), pool, 2, auto_pitch=True, **kw)
    want = _drive(auto, sess, pcm, 12)
    ranged = MS.MultiStreamConverter(*_nets(), pool, 2, pitch_range=True, **kw)
    got = _drive(ranged, sess, pcm, 12)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert torch.equal(ranged.reg_state[:, :2], auto.reg_state) and torch.equal(ranged.shift_eff, auto.shift_eff)
    assert float(ranged.reg_state[0, 2]) > 0 and ranged.reg_state[1].abs().sum().item() == 0.0
    assert ranged.inton_eff.tolist() == [1.0, 1.0] and ranged.centre_on.tolist() == [0, 0]
    # both keywords are refused on a converter built without pitch_range, and checked
    with pytest.raises(ValueError, match="slot 0: intonation=1.5 / auto_range=False need a converter built with"):
        plain.set(0, intonation=1.5)
    with pytest.raises(ValueError, match="slot 0: intonation=1.0 / auto_range=True need a converter built with"):
        auto.set(0, auto_range=True)
    with pytest.raises(ValueError, match="pitch_range_state needs a converter built with"):
        plain.pitch_range_state()
    for bad in (-0.1, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="slot 0: intonation=.* must be a finite number >= 0"):
            ranged.set(0, intonation=bad)
    with pytest.raises(ValueError, match="slot 0: auto_range must be a bool"):
        ranged.set(0, auto_range=1)


def test_auto_range_on_a_voice_without_a_range_is_refused_before_anything_changes(pool):
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, blend=2, pitch_range=True)
    conv.open(0, "v0", pitch=1.0, intonation=1.5, auto_range=True)
    assert float(conv.target_sd[0]) == pool.pitch_range("v0") and int(conv.range_on[0]) == 1 and float(conv.intonation[0]) == 1.5
    arrays = ("seg_lo", "seg_len", "weight", "alpha", "f0_rate", "pitch", "auto_on", "target", "reg_state", "intonation", "range_on",
              "target_sd", "in_post", "out_pre")
    before = {a: getattr(conv, a).clone() for a in arrays}
    with pytest.raises(ValueError, match="slot 1: auto range: voice 'v3' has no pitch range"):
        conv.open(1, "v3", auto_range=True)
    with pytest.raises(ValueError, match="slot 0: auto range: voice 'v3' has no pitch range"):
        conv.set(0, voice={"v1": 1, "v3": 1}, pitch=3.0)
    assert all(torch.equal(getattr(conv, a), before[a]) for a in arrays)
    assert not conv.is_open[1] and conv.params[0]["voice"] == "v0"
    conv.open(1, "v3", intonation=0.5)                                       # the same voice with a plain intonation is fine
    conv.set(0, voice={"v1": 1, "v2": 3})
    assert float(conv.target_sd[0]) == 0.25 * ST["v1"] + 0.75 * ST["v2"] == pool.blend_range(["v1", "v2"], [0.25, 0.75])
    conv.close(0)
    assert (float(conv.intonation[0]), int(conv.range_on[0]), float(conv.target_sd[0])) == (1.0, 0, 0.0)
    assert conv.reg_state[0].abs().sum().item() == 0.0


def test_a_session_on_intonation_and_auto_range_follows_the_recurrence_of_its_twins_f0(pool):
    """slot 0 at intonation 1.5 with auto range (offset 0.5) and slot 1 plain at pitch 0 get the same chunks, voice and f0_rate: the
    twin's f0 is the source's (rate applied, shift 0), so the restated recurrence over its pitch gives the centre, the effective
    intonation and the f0 slot 0 must carry on that tick.  The host inverts the twin's float32 transform: a voiced frame's pitch is off
    by ~1e-6 semitones from that round trip and up to 4e-6 from its own float32 rounding at magnitude <= 64, together dp = 1e-5 with a
    factor two to spare.  The centre moves by at most dp plus its float32 rounding (4e-6); r = sd_t / sd_s moves by r * dp / sd_s, so
    I_eff by at most 1.5 * range_max * dp / sd_s plus its float32 rounding; the f0 bar is the twin test's 1e-5 relative times
    max(1, I_eff), because the scaling multiplies the inverted pitch's error."""
    ticks, rmax, dp = BS + 8, 2.0, 1e-5
    one = _pcm(CHUNK * ticks, 51)
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, pitch_range=True, pitch_range_max=rmax)
    decay, prior = 2.0 ** (-(CHUNK / 16000) / 10.0), 0.5 * 50 * BS
    assert (conv.auto_decay, conv.auto_prior, conv.range_max) == (decay, prior, rmax)
    sd_t = pool.pitch_range("v0")
    assert abs(sd_t - ST["v0"]) < 1e-12
    seen = dict(state=np.zeros((1, 3)), inton=[], voiced=0, frames=0)

    def check(c, tick):
        f0 = c.last_f0.cpu().numpy()[:, 0]
        twin = f0[1]
        p = PR.pitch(twin)
        v = PR.voiced(p)
        seen["voiced"] += int(v.sum())
        seen["frames"] += v.size
        seen["state"], shift, it, centre, on = RR.follow2_rows(seen["state"], twin[None], [1.0], [0.5], [0], [0.0], [1.5], [1], [sd_t],
                                                               [1], decay, prior, rmax)
        m, var = RR.mean_var(*seen["state"][0])
        assert var > 0.0                                                     # the source has a range to match
        sd_s = float(np.sqrt(var))
        got_m, got_sd, got_i = c.pitch_range_state()[0]
        I = float(it[0])
        want = twin.astype(np.float64) * 2.0 ** (((p.astype(np.float64) - float(centre[0])) * (I - 1.0) + float(shift[0])) / 12.0)
        rel = np.abs(f0[0][v] - want[v]) / want[v]
        print(f"tick {tick}: source mean {m:+.4f} sd {sd_s:.4f} (device {got_m:+.4f}, {got_sd:.4f}), I_eff {I:.6f} (device {got_i:.6f}), "
              f"centre {float(centre[0]):+.5f} (device {float(c.centre[0]):+.5f}), voiced {int(v.sum())}/{v.size}, "
              f"max relative f0 error {rel.max():.2e}")
        assert shift[0] == np.float32(0.5) == np.float32(float(c.shift_eff[0])) and int(c.centre_on[0]) == int(on[0]) == 1
        assert abs(float(c.centre[0]) - float(centre[0])) <= dp + 4e-6
        assert abs(got_i - I) <= 1.5 * rmax * dp / sd_s + 2.4e-7 * I
        assert np.all(rel <= 1e-5 * max(1.0, I)) and np.all(f0[0][~v] == 0.0)
        assert float(c.shift_eff[1]) == 0.0 and float(c.inton_eff[1]) == 1.0 and int(c.centre_on[1]) == 0
        seen["inton"].append(I)
    _drive(conv, [dict(voice="v0", pitch=0.5, f0_rate=0.8, intonation=1.5, auto_range=True), dict(voice="v0", pitch=0.0, f0_rate=0.8)],
           [one, one], ticks, after=check)
    assert len(seen["inton"]) == ticks - BS and 2 * seen["voiced"] >= seen["frames"]          # at least half the frames voiced
    away = [abs(i - 1.0) for i in seen["inton"]]
    assert away[0] > 0.0 and all(b > a for a, b in zip(away, away[1:]))                       # growing with the evidence
    S, W, Q = conv.reg_state[0].tolist()
    # (the host inverted the twin's transform: |dS| <= dp * W, and |dQ| <= 2 dp sum w |p| <= 2 dp sqrt(W Q) by Cauchy-Schwarz)
    assert W == seen["state"][0, 1] and abs(S - seen["state"][0, 0]) <= dp * W and abs(Q - seen["state"][0, 2]) <= 2 * dp * np.sqrt(W * Q)
    assert conv.reg_state[1].abs().sum().item() == 0.0
    conv.close(0)
    assert conv.reg_state[0].abs().sum().item() == 0.0 and int(conv.range_on[0]) == 0


def test_graph_replay_is_bitwise_eager_through_switches_of_intonation_auto_range_and_voice(pool):
    ticks = BS + 11
    pcm = [_pcm(CHUNK * ticks, 60 + s) for s in range(3)]
    sess = [dict(voice="v0", pitch=1.0), dict(voice={"v1": 2, "v2": 1}, f0_rate=0.9, intonation=1.2, auto_range=True),
            dict(voice="v3", alpha=0.1)]
    acts = {BS + 2: [lambda c: c.set(0, intonation=1.5)], BS + 5: [lambda c: c.set(0, voice="v2", auto_range=True)],
            BS + 8: [lambda c: c.set(0, intonation=1.0, auto_range=False), lambda c: c.set(1, auto_pitch=True, pitch=-0.5)]}
    states = {}
    arrays = ("reg_state", "shift_eff", "inton_eff", "centre", "centre_on")

    def make():
        return MS.MultiStreamConverter(*_nets(), pool, 3, chunk=CHUNK, buffersize=BS, k=4, blend=2, pitch_range=True)

    def record(key):
        return lambda c, tick: states.setdefault(key, []).append([getattr(c, a).clone() for a in arrays])
    graph = make().enable_graph()
    got = _drive(graph, sess, pcm, ticks, acts, record("graph"))
    assert graph.captures == 1
    want = _drive(make(), sess, pcm, ticks, acts, record("eager"))
    assert all(len(o) == ticks - BS for o in got) and all(_same(a, b) for a, b in zip(got, want))
    for g_, e_ in zip(states["graph"], states["eager"]):
        assert all(torch.equal(a, b) for a, b in zip(g_, e_))
    # the switches did something: slot 0 follows between the switches only; the third state column moves with the others
    i0 = [float(s[2][0]) for s in states["graph"]]
    on0 = [int(s[4][0]) for s in states["graph"]]
    assert i0[0] == i0[1] == 1.0 and i0[-1] == 1.0 and all(i != 1.0 for i in i0[2:8]) and on0 == [0, 0] + [1] * 6 + [0] * 3
    assert i0[5] != i0[4]                                                    # auto range towards v2 joined the intonation
    sh1 = [float(s[1][1]) for s in states["graph"]]
    assert sh1[7] == 0.0 and sh1[8] != -0.5                                  # slot 1's auto pitch came on, on top of its new offset
    w = MS.blend_spec({"v1": 2, "v2": 1})[1]
    assert float(graph.target_sd[1]) == w[0] * ST["v1"] + w[1] * ST["v2"]
    # enable_graph mid-session: capture_step runs the step three times, all three state columns come back bit for bit
    before = graph.reg_state.clone()
    outs = [getattr(graph, a).clone() for a in arrays[1:]]
    latest = graph.pitch_range_state()
    assert before[1].abs().min().item() > 0 and before.shape == (3, 3) and latest[1][2] != 1.0
    graph.enable_graph()
    assert torch.equal(graph.reg_state, before) and graph.captures == 2
    # ... and the follower's outputs stay the latest tick's, so pitch_range_state() reports what it reported
    assert all(torch.equal(getattr(graph, a), o) for a, o in zip(arrays[1:], outs)) and graph.pitch_range_state() == latest


def test_a_stalled_slot_of_a_sparse_converter_keeps_its_three_state_values(pool):
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, pitch_range=True, sparse=True)
    pcm = [_pcm(CHUNK * (BS + 6), 70 + s) for s in range(2)]
    for s in range(2):
        conv.open(s, "v0", intonation=1.5, auto_range=True)
    at = [0, 0]

    def step(slots):
        feed = {}
        for s in slots:
            feed[s] = pcm[s][at[s] * CHUNK:(at[s] + 1) * CHUNK]
            at[s] += 1
        return conv.step(feed)
    for _ in range(BS + 2):
        step((0, 1))
    before = conv.reg_state.clone()
    assert before.abs().min().item() > 0
    for _ in range(2):                                                       # slot 1 sits two ticks out
        res = step((0,))
        assert sorted(res) == [0] and res[0] is not None
        assert torch.equal(conv.reg_state[1], before[1]) and not torch.equal(conv.reg_state[0], before[0])
    step((0, 1))
    assert not torch.equal(conv.reg_state[1], before[1])


def test_realtime_converter_with_intonation_is_a_one_slot_converter(pool, monkeypatch):
    from module.realtime import RealtimeConverter
    ticks = BS + 5
    pcm = _pcm(CHUNK * (ticks + 1), 81)
    lib = pool.tokens("v0")[None]
    kw = dict(chunk=CHUNK, buffersize=BS, k=4)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, f0_rate=0.9, intonation=1.5, **kw)
    assert rt.pitch_range and not rt.reuse
    ms = MS.MultiStreamConverter(*_nets(), pool, 1, pitch_range=True, **kw)
    ms.open(0, "v0", pitch=1.5, f0_rate=0.9, intonation=1.5)
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        if t == ticks - 1:
            saved = ms.phi.clone(), ms.reg_state.clone(), rt.phi, rt._reg_state.clone()
        a, b = rt.step(c), ms.step({0: c})[0]
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b), t
            assert torch.equal(rt._reg_state, ms.reg_state) and torch.equal(rt._inton_eff, ms.inton_eff)
    assert float(rt._inton_eff[0]) > 1.0 and int(rt._centre_on[0]) == 1 and float(rt._reg_state[0, 2]) > 0
    # the bf16 repeat starts from the state the tick started from: the same tick again gives the same samples and the same state
    monkeypatch.setattr(MS.ops, "switch_to_bf16", lambda *a: None)
    after = ms.reg_state.clone()
    assert not torch.equal(after, saved[1])
    lo, ln = ms._span(CHUNK)
    again = ms._repeat_on_bf16(saved[0], saved[1])
    assert np.array_equal(again[0, lo:lo + ln], b) and torch.equal(ms.reg_state, after)
    data = audio_io.pcm16_to_float(torch.from_numpy(np.concatenate(rt.ring)).to(DEV)).unsqueeze(0)
    again = rt._repeat_on_bf16(data, saved[2], saved_reg=saved[3])
    assert np.array_equal(again[lo:lo + ln], a) and torch.equal(rt._reg_state, after)
    rt.reset()
    assert rt._reg_state.abs().sum().item() == 0.0
    # interior reuse is off with an intonation: "auto" resolves to off where it would otherwise be on, True raises
    geo = dict(chunk=960, buffersize=26, k=4)
    assert RealtimeConverter(*_nets(), lib, "cuda", **geo).reuse and not RealtimeConverter(*_nets(), lib, "cuda", intonation=0.5, **geo).reuse
    with pytest.raises(ValueError, match="interior reuse cannot be combined with intonation"):
        RealtimeConverter(*_nets(), lib, "cuda", intonation=1.5, reuse_interior=True, **geo)
    plain = RealtimeConverter(*_nets(), lib, "cuda", intonation=1.0, **kw)
    assert not plain.pitch_range and not hasattr(plain, "_reg_state")       # without it the converter is what it was


def test_a_gated_realtime_converter_with_intonation_is_the_gated_one_slot_converter(pool):
    """-thr with -int: the follower learns from open ticks only, as a gated session of a pitch_range converter does.  The input is loud,
    silent over ticks 14 to 21, loud again: with no hold the gate closes a tick into the silence and the state stands still until it
    reopens"""
    from module.realtime import RealtimeConverter
    ticks, quiet = BS + 22, range(14, 22)
    pcm = _pcm(CHUNK * ticks, 83).copy()
    pcm[quiet[0] * CHUNK:(quiet[-1] + 1) * CHUNK] = 0
    lib = pool.tokens("v0")[None]
    kw = dict(chunk=CHUNK, buffersize=BS, k=4)
    rt = RealtimeConverter(*_nets(), lib, "cuda", f0_rate=0.9, intonation=1.5, gate_db=-40, gate_hold=0.0, **kw)
    ms = MS.MultiStreamConverter(*_nets(), pool, 1, pitch_range=True, gate=True, **kw)
    ms.open(0, "v0", f0_rate=0.9, intonation=1.5, gate_db=-40, gate_hold=0.0)
    states, opens = [], []
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b = rt.step(c), ms.step({0: c})[0]
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b), t
            assert torch.equal(rt._reg_state, ms.reg_state) and torch.equal(rt._inton_eff, ms.inton_eff), t
            assert rt.gate_open() == ms.gate_open()[0]
            states.append(rt._reg_state.clone())
            opens.append(rt.gate_open())
    closed = [i for i, o in enumerate(opens) if not o]
    assert len(closed) >= 4 and opens[0] and opens[-1]                       # open, a closed stretch, open again
    still = [i for i in closed[2:]]                                          # (both ends of the chunk closed: the row does not follow)
    assert still and all(torch.equal(states[i], states[i - 1]) for i in still)
    assert not torch.equal(states[-1], states[closed[-1]]) and float(states[-1][0, 1]) > 0


# ---------------------------------------------------------------------------------------------------- 4. convert_many
MANY_CHUNK = 3200


@pytest.fixture(scope="module")
def rig():
    from module.pipeline import Converter
    conv = Converter(*_nets(), DEV)
    g = torch.Generator(device=DEV).manual_seed(43)
    tokens = {"a": torch.randn(1, 768, 600, device=DEV, generator=g), "b": synthetic.make_library(512, 5).to(DEV),
              "bare": synthetic.make_library(100, 6).to(DEV)}
    pa = float(PR.pitch(np.float32(900.0)))
    pool_ = MS.VoicePool(tokens, device=DEV, registers={"a": (pa * 4.0, 4.0, 4.0 * (pa * pa + 9.0))})
    pool_.set_register("b", hz=300.0, range_st=1.25)
    utts = [synthetic.make_waveform(n, 310 + i).to(DEV) for i, n in enumerate((2 * MANY_CHUNK, 3 * MANY_CHUNK + 700, MANY_CHUNK))]
    return conv, pool_, [u / u.abs().max() for u in utts]


def _raw_f0(conv, u):
    """the raw f0 of the utterance's windows, as convert_many's transform sees it"""
    from module.pipeline import make_windows
    from module.spectrogram import spectrogram
    windows, _ = make_windows(u.reshape(1, -1), MANY_CHUNK)
    return conv.pe.estimate(spectrogram(windows))


def test_convert_many_auto_range_utterance_is_bitwise_alone_and_in_a_corpus(rig):
    conv, pool_, utts = rig
    kw = dict(chunk=MANY_CHUNK, k=4, trim_context=True)
    assert abs(pool_.pitch_range("a") - 3.0) < 1e-9
    alone = conv.convert_many(utts[:1], pool_, ["a"], pitch_shift=0.5, intonation=1.2, auto_range=True, **kw)[0]
    corpus = conv.convert_many(utts, pool_, ["a", {"a": 1, "b": 3}, "bare"], pitch_shift=[0.5, -1.0, 2.0], alpha=[0.0, 0.1, 0.0],
                               intonation=[1.2, 0.9, 1.1], auto_pitch=[False, True, False], auto_range=[True, True, False], **kw)
    assert alone.shape == (1, 2 * MANY_CHUNK) and torch.equal(alone, corpus[0])
    mid = conv.convert_many(utts[1:2], pool_, [{"a": 1, "b": 3}], pitch_shift=-1.0, alpha=0.1, intonation=0.9, auto_pitch=True,
                            auto_range=True, **kw)[0]
    assert torch.equal(mid, corpus[1])
    off = conv.convert_many([utts[2]], pool_, ["bare"], pitch_shift=2.0, intonation=1.1, **kw)[0]
    assert torch.equal(off, corpus[2])                                       # a plain utterance beside auto-range ones: as alone
    plain = conv.convert_many(utts[:1], pool_, ["a"], pitch_shift=0.5, intonation=1.2, **kw)[0]
    assert not torch.equal(plain, alone)                                     # auto range is at work
    with pytest.raises(ValueError, match="voice 'bare' has no pitch range"):
        conv.convert_many(utts[:1], pool_, [{"a": 1, "bare": 1}], auto_range=True, **kw)
    with pytest.raises(ValueError, match="auto_range: expected bools"):
        conv.convert_many(utts[:1], pool_, ["a"], auto_range=1, **kw)
    with pytest.raises(ValueError, match="auto_range: 2 values for 1 utterances"):
        conv.convert_many(utts[:1], pool_, ["a"], auto_range=[True, False], **kw)
    with pytest.raises(ValueError, match="convert_many: pitch_range_max=0.5 must be a finite number >= 1"):
        conv.convert_many(utts[:1], pool_, ["a"], auto_range=True, pitch_range_max=0.5, **kw)


@pytest.mark.parametrize("trim", [True, False])
def test_convert_many_with_auto_range_off_is_the_present_path(rig, trim):
    conv, pool_, utts = rig
    kw = dict(pitch_shift=[0.5, -1.0, 2.0], intonation=[1.0, 1.3, 0.8], auto_pitch=[False, True, False], chunk=MANY_CHUNK, k=4,
              trim_context=trim)
    voices = ["a", "b", "bare"]
    today = conv.convert_many(utts, pool_, voices, **kw)
    off = conv.convert_many(utts, pool_, voices, auto_range=[False] * 3, **kw)
    assert all(torch.equal(a, b) for a, b in zip(today, off))
    on = conv.convert_many(utts, pool_, voices, auto_range=[False, True, False], **kw)
    assert torch.equal(on[0], today[0]) and torch.equal(on[2], today[2]) and not torch.equal(on[1], today[1])


def test_a_voice_declared_at_the_utterances_own_moments_gives_r_one_around_the_utterances_mean(rig):
    """the voice's (sum, count, sumsq) are the utterance's own over its windows' centre thirds: the target sd is sqrt of the very
    variance the kernel forms, so r = sd / sqrt(v) is exactly 1, the intonation comes back bit for bit and the centre is the mean.
    The f0 then differs from the plain path's only in the centre -- the utterance's mean instead of each window's: c + (p - c) against
    m_w + (p - m_w), a few float32 roundings at magnitude <= 64 (4e-6 semitones each), inside the streaming bar of 1e-5 relative."""
    conv, pool_, utts = rig
    f0 = _raw_f0(conv, utts[1])
    n = f0.shape[0]
    first = _i32([0, n])
    stats = MS.pitch_stats2_groups(f0, first, MANY_CHUNK // 320, 2 * MANY_CHUNK // 320)
    s, c, q = stats[0].tolist()
    m, v = RR.mean_var(s, c, q)
    assert c > 0 and v > 0
    was = pool_.registers["a"], pool_.ranges["a"]
    try:
        pool_.set_register("a", register=(s, c, q))
        assert pool_.register("a") == float(m) and pool_.pitch_range("a") == float(np.sqrt(v))
        sd = pool_.blend_range(*MS.blend_spec("a"))
        it, centre, on = MS.pitch_range_groups(stats, first, n, _f32([1.0]), _i32([1]), _f64([sd]), 2.0)
        assert it.tolist() == [1.0] * n and on.tolist() == [1] * n and centre.tolist() == [float(np.float32(m))] * n
        it, _, _ = MS.pitch_range_groups(stats, first, n, _f32([0.7]), _i32([1]), _f64([sd]), 2.0)
        assert np.all(_bits(it.cpu().numpy()) == _bits(np.float32(0.7)))
        kw = dict(chunk=MANY_CHUNK, k=4, trim_context=True)
        auto = conv.convert_many(utts[1:2], pool_, ["a"], pitch_shift=-1.5, auto_pitch=True, auto_range=True, **kw)[0]
    finally:
        pool_.set_register("a", register=was[0] + (was[1],))
    assert auto.shape == (1, 3 * MANY_CHUNK + 700) and bool(torch.isfinite(auto).all())
    # the two transforms on the utterance's raw f0, as transform() composes them: auto pitch's shift is -1.5 + (m - m) = -1.5
    rate, shift = _f32([1.0] * n), _f32([-1.5] * n)
    it, centre, on = MS.pitch_range_groups(stats, first, n, _f32([1.0]), _i32([1]), _f64([sd]), 2.0)
    got = MS.pitch_transform_rows_centred_(f0.clone(), 0, rate, shift, it, centre, on).cpu().numpy()
    plain = MS.pitch_transform_rows_(f0.clone(), 0, rate, shift, _f32([1.0] * n)).cpu().numpy()
    vo = plain > 0
    rel = np.abs(got[vo] - plain[vo]) / plain[vo]
    print(f"own moments: mean {m:+.4f} sd {np.sqrt(v):.4f}, {int(vo.sum())} voiced frames, max relative f0 difference {rel.max():.2e}")
    assert vo.sum() > 20 and np.array_equal(got > 0, vo) and np.all(rel <= 1e-5)


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


def _pcm_of(path):
    g, sr = audio_io.load(str(path))
    assert sr == 16000
    return np.round(g[0].numpy() * 32768).astype(np.int16)


def test_multistream_cli_without_the_keys_writes_the_plain_converters_bytes_and_with_them_the_range_converters(tmp_path):
    import multistream_inference as msi
    d, ticks = tmp_path, BS + 4
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(300, 5)}, d / "voice_library.pt")
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), torch.from_numpy(_pcm(CHUNK * ticks, 90 + i).astype(np.float32) / 32767)[None], 16000)
    sessions = [dict(input="in0.wav", lib="voice_library.pt", pitch=1.0), dict(input="in1.wav", lib="voice_library.pt", f0_rate=0.9)]
    json.dump(sessions, open(d / "sessions.json", "w"))
    geo = ["-c", str(CHUNK), "-b", str(BS)]
    msi.main(nets + geo + ["-o", str(d / "out"), str(d / "sessions.json")])
    ss = msi.load_sessions(str(d / "sessions.json"))
    CE, PE, Dec = _loaded_nets(d)
    pool = MS.VoicePool()
    name = msi.voice_name(None, str(d / "voice_library.pt"))
    pool.add(name, msi.voice_tokens(CE, None, str(d / "voice_library.pt"), DEV))
    pcms = [msi.input_pcm(s["input"], 16000, DEV) for s in ss]
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, 2, chunk=CHUNK, buffersize=BS, k=4)
    want = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, pitch=1.0), dict(voice=name, f0_rate=0.9)])
    plain = [_pcm_of(d / "out" / f"{i}_in{i}.wav") for i in range(2)]
    assert all(len(w) == CHUNK * (ticks - BS) and np.array_equal(g, w) for g, w in zip(plain, want))
    # the keys on one session, the flag as the other's default switched off by its own key: the range converter's bytes
    sessions[0].update(intonation=1.5, auto_range=True, register_hz=180, range_st=2.5)
    sessions[1].update(intonation=1)
    json.dump(sessions, open(d / "sessions2.json", "w"))
    msi.main(nets + geo + ["-int", "0.5", "-o", str(d / "out2"), str(d / "sessions2.json")])
    pool.set_register(name, hz=180.0, range_st=2.5)
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, 2, chunk=CHUNK, buffersize=BS, k=4, pitch_range=True)
    want = msi.run(conv, pcms, [0, 0], CHUNK, [dict(voice=name, pitch=1.0, intonation=1.5, auto_range=True), dict(voice=name, f0_rate=0.9)])
    got = [_pcm_of(d / "out2" / f"{i}_in{i}.wav") for i in range(2)]
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(got[1], plain[1]) and not np.array_equal(got[0], plain[0])


def test_batch_cli_without_the_keys_writes_the_plain_paths_bytes_and_with_them_auto_ranges(tmp_path):
    import batch_inference as BI
    from module.pipeline import Converter
    d = tmp_path
    nets = _save_nets(d)
    lib = synthetic.make_library(512, 5)
    torch.save({"tokens": lib}, d / "voice_library.pt")
    wav = synthetic.make_waveform(16000, 91) * 0.5                   # 1 s mono at 16 kHz
    audio_io.save(str(d / "utt.wav"), wav, 16000)
    jobs = [dict(input="utt.wav", lib="voice_library.pt", pitch=1.0, intonation=1.2, output="plain.wav"),
            dict(input="utt.wav", lib="voice_library.pt", pitch=1.0, intonation=1.2, auto_range=True, register_hz=200, range_st=1.5,
                 output="ranged.wav")]
    (d / "jobs0.json").write_text(json.dumps(jobs[:1]))
    BI.main([str(d / "jobs0.json"), "-c", "4800"] + nets)
    plain = audio_io.load(str(d / "plain.wav"))[0]
    CE, PE, Dec = _loaded_nets(d)
    wf = audio_io.load(str(d / "utt.wav"))[0].to(DEV)
    wf = (wf / wf.abs().max()).mean(dim=0, keepdim=True)
    pool = MS.VoicePool({"l": lib.to(DEV)[0]}, device=DEV)
    conv = Converter(CE, PE, Dec, DEV)
    kw = dict(pitch_shift=[1.0], intonation=[1.2], f0_rate=[1.0], alpha=[0.0], world_pitch=[False], chunk=4800, k=4, window_batch=64,
              trim_context=True)
    many = conv.convert_many([wf], pool, ["l"], auto_pitch=False, **kw)
    assert torch.equal(plain, audio_io.resample(many[0], 16000, 16000, post_gain_db=1.0).cpu())
    (d / "jobs.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs.json"), "-c", "4800"] + nets)
    assert torch.equal(audio_io.load(str(d / "plain.wav"))[0], plain)        # beside an auto-range job: the same bytes
    pool.set_register("l", hz=200.0, range_st=1.5)
    many = conv.convert_many([wf], pool, ["l"], auto_range=[True], **kw)
    ranged = audio_io.load(str(d / "ranged.wav"))[0]
    assert torch.equal(ranged, audio_io.resample(many[0], 16000, 16000, post_gain_db=1.0).cpu()) and not torch.equal(ranged, plain)
