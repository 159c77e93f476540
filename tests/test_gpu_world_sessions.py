"""WORLD pitch per session and per job: the row-masked WORLD call (alive_world_f0_rows) against the unmasked one, in a graph whose
mask changes between replays; MultiStreamConverter(world_pitch=True) against RealtimeConverter(world_pitch=True), the CPU oracle
with the restatement's f0, itself without toggles and a world_pitch=False converter; convert_many with a mixed world_pitch list
against convert(world_pitch=...); and the world_pitch keys of both CLIs."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alive_oracle as O
from module import audio_io, ops, schema, synthetic
from module import multistream as MS
from module.common import PackedLibrary, compute_f0, compute_f0_rows, world_f0, world_f0_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "alive-vc_amd"))
import world_ref as W   # noqa: E402

DEV = "cuda"
CHUNK, BS = 960, 8                       # a 480-ms ring: WORLD is voiced inside it


def voices16(n, L, seed):
    """n rows at 16 kHz: harmonic voices with vibrato, two-voice sums, noise, zero-padded tails, voiced / silent alternation"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / 16000.0
    rows = []
    for i in range(n):
        kind = i % 5
        if kind == 3:
            rows.append(0.1 * rs.randn(L))
            continue
        x = np.zeros(L)
        for _ in range(2 if kind == 1 else 1):
            f0 = rs.uniform(70, 400)
            f = f0 * (1 + 0.04 * np.sin(2 * np.pi * rs.uniform(3, 7) * t))
            ph = 2 * np.pi * np.cumsum(f) / 16000.0
            x += sum(0.3 / k * np.sin(k * ph + rs.uniform(0, 6.28)) for k in range(1, 9))
        if kind == 2:
            x[rs.randint(L // 4, 3 * L // 4):] = 0.0
        if kind == 4:
            x *= np.abs(np.sin(2 * np.pi * 1.3 * t))
        rows.append(x)
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def voiced_pcm(n, seed, scale=20000):
    """one harmonic voice (kind 0 of voices16) as int16"""
    return (voices16(1, n, seed)[0].numpy() * 0.8 * scale).astype(np.int16)


def restated_f0(wf16_dev):
    """compute_f0 with the restatement's DIO + StoneMask on the device-resampled signal, torch's CPU interpolation"""
    l = wf16_dev.shape[1]
    x8 = audio_io.resample(wf16_dev, 16000, 8000).cpu().numpy()
    f0 = torch.from_numpy(W.dio_stonemask_rows(x8, 8000))[:, None]
    return F.interpolate(F.interpolate(f0, x8.shape[1] // 256, mode="linear"), l // 320, mode="linear")


def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _sds():
    return tuple(synthetic.make_state_dict(s, 2, p) for s, p in ((schema.content_encoder_schema(), "ce."),
                                                                (schema.f0_estimator_schema(), "pe."),
                                                                (schema.decoder_schema(), "dec.")))


def _masks(n):
    return {"all": [1] * n, "none": [0] * n, "alternating": [(r + 1) % 2 for r in range(n)], "one": [int(r == n // 2) for r in range(n)]}


# ---------------------------------------------------------------------------------------------------- 1. the masked call
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("L16", [7680, 144000])
def test_masked_rows_are_bitwise_the_unmasked_call_and_off_rows_zero(n, L16):
    x8 = audio_io.resample(voices16(n, L16, seed=n + L16).to(DEV), 16000, 8000).contiguous()
    full = world_f0(x8)
    assert full.any() or L16 < 144000
    for name, m in _masks(n).items():
        mask = torch.tensor(m, dtype=torch.int32, device=DEV)
        got = world_f0_rows(x8, mask)
        assert got.shape == full.shape
        for r in range(n):
            if m[r]:
                assert torch.equal(got[r], full[r]), (name, r)
            else:
                assert not got[r].any(), (name, r)
        on = [r for r in range(n) if m[r]]
        for r in on[:1] + on[-1:]:                       # alone: a one-row call
            assert torch.equal(world_f0(x8[r:r + 1].contiguous())[0], got[r]), (name, r)
    # compute_f0_rows (resample, masked call, resizes) against compute_f0
    wf = voices16(n, L16, seed=3).to(DEV)
    want = compute_f0(wf)
    m = _masks(n)["alternating"]
    got = compute_f0_rows(wf, torch.tensor(m, dtype=torch.int32, device=DEV))
    assert got.shape == want.shape == (n, 1, L16 // 320)
    for r in range(n):
        assert torch.equal(got[r], want[r]) if m[r] else not got[r].any()


@pytest.mark.parametrize("n,L16", [(5, 7680), (64, 144000)])
def test_masked_call_in_a_graph_follows_the_mask_between_replays(n, L16):
    wf = voices16(n, L16, seed=17).to(DEV)
    mask = torch.ones(n, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        compute_f0_rows(wf, mask)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = compute_f0_rows(wf, mask)
    full = compute_f0(wf)
    for name in ("alternating", "none", "one", "all", "alternating"):
        m = _masks(n)[name]
        mask.copy_(torch.tensor(m, dtype=torch.int32, device=DEV))
        g.replay()
        torch.cuda.synchronize()
        want = full * torch.tensor(m, dtype=torch.float32, device=DEV).view(n, 1, 1)
        assert torch.equal(out, want), name
        assert torch.equal(out, compute_f0_rows(wf, mask)), name


# ---------------------------------------------------------------------------------------------------- 2. B = 1
@pytest.mark.parametrize("graph", [False, True])
def test_one_world_slot_is_bitwise_the_realtime_converter(graph):
    from module.realtime import RealtimeConverter
    steps = 30
    lib = synthetic.make_library(1000, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    rt = RealtimeConverter(*_nets(), lib, DEV, f0_rate=0.5, pitch=1.5, alpha=0.2, k=4, world_pitch=True, **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, world_pitch=True, **kw)
    ms.open(0, "lib", pitch=1.5, f0_rate=0.5, alpha=0.2, world_pitch=True)      # f0_rate 0.5: not applied, as RealtimeConverter
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    pcm = voiced_pcm(CHUNK * (BS + steps), 67)
    emitted, voiced = 0, 0
    for s in range(BS + steps):
        c = pcm[s * CHUNK:(s + 1) * CHUNK]
        a, b = rt.step(c), ms.step({0: c})[0]
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b), s
            voiced += int(bool(ms.last_f0.any()))
            emitted += 1
    assert emitted == steps and voiced > 0
    assert ms.captures == (1 if graph else 0)


# ---------------------------------------------------------------------------------------------------- 3. parity per session
def _world_parity(rates):
    ce, pe, dec = _sds()
    B = 16
    voices = {f"v{i}": synthetic.make_library(m, 20 + i) for i, m in enumerate((300, 1000, 2000, 5000))}
    conv = MS.MultiStreamConverter(*_nets(), MS.VoicePool(voices), B, chunk=CHUNK, buffersize=BS, k=4, rates=rates,
                                   world_pitch=True)
    conv.enable_graph()
    rate = [rates[s % len(rates)] if rates else 16000 for s in range(B)]
    cr = [CHUNK * r // 16000 for r in rate]
    sess = [dict(voice=f"v{s % 4}", pitch=float(s % 5 - 2), f0_rate=0.5 + 0.1 * (s % 3), alpha=0.1 * (s % 4),
                 gain=-2.0 + 0.5 * (s % 3), input_gain=3.0 - (s % 4), world_pitch=s % 2 == 0) for s in range(B)]
    start = [s % 5 for s in range(B)]
    ticks = max(start) + BS + 3
    pcm = [voiced_pcm(cr[s] * ticks, 100 + s, 12000) if s % 4 != 3 else
           (synthetic.make_waveform(cr[s] * ticks, 100 + s)[0].numpy() * 12000).astype(np.int16) for s in range(B)]
    outs = [[] for _ in range(B)]
    for tick in range(ticks):
        for s in range(B):
            if tick == start[s]:
                conv.open(s, **(dict(sess[s], rate=rate[s]) if rates else sess[s]))
        feed = {s: pcm[s][(tick - start[s]) * cr[s]:(tick - start[s] + 1) * cr[s]] for s in range(B) if tick >= start[s]}
        for s, o in conv.step(feed).items():
            if o is not None:
                outs[s].append(o)
    assert conv.captures == 1
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    worst, voiced = 0.0, 0
    for s in range(B):
        p, r, c = sess[s], rate[s], cr[s]
        begin, end = O.realtime_geometry(c, BS, r)
        centre = BS * c // 2
        phi, want = 0, []
        for j in range(BS, ticks - start[s]):
            ring = torch.from_numpy(pcm[s][(j - BS + 1) * c:(j + 1) * c].astype(np.float32) / 32768)[None]
            x = O.gain(O.resample(ring, r, 16000), p["input_gain"])
            if p["world_pitch"]:
                f0 = restated_f0(x.contiguous().to(DEV))
                voiced += int(bool((f0 > 0).any()))
                f0 = O.pitch_transform_realtime(f0, p["pitch"])              # f0_rate is not applied to WORLD's f0
                content = O.match_features(O.content_encoder(ce, O.spectrogram(x)), voices[p["voice"]], k=4, alpha=p["alpha"])
                wave, phi_out = O.decoder(dec, content, f0, phi=phi, crop0=begin)
                phi = phi_out[:, :, end].unsqueeze(2)
            else:
                wave, phi = O.realtime_step(ce, pe, dec, x, voices[p["voice"]], phi, begin, end, k=4, alpha=p["alpha"],
                                            pitch_shift=p["pitch"], f0_rate=p["f0_rate"])
            y = O.resample(O.gain(wave, p["gain"]), 16000, r)[0]
            want.append((y.numpy() * 32768).astype(np.int16)[centre - c // 2: centre + c // 2])
        got = np.concatenate(outs[s]).astype(np.float64)
        want = np.concatenate(want).astype(np.float64)
        assert got.shape == want.shape == ((ticks - start[s] - BS) * (2 * (c // 2)),), s
        worst = max(worst, float(np.sqrt(np.mean((got - want) ** 2)) / 32768))
    assert voiced > 0
    return worst


def test_sixteen_sessions_half_on_world_match_the_oracle_each():
    rms = _world_parity(None)
    assert rms < 1e-3, rms


def test_sixteen_sessions_half_on_world_at_four_rates_match_the_oracle_each():
    rms = _world_parity([8000, 16000, 44100, 48000])
    assert rms < 1e-3, rms


# ---------------------------------------------------------------------------------------------------- 4. toggling
def _drive(conv, ticks, plan, pcm, check=None):
    outs = {}
    for tick in range(ticks):
        for a in plan.get(tick, []):
            a(conv)
        feed = {s: pcm[s][tick * CHUNK:(tick + 1) * CHUNK] for s in range(len(pcm)) if conv.is_open[s]}
        for s, o in conv.step(feed).items():
            if o is not None:
                outs.setdefault(s, []).append(o)
                if check:
                    check(conv, tick, s)
    return outs


def test_world_toggles_keep_one_capture_and_leave_other_sessions_alone():
    B, ticks = 6, BS + 16
    pool = MS.VoicePool({"a": synthetic.make_library(500, 31), "b": synthetic.make_library(900, 33)})
    pcm = [voiced_pcm(CHUNK * ticks, 300 + s) for s in range(B)]

    def opener(s, **kw):
        return lambda c: c.open(s, ("a", "b")[s % 2], pitch=float(s % 3) - 1.0, f0_rate=0.75, **kw)
    base_plan = {0: [opener(s) for s in (0, 1, 3, 5)]}
    toggles = {0: [opener(s) for s in (0, 1, 3, 5)] + [opener(2, world_pitch=True)],
               BS + 3: [lambda c: c.set(1, world_pitch=True)],
               BS + 7: [lambda c: c.set(1, world_pitch=False), lambda c: c.close(2), opener(4, world_pitch=True)],
               BS + 11: [lambda c: c.set(1, world_pitch=True, pitch=2.0), lambda c: c.set(5, world_pitch=True)]}
    world_from = {1: BS + 3, 5: BS + 11}
    world_checks = []

    def check(conv, tick, s):
        """a row on WORLD: last_f0 is the WORLD transform of its ring, from the tick it was switched on"""
        p = conv.params[s]
        if p is None or not p["world_pitch"]:
            return
        want = ops.pitch_transform_(compute_f0(conv._in[s:s + 1]).clone(), 1, f0_rate=1.0, pitch_shift=p["pitch"])
        assert torch.equal(conv.last_f0[s:s + 1], want), (tick, s)
        world_checks.append((tick, s))

    base = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, world_pitch=True).enable_graph()
    want = _drive(base, ticks, base_plan, pcm)
    conv = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, world_pitch=True).enable_graph()
    got = _drive(conv, ticks, toggles, pcm, check)
    assert conv.captures == 1 and base.captures == 1
    for s in (0, 3):                                            # untouched sessions: bitwise the run without toggles
        assert len(got[s]) == len(want[s]) == ticks - BS and all(np.array_equal(a, b) for a, b in zip(got[s], want[s])), s
    for s in (1, 5):                                            # before their switch: bitwise too; after it: WORLD's f0
        n = world_from[s] - BS
        assert all(np.array_equal(a, b) for a, b in zip(got[s][:n], want[s][:n])), s
        assert not all(np.array_equal(a, b) for a, b in zip(got[s][n:], want[s][n:])), s
    assert {(world_from[1], 1), (world_from[5], 5)} <= set(world_checks)
    assert {s for _, s in world_checks} == {1, 2, 4, 5}


# ---------------------------------------------------------------------------------------------------- 5. no WORLD session
@pytest.mark.parametrize("graph", [False, True])
def test_world_converter_without_world_sessions_is_bitwise_the_plain_one(graph):
    B, ticks = 4, BS + 6
    pool = MS.VoicePool({"a": synthetic.make_library(500, 31), "b": synthetic.make_library(900, 33)})
    pcm = [voiced_pcm(CHUNK * ticks, 500 + s) for s in range(B)]
    plan = {0: [lambda c, s=s: c.open(s, ("a", "b")[s % 2], pitch=float(s), f0_rate=0.5 + 0.25 * s, alpha=0.1) for s in range(B)]}
    outs = []
    for world in (False, True):
        conv = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, world_pitch=world)
        if graph:
            conv.enable_graph()
        outs.append(_drive(conv, ticks, plan, pcm))
    for s in range(B):
        assert len(outs[0][s]) == ticks - BS and all(np.array_equal(a, b) for a, b in zip(outs[0][s], outs[1][s])), s


# ---------------------------------------------------------------------------------------------------- 6. errors
def test_world_session_errors():
    pool = MS.VoicePool({"ok": synthetic.make_library(100, 2)})
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4)
    with pytest.raises(ValueError, match="world_pitch=True"):
        conv.open(0, "ok", world_pitch=True)
    assert not conv.is_open[0]
    conv.open(0, "ok")
    with pytest.raises(ValueError, match="world_pitch=True"):
        conv.set(0, world_pitch=True)
    assert conv.params[0]["world_pitch"] is False
    wconv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4, world_pitch=True)
    with pytest.raises(ValueError, match="bool"):
        wconv.open(0, "ok", world_pitch=1)
    wconv.open(0, "ok", world_pitch=True, f0_rate=0.5)
    assert wconv.world_on.tolist() == [1, 0] and wconv.f0_rate_eff.tolist() == [1.0, 1.0]
    wconv.set(0, world_pitch=False)
    assert wconv.world_on.tolist() == [0, 0] and wconv.f0_rate_eff.tolist() == [0.5, 1.0]
    wconv.set(0, world_pitch=True)
    wconv.close(0)
    assert wconv.world_on.tolist() == [0, 0] and not wconv._world_sel.any()


# ---------------------------------------------------------------------------------------------------- 7. convert_many
SECONDS = [2.0, 6.5, 3.0, 1.0, 4.0]
WORLD = [True, False, True, True, False]
VOICE_OF = ["shared", "lib512", "shared", "lib512", "shared"]
PITCH = [0.0, 2.0, -3.0, 5.5, 1.0]
INTON = [1.0, 0.8, 1.2, 1.0, 0.5]
RATE = [0.5, 1.0, 1.0, 2.0, 0.75]
ALPHA = [0.0, 0.1, 0.3, 0.0, 0.5]


@pytest.fixture(scope="module")
def rig():
    from module.pipeline import Converter
    conv = Converter(*_nets(), DEV)
    g = torch.Generator(device=DEV).manual_seed(41)
    tokens = {"shared": torch.randn(1, 768, 3000, device=DEV, generator=g), "lib512": synthetic.make_library(512, 5).to(DEV)}
    pool = MS.VoicePool(tokens, device=DEV)
    utts = [voices16(1, int(s * 16000), 300 + i).to(DEV) for i, s in enumerate(SECONDS)]
    utts = [u / u.abs().max() for u in utts]
    return conv, pool, tokens, utts


@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("streams", ["1", "3"])
def test_convert_many_mixed_world_is_bitwise_each_utterance_alone(rig, monkeypatch, trim, streams):
    conv, pool, tokens, utts = rig
    monkeypatch.setenv("ALIVE_STREAMS", streams)
    before = ops.Fp16Guard.fallbacks
    outs = conv.convert_many(utts, pool, VOICE_OF, pitch_shift=PITCH, intonation=INTON, f0_rate=RATE, alpha=ALPHA, chunk=48000,
                             k=4, window_batch=5, trim_context=trim, world_pitch=WORLD)     # batches span WORLD and estimator windows
    assert ops.Fp16Guard.fallbacks == before, "the fp16 guard repeated the batch: batch composition could matter"
    for i, u in enumerate(utts):
        conv.set_library(PackedLibrary(tokens[VOICE_OF[i]][0], strict=True))
        ref = conv.convert(u, chunk=48000, k=4, alpha=ALPHA[i], pitch_shift=PITCH[i], intonation=INTON[i], f0_rate=RATE[i],
                           trim_context=trim, world_pitch=WORLD[i])
        assert outs[i].shape == ref.shape == (1, u.shape[1])
        assert torch.equal(outs[i], ref), f"utterance {i} (world_pitch={WORLD[i]}) differs from its single conversion"
    # WORLD changed something: the same batch without it differs on the WORLD utterances only
    plain = conv.convert_many(utts, pool, VOICE_OF, pitch_shift=PITCH, intonation=INTON, f0_rate=RATE, alpha=ALPHA, chunk=48000,
                              k=4, window_batch=5, trim_context=trim)
    for i in range(len(utts)):
        assert torch.equal(plain[i], outs[i]) != WORLD[i], i


def test_convert_many_world_pitch_argument_errors(rig):
    conv, pool, tokens, utts = rig
    with pytest.raises(ValueError, match="world_pitch"):
        conv.convert_many(utts[:2], pool, ["shared", "shared"], world_pitch=[True])
    with pytest.raises(ValueError, match="world_pitch"):
        conv.convert_many(utts[:2], pool, ["shared", "shared"], world_pitch=[1, 0])
    outs = conv.convert_many(utts[3:4], pool, ["lib512"], world_pitch=True, window_batch=2)
    conv.set_library(PackedLibrary(tokens["lib512"][0], strict=True))
    assert torch.equal(outs[0], conv.convert(utts[3], world_pitch=True))


# ---------------------------------------------------------------------------------------------------- 8. CLIs
def _save_nets(d):
    for name, sd in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _sds()):
        torch.save(sd, d / name)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    return ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt"), "-d", "cuda"]


def test_batch_cli_world_job_is_bitwise_inference_wpe(tmp_path, monkeypatch):
    import batch_inference
    import inference
    d = tmp_path
    nets = _save_nets(d) + ["-c", "16000"]
    audio_io.save(str(d / "a.wav"), voices16(1, 24000 * 2, 91) * 0.5, 24000)
    audio_io.save(str(d / "b.wav"), voices16(1, 16000 * 3, 92) * 0.3, 16000)
    jobs = [dict(input="a.wav", lib="voice_library.pt", pitch=2.0, f0_rate=0.5, world_pitch=True, output="out/a.wav"),
            dict(input="b.wav", lib="voice_library.pt", pitch=-1.0, world_pitch=False, output="out/b.wav")]
    os.makedirs(d / "out")
    (d / "jobs.json").write_text(json.dumps(jobs))
    batch_inference.main([str(d / "jobs.json")] + nets)
    monkeypatch.setenv("ALIVE_KNN_STRICT", "0")
    for j, job in enumerate(jobs):
        ind = d / f"in{j}"
        os.makedirs(ind)
        shutil.copy(d / job["input"], ind / job["input"])
        flags = ["-p", str(job["pitch"]), "-f0", str(job.get("f0_rate", 1.0)), "-lib", str(d / job["lib"])]
        if job["world_pitch"]:
            flags += ["-wpe", "True"]
        inference.main(["-i", str(ind), "-o", str(d / f"ref{j}"), "--knn-strict"] + flags + nets)
        ref, sr_ref = audio_io.load(str(d / f"ref{j}" / f"0_{os.path.splitext(job['input'])[0]}.wav"))
        got, sr = audio_io.load(str(d / job["output"]))
        assert sr == sr_ref and got.shape == ref.shape
        assert torch.equal(got, ref), f"job {j} differs from inference.py --knn-strict"


def test_multistream_cli_world_session_writes_what_the_converter_emits(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), voices16(1, 16000 * 2 + 4000 * i, 50 + i) * 0.5, 16000)
    sessions = [dict(input="in0.wav", lib="voice_library.pt", pitch=2.0, f0_rate=0.5, world_pitch=True),
                dict(input="in1.wav", lib="voice_library.pt", f0_rate=0.5, start=3)]
    json.dump(sessions, open(d / "sessions.json", "w"))
    msi.main(nets + ["-c", str(CHUNK), "-b", str(BS), "-o", str(d / "out"), str(d / "sessions.json")])
    CE, PE, Dec = (net.to(DEV) for net in _nets())
    for net, sd in zip((CE, PE, Dec), _sds()):
        net.load_state_dict(sd)
    ss = msi.load_sessions(str(d / "sessions.json"))
    assert [s["world_pitch"] for s in ss] == [True, False]
    pool = MS.VoicePool()
    pool.add("v", msi.voice_tokens(CE, None, ss[0]["lib"], torch.device(DEV)))
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, 2, chunk=CHUNK, buffersize=BS, k=4, world_pitch=True)
    params = [dict(voice="v", pitch=s["pitch"], f0_rate=s["f0_rate"], world_pitch=s["world_pitch"]) for s in ss]
    want = msi.run(conv, [msi.input_pcm(s["input"], 16000, DEV) for s in ss], [s["start"] for s in ss], CHUNK, params)
    for p, w in zip([d / "out" / "0_in0.wav", d / "out" / "1_in1.wav"], want):
        got, sr = audio_io.load(str(p))
        assert sr == 16000 and len(w) > 0
        assert np.array_equal(np.round(got[0].numpy() * 32768).astype(np.int16), w), p
