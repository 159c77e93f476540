"""Voice blending (alive_knn_blend_gather_rows, MultiStreamConverter(blend=...), Converter.convert_many with blends): the kernel
against a NumPy float32 mirror of its formula, the streaming and batch paths against their single-voice forms, against themselves
(independence of sessions and utterances, no re-capture) and against the blended CPU oracle, and the two CLIs' "blend" key."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import alive_oracle as O                                             # noqa: E402
from module import audio_io, schema, synthetic                       # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _sds():
    return tuple(synthetic.make_state_dict(s, 2, p) for s, p in ((schema.content_encoder_schema(), "ce."),
                                                                (schema.f0_estimator_schema(), "pe."),
                                                                (schema.decoder_schema(), "dec.")))


def _pcm(n, seed, scale=12000):
    return (synthetic.make_waveform(n, seed)[0].numpy() * scale).astype(np.int16)


def _blended_oracle(monkeypatch):
    """O.match_features with a blend [(tokens, weight), ...] as the reference: (1 - a) sum_s w_s match(feat, tgt_s, k, 0) + a feat"""
    plain = O.match_features

    def match(source, reference, k=4, alpha=0.0, return_indices=False):
        if not isinstance(reference, list):
            return plain(source, reference, k, alpha, return_indices)
        b = sum(w * plain(source, t, k, 0.0) for t, w in reference)
        return b * (1 - alpha) + source * alpha
    monkeypatch.setattr(O, "match_features", match)


# ---------------------------------------------------------------------------------------------------- 1. the kernel
def _mirror(idx, first, weight, alpha, rows, src):
    """NumPy float32 restatement of alive_knn_blend_gather_rows (include/alive_vc.h), every product and sum rounded on its own"""
    N, D, T = src.shape
    k = idx.shape[1]
    out = src.copy()
    for n in range(N):
        a = float(alpha[n])
        am, om = np.float32(a), np.float32(1.0 - a)
        b = np.zeros((T, D), np.float32)
        act = np.zeros(T, bool)
        for r in range(first[n], min(first[n + 1], first[n] + 4)):
            lst = idx[r * T:(r + 1) * T]                               # [T, k]
            on = lst[:, 0] >= 0
            acc = rows[np.where(on, lst[:, 0], 0)]
            for j in range(1, k):
                acc = acc + rows[np.where(on, lst[:, j], 0)]
            c = np.float32(weight[r]) * (acc / np.float32(k))
            b = np.where((on & act)[:, None], b + c, np.where(on[:, None], c, b))
            act |= on
        mixed = b * om + src[n].T * am
        out[n] = np.where(act[:, None], mixed, src[n].T).T
    return out


def _case(N, T, k, max_lists, seed, P=3000):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_lists + 1, size=N)
    if N > 2:
        counts[0], counts[1] = 0, min(3, max_lists)                   # a row with no list; a row with an inactive middle list
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    R = int(first[-1])
    idx = rng.integers(0, P, size=(max(R, 1) * T, k)).astype(np.int32)
    off = rng.random(max(R, 1) * T) < 0.2                              # inactive lists on some frames
    idx[off] = -1
    if N > 2 and counts[1] == 3:
        r = first[1] + 1
        idx[r * T:(r + 1) * T] = -1
    weight = rng.uniform(0.05, 3.0, size=max(R, 1))
    for n in range(N):                                                 # normalised per row, as blend_spec does
        s = slice(first[n], first[n + 1])
        if counts[n]:
            weight[s] = weight[s] / weight[s].sum()
    alpha = rng.choice([0.0, 0.3, 1.0], size=N)
    rows = rng.standard_normal((P, 768)).astype(np.float32)
    src = rng.standard_normal((N, 768, T)).astype(np.float32)
    return idx, first, weight, alpha, rows, src


def _run(idx, first, weight, alpha, rows, src):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)       # noqa: E731
    k = idx.shape[1]
    val = torch.zeros(idx.shape, dtype=torch.float32, device=DEV)
    out = MS.blend_gather_rows(val, t(idx, torch.int32), k, t(first, torch.int32), t(weight, torch.float64),
                               t(alpha, torch.float64), t(rows, torch.float32), t(src, torch.float32))
    return out.cpu().numpy()


@pytest.mark.parametrize("N,T,k,lists", [(6, 33, k, 4) for k in range(1, 9)] + [(80, 31, k, 4) for k in range(1, 9)] +
                         [(5, 1, 4, 4), (5, 32, 4, 4), (3, 450, 4, 4), (9, 450, 4, 4), (7, 31, 3, 2), (1024, 1, 3, 4), (1024, 2, 8, 4),
                          (2, 64, 5, 1)])
def test_blend_gather_is_bitwise_its_numpy_mirror(N, T, k, lists):
    """k = 1 .. 8, 0 .. 4 lists per row, inactive lists and rows without one, alpha 0 / 0.3 / 1, uneven weights, T = 1 .. 450,
    both grid forms (one block per 32 frames walking the 12 slabs, or 12 slab blocks when there are few frames), N up to 1024"""
    case = _case(N, T, k, lists, seed=1000 * k + N + T)
    got = _run(*case)
    want = _mirror(*case)
    assert np.array_equal(got, want), np.abs(got - want).max()


@pytest.mark.parametrize("k", range(1, 9))
def test_one_list_at_weight_one_is_bitwise_merge_gather_rows(k):
    _, _, _, alpha, rows, src = _case(5, 40, k, 1, seed=k)
    idx = np.random.default_rng(k).integers(0, rows.shape[0], size=(5 * 40, k)).astype(np.int32)
    idx[7] = -1                                                       # an inactive frame passes its source through
    first = np.arange(6, dtype=np.int32)
    got = _run(idx, first, np.ones(5), alpha, rows, src)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)       # noqa: E731
    want = MS.merge_gather_rows(torch.zeros(idx.shape, device=DEV), t(idx, torch.int32), k, t(alpha, torch.float64),
                                t(rows, torch.float32), t(src, torch.float32)).cpu().numpy()
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- 2.-5. streaming
CHUNK, BS = 160, 16


def _pool(n=5, sizes=(300, 1000, 2000, 5000, 700)):
    voices = {f"v{i}": synthetic.make_library(sizes[i % len(sizes)], 20 + i) for i in range(n)}
    return voices, MS.VoicePool(voices)


def _drive(conv, sess, start, pcm, ticks, actions=None, chunk=CHUNK):
    outs = [[] for _ in sess]
    for tick in range(ticks):
        for s, p in enumerate(sess):
            if p is not None and tick == start[s]:
                conv.open(s, **p)
        for a in (actions or {}).get(tick, []):
            a(conv)
        feed = {s: pcm[s][(tick - start[s]) * chunk:(tick - start[s] + 1) * chunk] for s in range(len(sess))
                if sess[s] is not None and tick >= start[s]}
        for s, o in conv.step(feed).items():
            if o is not None:
                outs[s].append(o)
    return outs


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("graph", [False, True])
def test_blend_converter_with_single_voices_is_bitwise_blend_one(graph):
    B = 16
    _, pool = _pool()
    sess = [dict(voice=f"v{s % 5}" if s % 3 else {f"v{s % 5}": 2.5}, pitch=float(s % 5 - 2), f0_rate=0.5 + 0.1 * (s % 3),
                 alpha=0.1 * (s % 4)) for s in range(B)]
    start = [s % 4 for s in range(B)]
    ticks = max(start) + BS + 5
    pcm = [_pcm(CHUNK * ticks, 100 + s) for s in range(B)]
    outs = []
    for blend in (1, 3):
        conv = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, blend=blend)
        if graph:
            conv.enable_graph()
        outs.append(_drive(conv, sess, start, pcm, ticks))
    for s in range(B):
        assert len(outs[0][s]) == ticks - start[s] - BS and _same(outs[0][s], outs[1][s]), s


@pytest.mark.parametrize("graph", [False, True])
def test_one_slot_blend_converter(graph):
    """B = 1: a single voice in a blend=2 converter is bitwise blend=1; a blend runs and is the same eager and in a graph"""
    _, pool = _pool()
    ticks = BS + 4
    pcm = [_pcm(CHUNK * ticks, 77)]
    outs = []
    for blend, voice in ((1, "v1"), (2, "v1"), (2, {"v1": 1, "v3": 2})):
        conv = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=CHUNK, buffersize=BS, k=4, blend=blend)
        if graph:
            conv.enable_graph()
        outs.append(_drive(conv, [dict(voice=voice, pitch=1.0, alpha=0.1)], [0], pcm, ticks)[0])
    assert len(outs[0]) == ticks - BS and _same(outs[0], outs[1]) and not _same(outs[1], outs[2])
    eager = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=CHUNK, buffersize=BS, k=4, blend=2)
    assert _same(outs[2], _drive(eager, [dict(voice={"v1": 1, "v3": 2}, pitch=1.0, alpha=0.1)], [0], pcm, ticks)[0])


def _blend_sessions(B):
    sess = []
    for s in range(B):
        v = [f"v{s % 5}", f"v{(s + 1) % 5}", f"v{(s + 3) % 5}"]
        if s % 4 == 1:
            voice = {v[0]: 0.7, v[1]: 0.3}                             # two voices
        elif s % 4 == 2:
            voice = [(v[0], 1.0), (v[1], 2.0), (v[2], 0.5)]            # three voices, uneven
        elif s % 4 == 3:
            voice = [("v0", 1.0), ("v1", 1.0)]                         # the same pair in several sessions
        else:
            voice = v[0]
        sess.append(dict(voice=voice, pitch=float(s % 5 - 2), f0_rate=0.5 + 0.1 * (s % 3), alpha=0.3 if s == 6 else 0.0))
    return sess


def test_blended_sessions_match_the_blended_oracle_and_are_independent(monkeypatch):
    """16 sessions, some blending 2 or 3 voices: each within 1e-3 RMS of the blended realtime_step oracle, and each bitwise the
    same session alone (the only open slot) in a blend=3 converter.  (Alone means alone in a converter of the same slot count:
    the networks choose their kernels by the batch's column count, so a one-slot batch rounds differently from a 16-slot one.)"""
    ce, pe, dec = _sds()
    B = 16
    voices, pool = _pool()
    sess = _blend_sessions(B)
    start = [s % 5 for s in range(B)]
    ticks = max(start) + BS + 4
    pcm = [_pcm(CHUNK * ticks, 600 + s) for s in range(B)]
    conv = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, blend=3).enable_graph()
    got = _drive(conv, sess, start, pcm, ticks)
    assert conv.captures == 1
    alone = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, blend=3)
    for s in range(B):
        one = [None] * B
        one[s] = sess[s]
        for c in range(B):
            alone.close(c)
        assert _same(got[s], _drive(alone, one, start, pcm, ticks)[s]), s

    _blended_oracle(monkeypatch)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    begin, end = O.realtime_geometry(CHUNK, BS, 16000)
    c = BS * CHUNK // 2
    worst = 0.0
    for s in range(B):
        p = sess[s]
        names, weights = MS.blend_spec(p["voice"])
        tgt = voices[names[0]] if len(names) == 1 else [(voices[n], w) for n, w in zip(names, weights)]
        phi, want = 0, []
        for j in range(BS, ticks - start[s]):
            ring = torch.from_numpy(pcm[s][(j - BS + 1) * CHUNK:(j + 1) * CHUNK].astype(np.float32) / 32768)[None]
            wave, phi = O.realtime_step(ce, pe, dec, ring, tgt, phi, begin, end, k=4, alpha=p["alpha"], pitch_shift=p["pitch"],
                                        f0_rate=p["f0_rate"])
            want.append((wave[0].numpy() * 32768).astype(np.int16)[c - CHUNK // 2: c + CHUNK // 2])
        g = np.concatenate(got[s]).astype(np.float64)
        w = np.concatenate(want).astype(np.float64)
        assert g.shape == w.shape, s
        worst = max(worst, float(np.sqrt(np.mean((g - w) ** 2)) / 32768))
    assert worst < 1e-3, worst


def test_set_switches_blends_without_a_recapture():
    B = 4
    _, pool = _pool()
    ticks = BS + 14
    pcm = [_pcm(CHUNK * ticks, 900 + s) for s in range(B)]
    sess = [dict(voice="v0", pitch=1.0), dict(voice={"v1": 1, "v2": 1}), dict(voice="v3", alpha=0.3), dict(voice="v4")]
    acts = {BS + 2: [lambda c: c.set(0, voice={"v0": 3, "v1": 1, "v2": 1})],
            BS + 5: [lambda c: c.set(1, voice="v1"), lambda c: c.set(2, voice=[("v3", 1.0), ("v4", 4.0)])],
            BS + 8: [lambda c: c.set(0, voice={"v0": 1, "v1": 3, "v2": 1}), lambda c: c.set(1, voice=[("v2", 1), ("v0", 1)])],
            BS + 10: [lambda c: c.close(3), lambda c: c.open(3, {"v2": 1, "v3": 2, "v4": 3}, pitch=-2.0)],
            BS + 12: [lambda c: c.set(2, voice="v3")]}
    start = [0] * B
    graph = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, blend=3).enable_graph()
    g = _drive(graph, sess, start, pcm, ticks, acts)
    assert graph.captures == 1
    eager = MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, blend=3)
    e = _drive(eager, sess, start, pcm, ticks, acts)
    for s in range(B):
        assert len(g[s]) > 0 and _same(g[s], e[s]), s
    # the switches took effect: session 0 before / after its first switch differs from a run that never switched
    plain = _drive(MS.MultiStreamConverter(*_nets(), pool, B, chunk=CHUNK, buffersize=BS, k=4, blend=3).enable_graph(),
                   sess, start, pcm, ticks)
    assert _same(g[0][:2], plain[0][:2]) and not _same(g[0][2:], plain[0][2:])
    with pytest.raises(ValueError, match="at most 3"):
        graph.set(0, voice={"v0": 1, "v1": 1, "v2": 1, "v3": 1})
    with pytest.raises(ValueError, match="at most 1"):
        MS.MultiStreamConverter(*_nets(), pool, 2, chunk=CHUNK, buffersize=BS, k=4).open(0, {"v0": 1, "v1": 1})


@pytest.mark.parametrize("kind", ["rates", "world"])
def test_blended_session_stays_independent_with_rates_and_world(kind):
    B = 4
    _, pool = _pool()
    if kind == "rates":
        kw, rate, sr = dict(rates=[16000, 48000]), 48000, 16000
        chunk = CHUNK * rate // sr
        extra = dict(rate=rate)
    else:
        kw, chunk, extra = dict(world_pitch=True), 960, dict(world_pitch=True)
    bs = BS if kind == "rates" else 8
    ticks = bs + 5
    pcm = [_pcm(chunk * ticks, 950 + s) for s in range(B)]
    sess = [dict(voice={"v0": 2, "v2": 1}, pitch=1.0, **extra), dict(voice="v1"), dict(voice=[("v3", 1), ("v4", 1), ("v1", 2)]),
            dict(voice="v2", alpha=0.3)]
    conv_chunk = CHUNK if kind == "rates" else 960
    conv = MS.MultiStreamConverter(*_nets(), pool, B, chunk=conv_chunk, buffersize=bs, k=4, blend=3, **kw).enable_graph()
    chunks = [chunk] + [conv_chunk] * (B - 1)

    def drive(c, which):
        outs = [[] for _ in range(B)]
        for tick in range(ticks):
            if tick == 0:
                for s in which:
                    c.open(s, **sess[s])
            feed = {s: pcm[s][tick * chunks[s]:(tick + 1) * chunks[s]] for s in which}
            for s, o in c.step(feed).items():
                if o is not None:
                    outs[s].append(o)
        return outs
    got = drive(conv, range(B))
    alone = MS.MultiStreamConverter(*_nets(), pool, B, chunk=conv_chunk, buffersize=bs, k=4, blend=3, **kw).enable_graph()
    want = drive(alone, [0])
    assert len(got[0]) == ticks - bs and _same(got[0], want[0])
    assert len(got[0][0]) == (chunk if kind == "rates" else 960)


# ---------------------------------------------------------------------------------------------------- 6. convert_many
SECONDS = [1.0, 6.0, 3.5, 2.0, 4.25, 1.5]


@pytest.fixture(scope="module")
def rig():
    from module.pipeline import Converter
    conv = Converter(*_nets(), DEV)
    g = torch.Generator(device=DEV).manual_seed(41)
    tokens = {"a": torch.randn(1, 768, 3000, device=DEV, generator=g), "b": synthetic.make_library(512, 5).to(DEV),
              "c": synthetic.make_library(900, 6).to(DEV)}
    pool = MS.VoicePool(tokens, device=DEV)
    utts = [synthetic.make_waveform(int(s * 16000), 300 + i).to(DEV) for i, s in enumerate(SECONDS)]
    utts = [u / u.abs().max() for u in utts]
    return conv, pool, tokens, utts


VOICES = [{"a": 2, "b": 1}, "c", [("b", 1.0), ("c", 3.0), ("a", 0.5)], {"c": 1}, "a", [("a", 1), ("c", 1)]]
ALPHA = [0.0, 0.1, 0.3, 0.0, 0.2, 0.0]
PITCH = [0.0, 2.0, -3.0, 1.0, 0.5, -1.0]


def test_convert_many_blends_are_bitwise_each_utterance_alone(rig, monkeypatch):
    conv, pool, tokens, utts = rig
    monkeypatch.setenv("ALIVE_STREAMS", "3")
    kw = dict(chunk=16000, k=4, trim_context=True)
    outs = conv.convert_many(utts, pool, VOICES, pitch_shift=PITCH, alpha=ALPHA, window_batch=5, **kw)
    for i, u in enumerate(utts):
        alone = conv.convert_many([u], pool, [VOICES[i]], pitch_shift=PITCH[i], alpha=ALPHA[i], window_batch=64, **kw)[0]
        assert outs[i].shape == (1, u.shape[1]) and torch.equal(outs[i], alone), i
    # a one-component blend is its voice
    plain = conv.convert_many([utts[3]], pool, ["c"], pitch_shift=PITCH[3], alpha=ALPHA[3], **kw)[0]
    assert torch.equal(outs[3], plain)
    # the list rows searched in pieces: bitwise one call
    monkeypatch.setattr(MS, "POOL_PIECE_ROWS", 7)
    split = conv.convert_many(utts, pool, VOICES, pitch_shift=PITCH, alpha=ALPHA, window_batch=5, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, split))
    monkeypatch.setattr(MS, "POOL_PIECE_ROWS", 4096)
    monkeypatch.setattr(MS, "POOL_PIECE_FRAMES", 3 * 200)
    split = conv.convert_many(utts, pool, VOICES, pitch_shift=PITCH, alpha=ALPHA, window_batch=5, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, split))


def test_convert_many_blend_against_the_blended_oracle(rig, monkeypatch):
    conv, _, _, _ = rig
    a, b = synthetic.make_library(512, 5), synthetic.make_library(700, 9)
    pool = MS.VoicePool({"a": a.to(DEV), "b": b.to(DEV)}, device=DEV)
    wf = synthetic.make_waveform(16000, 91)
    wf = wf / wf.abs().max()
    out = conv.convert_many([wf.to(DEV)], pool, [{"a": 1.0, "b": 3.0}], pitch_shift=2.0, f0_rate=0.5, alpha=0.1, chunk=4800, k=4)[0]
    _blended_oracle(monkeypatch)
    cpu = _sds()
    ref = O.convert_utterance(cpu[0], cpu[1], cpu[2], wf, [(a, 0.25), (b, 0.75)], chunk=4800, k=4, alpha=0.1, pitch_shift=2.0,
                              f0_rate=0.5)
    err = (out.cpu() - ref).pow(2).mean().sqrt().item()
    assert err < 1e-3, err


# ---------------------------------------------------------------------------------------------------- 7. CLIs
def _save_nets(d):
    for name, sd in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _sds()):
        torch.save(sd, d / name)
    return ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]


def _loaded_nets(d):
    CE, PE, Dec = (net.to(DEV) for net in _nets())
    CE.load_state_dict(torch.load(d / "content_encoder.pt"))
    PE.load_state_dict(torch.load(d / "f0_estimator.pt"))
    Dec.load_state_dict(torch.load(d / "decoder.pt"))
    return CE, PE, Dec


def test_batch_cli_blend_job_writes_what_convert_many_makes(tmp_path):
    import batch_inference as BI
    from module.pipeline import Converter
    from module.spectrogram import spectrogram
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    audio_io.save(str(d / "target.wav"), synthetic.make_waveform(16000 * 3, 7) * 0.4, 16000)
    audio_io.save(str(d / "a.wav"), synthetic.make_waveform(16000 * 2, 91) * 0.5, 16000)
    jobs = [dict(input="a.wav", blend=[dict(target="target.wav", weight=1), dict(lib="voice_library.pt", weight=3)], pitch=1.0,
                 output="out_a.wav"),
            dict(input="a.wav", lib="voice_library.pt", output="out_b.wav")]
    (d / "jobs.json").write_text(json.dumps(jobs))
    BI.main([str(d / "jobs.json"), "-c", "16000"] + nets)
    CE, PE, Dec = _loaded_nets(d)
    wf = audio_io.load(str(d / "target.wav"))[0].to(DEV)
    wf = wf / wf.abs().max()                              # (a device max, as the CLI: a CPU scalar divides by its reciprocal)
    lib = torch.load(d / "voice_library.pt")["tokens"].to(DEV)
    pool = MS.VoicePool({"t": CE(spectrogram(wf[:1])), "l": lib}, device=DEV)
    u = audio_io.load(str(d / "a.wav"))[0].to(DEV)
    u = u / u.abs().max()
    conv = Converter(CE, PE, Dec, DEV)
    u = u.mean(dim=0, keepdim=True)
    want = conv.convert_many([u, u], pool, [[("t", 1), ("l", 3)], "l"], pitch_shift=[1.0, 0.0], chunk=16000, k=4,
                             trim_context=True)          # the whole jobs file, as the CLI runs it (one fp16 guard decision)
    for name, w in zip(("out_a.wav", "out_b.wav"), want):
        got, sr = audio_io.load(str(d / name))
        assert sr == 16000 and torch.equal(got, audio_io.resample(w, 16000, 16000, post_gain_db=1.0).cpu()), name


def test_multistream_cli_blend_session_writes_what_the_converter_emits(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    audio_io.save(str(d / "spk.wav"), synthetic.make_waveform(24000, 60) * 0.5, 24000)
    for i in range(2):
        audio_io.save(str(d / f"in{i}.wav"), synthetic.make_waveform(16000 + 3000 * i, 50 + i) * 0.5, 16000)
    sessions = [dict(input="in0.wav", blend=[dict(lib="voice_library.pt", weight=2), dict(target="spk.wav", weight=1)], pitch=2.0),
                dict(input="in1.wav", target="spk.wav", alpha=0.2, start=3)]
    json.dump(sessions, open(d / "sessions.json", "w"))
    msi.main(nets + ["-c", "320", "-b", "8", "-o", str(d / "out"), str(d / "sessions.json")])
    CE, PE, Dec = _loaded_nets(d)
    ss = msi.load_sessions(str(d / "sessions.json"))
    pool = MS.VoicePool()
    for target, lib in ((None, str(d / "voice_library.pt")), (str(d / "spk.wav"), None)):
        pool.add(msi.voice_name(target, lib), msi.voice_tokens(CE, target, lib, DEV))
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, 2, chunk=320, buffersize=8, k=4, blend=2)
    params = [dict(voice=msi.session_voice(s), pitch=s["pitch"], alpha=s["alpha"]) for s in ss]
    want = msi.run(conv, [msi.input_pcm(s["input"], 16000, DEV) for s in ss], [s["start"] for s in ss], 320, params)
    for p, w in zip((d / "out" / "0_in0.wav", d / "out" / "1_in1.wav"), want):
        got, sr = audio_io.load(str(p))
        assert sr == 16000 and len(w) > 0
        assert np.array_equal(np.round(got[0].numpy() * 32768).astype(np.int16), w), p
