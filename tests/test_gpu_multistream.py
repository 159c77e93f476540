"""Multi-session streaming (module/multistream.py): the grouped exact kNN search, the per-row edge kernels, and
MultiStreamConverter against RealtimeConverter, the CPU oracle and itself (independence of sessions, no re-capture)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import alive_oracle as O                                             # noqa: E402
from module import audio_io, ops, schema, synthetic                  # noqa: E402
from module import multistream as MS                                 # noqa: E402
from module.common import PackedLibrary, merge_gather               # noqa: E402

pytestmark = pytest.mark.gpu


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


# ---------------------------------------------------------------------------------------------------- 1. grouped search
def _pool_for_search():
    g = torch.Generator().manual_seed(7)
    sizes = (8, 100, 1000, 50000)
    voices = {}
    for i, m in enumerate(sizes):
        t = torch.randn(768, m, generator=g)
        if m >= 100:
            t[:, 50:60] = t[:, 10:20]                     # exact duplicates: ties, which go to the lower row
        voices[f"v{m}"] = t
    return voices, MS.VoicePool({n: t.cuda() for n, t in voices.items()})


@pytest.mark.parametrize("k", [1, 4, 8])
def test_grouped_search_is_bitwise_the_strict_search_per_segment(k):
    voices, pool = _pool_for_search()
    packed = {n: PackedLibrary(t.cuda(), strict=True) for n, t in voices.items()}
    # rows: several slots on one segment, every size, an inactive slot
    table = ["v50000", "v8", "v1000", None, "v50000", "v100", "v1000", "v50000"]
    lo = torch.tensor([pool.segment(n)[0] if n else 0 for n in table], dtype=torch.int32, device="cuda")
    ln = torch.tensor([pool.segment(n)[1] if n else 0 for n in table], dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(11 + k)
    for T in (8, 24, 48):
        src = torch.randn(len(table), 768, T, generator=g).cuda()
        src[1, :, 3] = 0.0                                # a zero-norm frame: val 0, the k lowest rows
        val, idx = MS.knn_search_grouped(src, pool.rows, pool.norms, lo, ln, k)
        val, idx = val.view(len(table), T, k), idx.view(len(table), T, k)
        for n, name in enumerate(table):
            if name is None:
                assert torch.all(idx[n] == -1) and torch.all(val[n] == -float("inf"))
                continue
            rv, ri = packed[name].search(src[n:n + 1].contiguous(), k)
            assert torch.equal(val[n], rv.view(T, k)), (name, T)
            assert torch.equal(idx[n] - pool.segment(name)[0], ri.view(T, k)), (name, T)
            # the top-k SET against an fp64 brute force where the k-th and (k+1)-th cosines are apart
            m = voices[name].shape[1]
            if m > k:
                rows = voices[name].double()
                q = src[n].double().cpu()
                cos = (rows / rows.norm(dim=0)).t() @ (q / q.norm(dim=0).clamp_min(1e-30))        # [M, T]
                top = torch.topk(cos, k + 1, dim=0)
                sep = (top.values[k - 1] - top.values[k]) > 1e-5
                for t in torch.nonzero(sep).flatten().tolist():
                    assert set(top.indices[:k, t].tolist()) == set((idx[n, t] - pool.segment(name)[0]).cpu().tolist())


def test_voice_pool_norms_are_those_of_packed_library():
    voices, pool = _pool_for_search()
    for name, t in voices.items():
        lo, m = pool.segment(name)
        p = PackedLibrary(t.cuda())
        assert torch.equal(pool.norms[lo:lo + m], p.norms) and torch.equal(pool.rows[lo:lo + m], p.rows)


# ---------------------------------------------------------------------------------------------------- 2. per-row edges
def test_per_row_edges_equal_the_scalar_entry_points():
    g = torch.Generator().manual_seed(3)
    N, T, k = 5, 24, 4
    lib = PackedLibrary(torch.randn(768, 700, generator=g).cuda())
    src = torch.randn(N, 768, T, generator=g).cuda()
    val, idx = lib.search(src, k)
    alphas = [0.0, 0.25, 0.5, 0.8, 1.0]
    same = MS.merge_gather_rows(val, idx, k, torch.full((N,), 0.3, dtype=torch.float64, device="cuda"), lib.rows, src)
    assert torch.equal(same, merge_gather(val, idx, 1, k, 0.3, lib.rows, src))
    rows_out = MS.merge_gather_rows(val, idx, k, torch.tensor(alphas, dtype=torch.float64, device="cuda"), lib.rows, src)
    for n, a in enumerate(alphas):
        s = src[n:n + 1].contiguous()
        want = merge_gather(val.view(N, T, k)[n].contiguous(), idx.view(N, T, k)[n].contiguous(), 1, k, a, lib.rows, s)
        assert torch.equal(rows_out[n:n + 1], want), a

    f0 = (torch.rand(N, 1, 40, generator=g) * 300 + 60).cuda()
    f0[:, :, 5] = 0.0
    rates, shifts, inton = [1.0, 0.5, 1.3, 2.0, 0.75], [0.0, -3.0, 2.5, 12.0, -7.25], [1.0, 0.5, 1.2, 1.0, 0.0]
    dev = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")
    for mode in (0, 1):
        got = MS.pitch_transform_rows_(f0.clone(), mode, dev([0.5] * N), dev([2.0] * N), dev([1.1] * N))
        assert torch.equal(got, ops.pitch_transform_(f0.clone(), mode, 0.5, 2.0, 1.1))
        got = MS.pitch_transform_rows_(f0.clone(), mode, dev(rates), dev(shifts), dev(inton))
        for n in range(N):
            assert torch.equal(got[n:n + 1], ops.pitch_transform_(f0[n:n + 1].clone(), mode, rates[n], shifts[n], inton[n]))

    x = torch.randn(N, 4800, generator=g).cuda() * 0.3
    pre_db, post_db = [0.0, 3.0, -2.0, 6.0, 0.0], [0.0, -1.5, 0.0, 2.0, 4.0]
    pre, post = dev([MS.db_scale(v) for v in pre_db]), dev([MS.db_scale(v) for v in post_db])
    for o, nw in ((16000, 16000), (24000, 16000), (16000, 24000), (44100, 16000)):
        got = MS.resample_rows(x, o, nw, dev([1.0] * N), dev([1.0] * N))
        assert torch.equal(got, audio_io.resample(x, o, nw))
        got = MS.resample_rows(x, o, nw, pre, post)
        for n in range(N):
            assert torch.equal(got[n:n + 1], audio_io.resample(x[n:n + 1], o, nw, pre_gain_db=pre_db[n], post_gain_db=post_db[n]))


# ---------------------------------------------------------------------------------------------------- 3. B = 1
@pytest.mark.parametrize("graph", [False, True])
def test_one_slot_is_bitwise_the_realtime_converter(graph):
    from module.realtime import RealtimeConverter
    chunk, bs, steps = 160, 16, 56
    lib = synthetic.make_library(1000, 1)
    kw = dict(chunk=chunk, buffersize=bs)
    rt = RealtimeConverter(*_nets(), lib, "cuda", f0_rate=0.5, pitch=1.5, alpha=0.2, k=4, reuse_interior=False, **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, **kw)
    ms.open(0, "lib", pitch=1.5, f0_rate=0.5, alpha=0.2)
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    pcm = _pcm(chunk * (bs + steps), 67, 20000)
    emitted = 0
    for s in range(bs + steps):
        c = pcm[s * chunk:(s + 1) * chunk]
        a, b = rt.step(c), ms.step({0: c})[0]
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b), s
            emitted += 1
    assert emitted == steps


# ---------------------------------------------------------------------------------------------------- 4. parity per session
def _parity(chunk, bs, sr, gains, ticks_after=4):
    """16 slots, 4 voices of different sizes, per-session pitch / f0 rate / alpha (and gains), staggered joins: every session's
    emitted stream against the oracle's realtime step driven with that session's ring, voice and parameters"""
    ce, pe, dec = _sds()
    B = 16
    voices = {f"v{i}": synthetic.make_library(m, 20 + i) for i, m in enumerate((300, 1000, 2000, 5000))}
    conv = MS.MultiStreamConverter(*_nets(), MS.VoicePool(voices), B, chunk=chunk, buffersize=bs, input_sr=sr, output_sr=sr, k=4)
    conv.enable_graph()
    sess = [dict(voice=f"v{s % 4}", pitch=float(s % 5 - 2), f0_rate=0.5 + 0.1 * (s % 3), alpha=0.1 * (s % 4),
                 gain=(-2.0 + 0.5 * (s % 3)) if gains else 0.0, input_gain=(3.0 - (s % 4)) if gains else 0.0) for s in range(B)]
    start = [s % 5 for s in range(B)]
    ticks = max(start) + bs + ticks_after
    pcm = [_pcm(chunk * ticks, 100 + s) for s in range(B)]
    outs = [[] for _ in range(B)]
    for tick in range(ticks):
        for s in range(B):
            if tick == start[s]:
                conv.open(s, **sess[s])
        res = conv.step({s: pcm[s][(tick - start[s]) * chunk:(tick - start[s] + 1) * chunk] for s in range(B) if tick >= start[s]})
        for s, o in res.items():
            if o is not None:
                outs[s].append(o)
    begin, end = O.realtime_geometry(chunk, bs, sr)
    c = bs * chunk // 2
    worst = 0.0
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for s in range(B):
        p, phi, want = sess[s], 0, []
        n = ticks - start[s]
        for j in range(bs, n):
            ring = torch.from_numpy(pcm[s][(j - bs + 1) * chunk:(j + 1) * chunk].astype(np.float32) / 32768)[None]
            x = O.gain(O.resample(ring, sr, 16000), p["input_gain"])
            wave, phi = O.realtime_step(ce, pe, dec, x, voices[p["voice"]], phi, begin, end, k=4, alpha=p["alpha"],
                                        pitch_shift=p["pitch"], f0_rate=p["f0_rate"])
            y = O.resample(O.gain(wave, p["gain"]), 16000, sr)[0]
            want.append((y.numpy() * 32768).astype(np.int16)[c - chunk // 2: c + chunk // 2])
        got = np.concatenate(outs[s]).astype(np.float64)
        want = np.concatenate(want).astype(np.float64)
        assert got.shape == want.shape == ((n - bs) * chunk,), s
        worst = max(worst, float(np.sqrt(np.mean((got - want) ** 2)) / 32768))
    return worst


def test_sixteen_sessions_match_the_oracle_each():
    rms = _parity(160, 16, 16000, gains=False)
    assert rms < 1e-3, rms


def test_sixteen_sessions_at_24khz_with_gains_match_the_oracle_each():
    rms = _parity(480, 12, 24000, gains=True)
    assert rms < 1e-3, rms


def test_sixteen_sessions_on_bf16_planes_match_the_oracle_each():
    env = dict(os.environ, ALIVE_ENCODER_PRECISION="2", ALIVE_DECODER_PRECISION="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "parity"], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "parity ok" in r.stdout


# ---------------------------------------------------------------------------------------------------- 5./6. independence, no re-capture
def _drive(conv, ticks, plan, chunk):
    """plan(tick) -> (actions, {slot: chunk}); actions: list of callables run on conv before the tick"""
    outs = {}
    for tick in range(ticks):
        actions, feed = plan(tick)
        for a in actions:
            a(conv)
        for s, o in conv.step(feed).items():
            if o is not None:
                outs.setdefault(s, []).append(o)
    return outs


def test_sessions_are_independent_and_the_graph_is_captured_once():
    chunk, bs, B = 160, 16, 16
    voices = {"a": synthetic.make_library(500, 31), "b": synthetic.make_library(2000, 32), "c": synthetic.make_library(900, 33)}
    pool = MS.VoicePool(voices)
    mine = _pcm(chunk * 80, 77)
    other = [_pcm(chunk * 80, 200 + s) for s in range(B)]
    other2 = [_pcm(chunk * 80, 400 + s) for s in range(B)]

    def scenario(variant, join=0):
        def plan(tick):
            acts, feed = [], {}
            if tick == 0:
                acts += [lambda c, s=s: c.close(s) for s in range(B)]           # (a converter driven before starts empty)
                for s in range(B):
                    if s == 3:
                        continue
                    if variant == 1 and s in (5, 6):
                        continue                               # closed slots
                    v = ("a", "b", "c")[s % 3] if variant == 0 else ("c", "a", "b")[s % 3]
                    acts.append(lambda c, s=s, v=v: c.open(s, v, pitch=float(s % 3) if variant == 0 else -4.0, alpha=0.1))
            if tick == join:
                acts.append(lambda c: c.open(3, "b", pitch=2.0, f0_rate=0.75, alpha=0.3))
            if variant == 1 and tick == 20:
                acts += [lambda c: c.set(7, voice="b", pitch=5.0), lambda c: c.close(8), lambda c: c.open(5, "a")]
            src = other if variant == 0 else other2
            for s in range(B):
                if s == 3 and tick >= join:
                    feed[3] = mine[(tick - join) * chunk:(tick - join + 1) * chunk]
                elif s != 3 and not (variant == 1 and (s == 6 or (s == 5 and tick < 20) or (s == 8 and tick >= 20))):
                    feed[s] = src[s][tick * chunk:(tick + 1) * chunk]
            return acts, feed
        return plan

    ticks = 40 + bs + 12
    g = MS.MultiStreamConverter(*_nets(), pool, B, chunk=chunk, buffersize=bs, k=4).enable_graph()
    base = _drive(g, ticks, scenario(0), chunk)[3]
    g2 = MS.MultiStreamConverter(*_nets(), pool, B, chunk=chunk, buffersize=bs, k=4).enable_graph()
    changed = _drive(g2, ticks, scenario(1), chunk)
    assert g2.captures == 1                                  # set / open / close between replays: no re-capture
    assert len(changed[3]) == len(base) and all(np.array_equal(a, b) for a, b in zip(base, changed[3]))
    late = _drive(g2, ticks, scenario(0, join=40), chunk)[3]
    assert g2.captures == 1
    assert len(late) == ticks - 40 - bs
    assert all(np.array_equal(a, b) for a, b in zip(base, late))
    eager = MS.MultiStreamConverter(*_nets(), pool, B, chunk=chunk, buffersize=bs, k=4)
    want = _drive(eager, ticks, scenario(1), chunk)
    assert sorted(want) == sorted(changed)
    for s in want:
        assert len(want[s]) == len(changed[s]) and all(np.array_equal(a, b) for a, b in zip(want[s], changed[s])), s


# ---------------------------------------------------------------------------------------------------- 7. errors
def test_session_errors_raise_value_error():
    pool = MS.VoicePool({"tiny": synthetic.make_library(3, 1), "ok": synthetic.make_library(100, 2)})
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=160, buffersize=16, k=4)
    with pytest.raises(ValueError, match="fewer than k"):
        conv.open(0, "tiny")
    with pytest.raises(ValueError, match="unknown voice"):
        conv.open(0, "nobody")
    with pytest.raises(ValueError, match="out of range"):
        conv.open(2, "ok")
    conv.open(0, "ok").open(1, "ok")
    with pytest.raises(ValueError, match="supplied no chunk"):
        conv.step({0: np.zeros(160, np.int16)})
    with pytest.raises(ValueError, match="out of range"):
        conv.step({0: np.zeros(160, np.int16), 1: np.zeros(160, np.int16), 5: np.zeros(160, np.int16)})
    with pytest.raises(ValueError, match="k=9"):
        MS.MultiStreamConverter(*_nets(), pool, 2, chunk=160, buffersize=16, k=9)


# ---------------------------------------------------------------------------------------------------- 8. CLI
def test_multistream_cli_writes_what_the_converter_emits(tmp_path):
    import json
    import multistream_inference as msi
    d = tmp_path
    ce, pe, dec = _sds()
    for name, sd in (("content_encoder.pt", ce), ("f0_estimator.pt", pe), ("decoder.pt", dec)):
        torch.save(sd, d / name)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    for i in range(3):
        audio_io.save(str(d / f"in{i}.wav"), synthetic.make_waveform(16000 + 3000 * i, 50 + i) * 0.5, 16000)
    audio_io.save(str(d / "spk.wav"), synthetic.make_waveform(24000, 60) * 0.5, 24000)
    sessions = [dict(input="in0.wav", lib="voice_library.pt", pitch=2.0),
                dict(input="in1.wav", target="spk.wav", f0_rate=0.5, alpha=0.2, start=7),
                dict(input="in2.wav", target="spk.wav", lib="voice_library.pt", gain=-3.0, input_gain=2.0, start=3,
                     output="third.wav")]
    json.dump(sessions, open(d / "sessions.json", "w"))
    args = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt"),
            "-c", "320", "-b", "8", "-o", str(d / "out"), str(d / "sessions.json")]
    msi.main(args)
    # the same sessions through the converter directly
    CE, PE, Dec = (net.to("cuda") for net in _nets())
    CE.load_state_dict(ce)
    PE.load_state_dict(pe)
    Dec.load_state_dict(dec)
    ss = msi.load_sessions(str(d / "sessions.json"))
    pool, names = MS.VoicePool(), []
    for s in ss:
        name = json.dumps([s["target"], s["lib"]])
        if name not in pool.segments:
            pool.add(name, msi.voice_tokens(CE, s["target"], s["lib"], torch.device("cuda")))
        names.append(name)
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, 3, chunk=320, buffersize=8, k=4)
    params = [dict(voice=n, pitch=s["pitch"], f0_rate=s["f0_rate"], alpha=s["alpha"], gain=s["gain"], input_gain=s["input_gain"])
              for n, s in zip(names, ss)]
    want = msi.run(conv, [msi.input_pcm(s["input"], 16000, "cuda") for s in ss], [s["start"] for s in ss], 320, params)
    paths = [d / "out" / "0_in0.wav", d / "out" / "1_in1.wav", d / "third.wav"]
    for p, w in zip(paths, want):
        got, sr = audio_io.load(str(p))
        assert sr == 16000 and len(w) > 0
        assert np.array_equal(np.round(got[0].numpy() * 32768).astype(np.int16), w), p


if __name__ == "__main__" and sys.argv[1:] == ["parity"]:
    assert ops.encoder_precision(0) == 2 and ops.decoder_precision(0) == 2
    rms = _parity(160, 16, 16000, gains=True)
    assert rms < 1e-3, rms
    print("parity ok", rms)
