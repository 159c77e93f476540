"""Per-session sample rates in multi-session streaming: the per-row multi-rate resampler (alive_resample_rows_multi) bitwise
against the single-pair resampler row by row, and MultiStreamConverter(rates=...) against RealtimeConverter, single-rate
converters, the CPU oracle and the CLI."""
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
from module import _native as nat                                    # noqa: E402
from module import audio_io, schema, synthetic                       # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu

RATES = (8000, 16000, 24000, 44100, 48000)
PAIRS = [(r, 16000) for r in RATES] + [(16000, r) for r in RATES]


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


def _dev(v, dtype=torch.int32):
    return torch.tensor(v, dtype=dtype, device="cuda")


# ---------------------------------------------------------------------------------------------------- 1. the kernel
GUARD = 4096
SENTINEL = 12345.0


def _launch(x, len_in, pair, rt, len_out, ld_out, pre, post):
    """alive_resample_rows_multi into a sentinel-filled buffer with a guard band after y -> (y [B, ld_out], guard band)"""
    B = x.shape[0]
    buf = torch.full((B * ld_out + GUARD,), SENTINEL, device="cuda")
    nat.check(nat.lib().alive_resample_rows_multi(nat.ptr(x), B, x.shape[1], nat.ptr(len_in), nat.ptr(pair), nat.ptr(rt.table),
                                                  len(rt.entries), nat.ptr(rt.filt), rt.filt_len, rt.lds_bytes, nat.ptr(pre),
                                                  nat.ptr(post), buf.data_ptr(), ld_out, nat.ptr(len_out), nat.stream()),
              "alive_resample_rows_multi")
    return buf[:B * ld_out].view(B, ld_out), buf[B * ld_out:]


def _row_reference(x, lin, lout, o, n, pre, post):
    """the row alone through resample_rows at its pair and gains, cut to lout"""
    row = x[None, :lin].contiguous()
    got = MS.resample_rows(row, o, n, _dev([pre], torch.float32), _dev([post], torch.float32))
    return got[0, :lout]


def _rows_case(B, seed, ld_in=7056):
    g = np.random.default_rng(seed)
    L_ = nat.lib()
    pair_of = [PAIRS[i % len(PAIRS)] for i in range(B)]
    g.shuffle(pair_of)
    lin, lout = [], []
    for i, (o, n) in enumerate(pair_of):
        if i % 7 == 3:
            m = int(g.integers(1, 12))                               # shorter than the filter (2 width + orig taps)
        else:
            m = int(g.integers(ld_in // 2, ld_in + 1))
        full = int(L_.alive_resample_length(m, *audio_io._reduced(o, n)))
        lin.append(m)
        lout.append(full if i % 3 else int(g.integers(1, full + 1)))    # the whole resampled row, or a shorter cut
    pre = [float(MS.db_scale(v)) for v in g.uniform(-6, 6, B)]
    post = [float(MS.db_scale(v)) for v in g.uniform(-6, 6, B)]
    pre[0] = post[0] = 1.0
    x = torch.from_numpy(g.standard_normal((B, ld_in)).astype(np.float32) * 0.3).cuda()
    return pair_of, lin, lout, pre, post, x


def _check_rows(y, guard, x, pair_of, lin, lout, pre, post, rows):
    assert torch.all(guard == SENTINEL), "the guard band after y was written"
    for b in rows:
        o, n = pair_of[b]
        want = _row_reference(x[b], lin[b], lout[b], o, n, pre[b], post[b])
        assert torch.equal(y[b, :lout[b]], want), (b, pair_of[b], lin[b], lout[b])
        assert torch.all(y[b, lout[b]:] == 0.0), (b, "padding")


def test_multi_rate_rows_are_bitwise_the_single_pair_resampler():
    """one launch, 40 rows at 8, 16, 24, 44.1 and 48 kHz into and out of 16 kHz with random gains, rows shorter than their
    filter, the 44.1 kHz banks in global memory beside LDS-staged banks: each row equals resample_rows of that row alone, the
    padding is 0 and a guard band after y is untouched"""
    rt = MS.RateTable(PAIRS)
    big = [(o, n) for o, n, w, _ in rt.entries if o != n and n * (2 * w + o) * 4 > 16 * 1024]
    small = [(o, n) for o, n, w, _ in rt.entries if o != n and n * (2 * w + o) * 4 <= 16 * 1024]
    assert big and small and 0 < rt.lds_bytes <= 16 * 1024
    B = 40
    pair_of, lin, lout, pre, post, x = _rows_case(B, 5)
    ld_out = max(lout) + 37
    y, guard = _launch(x, _dev(lin), _dev([rt.pair(o, n) for o, n in pair_of]), rt, _dev(lout), ld_out,
                       _dev(pre, torch.float32), _dev(post, torch.float32))
    torch.cuda.synchronize()
    _check_rows(y, guard, x, pair_of, lin, lout, pre, post, range(B))
    # unit gains and whole rows: audio_io.resample itself
    for b in range(B):
        o, n = pair_of[b]
        if pre[b] == post[b] == 1.0 and o != n:
            want = audio_io.resample(x[b:b + 1, :lin[b]], o, n)[0, :lout[b]]
            assert torch.equal(y[b, :lout[b]], want)


def test_multi_rate_rows_at_1024_rows():
    """B = 1024 (the largest batch), every pair: a sample of 96 rows, the first and last included, against resample_rows"""
    rt = MS.RateTable(PAIRS)
    B = 1024
    pair_of, lin, lout, pre, post, x = _rows_case(B, 9, ld_in=2560)
    ld_out = max(lout)
    y, guard = _launch(x, _dev(lin), _dev([rt.pair(o, n) for o, n in pair_of]), rt, _dev(lout), ld_out,
                       _dev(pre, torch.float32), _dev(post, torch.float32))
    torch.cuda.synchronize()
    rows = sorted({0, B - 1} | set(np.random.default_rng(1).choice(B, 94, replace=False).tolist()))
    _check_rows(y, guard, x, pair_of, lin, lout, pre, post, rows)


def test_multi_rate_rows_in_a_graph_with_pairs_rewritten_between_replays():
    """one captured launch replayed over three pair assignments (and their lengths) written into the same device arrays"""
    rt = MS.RateTable(PAIRS)
    B, ld_in = 24, 2560
    g = np.random.default_rng(3)
    x = torch.from_numpy(g.standard_normal((B, ld_in)).astype(np.float32) * 0.3).cuda()
    pre = _dev([float(MS.db_scale(v)) for v in g.uniform(-4, 4, B)], torch.float32)
    post = _dev([float(MS.db_scale(v)) for v in g.uniform(-4, 4, B)], torch.float32)
    L_ = nat.lib()
    ld_out = max(int(L_.alive_resample_length(ld_in, *audio_io._reduced(o, n))) for o, n in PAIRS)
    pair, len_in, len_out = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    y = torch.empty(B, ld_out, device="cuda")

    def assign(pairs):
        lin = [ld_in - 7 * (b % 5) for b in range(B)]
        lout = [int(L_.alive_resample_length(m, *audio_io._reduced(o, n))) for m, (o, n) in zip(lin, pairs)]
        pair.copy_(_dev([rt.pair(o, n) for o, n in pairs]))
        len_in.copy_(_dev(lin))
        len_out.copy_(_dev(lout))
        return lin, lout

    def launch():
        nat.check(L_.alive_resample_rows_multi(nat.ptr(x), B, ld_in, nat.ptr(len_in), nat.ptr(pair), nat.ptr(rt.table),
                                               len(rt.entries), nat.ptr(rt.filt), rt.filt_len, rt.lds_bytes, nat.ptr(pre),
                                               nat.ptr(post), nat.ptr(y), ld_out, nat.ptr(len_out), nat.stream()),
                  "alive_resample_rows_multi")

    assign([PAIRS[0]] * B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for seed in range(3):
        pairs = [PAIRS[int(i)] for i in np.random.default_rng(40 + seed).integers(0, len(PAIRS), B)]
        lin, lout = assign(pairs)
        y.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        pv, qv = pre.tolist(), post.tolist()
        for b in range(B):
            o, n = pairs[b]
            assert torch.equal(y[b, :lout[b]], _row_reference(x[b], lin[b], lout[b], o, n, pv[b], qv[b])), (seed, b, pairs[b])
            assert torch.all(y[b, lout[b]:] == 0.0), (seed, b)


# ---------------------------------------------------------------------------------------------------- 2. one slot
@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("graph", [False, True])
def test_one_slot_at_its_own_rate_is_bitwise_the_realtime_converter(rate, graph):
    """a one-slot 16 kHz converter with its session at 48 / 44.1 kHz emits what RealtimeConverter at that rate emits"""
    from module.realtime import RealtimeConverter
    chunk, bs, steps = 160, 16, 40
    cr = chunk * rate // 16000
    lib = synthetic.make_library(1000, 1)
    rt = RealtimeConverter(*_nets(), lib, "cuda", chunk=cr, buffersize=bs, input_sr=rate, output_sr=rate, f0_rate=0.5, pitch=1.5,
                           alpha=0.2, gain=-2.0, input_gain=3.0, k=4, reuse_interior=False)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, chunk=chunk, buffersize=bs, k=4, rates=[rate])
    ms.open(0, "lib", pitch=1.5, f0_rate=0.5, alpha=0.2, gain=-2.0, input_gain=3.0, rate=rate)
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    pcm = _pcm(cr * (bs + steps), 67, 20000)
    emitted = 0
    for s in range(bs + steps):
        c = pcm[s * cr:(s + 1) * cr]
        a, b = rt.step(c), ms.step({0: c})[0]
        assert (a is None) == (b is None)
        if a is not None:
            assert len(b) == 2 * (cr // 2)
            assert np.array_equal(a, b), s
            emitted += 1
    assert emitted == steps


# ---------------------------------------------------------------------------------------------------- 3. mixed batch
def _drive_sessions(conv, sess, start, pcm, chunks, ticks):
    outs = [[] for _ in sess]
    for tick in range(ticks):
        for s, p in enumerate(sess):
            if tick == start[s]:
                conv.open(s, **p)
        feed = {s: pcm[s][(tick - start[s]) * chunks[s]:(tick - start[s] + 1) * chunks[s]] for s in range(len(sess))
                if tick >= start[s]}
        for s, o in conv.step(feed).items():
            if o is not None:
                outs[s].append(o)
    return outs


def test_mixed_rate_batch_matches_single_rate_converters_and_the_oracle():
    """B = 16 at -c 160 -b 16, sessions over five rates with their own voices, pitches, gains and staggered joins: each session
    is bitwise the same session in a 16-slot converter whose slots all run at its rate, and matches the oracle's realtime step at
    its rate (< 1e-3 RMS of full scale)"""
    ce, pe, dec = _sds()
    chunk, bs, B = 160, 16, 16
    voices = {f"v{i}": synthetic.make_library(m, 20 + i) for i, m in enumerate((300, 1000, 2000, 5000))}
    pool = MS.VoicePool(voices)
    rate = [RATES[s % len(RATES)] for s in range(B)]
    cr = [chunk * r // 16000 for r in rate]
    sess = [dict(voice=f"v{s % 4}", pitch=float(s % 5 - 2), f0_rate=0.5 + 0.1 * (s % 3), alpha=0.1 * (s % 4),
                 gain=-2.0 + 0.5 * (s % 3), input_gain=3.0 - (s % 4)) for s in range(B)]
    start = [s % 5 for s in range(B)]
    ticks = max(start) + bs + 4
    pcm = {(s, r): _pcm(chunk * r // 16000 * ticks, 100 + s) for s in range(B) for r in RATES}

    conv = MS.MultiStreamConverter(*_nets(), pool, B, chunk=chunk, buffersize=bs, k=4, rates=RATES).enable_graph()
    mixed = _drive_sessions(conv, [dict(p, rate=r) for p, r in zip(sess, rate)], start, [pcm[s, rate[s]] for s in range(B)],
                            cr, ticks)
    assert conv.captures == 1
    for r in RATES:
        c = chunk * r // 16000
        single = MS.MultiStreamConverter(*_nets(), pool, B, chunk=c, buffersize=bs, input_sr=r, output_sr=r, k=4).enable_graph()
        want = _drive_sessions(single, sess, start, [pcm[s, r] for s in range(B)], [c] * B, ticks)
        for s in range(B):
            if rate[s] == r:
                assert len(mixed[s]) == len(want[s]) == ticks - start[s] - bs, (s, r)
                assert all(np.array_equal(a, b) for a, b in zip(mixed[s], want[s])), (s, r)

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    worst = 0.0
    for s in range(B):
        p, r, c = sess[s], rate[s], cr[s]
        begin, end = O.realtime_geometry(c, bs, r)
        centre = bs * c // 2
        phi, want = 0, []
        for j in range(bs, ticks - start[s]):
            ring = torch.from_numpy(pcm[s, r][(j - bs + 1) * c:(j + 1) * c].astype(np.float32) / 32768)[None]
            x = O.gain(O.resample(ring, r, 16000), p["input_gain"])
            wave, phi = O.realtime_step(ce, pe, dec, x, voices[p["voice"]], phi, begin, end, k=4, alpha=p["alpha"],
                                        pitch_shift=p["pitch"], f0_rate=p["f0_rate"])
            y = O.resample(O.gain(wave, p["gain"]), 16000, r)[0]
            want.append((y.numpy() * 32768).astype(np.int16)[centre - c // 2: centre + c // 2])
        got = np.concatenate(mixed[s]).astype(np.float64)
        want = np.concatenate(want).astype(np.float64)
        assert got.shape == want.shape, s
        worst = max(worst, float(np.sqrt(np.mean((got - want) ** 2)) / 32768))
    assert worst < 1e-3, worst


# ---------------------------------------------------------------------------------------------------- 4. one capture
def test_sessions_reopen_at_other_rates_without_a_new_capture():
    """sessions open, close and reopen at different rates over 36 ticks: one capture, and every emitted chunk is the length of
    its session's chunk (one less when it is odd), bitwise what an eager converter emits"""
    chunk, bs, B = 160, 16, 4
    pool = MS.VoicePool({"a": synthetic.make_library(400, 3), "b": synthetic.make_library(900, 4)})
    src = {(s, r): _pcm(chunk * r // 16000 * 40, 500 + s) for s in range(B) for r in RATES}
    plan = {0: [(0, 48000), (1, 8000), (2, 16000)], 6: [(3, 44100)], 12: [(1, None), (1, 44100)], 20: [(0, None), (2, None),
                                                                                                        (0, 24000)],
            27: [(2, 8000), (3, None), (3, 16000)]}

    def drive(conv):
        state, outs = {}, []
        for tick in range(36):
            for s, r in plan.get(tick, []):
                if r is None:
                    conv.close(s)
                    state.pop(s)
                else:
                    conv.open(s, "ab"[s % 2], pitch=float(s), rate=r)
                    state[s] = (r, tick)
            feed = {}
            for s, (r, t0) in state.items():
                c = chunk * r // 16000
                feed[s] = src[s, r][(tick - t0) * c:(tick - t0 + 1) * c]
            res = conv.step(feed)
            for s, o in res.items():
                if o is not None:
                    c = chunk * state[s][0] // 16000
                    assert len(o) == 2 * (c // 2), (tick, s)
                    outs.append((tick, s, o))
        return outs

    g = MS.MultiStreamConverter(*_nets(), pool, B, chunk=chunk, buffersize=bs, k=4, rates=RATES).enable_graph()
    got = drive(g)
    assert g.captures == 1
    want = drive(MS.MultiStreamConverter(*_nets(), pool, B, chunk=chunk, buffersize=bs, k=4, rates=RATES))
    assert len(got) == len(want) > 20
    assert all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(got, want))
    assert {s for _, s, _ in got} == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------- 5. errors
def test_rate_errors_raise_value_error():
    """an undeclared rate, a non-integer session chunk, rates with input_sr != output_sr, a chunk of the converter's length from
    a 48 kHz session, set(rate=...)"""
    pool = MS.VoicePool({"ok": synthetic.make_library(100, 2)})
    conv = MS.MultiStreamConverter(*_nets(), pool, 2, chunk=160, buffersize=16, k=4, rates=[16000, 48000])
    with pytest.raises(ValueError, match="was not declared"):
        conv.open(0, "ok", rate=44100)
    assert not conv.is_open[0]
    with pytest.raises(ValueError, match="220.5 samples"):
        MS.MultiStreamConverter(*_nets(), pool, 2, chunk=160, buffersize=16, k=4, rates=[22050])
    with pytest.raises(ValueError, match="input_sr == output_sr"):
        MS.MultiStreamConverter(*_nets(), pool, 2, chunk=160, buffersize=16, input_sr=16000, output_sr=48000, k=4,
                                rates=[16000, 48000])
    conv.open(0, "ok", rate=48000).open(1, "ok")
    with pytest.raises(ValueError, match="expected 480"):
        conv.step({0: np.zeros(160, np.int16), 1: np.zeros(160, np.int16)})
    with pytest.raises(ValueError, match="rate is fixed"):
        conv.set(0, rate=16000)
    single = MS.MultiStreamConverter(*_nets(), pool, 1, chunk=160, buffersize=16, k=4)
    with pytest.raises(ValueError, match="was not declared"):
        single.open(0, "ok", rate=48000)


# ---------------------------------------------------------------------------------------------------- 6. CLI
def test_cli_sessions_at_two_rates_write_what_the_converter_emits(tmp_path):
    """a sessions file with 48 kHz and 8 kHz sessions (and one at -isr): wavs at those rates, bitwise the converter's output"""
    import multistream_inference as msi
    d = tmp_path
    ce, pe, dec = _sds()
    for name, sd in (("content_encoder.pt", ce), ("f0_estimator.pt", pe), ("decoder.pt", dec)):
        torch.save(sd, d / name)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    for i in range(3):
        audio_io.save(str(d / f"in{i}.wav"), synthetic.make_waveform(16000 + 3000 * i, 50 + i) * 0.5, 16000)
    sessions = [dict(input="in0.wav", lib="voice_library.pt", pitch=2.0, sr=48000),
                dict(input="in1.wav", lib="voice_library.pt", f0_rate=0.5, start=4, sr=8000),
                dict(input="in2.wav", lib="voice_library.pt", gain=-3.0, start=2)]
    json.dump(sessions, open(d / "sessions.json", "w"))
    args = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt"),
            "-c", "320", "-b", "8", "-o", str(d / "out"), str(d / "sessions.json")]
    msi.main(args)
    CE, PE, Dec = (net.to("cuda") for net in _nets())
    CE.load_state_dict(ce)
    PE.load_state_dict(pe)
    Dec.load_state_dict(dec)
    ss = msi.load_sessions(str(d / "sessions.json"))
    pool = MS.VoicePool({"v": msi.voice_tokens(CE, None, ss[0]["lib"], torch.device("cuda"))})
    rates = [48000, 8000, 16000]
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, 3, chunk=320, buffersize=8, k=4, rates=rates)
    params = [dict(voice="v", pitch=s["pitch"], f0_rate=s["f0_rate"], alpha=s["alpha"], gain=s["gain"], input_gain=s["input_gain"],
                   rate=r) for s, r in zip(ss, rates)]
    want = msi.run(conv, [msi.input_pcm(s["input"], r, "cuda") for s, r in zip(ss, rates)], [s["start"] for s in ss],
                   [320 * r // 16000 for r in rates], params)
    for i, (name, r) in enumerate(zip(("in0", "in1", "in2"), rates)):
        got, sr = audio_io.load(str(d / "out" / f"{i}_{name}.wav"))
        assert sr == r and len(want[i]) > 0
        assert np.array_equal(np.round(got[0].numpy() * 32768).astype(np.int16), want[i]), name
