"""Live enrolment on the device: alive_pool_append against alive_library_pack_rows, alive_pool_move_rows against a host copy, a
reserved VoicePool against a fresh default pool after every operation (rows, norms and the grouped search), running sessions
through add / extend / remove / compact against a converter over a default pool, enrol_voice against voice_tokens + add, the
multistream CLI with --pool-rows against the run without it, and convert_many on a reserved pool with a hole.  Every comparison
is bitwise: both sides run the same arithmetic on the same operands."""
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

from module import _native as nat                                    # noqa: E402
from module import audio_io, schema, synthetic                       # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64                   # guard rows on either side of the rows a call may write


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


def _randn(*shape, seed):
    return torch.randn(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _guarded_table(cap, seed=3):
    """rows[cap, 768] / norms[cap] where EVERY row is the direction u that every frame of the tests leans to (as the guard rows of
    test_gpu_multistream_limits.py): a row written or left outside its range would be every frame's best match"""
    u = _randn(768, seed=seed)
    return u[None, :].expand(cap, 768).contiguous(), torch.full((cap,), float(u.norm()), device=DEV), u


def _append(tok, rows, norms, at, report, cap=None):
    return nat.lib().alive_pool_append(tok.data_ptr(), tok.stride(0), tok.stride(1), tok.shape[1], tok.shape[0], nat.ptr(rows),
                                       nat.ptr(norms), rows.shape[0] if cap is None else cap, at, nat.ptr(report), nat.stream())


def _packed(tok):
    m = tok.shape[1]
    rows, norms = torch.empty(m, 768, device=DEV), torch.empty(m, device=DEV)
    nat.check(nat.lib().alive_library_pack_rows(nat.ptr(tok.contiguous()), m, 768, nat.ptr(rows), nat.ptr(norms), nat.stream()))
    return rows, norms


# ---------------------------------------------------------------------------------------------------- 1. alive_pool_append
def _views(m, seed):
    """the same [768, m] tokens three ways: contiguous, a column slice of a wider matrix (row-strided), and the every-4th-frame
    view of an encoder-output-like [768, 4 m - 3] (column-strided)"""
    base = _randn(768, m, seed=seed)
    wide = _randn(768, m + 37, seed=seed + 1)
    wide[:, 11:11 + m] = base
    frames = _randn(768, 4 * m - 3, seed=seed + 2)
    frames[:, ::4] = base
    return base, {"contiguous": base, "row-strided": wide[:, 11:11 + m], "column-strided": frames[:, ::4]}


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000, 50000])
def test_pool_append_is_bitwise_pack_rows_at_every_offset_and_stride(m):
    base, views = _views(m, 100 + m)
    want_rows, want_norms = _packed(base)
    cap = m + 2 * G
    report = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    for how, tok in views.items():
        assert m == 1 or tok.stride() == {"contiguous": (m, 1), "row-strided": (m + 37, 1), "column-strided": (4 * m - 3, 4)}[how]
        for at in (0, 1, G, cap - m):
            rows, norms, u = _guarded_table(cap)
            assert _append(tok, rows, norms, at, report) == 0, nat.lib().alive_last_error()
            assert torch.equal(rows[at:at + m], want_rows) and torch.equal(norms[at:at + m], want_norms), (how, at)
            outside = torch.ones(cap, dtype=torch.bool, device=DEV)
            outside[at:at + m] = False
            assert bool((rows[outside] == u).all()) and bool((norms[outside] == float(u.norm())).all()), (how, at)
            assert report.tolist() == [0, 2 ** 31 - 1]


def test_pool_append_reports_zero_nan_and_inf_rows():
    m, at = 200, 17
    tok = _randn(768, m, seed=5)
    tok[:, 70] = 0.0
    tok[3, 131] = float("nan")
    tok[700, 199] = float("inf")
    rows, norms, _ = _guarded_table(m + 2 * G)
    report = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert _append(tok, rows, norms, at, report) == 0
    assert report.tolist() == [3, at + 70]
    tok[:, 70] = 1.0
    assert _append(tok, rows, norms, at, report) == 0
    assert report.tolist() == [2, at + 131]                  # the report is reset by every call
    tok[3, 131] = 0.0
    assert _append(tok, rows, norms, at, report) == 0
    assert report.tolist() == [1, at + 199]
    # through the pool: the voice is refused and the pool is as it was
    pool = MS.VoicePool({"a": _randn(768, 10, seed=6)}, capacity=500)
    with pytest.raises(ValueError, match=r"row 209 has zero or non-finite norm \(1 such"):
        pool.add("bad", tok)
    assert pool.segments == {"a": (0, 10)} and pool.free_rows == 490
    with pytest.raises(ValueError, match="row 209"):
        pool.extend("a", tok)
    assert pool.segments == {"a": (0, 10)} and pool.layout == 0


def test_pool_append_refuses_rows_past_the_capacity_and_writes_nothing():
    m = 100
    tok = _randn(768, m, seed=8)
    rows, norms, u = _guarded_table(m + 2 * G)
    report = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    for cap, at in ((m + G, G + 1), (m - 1, 0), (m + G, m + G)):           # at + M = capacity + 1, M > capacity, at = capacity
        assert _append(tok, rows, norms, at, report, cap=cap) == -1
        assert b"outside the table" in nat.lib().alive_last_error()
    torch.cuda.synchronize()
    assert bool((rows == u).all()) and bool((norms == float(u.norm())).all()) and report.tolist() == [7, 7]


# ---------------------------------------------------------------------------------------------------- 2. alive_pool_move_rows
MOVES = [(n, src, dst) for n in (1, 2, 5, 64, 1000, 50000)
         for src, dst in ((G, G + n + 3), (G + n + 3, G),                                # disjoint, up and down
                          (G + 1, G), (G + n - 1, G), (G + n, G),                        # down by 1, n - 1, n rows
                          (G, G + 1), (G, G + n - 1), (G, G + n),                        # up by 1, n - 1, n rows
                          (G + n // 3 + 1, G), (G, G + n // 3 + 1))]                     # by about a third of the range


@pytest.mark.parametrize("n", [1, 2, 5, 64, 1000, 50000])
def test_pool_move_rows_is_bitwise_a_host_copy_for_overlapping_ranges(n):
    cap = 2 * n + 3 + 2 * G
    table, tnorms = _randn(cap, 768, seed=n), _randn(cap, seed=n + 1)
    for _, src, dst in [mv for mv in MOVES if mv[0] == n]:
        rows, norms = table.clone(), tnorms.clone()
        want_rows, want_norms = table.clone(), tnorms.clone()
        want_rows[dst:dst + n] = table[src:src + n]
        want_norms[dst:dst + n] = tnorms[src:src + n]
        nat.check(nat.lib().alive_pool_move_rows(nat.ptr(rows), nat.ptr(norms), cap, src, dst, n, nat.stream()))
        assert torch.equal(rows.view(torch.int32), want_rows.view(torch.int32)), (n, src, dst)        # bytes: guards included
        assert torch.equal(norms.view(torch.int32), want_norms.view(torch.int32)), (n, src, dst)
    rows = table.clone()
    assert nat.lib().alive_pool_move_rows(nat.ptr(rows), nat.ptr(tnorms), cap, cap - n + 1, 0, n, nat.stream()) == -1
    assert nat.lib().alive_pool_move_rows(nat.ptr(rows), nat.ptr(tnorms), cap, 0, cap - n + 1, n, nat.stream()) == -1
    assert torch.equal(rows, table)


# ---------------------------------------------------------------------------------------------------- 3. pool against pool
def _grouped(src, pool, names, k):
    lo = torch.tensor([pool.segment(n)[0] for n in names], dtype=torch.int32, device=DEV)
    ln = torch.tensor([pool.segment(n)[1] for n in names], dtype=torch.int32, device=DEV)
    val, idx = MS.knn_search_grouped(src, pool.rows, pool.norms, lo, ln, k)
    t = src.shape[2]
    rel = torch.where(idx >= 0, idx - lo.repeat_interleave(t)[:, None], idx)      # (a voice shorter than k: idx -1 on both sides)
    return val, rel


def test_reserved_pool_is_bitwise_a_fresh_default_pool_after_every_operation():
    tok = {n: _randn(768, m, seed=40 + i) for i, (n, m) in
           enumerate(dict(a=300, b=200, c=8, k1=1, k4=4, d=120, e=250, a2=100, c2=33).items())}
    u = _randn(768, seed=3)
    pool = MS.VoicePool(capacity=1500)
    pool.rows.copy_(u[None, :].expand(1500, 768))            # the free rows: every frame's best match, were they ever read
    pool.norms.fill_(float(u.norm()))
    rows_ptr, norms_ptr = pool.rows.data_ptr(), pool.norms.data_ptr()
    live = {}

    def check(step):
        fresh = MS.VoicePool(live)
        assert sorted(pool.segments) == sorted(fresh.segments), step
        for n in live:
            lo, m = pool.segment(n)
            flo, fm = fresh.segment(n)
            assert m == fm == live[n].shape[1]
            assert torch.equal(pool.rows[lo:lo + m], fresh.rows[flo:flo + fm]), (step, n)
            assert torch.equal(pool.norms[lo:lo + m], fresh.norms[flo:flo + fm]), (step, n)
            assert torch.equal(pool.tokens(n), live[n]), (step, n)
        names = sorted(live)
        src = 40.0 * u[None, :, None] + _randn(len(names), 768, 7, seed=len(step))
        for k in (1, 4, 8):
            got, want = _grouped(src, pool, names, k), _grouped(src, fresh, names, k)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (step, k)
            for i, n in enumerate(names):                    # active exactly where the voice has k rows or more
                assert bool((got[1][i * 7:(i + 1) * 7] >= 0).all()) == (live[n].shape[1] >= k), (step, k, n)
        assert (pool.rows.data_ptr(), pool.norms.data_ptr(), pool.P, pool.version) == (rows_ptr, norms_ptr, 1500, 0)
        assert pool.free_rows == 1500 - sum(t.shape[1] for t in live.values())

    for n in ("a", "b", "c", "k1", "k4"):
        pool.add(n, tok[n])
        live[n] = tok[n]
    assert pool.segments == dict(a=(0, 300), b=(300, 200), c=(500, 8), k1=(508, 1), k4=(509, 4))
    check("add a b c k1 k4")
    pool.remove("b")
    del live["b"]
    check("remove b")
    pool.add("d", tok["d"])                                   # smaller than b's hole: goes into it
    live["d"] = tok["d"]
    assert pool.segment("d") == (300, 120) and pool.largest_hole == 1500 - 513
    check("add d")
    pool.add("e", tok["e"])                                   # larger than what is left of it: behind the last voice
    live["e"] = tok["e"]
    assert pool.segment("e") == (513, 250) and pool.layout == 0
    check("add e")
    pool.extend("c", tok["c2"])                               # no room behind c: it moves into what is left of b's hole
    live["c"] = torch.cat([tok["c"], tok["c2"]], 1)
    assert pool.segment("c") == (420, 41) and pool.layout == 1
    check("extend c (moved)")
    pool.extend("a", tok["a2"])                               # no room behind a either: 400 rows move behind the last voice
    live["a"] = torch.cat([tok["a"], tok["a2"]], 1)
    assert pool.segment("a") == (763, 400) and pool.layout == 2
    check("extend a (moved)")
    pool.extend("a", tok["d"][:, :50])                        # the last voice grows in place
    live["a"] = torch.cat([live["a"], tok["d"][:, :50]], 1)
    assert pool.segment("a") == (763, 450) and pool.layout == 3
    check("extend a (in place)")
    pool.compact()                                            # d down by 300 > its 120 rows; a by 347 < its 450: overlapping
    assert pool.segments == dict(d=(0, 120), c=(120, 41), k1=(161, 1), k4=(162, 4), e=(166, 250), a=(416, 450))
    assert pool.layout == 4 and pool.largest_hole == pool.free_rows == 1500 - 866
    check("compact")
    with pytest.raises(ValueError, match=r"needs 700 rows.* 634 free .*largest hole is 634"):
        pool.add("big", _randn(768, 700, seed=1))
    check("refused add")


# ---------------------------------------------------------------------------------------------------- 4. sessions
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_sessions_run_through_enrol_extend_remove_and_compact_without_a_recapture(graph):
    """4 slots at -c 160 -b 16 on a reserved pool against the same sessions on a default pool that is re-packed (and, in graph
    mode, re-captured) at every change: tick for tick the same PCM.  Slot 2 is a blend of c and e; the compact moves both."""
    chunk, bs, ticks = 160, 16, 75
    tok = dict(a=synthetic.make_library(600, 31)[0], b=synthetic.make_library(400, 32)[0], c=synthetic.make_library(500, 33)[0],
               e=synthetic.make_library(300, 34)[0], d=synthetic.make_library(700, 35)[0], a2=synthetic.make_library(350, 36)[0])
    tok = {n: t.to(DEV) for n, t in tok.items()}
    first = {n: tok[n] for n in "abce"}
    res = MS.VoicePool(first, capacity=4000)
    ref = MS.VoicePool(first)
    pcm = [_pcm(chunk * ticks, 500 + s) for s in range(4)]
    convs = [MS.MultiStreamConverter(*_nets(), p, 4, chunk=chunk, buffersize=bs, k=4, blend=2) for p in (res, ref)]
    if graph:
        for c in convs:
            c.enable_graph()
    rconv, dconv = convs
    rows_ptr = res.rows.data_ptr()
    open_ = {0: dict(voice="a", pitch=1.0), 1: dict(voice="b", alpha=0.2), 2: dict(voice={"c": 2.0, "e": 1.0}, pitch=-2.0)}
    for c in convs:
        for s, p in open_.items():
            c.open(s, **p)
    with pytest.raises(ValueError, match=r"in use by MultiStreamConverter\(slots=4\)"):
        res.remove("e")                                      # a blend component is held too
    feeding, start = {0, 1, 2}, {0: 0, 1: 0, 2: 0}
    emitted = {s: 0 for s in range(4)}
    for tick in range(ticks):
        if tick == 25:                                       # a voice is enrolled mid-stream and a session opens on it
            res.add("d", tok["d"])
            ref.add("d", tok["d"])
            for c in convs:
                c.open(3, "d", f0_rate=0.8)
            feeding.add(3)
            start[3] = 25
        if tick == 35:                                       # a voice grows under a running session (here it has to move)
            res.extend("a", tok["a2"])
            assert res.segment("a")[0] != 0
            ref.add("a", torch.cat([tok["a"], tok["a2"]], 1))
        if tick == 45:                                       # a session closes and its voice goes
            with pytest.raises(ValueError, match="in use by"):
                res.remove("b")
            for c in convs:
                c.close(1)
            feeding.discard(1)
            res.remove("b")
        if tick == 55:                                       # the pool is compacted under the running sessions
            before = dict(res.segments)
            res.compact()
            assert all(res.segments[n] != before[n] for n in "ced") and res.free_rows == res.largest_hole
        if tick in (25, 35):                                 # the default side: the re-packed pool moved every voice
            for s in sorted(feeding):
                dconv.set(s, voice=dconv.params[s]["voice"])
        feed = {s: pcm[s][(tick - start[s]) * chunk:(tick - start[s] + 1) * chunk] for s in feeding}
        got, want = rconv.step(feed), dconv.step(feed)
        assert sorted(got) == sorted(want) == sorted(feeding)
        for s in feeding:
            assert (got[s] is None) == (want[s] is None), (tick, s)
            if got[s] is not None:
                assert np.array_equal(got[s], want[s]), (tick, s)
                emitted[s] += 1
    assert emitted == {0: ticks - bs, 1: 45 - bs, 2: ticks - bs, 3: ticks - 25 - bs}
    assert res.rows.data_ptr() == rows_ptr and res.version == 0 and res.layout == 2
    assert rconv.captures == (1 if graph else 0)
    if graph:
        assert dconv.captures == 3                           # the default pool's re-capture on a version change stays
    for s in (0, 2, 3):
        rconv.close(s)
    for n in "acde":
        res.remove(n)                                        # every hold was released
    assert res.free_rows == 4000


# ---------------------------------------------------------------------------------------------------- 5. enrol_voice
def _voice_files(d):
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    audio_io.save(str(d / "spk.wav"), synthetic.make_waveform(24000 * 3, 60).repeat(2, 1) * torch.tensor([[0.5], [0.25]]), 24000)
    return str(d / "spk.wav"), str(d / "voice_library.pt")


@pytest.mark.parametrize("sources", ["target", "lib", "both"])
def test_enrol_voice_rows_are_bitwise_voice_tokens_then_add(tmp_path, sources):
    import multistream_inference as msi
    spk, libf = _voice_files(tmp_path)
    target, lib = (spk if sources != "lib" else None), (libf if sources != "target" else None)
    CE = _nets()[0].to(DEV)
    want = MS.VoicePool({"v": msi.voice_tokens(CE, target, lib, torch.device(DEV))})
    m = want.segment("v")[1]
    assert m >= (512 if lib else 30)
    wav, sr = audio_io.load(target) if target else (None, None)
    for max_frames in (None, 1000, 37, 7):                   # one call, one piece, pieces that split the wav's frames and the file's
        pool = MS.VoicePool({"other": _randn(768, 29, seed=2)}, capacity=1000)
        layout = pool.layout
        assert MS.enrol_voice(pool, "v", CE, wav, sr, lib=lib, max_frames=max_frames) == m
        assert pool.segment("v") == (29, m)
        assert torch.equal(pool.rows[29:29 + m], want.rows) and torch.equal(pool.norms[29:29 + m], want.norms), max_frames
        pieces = 1 if max_frames is None else -(-m // max_frames)
        assert pool.layout - layout == pieces - 1            # `add`, then one `extend` per further piece
    steps = list(MS.enrol_steps(MS.VoicePool(capacity=1000), "v", CE, wav, sr, lib=lib, max_frames=100))
    assert steps == list(range(100, m, 100)) + [m]
    small = MS.VoicePool({"other": _randn(768, 29, seed=2)}, capacity=29 + m - 1)
    with pytest.raises(ValueError, match=f"needs {m} rows"):
        MS.enrol_voice(small, "v", CE, wav, sr, lib=lib)
    with pytest.raises(ValueError, match="needs"):           # pieces: what went in is taken out again
        MS.enrol_voice(small, "v", CE, wav, sr, lib=lib, max_frames=20)
    assert sorted(small.segments) == ["other"] and small.free_rows == m - 1
    with pytest.raises(ValueError, match="reserved pool"):
        MS.enrol_voice(MS.VoicePool(), "v", CE, wav, sr, lib=lib)


# ---------------------------------------------------------------------------------------------------- 6. the CLI
def test_multistream_cli_with_pool_rows_writes_the_same_files(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    for name, sd in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _sds()):
        torch.save(sd, d / name)
    _voice_files(d)
    torch.save({"tokens": synthetic.make_library(640, 9)}, d / "second_library.pt")
    for i in range(5):
        audio_io.save(str(d / f"in{i}.wav"), synthetic.make_waveform(16000 + 3000 * i, 50 + i) * 0.5, 16000)
    sessions = [dict(input="in0.wav", lib="voice_library.pt", pitch=2.0),                                      # ticks 0..49
                dict(input="in1.wav", target="spk.wav", f0_rate=0.5, alpha=0.2, start=7),
                dict(input="in2.wav", target="spk.wav", lib="voice_library.pt", gain=-3.0, start=3, output="third.wav"),
                dict(input="in3.wav", blend=[dict(lib="second_library.pt", weight=3), dict(target="spk.wav", weight=1)], start=60),
                dict(input="in4.wav", lib="voice_library.pt", start=75)]                        # the first voice again, after it went
    json.dump(sessions, open(d / "sessions.json", "w"))
    common = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt"),
              "-c", "320", "-b", "8", str(d / "sessions.json")]
    # the host plan, with the row counts of the voices
    ss = msi.load_sessions(str(d / "sessions.json"))
    CE = _nets()[0].to(DEV)
    CE.load_state_dict(_sds()[0])
    rows = {msi.voice_name(t, lb): msi.voice_tokens(CE, t, lb, torch.device(DEV)).shape[1] for s in ss for t, lb in msi.session_sources(s)}
    plan = [dict(start=s["start"], ticks=len(msi.input_pcm(s["input"], 16000, DEV)) // 320,
                 voices={msi.voice_name(t, lb): rows[msi.voice_name(t, lb)] for t, lb in msi.session_sources(s)}) for s in ss]
    events, peak = msi.enrol_plan(plan)
    assert [e[1] for e in events].count("enrol") == 5 and len(rows) == 4        # the library voice is enrolled twice
    assert peak < sum(rows.values())
    names = ["0_in0.wav", "1_in1.wav", "3_in3.wav", "4_in4.wav"]

    def run(out, extra):
        s2 = [dict(s, output=str(d / out / "third.wav")) if s.get("output") else s for s in sessions]
        json.dump(s2, open(d / "sessions.json", "w"))
        msi.main(["-o", str(d / out)] + extra + common)
        return [open(d / out / n, "rb").read() for n in names + ["third.wav"]]
    want = run("plain", [])
    assert all(len(w) > 44 + 2 * 320 for w in want)
    assert run("reserved", ["--pool-rows", str(peak)]) == want
    assert run("reserved_no_graph", ["--pool-rows", str(peak + 100), "--no-graph"]) == want
    with pytest.raises(ValueError, match=r"needs \d+ rows"):
        run("too_small", ["--pool-rows", str(peak - 1)])
    assert not os.path.exists(d / "too_small")               # it failed before any audio was written


# ---------------------------------------------------------------------------------------------------- 7. convert_many
def test_convert_many_on_a_reserved_pool_with_a_hole_is_bitwise_the_default_pool():
    from module.pipeline import Converter
    conv = Converter(*_nets(), torch.device(DEV))
    tok = {"shared": _randn(768, 3000, seed=41), "lib512": synthetic.make_library(512, 5)[0].to(DEV), "small": _randn(768, 40, seed=42)}
    utts = [synthetic.make_waveform(int(s * 16000), 300 + i).to(DEV) for i, s in enumerate((1.0, 3.5, 2.0, 4.25))]
    utts = [w / w.abs().max() for w in utts]
    voices = ["shared", "lib512", {"small": 1.0, "shared": 3.0}, "small"]
    kw = dict(pitch_shift=[0.0, 2.0, -3.0, 1.0], alpha=[0.0, 0.1, 0.3, 0.0], chunk=48000, k=4, window_batch=3)
    want = conv.convert_many(utts, MS.VoicePool(tok), voices, **kw)
    pool = MS.VoicePool(capacity=6000)
    u = _randn(768, seed=3)
    pool.rows.copy_(u[None, :].expand(6000, 768))
    pool.norms.fill_(float(u.norm()))
    pool.add("gone0", _randn(768, 700, seed=43)).add("shared", tok["shared"]).add("gone1", _randn(768, 333, seed=44))
    pool.add("small", tok["small"]).add("lib512", tok["lib512"])
    pool.search_images()                                      # images of the pool as it was: they must not survive a change
    pool.remove("gone0").remove("gone1")
    assert pool.holes() == [(0, 700), (3700, 333), (4585, 1415)]
    got = conv.convert_many(utts, pool, voices, **kw)
    assert pool.search_images()["names"] == ["shared", "small", "lib512"] and pool.P == 6000
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"utterance {i}"
    pool.compact()
    for i, (g, w) in enumerate(zip(conv.convert_many(utts, pool, voices, **kw), want)):
        assert torch.equal(g, w), f"utterance {i} after compact"
