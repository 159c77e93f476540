"""Tick latency of MultiStreamConverter (module/multistream.py): p50 / p99 of one tick, eager and hipGraph, for B sessions at
-c 160 -b 16 and -c 960 -b 8, with one shared 50 k-vector voice or B distinct ones; sessions served in real time (p99 below
the chunk period); and the grouped search alone: bytes of the segments it reads per tick over its kernel time.

Timing: every tick is bracketed by torch.cuda.synchronize() (the tick itself ends in a device -> host copy), after warm-up
ticks; the search is timed with events around repeated calls.  --rates spreads the sessions over a list of sample rates
(session s at rates[s % len]; MultiStreamConverter(rates=...), the per-row multi-rate edges) and adds that batch's tick p50 / p99
(mixed_<mode>_tick_p50_ms / _p99_ms) next to the single-rate figures of the same B.  --world adds the graph tick p50 / p99 of
the same batch per WORLD setting (world_<setting>_tick_p50_ms / _p99_ms): "off" is a world_pitch=False converter, a number f a
world_pitch=True converter with sessions s < round(f B) on WORLD (0: the masked branch with every row off).  --blend adds the graph
tick p50 / p99 of voice blending: blend3_single_* a blend=3 converter whose sessions are single voices, blend2_* / blend3_* every
session blending 2 / 3 voices (session s: voices s, s + 1, s + 2, weights 1, 2, 3) in a converter of that blend; distinct voices
only.  --mixed-k adds the graph tick p50 / p99 of the per-session k (MultiStreamConverter(k_max=8), the per-row-k entry points):
kmax8_uniform4_* every session at k = 4 through them (next to graph_tick_*: the same batch through the uniform entry points),
kmax8_mixed_* session s at k = (1, 2, 4, 8)[s % 4] -- on the shared voice that is one pass over the voice per k.  --auto-pitch adds
the graph tick p50 / p99 of an auto_pitch=True converter with every session on auto pitch (auto_pitch_tick_*: one more small launch on
the f0 side stream, alive_pitch_follow_rows; voice v_i is declared a register of 110 + 10 (i % 12) Hz) next to graph_tick_* of the same
batch.  --pitch-range adds the graph tick p50 / p99 of a pitch_range=True converter with every session on auto pitch, auto range and an
intonation of 1.2 (pitch_range_tick_*: alive_pitch_follow2_rows in place of alive_pitch_follow_rows and the centred transform in place
of the plain one; voice v_i is also declared a range of 1.5 + 0.25 (i % 8) semitones) between two measurements of the auto_pitch=True
converter with every session on auto pitch (pr_auto_pitch_tick_*, pr_auto_pitch_again_tick_*): the spread between those two is the
yardstick for the difference.  --gated adds, per fraction f, the graph tick p50 / p99 of a gate=True converter (the input gate: csrc/gate.hip) whose sessions all
carry a -40 dB gate, sessions s < round(f B) fed digital silence (their gates stay closed: no search for them) and the others the usual
speech-level signal (their gates stay open), and the event-timed grouped search over the segment lengths that tick left in seg_len_eff
(gated_<f>_tick_p50_ms / _p99_ms / _search_ms / _live_rows); and the gate=False converter a second time (gate_off_again_tick_*): the
spread between its two measurements is the yardstick for the gate's overhead at fraction 0.
--crossfade adds the graph tick p50 / p99 of a crossfade=True converter with every session crossfading over 10 ms (crossfade_tick_*:
one more launch of one block per session, alive_seam_rows, csrc/seam.hip), the seam statistic of its last tick over the sessions
(crossfade_seam_db_min / _median / _max: 10 log10 of how far two successive decodes disagree over the faded head -- on SYNTHETIC weights
and synthetic input, so it says nothing about how a trained model sounds), and the converter built without crossfade a second time
(crossfade_off_again_tick_*): the spread between its two measurements is the yardstick for the crossfade's cost.
--limit adds the graph tick p50 / p99 of a limiter=True converter with every session limiting at -12 dBFS with the default 5 ms lookahead
and 20 ms hold (limit_tick_*: one more launch of one block per session, alive_limit_rows, csrc/limit.hip), how far the limiter turned
the sessions down in its last tick (limit_db_min / _median / _max: 20 log10 of the smallest gain, on SYNTHETIC weights and input), and
the converter built without the limiter a second time (limit_off_again_tick_*): the spread between its two measurements is the
yardstick for the limiter's cost.
--envelope adds the graph tick p50 / p99 of an envelope=True converter with every session following at amount 1 (envelope_tick_*: one
more launch pair after the decoder, alive_envelope_waves, csrc/envelope.hip) beside the plain converter, both alive in the one process
and timed in alternating rounds (envelope_off_tick_*; the medians over the rounds, and the spread of the plain converter's rounds as the
yardstick), the call's own time by device events around 200 back-to-back eager calls at the tick's shapes (envelope_call_us, its fill
launch included) with the 12 B L bytes it moves (envelope_call_bytes), and the gains of the last tick (envelope_db_min / _max).
--post-filter does the same for a post_filter=True converter with every session at alpha 0.8 (post_filter_tick_* beside
post_filter_off_tick_*, post_filter_call_us for alive_postfilter_waves at the tick's shapes, csrc/postfilter.hip; post_filter_db_min /
_max).  --post-filter-offline times the offline call alone at 384 rows of 144 000 samples (post_filter_offline_ms).
--loudness adds the graph tick p50 / p99 of a loudness=True converter with every session normalised to -23 LUFS (loudness_tick_*: one
more launch between the gate's edge and the limiter, alive_loudness_rows, csrc/loudness.hip) beside the plain converter, both alive in
the one process and timed in alternating rounds (loudness_off_tick_*; the medians over the rounds, and the spread of the plain
converter's rounds as the yardstick), the call's own time by device events around 200 back-to-back eager calls on the converter's own
arrays (loudness_call_us, spans of loudness_span samples) and the gains of the last tick (loudness_gain_db_min / _max, on SYNTHETIC
weights).
--loudness-offline runs the offline loudness leg ALONE: alive_loudness_measure_waves (measure_us) and measure + apply, what
normalize_loudness launches (measure_apply_us), over 64 rows of 10 s and 8 rows of 60 s at 48 kHz, by device events around 20 calls.
--pitch-track adds the graph tick p50 / p99 of a pitch_track=True converter with no session tracking (track_none_tick_*: the class
scores stored, their argmax, and the tracker's blocks returning at once) and with every session tracking at the defaults
(track_all_tick_*: alive_f0_track_rows over every ring, csrc/f0_track.hip) beside the converter built without it (track_off_tick_*),
all three alive in the one process and timed in alternating rounds (the medians over the rounds; the spread of track_off's rounds is
the yardstick), the tracker call alone by device events around 200 back-to-back eager calls on the last tick's scores
(track_call_us), and how many frames it moved in the last tick (track_changed_mean, on SYNTHETIC weights and input).
--voicing adds the graph tick p50 / p99 of a voicing=True converter with no session deciding (voicing_none_tick_*: the two kernels'
blocks returning at once) and with every session deciding at the defaults (voicing_all_tick_*: alive_voicing_rows over every ring,
csrc/voicing.hip) beside the converter built without it (voicing_off_tick_*), all three alive in the one process and timed in
alternating rounds as --pitch-track's are, the call alone by device events around 200 back-to-back eager calls on the last tick's
rings (voicing_call_us), and how many frames it set to 0 in the last tick (voicing_changed_mean, on SYNTHETIC weights and input).
--voicing-offline runs the bare call ALONE over 384 windows of 450 frames (144 000 samples each), by device events around 20 calls.
--enrol runs the live-enrolment leg ALONE: B = 64 sessions on distinct 50 000-row voices at -c 160 -b 16, graph mode, and
one more 50 000-row voice added between two ticks, once on a default pool (the add re-packs the pool and the next tick
re-captures) and once on a reserved pool of 65 x 50 000 rows (VoicePool(capacity=...): alive_pool_append into the table in
place); per pool the wall time of the add (bracketed by device synchronisation; add_device_ms: events around it), the latency of
the tick that follows and the p50 / p99 of the 30 steady ticks before it.  On the reserved pool it asserts that the graph was
captured once, that the row table did not move and that nothing of table size was allocated, and adds the worst compaction: the
lowest voice is removed and `compact` slides the other 64 down by one voice (compact_wall_ms, tick_after_compact_ms).  Profile in a separate run (rocprofv3 --kernel-trace --stats --
python tools/bench_multistream.py --quick).  Prints one JSON line per configuration and writes the list to --out.
--sparse runs the sparse-ticks leg ALONE (MultiStreamConverter(sparse=True): the rings on the device, csrc/ring.hip), graph mode, k = 4.
All present: B = 128 and B = 1024 sessions on one shared 50 000-row voice at -c 160 -b 16 (16 kHz sessions) and at -c 960 -b 8 with 48 kHz
sessions, the dense and the sparse converter ALTERNATED in one process, two runs each (dense_tick_* / sparse_tick_* lists: the spread
between the two runs of one side is the yardstick for the difference between the sides), and beside them the bytes each converter
copies per tick in each direction, computed from its shapes.  Half absent: B = 64 distinct voices at -c 160 -b 16, the sparse converter
with every session present against sessions present on alternate ticks (even slots on even ticks, odd on odd): the tick, and the
grouped search alone, event-timed, over the segment lengths that tick left in seg_len_tick.
--conceal runs the lost-chunk leg ALONE (MultiStreamConverter(sparse=True, conceal=True): csrc/conceal.hip), graph mode, k = 4, B = 128
and B = 1024 sessions on one shared 50 000-row voice at -c 160 -b 16: a conceal=False sparse converter (conceal_off_tick_*) and
conceal=True converters with 0 %, 5 % and 100 % of the sessions losing EVERY tick (conceal_0_ / conceal_5_ / conceal_100_tick_*; a
session that loses every tick is in one long run: the period is searched on its first lost chunk only), ALTERNATED in one process, two
runs each: the spread between the two conceal_off runs is the yardstick, and the 0 % converter launches what conceal_off launches.
Beside them the calls alone on the converter's own arrays, by device events around 200 back-to-back eager calls: alive_conceal_rows
with every row lost and its state cleared before each call (conceal_call_search_us: every session's FIRST lost chunk, the period
search, the worst case; the clearing fill is timed alone and taken off), with every row in a run (conceal_call_run_us) and
alive_ring_push_rows with every row present (push_call_us).

    python tools/bench_multistream.py [--batches 1,8,32,64,128] [--ticks 40] [--warmup 6] [--rates 8000,16000,44100,48000]
                                      [--world off,0,0.5,1] [--voices shared,distinct] [--blend] [--mixed-k] [--auto-pitch] [--pitch-range]
                                      [--gated 0,0.5,1] [--crossfade] [--limit] [--envelope] [--post-filter] [--loudness] [--pitch-track] [--voicing] [--match-path]
                                      [--out multistream.json]
    python tools/bench_multistream.py --loudness-offline [--out loudness_offline.json]
    python tools/bench_multistream.py --voicing-offline [--out voicing_offline.json]
    python tools/bench_multistream.py --match-path-offline [--out match_path_call.json]
    python tools/bench_multistream.py --enrol [--out profiles/multistream_enrol.json]
    python tools/bench_multistream.py --sparse [--batches 128,1024] [--ticks 40] [--out profiles/multistream_sparse_bench.json]
    python tools/bench_multistream.py --conceal [--batches 128,1024] [--ticks 40] [--out profiles/multistream_conceal_bench.json]
    python tools/bench_multistream.py --pool-dtype fp16 [--batches 64,128] [--out profiles/pool_f16_bench.json]

--pool-dtype fp16 (pool_dtype_leg): the half-precision pool (VoicePool(dtype=torch.float16)) beside the fp32 pool of the same voices,
the two alternated run by run in one process, three runs each: tick p50 / p99, the event-timed grouped search alone, the spread
between runs and the search's read rate, then two fidelity figures on a synthetic voice (pool_dtype_fidelity).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alive-vc_amd"))

from module import multistream as MS           # noqa: E402
from module import synthetic                   # noqa: E402
from module.content_encoder import ContentEncoder   # noqa: E402
from module.decoder import Decoder             # noqa: E402
from module.f0_estimator import F0Estimator    # noqa: E402

VOICE_ROWS = 50000


def make_pool(n_voices, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return MS.VoicePool({f"v{i}": torch.randn(768, VOICE_ROWS, device="cuda", generator=g) for i in range(n_voices)})


def time_ticks(conv, B, chunk, ticks, warmup, seed, silent=0, present=None, lost=None):
    """chunk: one length, or a list of per-slot lengths (sessions at their own rates); sessions s < silent send digital silence;
    present(t, s) (a sparse converter): whether session s sends a chunk on tick t (default: every session, every tick);
    lost(t, s) (a concealing converter): whether session s's chunk of tick t is lost (default: none)"""
    cs = list(chunk) if isinstance(chunk, (list, tuple)) else [chunk] * B
    pcm = [(synthetic.make_waveform(cs[s] * 4, seed + s)[0].numpy() * (0 if s < silent else 12000)).astype(np.int16) for s in range(B)]
    ts = []
    for t in range(warmup + ticks):
        feed = {s: pcm[s][(t % 4) * cs[s]:(t % 4 + 1) * cs[s]] for s in range(B) if present is None or present(t, s)}
        gone = [s for s in feed if lost(t, s)] if lost is not None else []
        for s in gone:
            del feed[s]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        conv.step(feed, gone) if gone else conv.step(feed)
        torch.cuda.synchronize()
        if t >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.percentile(ts, 50)), float(np.percentile(ts, 99))


def time_calls(fn, reps=200):
    """microseconds per call of fn, by device events around `reps` back-to-back calls"""
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def loudness_offline_leg(shapes=((64, 10.0), (8, 60.0)), rate=48000):
    """measure_loudness_rows alone and measure + apply (what normalize_loudness launches) over N rows of `seconds` at `rate` Hz,
    device time per call: one record per shape"""
    recs = []
    coef, ap = MS.loudness_filter(rate)
    hop_ = MS.loudness_hop(rate)
    for n, seconds in shapes:
        ld = int(seconds * rate)
        y = torch.randn(n, ld, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 0.1
        lens = torch.full((n,), ld, dtype=torch.int32, device="cuda")
        hop = torch.full((n,), hop_, dtype=torch.int32, device="cuda")
        coefs = torch.tensor([coef] * n, dtype=torch.float64, device="cuda")
        aps = torch.tensor([ap] * n, dtype=torch.float64, device="cuda")
        z_t = torch.full((n,), MS.loudness_z(-23.0), dtype=torch.float64, device="cuda")
        z_abs, tiles = MS.loudness_z(MS.LOUDNESS_GATE_LUFS), ld // hop_

        def both():
            zI, _, c2 = MS.measure_loudness_rows(y, lens, hop, coefs, aps, z_abs, tiles)
            return MS.apply_loudness_rows(y, lens, zI, c2, z_t, 4.0)
        rec = dict(rows=n, seconds=seconds, rate=rate, tiles_per_row=tiles,
                   measure_us=round(time_calls(lambda: MS.measure_loudness_rows(y, lens, hop, coefs, aps, z_abs, tiles), 20), 1),
                   measure_apply_us=round(time_calls(both, 20), 1), bytes_read_once=4 * n * ld)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del y
    return recs


def post_filter_offline_leg(rows=384, samples=144000):
    """the offline post_filter call (its two small tensors and the output allocation included) over `rows` rows of `samples` samples of
    make_voiced speech at alpha 0.8 and the defaults; a copy of the same rows by the same call at alpha 0 beside it"""
    y = synthetic.make_voiced(samples, 3)[0].cuda().repeat(rows, 1).contiguous()
    us = time_calls(lambda: MS.post_filter(y, None, 0.8), reps=10)
    us0 = time_calls(lambda: MS.post_filter(y, None, 0.0), reps=10)
    rec = {"leg": "post_filter_offline", "rows": rows, "samples": samples, "post_filter_offline_ms": round(us / 1e3, 3),
           "post_filter_offline_copy_ms": round(us0 / 1e3, 3), "ns_per_sample": round(us * 1e3 / (rows * samples), 4)}
    print(json.dumps(rec), flush=True)
    return [rec]


def voicing_offline_leg(windows=384, frames=450):
    """the bare voicing call over `windows` windows of `frames` frames of make_voiced speech at the defaults"""
    from module import common, ops
    o = common.voicing_options(True)
    x = synthetic.make_voiced(320 * frames, 3)[0].cuda().repeat(windows, 1).contiguous()
    f0 = torch.full((windows, 1, frames), 120.0, device="cuda")
    per_row = [torch.full((windows,), o[key], dtype=torch.float64, device="cuda") for key in ("on", "off", "floor_e")]
    us = time_calls(lambda: ops.voicing_rows_(f0, x, o, None, *per_row), reps=20)
    rec = {"windows": windows, "frames": frames, "lags": [o["lag_lo"], o["lag_hi"]], "W": o["W"], "voicing_call_us": round(us, 1),
           "us_per_frame": round(us / (windows * frames), 4)}
    print(json.dumps(rec), flush=True)
    return [rec]


def match_path_offline_leg(shapes=((1, 24), (16, 24), (128, 24), (384, 450)), rows_n=4096):
    """the bare path call (alive_knn_path_rows: join + path) on R list rows of T frames at k_max = 4 and 8, every row on"""
    g = torch.Generator(device="cuda").manual_seed(9)
    rows = torch.randn(rows_n, 768, device="cuda", generator=g)
    norms = rows.double().pow(2).sum(dim=1).sqrt().float()
    recs = []
    for R, T in shapes:
        rec = {"leg": "match_path_call", "R": R, "T": T, "table_rows": rows_n}
        for k in (4, 8):
            us = path_call_us(R, T, k, rows, norms)
            rec[f"path_call_k{k}_us"] = round(us, 2)
            rec[f"k{k}_us_per_frame"] = round(us / (R * T), 4)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def conceal_leg(nets, batches=(128, 1024), ticks=40, warmup=6):
    """a conceal=False sparse converter against conceal=True ones with 0 %, 5 % and 100 % of the sessions losing every tick, alternated,
    two runs each; then the conceal call and the push alone: one record per B"""
    recs = []
    shared = make_pool(1, 1)
    chunk, bs = 160, 16
    sides = (("conceal_off", False, 0.0), ("conceal_0", True, 0.0), ("conceal_5", True, 0.05), ("conceal_100", True, 1.0))
    for B in batches:
        rec = {"leg": "conceal", "chunk": chunk, "buffersize": bs, "B": B, "voices": "shared", "voice_rows": VOICE_ROWS,
               "chunk_period_ms": chunk / 16.0}
        for name, _, _ in sides:
            rec[f"{name}_tick_p50_ms"], rec[f"{name}_tick_p99_ms"] = [], []
        for run in range(2):
            for name, conceal, frac in sides:
                conv = MS.MultiStreamConverter(*nets, shared, B, chunk=chunk, buffersize=bs, k=4, sparse=True, conceal=conceal)
                for s in range(B):
                    conv.open(s, "v0", pitch=float(s % 5), f0_rate=0.5)
                conv.enable_graph()
                losing = int(round(frac * B))
                fill = warmup + bs + 1                         # the losses start once the rings are full of speech
                p50, p99 = time_ticks(conv, B, chunk, ticks, fill, 300, lost=(lambda t, s: t >= bs + 1 and s < losing) if losing else None)
                rec[f"{name}_tick_p50_ms"].append(round(p50, 3))
                rec[f"{name}_tick_p99_ms"].append(round(p99, 3))
                assert conv.captures == 1, conv.captures
                if conceal:
                    assert conv.conceals == (ticks + warmup if losing else 0), (conv.conceals, losing)
                    rec[f"{name}_sessions_losing"] = losing
                if name == "conceal_100" and run == 1:         # the calls alone, on this converter's own arrays and full rings
                    st, flags = conv._conceal_state, conv._flags
                    def call():                                # noqa: E306
                        MS.conceal_rows_(conv.ring_dev, conv.ring_len, conv._chunks_dev, conv.chunk_len, conv.present, conv.lost,
                                         conv.conceal_on, conv._conceal_consts, st, conv.conceal_tmpl)
                    flags[0], flags[2] = True, True            # every row present and lost
                    fill_us = time_calls(lambda: st.zero_())
                    both_us = time_calls(lambda: (st.zero_(), call()))
                    assert int((st[:, 0] == chunk).sum()) == B and int((st[:, 1] >= 40).sum()) == B
                    rec["conceal_call_search_us"] = round(both_us - fill_us, 2)
                    rec["conceal_call_run_us"] = round(time_calls(call), 2)
                    flags[2] = False
                    rec["push_call_us"] = round(time_calls(lambda: MS.ring_push_rows_(
                        conv.ring_dev, conv._chunks_dev, conv.chunk_len, conv.ring_len, conv.present, conv._in, conv.seg_len,
                        conv.seg_len_tick, conv.S)), 2)
                del conv
                torch.cuda.empty_cache()
        lo, hi = min(rec["conceal_off_tick_p50_ms"]), max(rec["conceal_off_tick_p50_ms"])
        rec["conceal_0_inside_the_spread_of_conceal_off"] = all(lo <= v <= hi for v in rec["conceal_0_tick_p50_ms"])
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def enrol_leg(nets, B=64, chunk=160, bs=16, steady=30, warmup=6):
    """the cost of one more voice for B running sessions, on a default and on a reserved pool: one record per pool"""
    def tokens(i):
        return torch.randn(768, VOICE_ROWS, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1000 + i))
    pcm = [(synthetic.make_waveform(chunk * 4, 300 + s)[0].numpy() * 12000).astype(np.int16) for s in range(B)]

    def tick(conv, t):
        feed = {s: pcm[s][(t % 4) * chunk:(t % 4 + 1) * chunk] for s in range(B)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        conv.step(feed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    recs = []
    for kind in ("default", "reserved"):
        if kind == "reserved":
            pool = MS.VoicePool(capacity=(B + 1) * VOICE_ROWS)
            for i in range(B):
                pool.add(f"v{i}", tokens(i))
        else:
            pool = MS.VoicePool({f"v{i}": tokens(i) for i in range(B)})
        conv = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4)
        for s in range(B):
            conv.open(s, f"v{s}", pitch=float(s % 5), f0_rate=0.5)
        conv.enable_graph()
        t = 0
        for _ in range(bs + 1 + warmup):
            tick(conv, t)
            t += 1
        ts = []
        for _ in range(steady):
            ts.append(tick(conv, t))
            t += 1
        new = tokens(B)
        table, table_bytes = pool.rows.data_ptr(), pool.rows.numel() * 4
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        a.record()
        pool.add("new", new)
        b.record()
        torch.cuda.synchronize()
        add_ms = (time.perf_counter() - t0) * 1e3
        after_ms = tick(conv, t)
        t += 1
        grown = torch.cuda.max_memory_allocated() - before
        later = [tick(conv, t + i) for i in range(5)]
        rec = {"pool": kind, "B": B, "chunk": chunk, "buffersize": bs, "voice_rows": VOICE_ROWS, "pool_rows": pool.P,
               "add_wall_ms": round(add_ms, 3), "add_device_ms": round(a.elapsed_time(b), 3), "tick_after_add_ms": round(after_ms, 3),
               "steady_tick_p50_ms": round(float(np.percentile(ts, 50)), 3), "steady_tick_p99_ms": round(float(np.percentile(ts, 99)), 3),
               "ticks_after_that_ms": [round(x, 3) for x in later], "captures": conv.captures, "table_moved": pool.rows.data_ptr() != table,
               "peak_allocation_during_add_and_tick_MB": round(grown / 2 ** 20, 1), "table_MB": round(table_bytes / 2 ** 20, 1)}
        if kind == "reserved":
            rec["tick_after_add_within_p99_plus_add"] = after_ms <= rec["steady_tick_p99_ms"] + a.elapsed_time(b)
            # the worst compaction: session 0 ends, its voice (the lowest) goes, and all 64 others slide down by one voice
            conv.close(0)
            pool.remove("v0")
            conv.open(0, "new", f0_rate=0.5)              # (slot 0 starts again on the new voice: B sessions still feed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pool.compact()
            torch.cuda.synchronize()
            rec["compact_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            rec["compact_moved_MB"] = round(B * VOICE_ROWS * (768 + 1) * 4 / 2 ** 20, 1)
            rec["tick_after_compact_ms"] = round(tick(conv, t + 5), 3)
            assert conv.captures == 1, conv.captures
            assert not rec["table_moved"] and pool.version == 0
            assert grown < table_bytes // 8, f"{grown} bytes allocated during the add and the tick after it"
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del conv, pool, new
        torch.cuda.empty_cache()
    return recs


def sparse_leg(nets, batches=(128, 1024), ticks=40, warmup=6):
    """dense against sparse with every session present, alternated, two runs each; then half the sessions absent: one record per
    configuration"""
    recs = []
    shared = make_pool(1, 1)
    for chunk, bs, rate in ((160, 16, 16000), (960, 8, 48000)):
        for B in batches:
            rec = {"leg": "all_present", "chunk": chunk, "buffersize": bs, "session_rate": rate, "B": B, "voices": "shared",
                   "voice_rows": VOICE_ROWS, "chunk_period_ms": chunk / 16.0, "dense_tick_p50_ms": [], "dense_tick_p99_ms": [],
                   "sparse_tick_p50_ms": [], "sparse_tick_p99_ms": []}
            for run in range(2):
                for side in ("dense", "sparse"):
                    conv = MS.MultiStreamConverter(*nets, shared, B, chunk=chunk, buffersize=bs, k=4, rates=[rate],
                                                   sparse=side == "sparse")
                    for s in range(B):
                        conv.open(s, "v0", pitch=float(s % 5), f0_rate=0.5, rate=rate)
                    conv.enable_graph()
                    p50, p99 = time_ticks(conv, B, conv.slot_chunk, ticks, warmup + bs + 1, 300)
                    rec[f"{side}_tick_p50_ms"].append(round(p50, 3))
                    rec[f"{side}_tick_p99_ms"].append(round(p99, 3))
                    assert conv.captures == 1, conv.captures
                    if run == 0:                           # what the tick copies, from the converter's own shapes
                        wave = conv._wave_len(rate)
                        up = conv._chunks_dev.numel() * 2 + conv._flags.numel() if conv.sparse else B * conv.ld_in * 2 + B
                        down = conv._pcm.numel() * 2 if conv.sparse else B * wave * 2
                        rec[f"{side}_bytes_up_per_tick"], rec[f"{side}_bytes_down_per_tick"] = int(up), int(down)
                    del conv
                    torch.cuda.empty_cache()
            rec["bytes_the_sessions_sent_per_tick"] = B * chunk * rate // 16000 * 2
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    del shared
    torch.cuda.empty_cache()
    B, chunk, bs = 64, 160, 16
    pool = make_pool(B, 2)
    rec = {"leg": "half_absent", "chunk": chunk, "buffersize": bs, "B": B, "voices": "distinct", "voice_rows": VOICE_ROWS}
    for name, present, fill in (("all_present", None, bs + 1), ("alternating", lambda t, s: (t + s) % 2 == 0, 2 * (bs + 1))):
        conv = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, sparse=True)
        for s in range(B):
            conv.open(s, f"v{s}", pitch=float(s % 5), f0_rate=0.5)
        conv.enable_graph()
        p50, p99 = time_ticks(conv, B, chunk, ticks, warmup + fill, 300, present=present)
        live = int((conv.seg_len_tick > 0).sum())
        assert live == (B if present is None else B // 2) and conv.captures == 1, (live, conv.captures)
        ms, nbytes = time_search(conv, B, seg_len=conv.seg_len_tick)
        rec.update({f"{name}_tick_p50_ms": round(p50, 3), f"{name}_tick_p99_ms": round(p99, 3), f"{name}_live_rows": live,
                    f"{name}_search_ms": round(ms, 4), f"{name}_search_bytes": nbytes})
        del conv
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    recs.append(rec)
    return recs


def pool_dtype_leg(nets, batches, configs, mixes, ticks, warmup, runs=3):
    """--pool-dtype fp16: the shared / distinct legs on an fp32 and on a half pool of the same voices (two reserved pools filled voice
    by voice, so no second copy of the tokens is kept), the two ALTERNATED run by run inside this one process, `runs` runs each.  Per
    leg and dtype: the graph tick's p50 / p99 and the event-timed grouped search alone (time_search) of every run, their medians,
    the spread between runs ((max - min) / median of the runs' p50s and search times), and the search's read rate in TB/s: the
    bytes of the distinct segments, rows and norms, read once, over the median search time.  Then the fidelity figures."""
    n_voices = max(batches) if "distinct" in mixes else 1
    pools = {"fp32": MS.VoicePool(capacity=n_voices * VOICE_ROWS), "fp16": MS.VoicePool(capacity=n_voices * VOICE_ROWS, dtype=torch.float16)}
    g = torch.Generator(device="cuda").manual_seed(2)
    for i in range(n_voices):
        tok = torch.randn(768, VOICE_ROWS, device="cuda", generator=g)
        for pool in pools.values():
            pool.add(f"v{i}", tok)
        del tok
    recs = []
    for chunk, bs in configs:
        for mix in mixes:
            for B in batches:
                rec = {"leg": "pool_dtype", "chunk": chunk, "buffersize": bs, "B": B, "voices": mix, "voice_rows": VOICE_ROWS,
                       "chunk_period_ms": chunk / 16.0, "runs": runs}
                per = {name: {"tick_p50_ms": [], "tick_p99_ms": [], "search_ms": []} for name in pools}
                nbytes = {}
                for run in range(runs):
                    for name, pool in pools.items():           # alternated: fp32, fp16, fp32, fp16, ...
                        conv = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4)
                        for s in range(B):
                            conv.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5)
                        conv.enable_graph()
                        p50, p99 = time_ticks(conv, B, chunk, ticks, warmup + bs + 1, 300)
                        ms, _ = time_search(conv, B, reps=60)
                        segs = {(int(lo), int(ln)) for lo, ln in zip(conv.seg_lo.tolist(), conv.seg_len.tolist()) if ln > 0}
                        nbytes[name] = sum(ln for _, ln in segs) * (pool.row_bytes + 4)
                        per[name]["tick_p50_ms"].append(round(p50, 3))
                        per[name]["tick_p99_ms"].append(round(p99, 3))
                        per[name]["search_ms"].append(round(ms, 4))
                        for s in range(B):
                            conv.close(s)
                        del conv
                for name, d in per.items():
                    med = {key: float(np.median(v)) for key, v in d.items()}
                    rec[name] = dict(d, tick_p50_ms_median=round(med["tick_p50_ms"], 3), tick_p99_ms_median=round(med["tick_p99_ms"], 3),
                                     search_ms_median=round(med["search_ms"], 4),
                                     tick_p50_spread=round((max(d["tick_p50_ms"]) - min(d["tick_p50_ms"])) / med["tick_p50_ms"], 4),
                                     search_spread=round((max(d["search_ms"]) - min(d["search_ms"])) / med["search_ms"], 4),
                                     search_bytes=nbytes[name], search_TB_per_s=round(nbytes[name] / (med["search_ms"] * 1e-3) / 1e12, 3),
                                     pool_table_bytes=pools[name].rows.numel() * pools[name].rows.element_size())
                rec["search_fp16_over_fp32"] = round(rec["fp16"]["search_ms_median"] / rec["fp32"]["search_ms_median"], 4)
                rec["tick_p50_fp16_over_fp32"] = round(rec["fp16"]["tick_p50_ms_median"] / rec["fp32"]["tick_p50_ms_median"], 4)
                rec["real_time"] = {name: rec[name]["tick_p99_ms_median"] < rec["chunk_period_ms"] for name in pools}
                print(json.dumps(rec), flush=True)
                recs.append(rec)
    del pools
    recs.append(pool_dtype_fidelity(nets))
    print(json.dumps(recs[-1]), flush=True)
    return recs


def pool_dtype_fidelity(nets, rows_n=5000, k=4, chunk=960, bs=8, ticks=350):
    """Two figures, no bar: a half pool against an fp32 pool of the UNROUNDED tokens of a synthetic voice (synthetic.make_library, the
    voices of the tests).  (a) the share of frames whose top-k SET differs, over the content encoder's frames of 350 s / 10 of
    synthetic audio (>= 1000 frames), each pool searched by its own kernel; (b) one session streamed through a converter on each
    pool in lockstep: the RMS of the difference of the two emitted int16 streams over 32768, beside the stream's own RMS."""
    from module.spectrogram import spectrogram
    tok = synthetic.make_library(rows_n, 31)[0].to("cuda")
    pools = [MS.VoicePool({"v": tok}, dtype=torch.float16), MS.VoicePool({"v": tok})]
    wav = synthetic.make_waveform(320 * 1100, 77).to("cuda")
    ce = nets[0].to("cuda")
    feat = torch.cat([ce(spectrogram(wav[:, i:i + 320 * 110])) for i in range(0, 320 * 1100, 320 * 110)], dim=2).contiguous()
    n_frames = feat.shape[2]
    lo = torch.zeros(1, dtype=torch.int32, device="cuda")
    ln = torch.full((1,), rows_n, dtype=torch.int32, device="cuda")
    sets = [MS.knn_search_grouped(feat, p.rows, p.norms, lo, ln, k)[1].sort(dim=1).values for p in pools]
    differ = int((sets[0] != sets[1]).any(dim=1).sum())
    convs = [MS.MultiStreamConverter(*nets, p, 1, chunk=chunk, buffersize=bs, k=k) for p in pools]
    for c in convs:
        c.open(0, "v")
        c.enable_graph()
    pcm = (synthetic.make_waveform(chunk * ticks, 78)[0].numpy() * 12000).astype(np.int16)
    out = [[], []]
    for t in range(ticks):
        for c, o in zip(convs, out):
            y = c.step({0: pcm[t * chunk:(t + 1) * chunk]})[0]
            if y is not None:
                o.append(y.astype(np.float64))
    a, b = (np.concatenate(o) for o in out)
    return {"leg": "pool_dtype_fidelity", "voice_rows": rows_n, "k": k, "frames_searched": n_frames, "frames_topk_set_differs": differ,
            "share_topk_set_differs": round(differ / n_frames, 5), "stream_samples": int(a.size), "stream_frames": int(a.size // 320),
            "stream_rms_diff_over_32768": float(np.sqrt(np.mean((a - b) ** 2)) / 32768),
            "stream_rms_over_32768": float(np.sqrt(np.mean(b ** 2)) / 32768), "stream_samples_differing": int((a != b).sum())}


def time_search(conv, B, reps=20, seg_len=None):
    """the grouped search alone on the tick's shape: (ms per call, bytes of distinct segments read once).  seg_len: the segment
    lengths to search with (default: the converter's; a gated converter's seg_len_eff has its closed rows at 0)"""
    seg_len = conv.seg_len if seg_len is None else seg_len
    src = torch.randn(B, 768, conv.frames, device="cuda")
    for _ in range(3):
        MS.knn_search_grouped(src, conv.pool.rows, conv.pool.norms, conv.seg_lo, seg_len, conv.k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        MS.knn_search_grouped(src, conv.pool.rows, conv.pool.norms, conv.seg_lo, seg_len, conv.k)
    b.record()
    torch.cuda.synchronize()
    segs = {(int(lo), int(ln)) for lo, ln in zip(conv.seg_lo.tolist(), seg_len.tolist()) if ln > 0}
    return a.elapsed_time(b) / reps, sum(ln for _, ln in segs) * (768 + 1) * 4


def path_call_us(R, T, k, rows, norms, seed=5):
    """alive_knn_path_rows alone on R list rows of T frames at k_max = k: random descending cosines, indices that repeat a third of
    the frame before's (as neighbouring frames of speech do), every row on at weight 1; device events around 200 back-to-back calls"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    val = torch.sort(torch.rand(R * T, k, device="cuda", generator=g) * 0.3 + 0.6, dim=1, descending=True)[0].contiguous()
    idx = torch.randint(0, rows.shape[0], (R, T, k), device="cuda", generator=g, dtype=torch.int32)
    keep = torch.rand(R, T, k, device="cuda", generator=g) < 0.35
    for t in range(1, T):
        idx[:, t] = torch.where(keep[:, t], idx[:, t - 1], idx[:, t])
    idx = idx.view(R * T, k).contiguous()
    k_row = torch.full((R,), k, dtype=torch.int32, device="cuda")
    on = torch.ones(R, dtype=torch.int32, device="cuda")
    w = torch.ones(R, dtype=torch.float64, device="cuda")
    moved = torch.zeros(R, dtype=torch.int32, device="cuda")
    return time_calls(lambda: MS.knn_path_rows(val, idx, k_row, k, on, w, rows, norms, moved=moved))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default=None, help="comma-separated batch sizes (default 1,8,32,64,128; with --sparse 128,1024)")
    ap.add_argument("--configs", default="160x16,960x8")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--quick", action="store_true", help="B = 64 at -c 160 -b 16, distinct voices, graph only (profiler runs)")
    ap.add_argument("--rates", default=None, help="comma-separated session rates: also time a batch spread over them")
    ap.add_argument("--world", default=None, help="comma-separated WORLD settings: off, or the fraction of sessions on WORLD")
    ap.add_argument("--voices", default="shared,distinct", help="voice mixes to run: shared, distinct")
    ap.add_argument("--blend", action="store_true", help="also time voice blending (blend=3 single voices, 2- and 3-voice blends)")
    ap.add_argument("--mixed-k", action="store_true", help="also time a k_max=8 converter: every session at k = 4, and an even "
                                                           "mix of k = 1, 2, 4, 8")
    ap.add_argument("--auto-pitch", action="store_true", help="also time an auto_pitch=True converter, every session on auto pitch")
    ap.add_argument("--pitch-range", action="store_true", help="also time a pitch_range=True converter, every session on auto pitch, "
                    "auto range and an intonation of 1.2, against an auto_pitch=True converter with every session on auto pitch, and that "
                    "one once more for the run-to-run spread")
    ap.add_argument("--gated", default=None, help="comma-separated fractions: also time a gate=True converter, every session behind "
                                                  "a -40 dB gate and that fraction of them fed digital silence")
    ap.add_argument("--crossfade", action="store_true", help="also time a crossfade=True converter, every session crossfading over "
                                                             "10 ms, and the plain converter a second time")
    ap.add_argument("--limit", action="store_true", help="also time a limiter=True converter, every session limiting at -12 dBFS, "
                                                         "and the plain converter a second time")
    ap.add_argument("--post-filter", action="store_true", help="also time a post_filter=True converter, every session at alpha 0.8, "
                    "beside the plain one in alternating rounds, and the call alone")
    ap.add_argument("--post-filter-offline", action="store_true", help="only time the offline post_filter call at 384 x 144000")
    ap.add_argument("--envelope", action="store_true", help="also time an envelope=True converter, every session following at amount "
                                                            "1, against the plain converter in alternating rounds, and the call alone")
    ap.add_argument("--loudness", action="store_true", help="also time a loudness=True converter, every session normalised to -23 LUFS, "
                    "alternated with a plain one, and the loudness call alone")
    ap.add_argument("--loudness-offline", action="store_true", help="the offline loudness leg alone: measure_loudness and "
                    "normalize_loudness over 64 rows of 10 s at 48 kHz, and over 8 rows of 60 s")
    ap.add_argument("--pitch-track", action="store_true", help="also time a pitch_track=True converter with no session and with "
                    "every session tracking, beside the plain converter in alternating rounds")
    ap.add_argument("--voicing", action="store_true", help="also time a voicing=True converter with no session and with every session "
                    "deciding, beside the plain converter in alternating rounds")
    ap.add_argument("--match-path", action="store_true", help="also time a match_path=True converter with no session and with every "
                                                              "session on the path, against a plain one in alternating rounds, and "
                                                              "the path call alone at k_max = 4 and 8")
    ap.add_argument("--match-path-offline", action="store_true", help="the bare path call alone over 384 windows of 450 frames")
    ap.add_argument("--voicing-offline", action="store_true", help="the bare voicing call alone over 384 windows of 450 frames")
    ap.add_argument("--enrol", action="store_true", help="the live-enrolment leg alone: one more voice between two ticks, on a "
                                                         "default and on a reserved pool")
    ap.add_argument("--sparse", action="store_true", help="the sparse-ticks leg alone: dense against sparse(=True) converters, "
                                                          "alternated, and half the sessions absent")
    ap.add_argument("--conceal", action="store_true", help="the lost-chunk leg alone: a conceal=False sparse converter against "
                                                           "conceal=True ones with 0, 5 and 100 %% of the sessions losing every tick, "
                                                           "alternated, and the conceal call and the push alone")
    ap.add_argument("--pool-dtype", default=None, choices=["fp16"], help="the half-pool leg alone: the shared / distinct legs (default "
                    "B = 64,128) on an fp32 and on an fp16 pool, alternated, three runs each, and the fidelity figures")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batches = [int(b) for b in (args.batches or ("128,1024" if args.sparse or args.conceal else "1,8,32,64,128")).split(",")]
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
    rates = [int(r) for r in args.rates.split(",")] if args.rates else None
    mixes = tuple(args.voices.split(","))
    worlds = args.world.split(",") if args.world else []
    gated = args.gated.split(",") if args.gated else []
    if args.quick:
        batches, configs, mixes = [64], [(160, 16)], ("distinct",)
    nets = (ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2))
    if args.pool_dtype:
        rows = pool_dtype_leg(nets, [int(b) for b in (args.batches or "64,128").split(",")], configs, mixes, args.ticks, args.warmup)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    if args.conceal:
        rows = conceal_leg(nets, batches, args.ticks, args.warmup)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    if args.sparse:
        rows = sparse_leg(nets, batches, args.ticks, args.warmup)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    if args.loudness_offline:
        rows = loudness_offline_leg()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    if args.post_filter_offline:
        rows = post_filter_offline_leg()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    if args.voicing_offline:
        rows = voicing_offline_leg()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    if args.match_path_offline:
        rows = match_path_offline_leg()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    if args.enrol:
        rows = enrol_leg(nets)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rows, open(args.out, "w"), indent=1)
        return
    shared = make_pool(1, 1)
    distinct = make_pool(max(batches) + (2 if args.blend else 0), 2)
    if args.auto_pitch or args.pitch_range:                    # (host floats beside the voices: nothing else changes)
        for pool in (shared, distinct):
            for i, name in enumerate(pool.segments):
                pool.set_register(name, hz=110.0 + 10.0 * (i % 12),
                                  **(dict(range_st=1.5 + 0.25 * (i % 8)) if args.pitch_range else {}))
    rows = []
    for chunk, bs in configs:
        period_ms = chunk / 16.0
        for mix in mixes:
            pool = shared if mix == "shared" else distinct
            for B in batches:
                rec = {"chunk": chunk, "buffersize": bs, "B": B, "voices": mix, "voice_rows": VOICE_ROWS, "chunk_period_ms": period_ms}
                for mode in (("graph",) if args.quick else ("eager", "graph")):
                    conv = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4)
                    for s in range(B):
                        conv.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5)
                    if mode == "graph":
                        conv.enable_graph()
                    p50, p99 = time_ticks(conv, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec[f"{mode}_tick_p50_ms"], rec[f"{mode}_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                rec["real_time"] = rec["graph_tick_p99_ms"] < period_ms
                rec["sessions_served_in_real_time"] = B if rec["real_time"] else 0
                ms, nbytes = time_search(conv, B)
                if rates:
                    rec["rates"] = rates
                    for mode in (("graph",) if args.quick else ("eager", "graph")):
                        mixed = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, rates=rates)
                        for s in range(B):
                            mixed.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5,
                                       rate=rates[s % len(rates)])
                        if mode == "graph":
                            mixed.enable_graph()
                        p50, p99 = time_ticks(mixed, B, mixed.slot_chunk, args.ticks, args.warmup + bs + 1, 300)
                        rec[f"mixed_{mode}_tick_p50_ms"], rec[f"mixed_{mode}_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                        del mixed
                for w in worlds:
                    wc = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, world_pitch=w != "off")
                    on = 0 if w == "off" else int(round(float(w) * B))
                    for s in range(B):
                        wc.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, world_pitch=s < on)
                    wc.enable_graph()
                    p50, p99 = time_ticks(wc, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec[f"world_{w}_tick_p50_ms"], rec[f"world_{w}_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    del wc
                blends = (("blend3_single", 3, 1), ("blend2", 2, 2), ("blend3", 3, 3)) if args.blend and mix == "distinct" else ()
                for name, S, n_mix in blends:                  # (distinct voices only: a blend mixes different voices)
                    bc = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, blend=S)
                    for s in range(B):
                        vs = [f"v{s + j}" for j in range(n_mix)]
                        bc.open(s, vs[0] if n_mix == 1 else [(v, j + 1.0) for j, v in enumerate(vs)], pitch=float(s % 5), f0_rate=0.5)
                    bc.enable_graph()
                    p50, p99 = time_ticks(bc, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec[f"{name}_tick_p50_ms"], rec[f"{name}_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    rec[f"{name}_real_time"] = p99 < period_ms
                    del bc
                for name, ks in ((("kmax8_uniform4", (4,)), ("kmax8_mixed", (1, 2, 4, 8))) if args.mixed_k else ()):
                    kc = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, k_max=8)
                    for s in range(B):
                        kc.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, k=ks[s % len(ks)])
                    kc.enable_graph()
                    p50, p99 = time_ticks(kc, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec[f"{name}_tick_p50_ms"], rec[f"{name}_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    rec[f"{name}_real_time"] = p99 < period_ms
                    del kc
                if args.auto_pitch:
                    ac = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, auto_pitch=True)
                    for s in range(B):
                        ac.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, auto_pitch=True)
                    ac.enable_graph()
                    p50, p99 = time_ticks(ac, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec["auto_pitch_tick_p50_ms"], rec["auto_pitch_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    rec["auto_pitch_real_time"] = p99 < period_ms
                    del ac
                if args.pitch_range:                           # the same box, the same run: auto pitch only, pitch range, auto pitch again
                    for name, kw, sess in (("pr_auto_pitch", dict(auto_pitch=True), dict(auto_pitch=True)),
                                           ("pitch_range", dict(pitch_range=True), dict(auto_pitch=True, auto_range=True, intonation=1.2)),
                                           ("pr_auto_pitch_again", dict(auto_pitch=True), dict(auto_pitch=True))):
                        pc = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, **kw)
                        for s in range(B):
                            pc.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, **sess)
                        pc.enable_graph()
                        p50, p99 = time_ticks(pc, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                        rec[f"{name}_tick_p50_ms"], rec[f"{name}_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                        assert pc.captures == 1
                        del pc
                    rec["pitch_range_real_time"] = rec["pitch_range_tick_p99_ms"] < period_ms
                for f in gated:
                    gc = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, gate=True)
                    silent = int(round(float(f) * B))
                    for s in range(B):
                        gc.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, gate_db=-40.0)
                    gc.enable_graph()
                    p50, p99 = time_ticks(gc, B, chunk, args.ticks, args.warmup + bs + 1, 300, silent=silent)
                    rec[f"gated_{f}_tick_p50_ms"], rec[f"gated_{f}_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    live = sum(gc.gate_open())
                    assert live == B - silent and gc.captures == 1, (live, B, silent, gc.captures)
                    rec[f"gated_{f}_live_rows"] = live
                    rec[f"gated_{f}_search_ms"] = round(time_search(gc, B, seg_len=gc.seg_len_eff)[0], 4)
                    del gc
                if gated:                                      # the gate=False converter once more: the run-to-run spread
                    again = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4)
                    for s in range(B):
                        again.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5)
                    again.enable_graph()
                    p50, p99 = time_ticks(again, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec["gate_off_again_tick_p50_ms"], rec["gate_off_again_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    del again
                if args.crossfade:
                    xc = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, crossfade=True)
                    for s in range(B):
                        xc.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, crossfade_ms=10.0)
                    xc.enable_graph()
                    p50, p99 = time_ticks(xc, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec["crossfade_tick_p50_ms"], rec["crossfade_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    db = np.array(xc.seam_db())
                    assert np.isfinite(db).all() and xc.captures == 1, (db, xc.captures)
                    rec["crossfade_seam_db_min"], rec["crossfade_seam_db_median"], rec["crossfade_seam_db_max"] = (
                        round(float(db.min()), 2), round(float(np.median(db)), 2), round(float(db.max()), 2))
                    del xc
                    again = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4)
                    for s in range(B):
                        again.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5)
                    again.enable_graph()
                    p50, p99 = time_ticks(again, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec["crossfade_off_again_tick_p50_ms"], rec["crossfade_off_again_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    del again
                if args.limit:
                    lc = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, limiter=True)
                    for s in range(B):
                        lc.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, limit_db=-12.0)
                    lc.enable_graph()
                    p50, p99 = time_ticks(lc, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec["limit_tick_p50_ms"], rec["limit_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    db = np.array(lc.limit_db())
                    assert not np.isnan(db).any() and lc.captures == 1, (db, lc.captures)
                    rec["limit_db_min"], rec["limit_db_median"], rec["limit_db_max"] = (
                        round(float(db.min()), 2), round(float(np.median(db)), 2), round(float(db.max()), 2))
                    del lc
                    again = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4)
                    for s in range(B):
                        again.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5)
                    again.enable_graph()
                    p50, p99 = time_ticks(again, B, chunk, args.ticks, args.warmup + bs + 1, 300)
                    rec["limit_off_again_tick_p50_ms"], rec["limit_off_again_tick_p99_ms"] = round(p50, 3), round(p99, 3)
                    del again
                if args.envelope:
                    both = {}
                    for name, kw, sess in (("envelope_off", {}, {}), ("envelope", dict(envelope=True), dict(envelope=1.0))):
                        c = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, **kw)
                        for s in range(B):
                            c.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, **sess)
                        c.enable_graph()
                        both[name] = c
                    times = {name: [] for name in both}
                    for _ in range(5):                         # alternating rounds in the one process
                        for name, c in both.items():
                            times[name].append(time_ticks(c, B, chunk, args.ticks, args.warmup + bs + 1, 300))
                    for name, ts in times.items():
                        rec[f"{name}_tick_p50_ms"] = round(float(np.median([t[0] for t in ts])), 3)
                        rec[f"{name}_tick_p99_ms"] = round(float(np.median([t[1] for t in ts])), 3)
                        rec[f"{name}_tick_p50_rounds_ms"] = [round(t[0], 3) for t in ts]
                    ec = both["envelope"]
                    db = np.array(ec.envelope_db())
                    assert np.isfinite(db).all() and ec.captures == 1, (db, ec.captures)
                    rec["envelope_db_min"], rec["envelope_db_max"] = round(float(db[:, 0].min()), 2), round(float(db[:, 1].max()), 2)
                    ld = ec._env_out.shape[1]
                    g = torch.Generator(device="cuda").manual_seed(5)
                    y, x = (torch.randn(B, ld, device="cuda", generator=g) * 0.1 for _ in range(2))
                    for _ in range(10):
                        ec._follow(y, x)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(200):
                        ec._follow(y, x)
                    b.record()
                    torch.cuda.synchronize()
                    rec["envelope_call_us"] = round(a.elapsed_time(b) * 1e3 / 200, 2)
                    rec["envelope_call_bytes"] = 12 * B * ld
                    del both, ec
                if args.post_filter:
                    both = {}
                    for name, kw, sess in (("post_filter_off", {}, {}), ("post_filter", dict(post_filter=True), dict(post_filter=0.8))):
                        c = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, **kw)
                        for s in range(B):
                            c.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, **sess)
                        c.enable_graph()
                        both[name] = c
                    times = {name: [] for name in both}
                    for _ in range(5):                         # alternating rounds in the one process
                        for name, c in both.items():
                            times[name].append(time_ticks(c, B, chunk, args.ticks, args.warmup + bs + 1, 300))
                    for name, ts in times.items():
                        rec[f"{name}_tick_p50_ms"] = round(float(np.median([t[0] for t in ts])), 3)
                        rec[f"{name}_tick_p99_ms"] = round(float(np.median([t[1] for t in ts])), 3)
                        rec[f"{name}_tick_p50_rounds_ms"] = [round(t[0], 3) for t in ts]
                    pc = both["post_filter"]
                    db = np.array(pc.post_filter_db())
                    assert np.isfinite(db).all() and pc.captures == 1, (db, pc.captures)
                    rec["post_filter_db_min"], rec["post_filter_db_max"] = round(float(db[:, 0].min()), 2), round(float(db[:, 1].max()), 2)
                    ld = pc._pf_out.shape[1]
                    g = torch.Generator(device="cuda").manual_seed(5)
                    y = torch.randn(B, ld, device="cuda", generator=g) * 0.1
                    for _ in range(10):
                        pc._postfilter(y)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(200):
                        pc._postfilter(y)
                    b.record()
                    torch.cuda.synchronize()
                    rec["post_filter_call_us"] = round(a.elapsed_time(b) * 1e3 / 200, 2)
                    rec["post_filter_call_samples"] = B * ld
                    del both, pc
                if args.loudness:
                    both = {}
                    for name, kw, sess in (("loudness_off", {}, {}), ("loudness", dict(loudness=True), dict(lufs=-23.0))):
                        c = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, **kw)
                        for s in range(B):
                            c.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, **sess)
                        c.enable_graph()
                        both[name] = c
                    times = {name: [] for name in both}
                    for _ in range(5):                         # alternating rounds in the one process
                        for name, c in both.items():
                            times[name].append(time_ticks(c, B, chunk, args.ticks, args.warmup + bs + 1, 300))
                    for name, ts in times.items():
                        rec[f"{name}_tick_p50_ms"] = round(float(np.median([t[0] for t in ts])), 3)
                        rec[f"{name}_tick_p99_ms"] = round(float(np.median([t[1] for t in ts])), 3)
                        rec[f"{name}_tick_p50_rounds_ms"] = [round(t[0], 3) for t in ts]
                    lc = both["loudness"]
                    read = lc.loudness()
                    assert lc.captures == 1 and all(np.isfinite(g) for _, g in read), (read, lc.captures)
                    rec["loudness_gain_db_min"], rec["loudness_gain_db_max"] = (round(min(g for _, g in read), 2),
                                                                                round(max(g for _, g in read), 2))
                    lo, ln = lc._span(chunk)
                    y = torch.randn(B, lo + ln + 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 0.1
                    emit = torch.ones(B, dtype=torch.bool, device="cuda")
                    state = lc.loud_state.clone()
                    rec["loudness_call_us"] = round(time_calls(lambda: MS.loudness_rows_(y, lc.span_lo, lc.span_len, emit, lc.loud_on,
                                                                                        lc.loud_hop, lc.loud_coef, lc.loud_par, state)), 2)
                    rec["loudness_span"] = ln
                    del both, lc
                if args.pitch_track:
                    three = {}
                    for name, kw, sess in (("track_off", {}, {}), ("track_none", dict(pitch_track=True), {}),
                                           ("track_all", dict(pitch_track=True), dict(pitch_track=True))):
                        c = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, **kw)
                        for s in range(B):
                            c.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, **sess)
                        c.enable_graph()
                        three[name] = c
                    times = {name: [] for name in three}
                    for _ in range(5):                         # alternating rounds in the one process
                        for name, c in three.items():
                            times[name].append(time_ticks(c, B, chunk, args.ticks, args.warmup + bs + 1, 300))
                    for name, ts in times.items():
                        rec[f"{name}_tick_p50_ms"] = round(float(np.median([t[0] for t in ts])), 3)
                        rec[f"{name}_tick_p99_ms"] = round(float(np.median([t[1] for t in ts])), 3)
                        rec[f"{name}_tick_p50_rounds_ms"] = [round(t[0], 3) for t in ts]
                    tc = three["track_all"]
                    assert tc.captures == 1 and three["track_none"].pitch_track_changed() == [0] * B
                    rec["track_changed_mean"] = round(float(np.mean(tc.pitch_track_changed())), 2)
                    lg = next(iter(tc._track_bufs.values()))
                    f0 = torch.zeros(B, 1, lg.shape[2], device="cuda")
                    rec["track_frames"], rec["track_states"] = int(lg.shape[2]), tc._track.states
                    rec["track_call_us"] = round(time_calls(lambda: tc._track.rows(lg, f0, tc.track_on, tc.track_weight, tc.track_jump)), 2)
                    del three, tc
                if args.voicing:
                    three = {}
                    for name, kw, sess in (("voicing_off", {}, {}), ("voicing_none", dict(voicing=True), {}),
                                           ("voicing_all", dict(voicing=True), dict(voicing=True))):
                        c = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, **kw)
                        for s in range(B):
                            c.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, **sess)
                        c.enable_graph()
                        three[name] = c
                    times = {name: [] for name in three}
                    for _ in range(5):                         # alternating rounds in the one process
                        for name, c in three.items():
                            times[name].append(time_ticks(c, B, chunk, args.ticks, args.warmup + bs + 1, 300))
                    for name, ts in times.items():
                        rec[f"{name}_tick_p50_ms"] = round(float(np.median([t[0] for t in ts])), 3)
                        rec[f"{name}_tick_p99_ms"] = round(float(np.median([t[1] for t in ts])), 3)
                        rec[f"{name}_tick_p50_rounds_ms"] = [round(t[0], 3) for t in ts]
                    vc = three["voicing_all"]
                    assert vc.captures == 1 and three["voicing_none"].voicing_state() == [(0, 0, 0.0)] * B
                    rec["voicing_changed_mean"] = round(float(np.mean([st[1] for st in vc.voicing_state()])), 2)
                    x = torch.from_numpy(vc.ring.astype(np.float32) / 32768.0).cuda() if not vc.sparse else None
                    f0 = torch.full((B, 1, vc.frames), 120.0, device="cuda")
                    rec["voicing_frames"] = vc.frames
                    rec["voicing_call_us"] = round(time_calls(lambda: MS.ops.voicing_rows_(f0, x, vc._voicing, vc.voicing_on, vc.voicing_thr_on,
                                                                                       vc.voicing_thr_off, vc.voicing_floor_e)), 2)
                    del three, vc
                if args.match_path:
                    three = {}
                    for name, kw, sess in (("path_off", {}, {}), ("path_none", dict(match_path=True), {}),
                                           ("path_all", dict(match_path=True), dict(match_path=True))):
                        c = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4, **kw)
                        for s in range(B):
                            c.open(s, "v0" if mix == "shared" else f"v{s}", pitch=float(s % 5), f0_rate=0.5, **sess)
                        c.enable_graph()
                        three[name] = c
                    times = {name: [] for name in three}
                    for _ in range(5):                         # alternating rounds in the one process
                        for name, c in three.items():
                            times[name].append(time_ticks(c, B, chunk, args.ticks, args.warmup + bs + 1, 300))
                    for name, ts in times.items():
                        rec[f"{name}_tick_p50_ms"] = round(float(np.median([t[0] for t in ts])), 3)
                        rec[f"{name}_tick_p99_ms"] = round(float(np.median([t[1] for t in ts])), 3)
                        rec[f"{name}_tick_p50_rounds_ms"] = [round(t[0], 3) for t in ts]
                    pc = three["path_all"]
                    assert pc.captures == 1 and three["path_none"].path_moved() == [0] * B
                    rec["path_moved_mean"] = round(float(np.mean(pc.path_moved())), 2)
                    rec["path_frames"] = pc.frames
                    for kk in (4, 8):
                        rec[f"path_call_k{kk}_us"] = round(path_call_us(B, pc.frames, kk, pool.rows, pool.norms), 2)
                    del three, pc
                rec.update(search_ms=round(ms, 4), search_bytes=nbytes, search_GBps=round(nbytes / ms / 1e6, 1))
                print(json.dumps(rec), flush=True)
                rows.append(rec)
                del conv
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
