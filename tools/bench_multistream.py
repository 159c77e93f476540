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
only.  Profile in a separate run (rocprofv3 --kernel-trace --stats --
python tools/bench_multistream.py --quick).  Prints one JSON line per configuration and writes the list to --out.

    python tools/bench_multistream.py [--batches 1,8,32,64,128] [--ticks 40] [--warmup 6] [--rates 8000,16000,44100,48000]
                                      [--world off,0,0.5,1] [--voices shared,distinct] [--blend] [--out multistream.json]
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


def time_ticks(conv, B, chunk, ticks, warmup, seed):
    """chunk: one length, or a list of per-slot lengths (sessions at their own rates)"""
    cs = list(chunk) if isinstance(chunk, (list, tuple)) else [chunk] * B
    pcm = [(synthetic.make_waveform(cs[s] * 4, seed + s)[0].numpy() * 12000).astype(np.int16) for s in range(B)]
    ts = []
    for t in range(warmup + ticks):
        feed = {s: pcm[s][(t % 4) * cs[s]:(t % 4 + 1) * cs[s]] for s in range(B)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        conv.step(feed)
        torch.cuda.synchronize()
        if t >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.percentile(ts, 50)), float(np.percentile(ts, 99))


def time_search(conv, B, reps=20):
    """the grouped search alone on the tick's shape: (ms per call, bytes of distinct segments read once)"""
    src = torch.randn(B, 768, conv.frames, device="cuda")
    for _ in range(3):
        MS.knn_search_grouped(src, conv.pool.rows, conv.pool.norms, conv.seg_lo, conv.seg_len, conv.k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        MS.knn_search_grouped(src, conv.pool.rows, conv.pool.norms, conv.seg_lo, conv.seg_len, conv.k)
    b.record()
    torch.cuda.synchronize()
    segs = {(int(lo), int(ln)) for lo, ln in zip(conv.seg_lo.tolist(), conv.seg_len.tolist()) if ln > 0}
    return a.elapsed_time(b) / reps, sum(ln for _, ln in segs) * (768 + 1) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32,64,128")
    ap.add_argument("--configs", default="160x16,960x8")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--quick", action="store_true", help="B = 64 at -c 160 -b 16, distinct voices, graph only (profiler runs)")
    ap.add_argument("--rates", default=None, help="comma-separated session rates: also time a batch spread over them")
    ap.add_argument("--world", default=None, help="comma-separated WORLD settings: off, or the fraction of sessions on WORLD")
    ap.add_argument("--voices", default="shared,distinct", help="voice mixes to run: shared, distinct")
    ap.add_argument("--blend", action="store_true", help="also time voice blending (blend=3 single voices, 2- and 3-voice blends)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
    rates = [int(r) for r in args.rates.split(",")] if args.rates else None
    mixes = tuple(args.voices.split(","))
    worlds = args.world.split(",") if args.world else []
    if args.quick:
        batches, configs, mixes = [64], [(160, 16)], ("distinct",)
    nets = (ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2))
    shared = make_pool(1, 1)
    distinct = make_pool(max(batches) + (2 if args.blend else 0), 2)
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
