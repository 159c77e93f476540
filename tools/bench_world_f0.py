"""WORLD pitch (`-wpe`) timings: device compute_f0 on 1 / 64 / 384 offline windows of 144 000 samples beside the float64
restatement's CPU time per window, and the streaming step p50 / p99 with and without world_pitch.  One JSON line per result.

  python tools/bench_world_f0.py [--reps 20] [--stream-steps 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")]


def signal(n, L, seed=0):
    rs = np.random.RandomState(seed)
    t = np.arange(L) / 16000.0
    ph = 2 * np.pi * np.cumsum(rs.uniform(90, 300, (n, 1)) * (1 + 0.04 * np.sin(2 * np.pi * 5 * t)), axis=1) / 16000.0
    return torch.from_numpy(sum(0.3 / k * np.sin(k * ph) for k in range(1, 9)).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stream-steps", type=int, default=200)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from module.common import compute_f0
    for n in (1, 64, 384):
        wf = signal(n, 144000).cuda()
        for _ in range(2):
            compute_f0(wf)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            compute_f0(wf)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        print(json.dumps({"bench": "compute_f0", "windows": n, "ms_p50": float(np.median(ts)), "ms_min": float(min(ts))}))
    if not a.no_cpu:
        import world_ref as W
        from module import audio_io
        x8 = audio_io.resample(signal(1, 144000).cuda(), 16000, 8000).cpu().numpy()
        t0 = time.perf_counter()
        W.dio_stonemask_rows(x8, 8000)
        print(json.dumps({"bench": "restatement_cpu", "windows": 1, "ms": (time.perf_counter() - t0) * 1e3}))
    from module import schema, synthetic   # noqa: F401
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(1000, 1)
    for chunk, bs in ((960, 8), (160, 16)):
        for wpe in (False, True):
            rt = RealtimeConverter(ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2), lib, "cuda", chunk=chunk,
                                   buffersize=bs, world_pitch=wpe, reuse_interior=False).enable_graph()
            pcm = (signal(1, chunk * (bs + a.stream_steps + 10))[0].numpy() * 20000).astype(np.int16)
            ts = []
            for s in range(bs + a.stream_steps + 10):
                t0 = time.perf_counter()
                rt.step(pcm[s * chunk:(s + 1) * chunk])
                if s >= bs + 10:
                    ts.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"bench": "stream_step", "chunk": chunk, "buffersize": bs, "world_pitch": wpe,
                              "ms_p50": float(np.percentile(ts, 50)), "ms_p99": float(np.percentile(ts, 99))}))


if __name__ == "__main__":
    main()
