"""Voice codebooks (module/codebook.py), measured: what a build costs, what the update kernel reads per second, what a codebook buys a
streaming tick, and how far a codebook's match is from the full bank's on the data a machine without trained weights has.

  build      build_codebook of 50 000 -> 4 096 and 1 000 000 -> 65 536 rows, 10 iterations, on device-generated tokens with a shared
             component (randn + 1.0 * one fixed direction: synthetic.make_library's generator takes minutes on the host at 1 M rows);
             seconds per iteration split into search / index / update (each bracketed by device synchronisation).
  update     alive_codebook_update alone, event-timed over repeated calls, on the last assignment of each build (skewed lists, as
             k-means leaves them) and on even lists (row m in list m % C): rows' bytes (M x 3 072) over time.  The 154 MB of the
             50 000-row voice fit the Infinity Cache, the 3 GB of the 1 M-row one do not.
  tick       B = 64 sessions on distinct voices at -c 160 -b 16, k = 4 (tools/bench_multistream.py's harness): the grouped search and
             the graph tick on 50 000-row voices and on 4 096-row codebooks of them, two runs each, alternated, in one process.
  fidelity   2 048 content-encoder frames of synthetic audio against a bank of 50 000 content-encoder frames of other synthetic audio
             (the encoder at its seeded initialisation: NOT trained weights): the cosine between match_features on the full bank at
             k = 4 and on a codebook of 512 / 4 096 / 16 384 rows at k = 1 and k = 2, mean and 5th percentile.  These figures say
             nothing about conversion quality on real voices, which is not measured.

    python tools/bench_codebook.py [--only build,tick,fidelity,large] [--out profiles/codebook_bench.json]
("build" is the 50 000-row build with its update timings, "large" the 1 000 000-row one, run last.)  Prints one JSON line per record
and rewrites --out after every section."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bench_multistream as BM                  # noqa: E402
from module import codebook as CB               # noqa: E402
from module import multistream as MS            # noqa: E402
from module.common import match_features        # noqa: E402
from module.content_encoder import ContentEncoder   # noqa: E402
from module.decoder import Decoder              # noqa: E402
from module.f0_estimator import F0Estimator     # noqa: E402
from module.spectrogram import spectrogram      # noqa: E402

ROW_BYTES = 768 * 4


def dense_tokens(m, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shared = torch.randn(768, 1, device="cuda", generator=g)
    t = torch.randn(768, m, device="cuda", generator=g)
    t += shared
    return t


def time_update(rows, assign, size, reps=10):
    """ms per alive_codebook_update call (events around `reps` calls after 2 warm-up calls) and the lists' min / median / max"""
    order, seg_off, counts = CB.inverted_index(assign, size)
    cent = torch.zeros(size, 768, device="cuda")
    for _ in range(2):
        CB.update_centroids(rows, order, seg_off, cent)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        CB.update_centroids(rows, order, seg_off, cent)
    b.record()
    torch.cuda.synchronize()
    c = counts.cpu()
    return a.elapsed_time(b) / reps, [int(c.min()), float(c.median()), int(c.max())]


def build_and_update(m, size, iters=10):
    tok = dense_tokens(m, 17 + size)
    CB.build_codebook(tok[:, :max(size + 1, m // 16)], size // 16 + 1, iters=2)       # warm-up: code objects, workspaces
    st = {}
    book = CB.build_codebook(tok, size, iters=iters, stats=st)
    n = st["iterations"]
    rec = {"what": "build", "rows": m, "size": size, "iterations": n, "converged": st["converged"],
           "search_s_per_iteration": round(st["search_s"] / n, 5),
           "index_s_per_iteration": round(st["index_s"] / max(n - st["converged"], 1), 5),       # (no update after the assignment that converged)
           "update_s_per_iteration": round(st["update_s"] / max(n - st["converged"], 1), 5),
           "build_s": round(st["search_s"] + st["index_s"] + st["update_s"], 4), "moved": st["moved"],
           "mean_best_cosine_first_last": [round(st["objective"][0] / m, 4), round(st["objective"][-1] / m, 4)],
           "empty_clusters": st["empty_clusters"], "list_min_median_max": [st["list_min"], st["list_median"], st["list_max"]]}
    print(json.dumps(rec), flush=True)
    rows = tok.t().contiguous()
    assign = torch.empty(m, dtype=torch.int32, device="cuda")
    val = torch.empty(m, device="cuda")
    CB.assign_rows(tok, book.t().contiguous(), assign, val)
    recs = [rec]
    for lists, a in (("k-means", assign), ("even", (torch.arange(m, device="cuda") % size).to(torch.int32))):
        ms, lens = time_update(rows, a, size)
        r = {"what": "update", "rows": m, "size": size, "lists": lists, "list_min_median_max": lens, "update_ms": round(ms, 4),
             "row_bytes_read": m * ROW_BYTES, "TB_per_s": round(m * ROW_BYTES / ms / 1e9, 3),
             "rows_fit_infinity_cache": m * ROW_BYTES < 256 * 2 ** 20}
        print(json.dumps(r), flush=True)
        recs.append(r)
    return recs


def tick_leg(B=64, chunk=160, bs=16, rows=BM.VOICE_ROWS, size=4096, ticks=40, warmup=6):
    nets = (ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2))
    full = BM.make_pool(B, 2)
    books = MS.VoicePool({name: CB.build_codebook(full.tokens(name), size, iters=2) for name in full.segments})
    recs = []
    for run in range(2):
        for what, pool in (("full", full), ("codebook", books)):
            conv = MS.MultiStreamConverter(*nets, pool, B, chunk=chunk, buffersize=bs, k=4)
            for s in range(B):
                conv.open(s, f"v{s}", pitch=float(s % 5), f0_rate=0.5)
            conv.enable_graph()
            p50, p99 = BM.time_ticks(conv, B, chunk, ticks, warmup + bs + 1, 300)
            ms, nbytes = BM.time_search(conv, B)
            r = {"what": "tick", "run": run, "voices": what, "B": B, "chunk": chunk, "buffersize": bs, "k": 4,
                 "voice_rows": pool.segment("v0")[1], "graph_tick_p50_ms": round(p50, 3), "graph_tick_p99_ms": round(p99, 3),
                 "search_ms": round(ms, 4), "search_bytes": nbytes, "pool_MB": round(pool.rows.numel() * 4 / 2 ** 20, 1)}
            print(json.dumps(r), flush=True)
            recs.append(r)
            del conv
    return recs


def ce_frames(ce, n, seed, L=144000):
    """n content-encoder frames of synthetic audio on the device: noise plus a harmonic stack on a gliding fundamental per signal"""
    lf = L // 320
    sigs = (n + lf - 1) // lf
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(768, sigs * lf, device="cuda")
    t = torch.arange(L, device="cuda", dtype=torch.float32) / 16000.0
    for i in range(0, sigs, 64):
        b = min(64, sigs - i)
        f0 = 80.0 + 320.0 * torch.rand(b, 1, device="cuda", generator=g)
        glide = 1.0 + 0.2 * torch.sin(2 * np.pi * (0.3 + torch.rand(b, 1, device="cuda", generator=g)) * t[None])
        phase = 2 * np.pi * torch.cumsum(f0 * glide / 16000.0, dim=1)
        sig = 0.02 * torch.randn(b, L, device="cuda", generator=g)
        for h in range(1, 9):
            sig += (0.3 / h) * torch.sin(h * phase + float(h))
        env = 0.55 + 0.45 * torch.sin(2 * np.pi * (2.0 + 3.0 * torch.rand(b, 1, device="cuda", generator=g)) * t[None])
        feat = ce(spectrogram((sig * env).contiguous()))
        out[:, i * lf:(i + b) * lf] = feat.permute(1, 0, 2).reshape(768, -1)
    return out[:, :n].contiguous()


def fidelity_leg(bank_rows=50000, frames=2048, sizes=(512, 4096, 16384)):
    ce = ContentEncoder(seed=2).to("cuda")
    bank = ce_frames(ce, bank_rows, 900)
    query = ce_frames(ce, frames, 901)[None].contiguous()
    ref = match_features(query, bank[None], k=4)
    recs = []
    for size in sizes:
        st = {}
        book = CB.build_codebook(bank, size, iters=10, stats=st)
        for k in (1, 2):
            cos = torch.nn.functional.cosine_similarity(ref[0].double(), match_features(query, book[None], k=k)[0].double(), dim=0)
            r = {"what": "fidelity", "bank_rows": bank_rows, "frames": frames, "size": size, "k": k, "full_bank_k": 4,
                 "cosine_mean": round(float(cos.mean()), 5), "cosine_p5": round(float(torch.quantile(cos, 0.05)), 5),
                 "iterations": st["iterations"], "empty_clusters": st["empty_clusters"],
                 "data": "content-encoder frames of synthetic audio, seeded initialisation (no trained weights)"}
            print(json.dumps(r), flush=True)
            recs.append(r)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="build,tick,fidelity,large")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_codebook needs an MI355X: nothing here can be measured on a CPU")
    legs = args.only.split(",")
    recs = []

    def keep(new):
        recs.extend(new)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(recs, open(args.out, "w"), indent=1)

    if "build" in legs:
        keep(build_and_update(50000, 4096))
    if "tick" in legs:
        keep(tick_leg())
        torch.cuda.empty_cache()
    if "fidelity" in legs:
        keep(fidelity_leg())
        torch.cuda.empty_cache()
    if "large" in legs:
        keep(build_and_update(1000000, 65536))


if __name__ == "__main__":
    main()
