"""Voice codebooks: a voice of M rows condensed to `size` centroid rows by k-means (tools/codebook_ref.py is the float64 restatement).

Every cost of a voice grows with its row count: the grouped search of a streaming tick reads every fp32 row of every voice in use,
and a reserved pool holds 3 KB per row.  A codebook is the voice "in N rows": the centroids of a k-means over its rows, stored as
the voice.  match_features emits the mean of raw library rows; a centroid is such a mean, taken over a cluster instead of over k
neighbours, so sessions on a codebook want k = 1 or 2.

One iteration: the assignment of every row is the library's own deterministic search (PackedLibrary(centroids, strict=True), k = 1,
in chunks of 65536 rows; the centroids are repacked every iteration, cheap at `size` rows); alive_codebook_stats sums the best
cosines and counts the rows that changed cluster (the one host read of the iteration; 0 ends the loop); a stable torch.sort of
the assignment gives the inverted index (pack-time plumbing, as PackedLibrary._try_rotated's torch use); alive_codebook_update
forms every centroid as the mean of its raw fp32 member rows in fp64, in a fixed order and without float atomics.  A cluster that
lost all its members keeps its row.  The result is bitwise the same for the same arguments on the same build.

What a codebook does to conversion quality on trained checkpoints and real voices is NOT measured: DESIGN.md 5.6 gives fidelity
figures on synthetic data only.  A pack-time operation (it reads the device once per iteration): never call it inside a tick.
"""
import random
import time

import torch

from . import _native as nat
from .common import DIM, PackedLibrary

SEARCH_CHUNK = 65536
_ws = nat.Workspace()


def _tokens_2d(tokens):
    t = tokens
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"build_codebook: tokens must be a tensor, got {type(tokens).__name__}")
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2 or t.shape[0] != DIM:
        raise ValueError(f"build_codebook: a voice must be [768, M] or [1, 768, M], got {tuple(tokens.shape)}")
    return t


def check_size(size, what="codebook"):
    """a codebook size: an integer >= 1 (not a bool); ValueError otherwise"""
    if isinstance(size, bool) or not isinstance(size, int) or size < 1:
        raise ValueError(f"{what} must be an integer >= 1, got {size!r}")
    return size


def check_init(init, size, m):
    """`size` distinct row indices in [0, m) -> list of ints; ValueError otherwise (host logic, no device)"""
    try:
        idx = [int(i) for i in init]
        exact = all(int(i) == i for i in init)
    except (TypeError, ValueError):
        raise ValueError(f"build_codebook: init must be {size} row indices, got {init!r}") from None
    if not exact or len(idx) != size:
        raise ValueError(f"build_codebook: init must be {size} integer row indices, got {len(idx)}")
    if min(idx) < 0 or max(idx) >= m:
        raise ValueError(f"build_codebook: init row outside [0, {m})")
    if len(set(idx)) != size:
        raise ValueError("build_codebook: init holds a row twice")
    return idx


def assign_rows(tokens_DxM, centroid_rows, assign, val):
    """assign[m] / val[m] <- the centroid of highest cosine of row m and that cosine: the strict search's top-1 (ties to the lower
    centroid) of the tokens against a library of the centroids, in chunks"""
    lib = PackedLibrary(centroid_rows.t().contiguous(), strict=True)
    m = tokens_DxM.shape[1]
    for s in range(0, m, SEARCH_CHUNK):
        v, i = lib.search(tokens_DxM[:, s:s + SEARCH_CHUNK].unsqueeze(0).contiguous(), 1)
        val[s:s + SEARCH_CHUNK] = v[:, 0]
        assign[s:s + SEARCH_CHUNK] = i[:, 0]


def inverted_index(assign, size):
    """assign int32 [M] -> (order int32 [M]: the rows of cluster 0, then 1, ..., each in ascending row index; seg_off int32
    [size + 1]; counts int64 [size]) with a stable sort: unique, hence bitwise the same run to run"""
    order = torch.sort(assign, stable=True)[1].to(torch.int32)
    counts = torch.bincount(assign, minlength=size)
    seg_off = torch.zeros(size + 1, dtype=torch.int32, device=assign.device)
    seg_off[1:] = torch.cumsum(counts, 0)
    return order, seg_off, counts


def update_centroids(rows, order, seg_off, centroids):
    """alive_codebook_update in place on centroids [C, 768]: every non-empty list's mean of rows[order[...]]"""
    L = nat.lib()
    m, c = int(rows.shape[0]), int(centroids.shape[0])
    ws = _ws.get(L.alive_codebook_workspace_bytes(m, c), rows.device)
    nat.check(L.alive_codebook_update(nat.ptr(rows), m, DIM, nat.ptr(order), nat.ptr(seg_off), c, nat.ptr(centroids), nat.ptr(ws),
                                      nat.stream()), "alive_codebook_update")


def codebook_stats(assign, prev, val, out):
    """out (16 device bytes) <- (objective float64, moved int64) of alive_codebook_stats; prev None: every row counts as moved"""
    nat.check(nat.lib().alive_codebook_stats(nat.ptr(assign), nat.ptr(prev), nat.ptr(val), int(assign.shape[0]), out.data_ptr(),
                                             out.data_ptr() + 8, nat.stream()), "alive_codebook_stats")


def build_codebook(tokens, size, iters=10, seed=0, init=None, stats=None):
    """tokens [768, M] or [1, 768, M] on the device -> codebook [768, size] float32 on the device: `iters` k-means iterations at
    most from the rows `init` (size distinct row indices; default random.Random(seed).sample(range(M), size)), stopping early when
    an assignment moves no row.  size >= M returns the tokens unchanged.  stats, a dict, receives per-iteration "objective" and
    "moved", "iterations", "converged", "empty_clusters", "list_min" / "list_median" / "list_max" (of the last assignment) and the
    seconds spent in "search_s", "index_s" and "update_s" (it makes the phases wait for the device, to time them).
    ValueError: size < 1, iters < 1, a bad init, a CPU tensor or a wrong shape."""
    size = check_size(size, "build_codebook: size")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"build_codebook: iters must be an integer >= 1, got {iters!r}")
    t = _tokens_2d(tokens)
    if not t.is_cuda:
        raise ValueError("build_codebook: tokens must be on the device (got a CPU tensor)")
    m = int(t.shape[1])
    if init is not None:
        init = check_init(init, size, m) if size < m else None
    if size >= m:
        return t
    if init is None:
        init = random.Random(seed).sample(range(m), size)
    dev = t.device
    t = t.float().contiguous()
    rows = torch.empty(m, DIM, dtype=torch.float32, device=dev)
    norms = torch.empty(m, dtype=torch.float32, device=dev)
    nat.check(nat.lib().alive_library_pack_rows(nat.ptr(t), m, DIM, nat.ptr(rows), nat.ptr(norms), nat.stream()),
              "alive_library_pack_rows")
    centroids = rows.index_select(0, torch.tensor(init, dtype=torch.int64, device=dev)).contiguous()
    assign = torch.empty(m, dtype=torch.int32, device=dev)
    prev = torch.empty(m, dtype=torch.int32, device=dev)
    val = torch.empty(m, dtype=torch.float32, device=dev)
    out = torch.zeros(16, dtype=torch.uint8, device=dev)
    objective, moves, converged = [], [], False
    secs = {"search_s": 0.0, "index_s": 0.0, "update_s": 0.0}

    def timed(key, fn):
        if stats is None:
            return fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        secs[key] += time.perf_counter() - t0
        return r

    for it in range(iters):
        timed("search_s", lambda: assign_rows(t, centroids, assign, val))
        codebook_stats(assign, prev if it else None, val, out)
        host = out.cpu()                                          # the iteration's one host read
        objective.append(float(host[:8].view(torch.float64)[0]))
        moves.append(int(host[8:].view(torch.int64)[0]))
        if moves[-1] == 0:
            converged = True
            break
        order, seg_off, _ = timed("index_s", lambda: inverted_index(assign, size))
        timed("update_s", lambda: update_centroids(rows, order, seg_off, centroids))
        assign, prev = prev, assign
    if stats is not None:
        last = prev if not converged else assign                  # (the buffers were swapped after the last update)
        counts = torch.bincount(last, minlength=size).cpu()
        stats.update(objective=objective, moved=moves, iterations=len(moves), converged=converged,
                     empty_clusters=int((counts == 0).sum()), list_min=int(counts.min()), list_median=float(counts.median()),
                     list_max=int(counts.max()), **{k: round(v, 6) for k, v in secs.items()})
    return centroids.t().contiguous()
