"""NumPy restatement of the voice codebook (module/codebook.py build_codebook; csrc/codebook.hip; include/alive_vc.h "Voice codebooks"):
k-means over a voice's rows with the centroids stored as the voice.  The CPU yardstick of alive_codebook_update, alive_codebook_stats
and build_codebook, as tools/gate_ref.py is the input gate's.

Everything is float64 except the stored rows and centroids, which are float32.  One iteration:
  assign   row m goes to the centroid of highest cosine -- divide row and centroid by their norms, then dot (the reference's
           arithmetic, module/common.py match_features) -- a tie to the lowest centroid index;
  stop     moved = rows whose assignment differs from the previous iteration's (every row in the first), objective = the sum of
           the rows' best cosines; moved == 0 ends the loop with the centroids that produced this assignment;
  update   centroid c = the mean of the RAW float32 member rows: per column, the members in ascending row index are cut into chunks
           of 512, each chunk is summed sequentially from +0.0, the chunk sums are added sequentially from +0.0 in chunk order, the
           total is divided by the count and rounded to float32 once.  A cluster without members keeps its row bit for bit.
The sums are explicit loops: ndarray.sum is pairwise.
"""
import numpy as np

CHUNK = 512
STATS_THREADS = 1024


def chunked_mean(members):
    """members float32 [n, D] in list order, n >= 1 -> float32 [D]: the update's mean of one list"""
    x = np.asarray(members, dtype=np.float32).astype(np.float64)
    total = np.zeros(x.shape[1], dtype=np.float64)
    for s in range(0, x.shape[0], CHUNK):
        acc = np.zeros(x.shape[1], dtype=np.float64)
        for row in x[s:s + CHUNK]:
            acc = acc + row
        total = total + acc
    return (total / float(x.shape[0])).astype(np.float32)


def update(rows, assign, centroids):
    """rows float32 [M, D], assign int [M], centroids float32 [C, D] -> the new centroids (a copy; empty clusters keep their rows)"""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.array(centroids, dtype=np.float32)
    order = np.argsort(np.asarray(assign), kind="stable")
    counts = np.bincount(np.asarray(assign), minlength=out.shape[0])
    at = 0
    for c, n in enumerate(counts):
        if n:
            out[c] = chunked_mean(rows[order[at:at + n]])
        at += n
    return out


def cosines(rows, centroids, block=4096):
    """float64 [M, C]: (row / |row|) . (centroid / |centroid|)"""
    r = np.asarray(rows, dtype=np.float32).astype(np.float64)
    c = np.asarray(centroids, dtype=np.float32).astype(np.float64)
    r = r / np.sqrt((r * r).sum(1))[:, None]
    c = c / np.sqrt((c * c).sum(1))[:, None]
    return np.concatenate([r[s:s + block] @ c.T for s in range(0, r.shape[0], block)], 0)


def assign_rows(rows, centroids, with_gap=False):
    """-> (assign int64 [M], best cosine float64 [M]) and, with_gap, the best-to-second gap (inf with one centroid); np.argmax
    takes the lowest index among equals"""
    cos = cosines(rows, centroids)
    a = np.argmax(cos, axis=1)
    best = cos[np.arange(cos.shape[0]), a]
    if not with_gap:
        return a, best
    if cos.shape[1] == 1:
        return a, best, np.full(cos.shape[0], np.inf)
    cos[np.arange(cos.shape[0]), a] = -np.inf
    return a, best, best - cos.max(axis=1)


def stats_sum(val):
    """the objective in alive_codebook_stats' order: partial sum t of 1024 adds val[t], val[t + 1024], ... in turn from +0.0, then
    acc[i] += acc[i + o] for o = 512, 256, ..., 1.  val float32 [M] -> float64"""
    v = np.asarray(val, dtype=np.float32).astype(np.float64)
    pad = -v.shape[0] % STATS_THREADS                    # (+ 0.0 leaves a sum that started at +0.0 as it is)
    v = np.concatenate([v, np.zeros(pad)]).reshape(-1, STATS_THREADS)
    acc = np.zeros(STATS_THREADS, dtype=np.float64)
    for j in range(v.shape[0]):
        acc = acc + v[j]
    o = STATS_THREADS // 2
    while o > 0:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o >>= 1
    return float(acc[0])


def moved(assign, prev=None):
    return int(len(assign)) if prev is None else int((np.asarray(assign) != np.asarray(prev)).sum())


def build_codebook(tokens, size, iters=10, init=None, seed=0, stats=None):
    """tokens float32 [768, M] -> codebook float32 [768, size].  init: `size` distinct row indices (default: random.Random(seed)
    .sample(range(M), size), as the device build).  stats, a dict, receives objective / moved per iteration, iterations, converged
    and empty_clusters (of the last assignment)."""
    import random
    tok = np.asarray(tokens, dtype=np.float32)
    rows = np.ascontiguousarray(tok.T)
    m = rows.shape[0]
    if size >= m:
        return tok
    if init is None:
        init = random.Random(seed).sample(range(m), size)
    cent = rows[np.asarray(init, dtype=np.int64)].copy()
    prev, objective, moves, converged, a = None, [], [], False, None
    for _ in range(iters):
        a, best = assign_rows(rows, cent)
        moves.append(moved(a, prev))
        s = 0.0
        for b in best:
            s += float(b)
        objective.append(s)
        if moves[-1] == 0:
            converged = True
            break
        cent = update(rows, a, cent)
        prev = a
    if stats is not None:
        stats.update(objective=objective, moved=moves, iterations=len(moves), converged=converged,
                     empty_clusters=0 if a is None else int((np.bincount(a, minlength=size) == 0).sum()))
    return np.ascontiguousarray(cent.T)
