"""NumPy restatement of the match path (csrc/match_path.hip; include/alive_vc.h "Match path"): the CPU yardstick of alive_knn_path_rows,
as tools/pitch_track_ref.py is the pitch tracker's.

Out of each frame's K candidates of a top-k list, one library row per frame, so that the sequence of chosen rows is close to the source
(target cost: the candidate's cosine below the frame's best one) and continuous in the library's own feature space (join cost: the
cosine between consecutive chosen rows, times a weight).  One list row: T frames, val[t][i] float32 / idx[t][i] int32 with i < k_max,
best first, K = k_row of them in use; rows float32 [P][768], norms float32 [P]; weight w >= 0.  Everything is float64 with every
operation rounded on its own.
    active frame    idx[t][0] >= 0 and no idx[t][i] >= P among i < K (an index outside the table is never dereferenced: its frame is
                    treated as a frame without a match)
    state i         exists when the frame is active, i < K and idx[t][i] >= 0
    e[t][i]         (double) val[t][i] - (double) val[t][0]
    c[t][i][j]      dot(a, b) / ((double) norms[a] * (double) norms[b]),  a = idx[t][i], b = idx[t - 1][j], for existing states of two
                    consecutive active frames.  dot: lane l of 64 sums (double) x[l + 64 q] * (double) y[l + 64 q] over q = 0 .. 11 in
                    ascending order from 0.0, then p[l] = p[l] + p[l + o] for o = 32, 16, .., 1 (a product of two floats is exact in
                    double: fusing the multiply and the add changes nothing)
    D[t][i]         e[t][i] at t = 0 and after an inactive frame (a new segment), else
                    e[t][i] + max_j (D[t - 1][j] + w * c[t][i][j]) over the existing j, the lowest j on ties: back[t][i]
    traceback       a segment ends at T - 1 or before an inactive frame: its end takes the lowest i attaining max D, before that
                    p[t - 1] = back[t][p[t]]
(in both maxima a NaN candidate counts as -inf, so that the choice is defined whatever the lists hold.)
    output          lists [T][k_max]: entry 0 is (val[t][p], idx[t][p]), the others (-inf, -1); an inactive frame is all (-inf, -1);
                    moved = the frames with p != 0.  A row that is off (on == 0, or k_row outside [1, k_max]) is copied, moved 0.
w = 0 gives p = 0 everywhere (e <= 0 with e[t][0] = 0, ties to the lowest index): the k = 1 match.
"""
import numpy as np

DIM = 768
WEIGHT = 1.0
MAX_K = 8                                       # ALIVE_KNN_PATH_MAX_K (include/alive_vc.h)
MAX_FRAMES = 1 << 20                            # ALIVE_KNN_PATH_MAX_FRAMES: R * T of one call


def dot64(x, y):
    """the prescribed fp64 dot of two float32 [768] rows"""
    p = (np.asarray(x, dtype=np.float32).astype(np.float64) * np.asarray(y, dtype=np.float32).astype(np.float64)).reshape(DIM // 64, 64)
    s = np.zeros(64)
    for q in range(DIM // 64):
        s = s + p[q]
    o = 32
    while o:
        s = s[:o] + s[o:2 * o]
        o //= 2
    return s[0]


def cosine(a, b, rows, norms):
    return dot64(rows[a], rows[b]) / (float(norms[a]) * float(norms[b]))


def cosine_table(rows, norms):
    """cosine(a, b) of every pair of a small table, float64 [P, P] (join(table=): each pair once however often the lists repeat it)"""
    P = len(norms)
    return np.array([[cosine(a, b, rows, norms) for b in range(P)] for a in range(P)])


def states(idx, K, P):
    """idx int32 [T, k_max] -> exists bool [T, k_max] (a row of it is all False on an inactive frame)"""
    idx = np.asarray(idx)
    T, k_max = idx.shape
    inside = np.arange(k_max)[None, :] < K
    active = (idx[:, 0] >= 0) & ~((idx >= P) & inside).any(axis=1)
    return active[:, None] & inside & (idx >= 0)


def join(idx, K, rows, norms, table=None):
    """(J float64 [T, k_max, k_max], written bool of the same shape): J[t][i][j] = c[t][i][j] where the device writes it"""
    idx = np.asarray(idx)
    T, k_max = idx.shape
    ex = states(idx, K, len(norms))
    J = np.zeros((T, k_max, k_max))
    written = np.zeros((T, k_max, k_max), dtype=bool)
    for t in range(1, T):
        written[t] = ex[t][:, None] & ex[t - 1][None, :]
        for i, j in zip(*np.nonzero(written[t])):
            a, b = idx[t, i], idx[t - 1, j]
            J[t, i, j] = cosine(a, b, rows, norms) if table is None else table[a, b]
    return J, written


def _lowest_argmax(v):
    v = np.where(np.isnan(v), -np.inf, v)
    return int(np.argmax(v)), v                 # (argmax: the lowest index of the maximum)


def path(val, idx, K, rows, norms, weight=WEIGHT, J=None):
    """one list row -> (p int64 [T] with -1 on inactive frames, score: the sum over the segments of D at their ends)"""
    val, idx, w = np.asarray(val, dtype=np.float32), np.asarray(idx), float(weight)
    T, k_max = idx.shape
    ex = states(idx, K, len(norms))
    active = ex[:, 0]
    if J is None:
        J = join(idx, K, rows, norms)[0]
    D = np.full((T, k_max), -np.inf)
    back = np.zeros((T, k_max), dtype=np.int64)
    for t in np.flatnonzero(active):
        e = val[t].astype(np.float64) - float(val[t, 0])
        for i in np.flatnonzero(ex[t]):
            if t == 0 or not active[t - 1]:
                D[t, i] = e[i]
                continue
            cand = np.full(k_max, -np.inf)
            for j in np.flatnonzero(ex[t - 1]):
                cand[j] = D[t - 1, j] + w * J[t, i, j]
            back[t, i], cand = _lowest_argmax(cand)
            D[t, i] = e[i] + cand[back[t, i]]
    p = np.full(T, -1, dtype=np.int64)
    score = 0.0
    for t in range(T - 1, -1, -1):
        if not active[t]:
            continue
        if t == T - 1 or not active[t + 1]:
            p[t] = _lowest_argmax(D[t])[0]
            score += D[t, p[t]]
        else:
            p[t] = back[t + 1, p[t + 1]]
    return p, score


def path_score(p, val, idx, K, rows, norms, weight=WEIGHT, J=None):
    """the score of a given path (p[t] an existing state on every active frame), summed as the recurrence sums it"""
    val, idx, w = np.asarray(val, dtype=np.float32), np.asarray(idx), float(weight)
    ex = states(idx, K, len(norms))
    if J is None:
        J = join(idx, K, rows, norms)[0]
    total, d = 0.0, None
    for t in range(len(p)):
        if not ex[t, 0]:
            if d is not None:
                total += d
            d = None
            continue
        e = float(val[t, p[t]]) - float(val[t, 0])
        d = e if d is None else e + (d + w * J[t, p[t], p[t - 1]])
    return total + (d if d is not None else 0.0)


def select(val, idx, p):
    """the output lists of a path: (val float32 [T, k_max], idx int32 [T, k_max])"""
    val, idx = np.asarray(val, dtype=np.float32), np.asarray(idx, dtype=np.int32)
    ov, oi = np.full(val.shape, -np.inf, dtype=np.float32), np.full(idx.shape, -1, dtype=np.int32)
    for t in np.flatnonzero(np.asarray(p) >= 0):
        ov[t, 0], oi[t, 0] = val[t, p[t]], idx[t, p[t]]
    return ov, oi


def path_rows(val, idx, k_row, on, weight, rows, norms, table=None):
    """alive_knn_path_rows: val / idx [R, T, k_max] -> (out_val, out_idx, moved int32 [R], paths: p per row, None where the row is off)"""
    val, idx = np.asarray(val, dtype=np.float32), np.asarray(idx, dtype=np.int32)
    R, T, k_max = idx.shape
    k_row, on = np.broadcast_to(np.asarray(k_row), (R,)), np.broadcast_to(np.asarray(on), (R,))
    weight = np.broadcast_to(np.asarray(weight, dtype=np.float64), (R,))
    ov, oi, moved, paths = val.copy(), idx.copy(), np.zeros(R, dtype=np.int32), []
    for r in range(R):
        if not on[r] or not (1 <= k_row[r] <= k_max):
            paths.append(None)
            continue
        p, _ = path(val[r], idx[r], int(k_row[r]), rows, norms, weight[r], join(idx[r], int(k_row[r]), rows, norms, table)[0])
        ov[r], oi[r] = select(val[r], idx[r], p)
        moved[r] = int((p > 0).sum())
        paths.append(p)
    return ov, oi, moved, paths


def exact_case(T=12, gap=None):
    """the worked case: a pool of 64 unit basis vectors, K = 2; entry 0 of frame t is row t + 1 at 0.75, entry 1 is row 0 at 0.625, so
    every join is exactly 0 or 1.  gap: a frame without a match.  -> (val [T, 2], idx [T, 2], rows [64, 768], norms [64])"""
    rows = np.eye(DIM, dtype=np.float32)[:64].copy()
    norms = np.ones(64, dtype=np.float32)
    idx = np.stack([np.arange(1, T + 1), np.zeros(T, dtype=np.int64)], axis=1).astype(np.int32)
    val = np.stack([np.full(T, 0.75), np.full(T, 0.625)], axis=1).astype(np.float32)
    if gap is not None:
        idx[gap], val[gap] = -1, -np.inf
    return val, idx, rows, norms
