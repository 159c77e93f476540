"""Cases and model for knn_rescore_kernel (csrc/knn.hip), the kernel every kNN search ends in: exact rescoring of a stage's
candidates, the top-k, the per-frame certificate, the list of failing frames and the threshold handed to the collect tier.  CPU only:
tests/test_host_knn_cert.py proves the promises made here, tests/test_gpu_knn_cert.py runs the cases through
alive_debug_knn_rescore / alive_debug_knn_rescore_pool and compares bits.

THE MODEL (model_frame / model_launch) restates the rule from the kernel's comments and DESIGN.md 3.1a / 3.1d, one frame at a time,
with Python lists and sorts -- nothing of the kernel's lanes, ballots or register arrays:
  floor      candidates are P * kp entries; each aligned group of list_len entries is one partial list whose floor is the minimum over
             ALL its entries -- an empty entry of an unseeded list holds -inf (no floor), an empty entry of a seeded list holds the seed
             with index -1 (the scoring kernels initialise a seeded list as `Lv = seed, Li = -1`); c_cut starts as the largest floor;
  selection  sk / s16 = k-th / 16th largest stage score among entries with index >= 0 (with multiplicity, -inf when there are fewer),
             cut = min(sk - prune, s16); entries at or above the cut are rescored, the others raise c_cut to their stage score; if more
             than 64 reach the cut the best are taken one by one by (score desc, index asc) until 64 are taken or, after at least 16,
             the first one below sk - prune, and what is left raises c_cut; prune = 2 zsig sd_prior / pre_scale (statistical),
             2 det_bound / pre_scale (deterministic), infinite without a certificate;
             det_bound = det_q[frame] + 1.004f * det_lib[voice or 0] + 1.0e-4f;
  score      sum_d s[d] * (row[d] / norm), in float64 (exact on the operands below);
  statistics over the rescored candidates e = pre * pre_scale - score; err_mu = min(mean e, 0), err_sd = max(sqrt(mean e^2), sd_prior),
             err_max = max |e|;
  bound      c_cut * pre_scale - err_mu + max(zsig * err_sd, 2 * err_max), or c_cut * pre_scale + det_bound;
  verdict    a frame is considered iff c_cut > -inf or it is forced; flagged iff !(vk > bound) or forced (pool form: never forced);
  threshold  vk - overflow_slack if overflow_slack > 0, else (vk - (bound - c_cut * pre_scale)) / pre_scale; a collect overflow
             records vk - overflow_slack;
  top-k      descending, ties to the lower library index, (-inf, -1) where fewer than k rows were scored, indices + idx_base, stride =
             the k argument (pool form: each group's own k, stride the call's k);
  collect    no pruning, no certificate; a -2 index is an overflow; the frame's current out_idx entries (minus idx_base, -1 skipped)
             join the candidates without duplicates on free lanes in ascending order, no free lane is an overflow, more than 64
             collected rows are an overflow; an overflowed frame is flagged;
  gates      no gate word: open; else open iff lo < word <= hi; gate_lo == GATE_BOOL: open iff word != 0; with a frame_list only slots
             below the word run; a frame_list entry < 0 is skipped; a closed gate or skipped slot leaves every output byte alone.
Every scalar step of statistics, bound and threshold is ONE correctly rounded fp32 operation in the kernel (the library is built with
-ffp-contract=off, division and sqrtf are IEEE); the model performs them in np.float32 in source order.

OPERANDS ON WHICH THE MODEL IS EXACT -- hence tolerance ZERO on every value, index, verdict and threshold of every case but one:
  scores     frames and rows hold small integers times a power of two, norms are powers of two (1/4 .. 4, most of them not 1): the
             quotient row / norm is exact whatever division is used, every product and every partial sum over the 768 terms is a
             multiple of one unit and sum |s| |row / norm| stays below 2^24 units, so the sum is exact in fp32 in any order and equal to
             the float64 sum.  Two families: `board` cases use one-hot frames (frame f is e_{d_f}), so row m's score for frame f is
             rows[m][d_f] / norm and can be ANY fp32 number, while the other elements of the row hold nonzero fillers that meet only
             zeros; `ramp` cases use frames of small integers (each of -96 .. 95 four times, permuted) against rows that are
             permutations of the ramp -384 .. 383 -- all 768 elements of a row differ, a wrong lane-to-element mapping changes the sum;
  stage      cv = (score + e) / pre_scale with pre_scale a power of two; score and e on a dyadic grid (board: scores multiples of
             2^-12, 2^-16 or, in the clusters, 2^-19, e multiples of 2^-14 with |e| <= 2^-5; ramp: scores multiples of 2^-24 below 1, e
             multiples of 2^-12), so cv, e = cv * pre_scale - score, e^2 and their sums over at most 64 candidates are exact in any
             order.  A candidate pinned to a bound has an arbitrary fp32 score and e = 0.
Only production's parameters: zsig 7; sd_prior 8.0e-5 / 1.5e-3 / 2.0e-3 / 2.5e-4; pre_scale 1, 1 / 32^2, 1 / 256^2; list_len 8 with kp 16
and 16 with kp 32; collect caps (kp) 4 .. 64; overflow_slack 0 or 3.0e-4.  LEFT OUT because no search launches them: force_fail
together with thr_list (the threshold of a forced frame without a floor is NaN), deterministic bounds behind block-scaled stages
(list_len 16), collect with a gate-less frame_list.  One collect case does pass a thr_list (the searches pass none) because the rule
names the value an overflow records.  Stage-score ties between two entries that the SAME lane holds (positions 64 apart) are kept
out of the more-than-64 walk: the kernel takes those in position order, the rule says index order, both leave a valid candidate set.

PINNING.  A verdict far from its bound says little about the bound.  Most certify frames therefore pin their k-th exact score: the
builder runs the model, moves the k-th candidate (e = 0, stage score = score / pre_scale) to the bound / its upper / its lower fp32
neighbour, and repeats until bound and candidate stand still.  The expected verdicts are then: at the bound flagged, one ulp above not
flagged, one ulp below flagged -- a wrong c_cut, statistic, rounding or comparison flips one of them.

THE REALISTIC CASE (realistic()) has inexact sums; its three tolerances:
  values     2e-6 absolute, the tolerance of test_knn_values_are_exact_fp32_cosines for fp32 cosines of unit vectors against float64;
  verdict    asserted only where |vk - bound| > margin = 2^-17 (|c_cut pre_scale| + |err_mu| + slack), slack = max(zsig err_sd,
             2 err_max).  The stage scores are inputs, bit-identical on both sides; the model sums e and e^2 in fp32 too, but in list
             order where the kernel sums a tree.  A 64-term fp32 sum of terms of one scale differs between two orders by at most
             64 * 2^-24 = 2^-18 of that scale; behind the sums come five single roundings on the way to the bound (the division, sqrtf,
             the product with zsig, the subtraction of err_mu, the final add), 5 * 2^-24 relative.  2^-18 + 5 * 2^-24 < 2^-17 relative
             to each of the bound's three terms -- c_cut pre_scale, err_mu, slack -- is the margin.  What it does not model is the error
             of the kernel's fp32 cosines against float64, which moves vk and every e: 2e-6 at worst by the tolerance above, about 1e-8
             as a random walk over 768 products of size 1e-3; a frame that this error alone carries across a margin of about 1e-6
             would fail the test with its figures printed, and none does at REAL_SEED;
  cap        at most 2 % of the 64 frames (one frame) may fall inside the margin; the host test asserts it for REAL_SEED on the model."""
import numpy as np

D = 768
GATE_BOOL = -2
SENT = 0x5A5A5A5A                 # sentinel word of untouched outputs and guard bands
F32 = np.float32
NINF = F32(-np.inf)
ZSIG = F32(7.0)
SD16, SD8, SD6, SD8R = F32(8.0e-5), F32(1.5e-3), F32(2.0e-3), F32(2.5e-4)
PS1, PS6, PS8 = F32(1.0), F32(1.0 / 32 ** 2), F32(1.0 / 256 ** 2)
SLACK = F32(3.0e-4)
COS_TOL = 2e-6
REAL_SEED = 3
REAL_CAP = 0.02


class Case:
    """one launch: every argument of the entry as NumPy arrays / scalars (attributes named after AliveRescoreArgs)"""

    def __init__(self, name, **kw):
        self.name = name
        self.frame_list = self.det_q = self.det_lib = self.force_fail = self.gate = self.pool = None
        self.certify, self.collect, self.thr, self.slack, self.idx_base, self.flag_cnt0 = True, 0, False, F32(0.0), 0, 0
        self.zsig, self.exact, self.pins = ZSIG, True, {}
        self.__dict__.update(kw)

    @property
    def R(self):
        return self.P * self.kp


def score64(c, ft, m):
    """the exact cosine as float64: sum_d s[d] * (row[d] / norm)"""
    return float(np.dot(c.s[ft].astype(np.float64), c.rows[m].astype(np.float64) / np.float64(c.norms[m])))


def kth_largest(vals, n):
    v = sorted(vals, reverse=True)
    return F32(v[n - 1]) if len(v) >= n else NINF


def model_frame(c, slot, ft, k, voice, cur_idx):
    """one frame by the rule; cur_idx: the frame's current out_idx row (collect mode reads it).  Returns a dict."""
    with np.errstate(all="ignore"):
        cv, ci = c.cand_val[slot], c.cand_idx[slot]
        ps, R = F32(c.pre_scale), c.R
        certify = c.certify and not c.collect
        det = c.det_q is not None
        det_bound = (F32(c.det_q[ft]) + F32(1.004) * F32(c.det_lib[voice])) + F32(1.0e-4) if det else F32(0.0)
        if not certify:
            prune = F32(np.inf)
        elif det:
            prune = (F32(2.0) * det_bound) / ps
        else:
            prune = ((F32(2.0) * F32(c.zsig)) * F32(c.sd_prior)) / ps
        # floor
        c_cut = NINF
        if certify:
            for l0 in range(0, R, c.list_len):
                c_cut = max(c_cut, F32(min(cv[l0:l0 + c.list_len])))
        # selection
        overflow = bool(c.collect and any(int(i) == -2 for i in ci))
        valid = [(F32(cv[e]), int(ci[e]), e) for e in range(R) if ci[e] >= 0]
        sk, s16 = kth_largest([v for v, _, _ in valid], k), kth_largest([v for v, _, _ in valid], 16)
        lim = F32(sk - prune)
        cut = min(lim, s16)
        reach = [x for x in valid if x[0] >= cut]
        if len(reach) <= 64:
            chosen = sorted(reach, key=lambda x: x[2])                 # in list order
            left = [x for x in valid if not x[0] >= cut]
        else:
            walk = sorted(valid, key=lambda x: (-x[0], x[1]))
            chosen = []
            for x in walk:
                if len(chosen) == 64 or (len(chosen) >= 16 and x[0] < lim):
                    break
                chosen.append(x)
            left = walk[len(chosen):]
            if c.collect and left:
                overflow = True
        if certify:
            for v, _, _ in left:
                c_cut = max(c_cut, v)
        # lanes: R <= 64 keeps every entry where it stands, more entries are compacted
        lanes = [(-1, F32(0.0))] * 64
        if R <= 64:
            keep = {x[2] for x in chosen}
            lanes = [(int(ci[e]), F32(cv[e])) if e in keep else (-1, F32(0.0)) for e in range(R)] + lanes[R:]
        else:
            lanes = [(i, v) for v, i, _ in chosen] + lanes[len(chosen):]
        if c.collect:
            for j in range(c.k):
                g = int(cur_idx[j])
                if g < 0:
                    continue
                el = g - c.idx_base
                if any(i == el for i, _ in lanes):
                    continue
                free = [n for n, (i, _) in enumerate(lanes) if i < 0]
                if not free:
                    overflow = True
                    break
                lanes[free[0]] = (el, F32(np.inf))
        # scores and statistics
        scored = []
        for i, pre in lanes:
            if i >= 0:
                scored.append((F32(score64(c, ft, i)), i, pre))
        err_mu = err_sd = err_max = F32(0.0)
        if certify:
            es = [F32(F32(pre * ps) - sc) for sc, _, pre in scored]
            n = max(F32(len(es)), F32(1.0))
            se, see = F32(0.0), F32(0.0)
            for e in es:
                se, see = F32(se + e), F32(see + F32(e * e))
            err_mu = min(F32(se / n), F32(0.0))
            err_sd = max(F32(np.sqrt(F32(see / n))), F32(c.sd_prior))
            err_max = max([abs(e) for e in es] + [F32(0.0)])
        # top-k
        order = sorted(scored, key=lambda x: (-x[0], x[1]))
        top, runner_up = order[:k], (order[k][0] if len(order) > k else NINF)
        out_val = [x[0] for x in top] + [NINF] * (k - len(top))
        out_idx = [(c.idx_base + x[1]) if x[0] > NINF else -1 for x in top] + [-1] * (k - len(top))
        vk = F32(out_val[k - 1])
        # verdict
        forced = bool(c.force_fail is not None and c.pool is None and c.force_fail[ft] != 0)
        flagged, why, thr, bound = False, None, None, None
        if certify and (c_cut > NINF or forced):
            base = F32(c_cut * ps)
            if det:
                bound = F32(base + det_bound)
            else:
                bound = F32(F32(base - err_mu) + max(F32(F32(c.zsig) * err_sd), F32(F32(2.0) * err_max)))
            if not (vk > bound) or forced:
                flagged, why = True, ("certificate" if not (vk > bound) else "forced")
                thr = F32(vk - F32(c.slack)) if c.slack > 0 else F32(F32(vk - F32(bound - base)) / ps)
        if c.collect and overflow:
            flagged, why, thr = True, "overflow", F32(vk - F32(c.slack))
        return dict(slot=slot, frame=ft, k=k, out_val=np.array(out_val, F32), out_idx=np.array(out_idx, np.int32), flagged=flagged, why=why,
                    thr=thr, c_cut=F32(c_cut), err_mu=err_mu, err_sd=err_sd, err_max=err_max, bound=bound, vk=vk, cut=F32(cut), sk=sk,
                    det_bound=det_bound, prune=prune, runner_up=runner_up, chosen=[(x[1], x[0]) for x in scored], ranked=len(reach) > 64, n_left=len(left))


def gate_open(c):
    """(open, slots that may run)"""
    if c.gate is None:
        return True, c.Tt
    kind, word, lo, hi = c.gate
    if kind == "bool":
        return word != 0, c.Tt
    return lo < word <= hi, (min(c.Tt, word) if c.frame_list is not None else c.Tt)


def model_launch(c):
    """the whole launch: dict(frames = model_frame results of the slots that ran, out_val / out_idx [frames][k] with SENT where nothing
    was written, flagged = sorted (frame, thr bits or None), pool: gfail [groups], fb sets)"""
    out_val = np.full((c.frames, c.k), SENT, np.uint32).view(F32)
    out_idx = c.out_idx0.copy()
    res, flagged = [], []
    is_open, nslot = gate_open(c)
    groups = c.pool["groups"] if c.pool else None
    fails = [[] for _ in groups] if groups else None
    for slot in range(nslot if is_open else 0):
        ft = int(c.frame_list[slot]) if c.frame_list is not None else slot
        if ft < 0:
            continue
        k, voice = c.k, 0
        if groups:
            g = int(c.pool["slot_grp"][slot])
            k, voice = groups[g]["k"], groups[g]["voice"]
        r = model_frame(c, slot, ft, k, voice, out_idx[ft])
        out_val[ft, :k], out_idx[ft, :k] = r["out_val"], r["out_idx"]
        res.append(r)
        if r["flagged"]:
            if groups:
                fails[g].append(slot)
            else:
                flagged.append((ft, int(r["thr"].view(np.uint32)) if c.thr else None))
    return dict(frames=res, out_val=out_val, out_idx=out_idx, flagged=sorted(flagged, key=lambda x: (x[0], x[1] or 0)), fails=fails,
                flag_cnt=c.flag_cnt0 + (sum(len(f) for f in fails) if groups else len(flagged)))


def check_indices(c):
    """what keeps a typo in a case from becoming a fault: every index the kernel dereferences with lies inside its array"""
    assert c.cand_val.shape == c.cand_idx.shape == (c.Tt, c.R) and c.cand_val.dtype == F32 and c.cand_idx.dtype == np.int32
    assert c.s.shape == (c.frames, D) and c.rows.shape == (c.M, D) and c.norms.shape == (c.M,) and c.M <= 2048
    assert c.out_idx0.shape == (c.frames, c.k) and 1 <= c.k <= 8 and c.R <= 1024
    assert int(c.cand_idx.min()) >= -2 and int(c.cand_idx.max()) < c.M, c.name
    if c.frame_list is not None:
        assert c.frame_list.shape == (c.Tt,) and int(c.frame_list.min()) >= -1 and int(c.frame_list.max()) < c.frames, c.name
    else:
        assert c.Tt <= c.frames
    if c.collect:
        el = c.out_idx0.astype(np.int64) - c.idx_base
        assert bool(np.all((c.out_idx0 == -1) | ((el >= 0) & (el < c.M)))), c.name
    for a in (c.det_q, c.force_fail):
        assert a is None or a.shape == (c.frames,)
    if c.pool:
        sg, groups = c.pool["slot_grp"], c.pool["groups"]
        assert sg.shape == (c.Tt,) and int(sg.min()) >= 0 and int(sg.max()) < len(groups) and c.frame_list is not None
        for g, rec in enumerate(groups):
            assert 1 <= rec["k"] <= c.k and 0 <= rec["voice"] < len(c.det_lib) and 0 <= rec["blk0"] < c.pool["fb_blocks"]
            assert int(np.sum((sg == g) & (c.frame_list >= 0))) <= 256
        assert len({rec["blk0"] for rec in groups}) == len(groups)
    elif c.det_lib is not None:
        assert len(c.det_lib) >= 1


# ---- exactness helpers (used by the host test) ------------------------------------------------------------------------------------
def lsb_exponent(x):
    """exponent of the lowest set bit of every nonzero float64 of x (the largest power of two dividing it)"""
    x = np.abs(np.asarray(x, np.float64))
    m, e = np.frexp(x[x != 0])
    mi = (m * 2.0 ** 53).astype(np.int64)
    return e - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)


def sum_units(terms):
    """sum |t| in units of the largest power of two dividing every term: below 2^24 means every partial sum, in any order, is an fp32
    number"""
    t = np.asarray(terms, np.float64).ravel()
    if not np.any(t != 0):
        return 0.0
    return float(np.sum(np.abs(t)) / 2.0 ** int(lsb_exponent(t).min()))


# ---- the board family: one-hot frames, any score ----------------------------------------------------------------------------------
class Board:
    """scores[f][m] chosen freely: frame f is the unit vector of dimension dim(f), row m holds scores[f][m] * norm at dim(f) and nonzero
    fillers elsewhere (which meet zeros only)"""

    def __init__(self, frames, M, seed):
        self.frames, self.M, self.rng = frames, M, np.random.default_rng(seed)
        m, f = np.arange(M), np.arange(frames)
        self.norms = (2.0 ** ((m % 5) - 2)).astype(F32)
        self.S = (((m[None, :] * 7 + f[:, None] * 13) % 256) + 1).astype(np.float64) / 1024.0     # default: (0, 0.25], multiples of 2^-10
        self.S = self.S.astype(F32)

    @staticmethod
    def dim(f):
        return (f * 67 + 5) % D

    def arrays(self):
        m, d = np.arange(self.M), np.arange(D)
        rows = (((m[:, None] * 31 + d[None, :] * 17) % 61) - 30.5) * 2.0                       # odd integers -61 .. 59
        rows = (rows * self.norms[:, None]).astype(F32)
        s = np.zeros((self.frames, D), F32)
        for f in range(self.frames):
            s[f, self.dim(f)] = 1.0
            rows[:, self.dim(f)] = self.S[f] * self.norms
        return s, rows, self.norms


def grid(x, bits=12):
    return np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits


class FrameBuilder:
    """the candidate lists of one frame of a board case"""

    def __init__(self, board, ft, R, list_len, ps):
        self.b, self.ft, self.R, self.L, self.ps = board, ft, R, list_len, np.float64(ps)
        self.cv, self.ci = np.full(R, -np.inf, F32), np.full(R, -1, np.int32)
        self.pool_rows = list(board.rng.permutation(board.M))

    def row(self):
        return int(self.pool_rows.pop())

    def put(self, e, score, err, idx=None):
        idx = self.row() if idx is None else idx
        stage = (np.float64(score) + np.float64(err)) / self.ps
        assert self.ci[e] == -1 and np.float64(F32(stage)) == stage and np.float64(F32(score)) == np.float64(score), (e, score, err)
        self.cv[e], self.ci[e], self.b.S[self.ft, idx] = F32(stage), idx, F32(score)
        return idx

    def put_stage(self, e, stage, score, idx=None):
        """an entry by its stage score (any fp32) and exact score"""
        idx = self.row() if idx is None else idx
        assert self.ci[e] == -1
        self.cv[e], self.ci[e], self.b.S[self.ft, idx] = F32(stage), idx, F32(score)
        return idx

    def seed(self, lst, value):
        """list `lst` was started from a seed: its empty entries hold the seed (stage units), index -1"""
        for e in range(lst * self.L, (lst + 1) * self.L):
            if self.ci[e] < 0:
                self.cv[e] = F32(value)

    def free(self, lists=None):
        """free positions, shuffled; lists: restrict to these lists"""
        es = [e for e in range(self.R) if self.ci[e] < 0 and (lists is None or e // self.L in lists)]
        return [int(e) for e in self.b.rng.permutation(es)]


ERRS = {
    "tiny": lambda i: (1 if i % 2 else -1) * 2.0 ** -12,              # rms and 2 max below the prior: zsig * sd_prior rules
    "rms": lambda i: (1 if i % 2 else -1) * 2.0 ** -8,                # zsig * rms rules
    "max": lambda i: -(2.0 ** -5) if i == 0 else (1 if i % 2 else -1) * 2.0 ** -12,     # one heavy error: 2 * err_max rules
    "neg": lambda i: -(2.0 ** -9) * (1 + i % 3),                      # negative mean raises the bound
    "pos": lambda i: (2.0 ** -9) * (1 + i % 3),                       # positive mean must not lower it
    "mix": lambda i: ((i * 5) % 9 - 4) * 2.0 ** -10,
    "small": lambda i: (1 if i % 2 else -1) * 2.0 ** -14,             # below every prior; no two cluster entries tie in stage score
}


def fill_frame(fb, k, n_valid, errs, full=(), seeds=None, top=0.9375, c=0.5, extra=()):
    """n_valid candidates: k - 1 clearly on top, one at 0.75 (the k-th, which pin() moves), the rest a cluster of distinct scores
    c + j 2^-18 (+ 2^-19 for odd places; all of them below any bound c + slack); `extra`: further (score, err) entries.  The lists in `full` are filled
    completely, every other list keeps at least one empty entry."""
    rng, nl = fb.b.rng, fb.R // fb.L
    pos = [e for l in full for e in range(l * fb.L, (l + 1) * fb.L)]
    other = [e for e in fb.free() if e // fb.L not in full and e % fb.L != fb.L - 1 - (e // fb.L) % 3]
    pos = (pos + other)[:n_valid + len(extra)]
    pos, xpos = pos[:max(len(pos) - len(extra), 0)], pos[max(len(pos) - len(extra), 0):]
    order = rng.permutation(len(pos))
    steps = rng.permutation(max(len(pos), 1))
    for i, j in enumerate(order):
        e = pos[int(j)]
        if i < k - 1:
            sc = top - i * 2.0 ** -8
        elif i == k - 1:
            sc = 0.75
        else:
            sc = c + int(steps[i]) * 2.0 ** -18 + (i % 2) * 2.0 ** -19       # (with errors that go by i's parity no two stage scores tie)
        fb.put(e, sc, errs(i) if i != k - 1 else 0.0)
    for e, (sc, err) in zip(xpos, extra):
        fb.put(e, sc, err)
    for l, v in (seeds or {}).items():
        assert l < nl
        fb.seed(l, v)


def pin(c, slot, where, k=None, voice=0):
    """move the k-th exact candidate of a certify frame onto its bound ('at'), the fp32 neighbour above / below; False if the frame has
    no bound, fewer than k candidates, or bound and candidate do not come to rest"""
    ft = int(c.frame_list[slot]) if c.frame_list is not None else slot
    k = c.k if k is None else k
    seen = None
    for _ in range(8):
        r = model_frame(c, slot, ft, k, voice, c.out_idx0[ft])
        if r["bound"] is None or not np.isfinite(r["bound"]) or not r["out_idx"][k - 1] >= 0 or not r["bound"] > 0:
            return False
        idx = int(r["out_idx"][k - 1]) - c.idx_base
        b = r["bound"]
        tgt = b if where == "at" else np.nextafter(b, F32(np.inf) if where == "above" else NINF)
        if seen == (idx, int(b.view(np.uint32))) and r["vk"] == tgt:
            c.pins[slot] = where
            return True
        seen = (idx, int(b.view(np.uint32)))
        e = [x for x in range(c.R) if c.cand_idx[slot, x] == idx]
        stage = np.float64(tgt) / np.float64(c.pre_scale)
        if len(e) != 1 or np.float64(F32(stage)) != stage:
            return False
        c.cand_val[slot, e[0]] = F32(stage)
        c.rows[idx, Board.dim(ft)] = F32(np.float64(tgt) * np.float64(c.norms[idx]))
    return False


def board_case(name, P, kp, list_len, k, Tt, ps, prior, plan, seed, frames=None, M=None, **kw):
    """plan(fb, slot) fills the lists of each slot's frame; returns the Case (unpinned)"""
    frames = Tt if frames is None else frames
    R = P * kp
    M = M if M is not None else int(min(2048, max(256, 2 * R)))
    b = Board(frames, M, seed)
    fl = kw.get("frame_list")
    cv, ci = np.full((Tt, R), -np.inf, F32), np.full((Tt, R), -1, np.int32)
    for slot in range(Tt):
        ft = int(fl[slot]) if fl is not None else slot
        if ft < 0:
            continue
        fb = FrameBuilder(b, ft, R, list_len, ps)
        plan(fb, slot)
        cv[slot], ci[slot] = fb.cv, fb.ci
    s, rows, norms = b.arrays()
    out_idx0 = kw.pop("out_idx0", None)
    c = Case(name, P=P, kp=kp, list_len=list_len, k=k, Tt=Tt, frames=frames, M=M, pre_scale=F32(ps), sd_prior=F32(prior), s=s, rows=rows,
             norms=norms, cand_val=cv, cand_idx=ci, out_idx0=np.full((frames, k), SENT, np.int32) if out_idx0 is None else out_idx0, **kw)
    return c


# ---- the case matrix -----------------------------------------------------------------------------------------------------------------
SHAPES = [  # (P, kp, list_len): R on both sides of every switch of PER, both list lengths at PER 0 and 3
    (1, 16, 8), (4, 16, 8), (5, 16, 8), (12, 16, 8), (13, 16, 8), (16, 16, 8),
    (9, 32, 16), (16, 32, 16), (17, 32, 16), (32, 32, 16), (2, 32, 16), (6, 32, 16),
]
TTS = [1, 3, 4, 5, 9]
KS = [1, 2, 4, 8, 4, 2, 8, 1, 4, 8, 3, 4]
WHERE = ["at", "above", "below"]


def shape_cases():
    """every shape, certify mode: frames of every kind, pinned where they can be"""
    out = []
    for n, (P, kp, L) in enumerate(SHAPES):
        R, k, Tt = P * kp, KS[n], TTS[n % 5] if n != 9 else 3
        if L == 8:
            ps, prior = PS1, SD16
        else:
            ps, prior = [(PS6, SD6), (PS8, SD8), (PS8, SD8R)][n % 3]
        nl = R // L
        kinds = ["full", "seeded", "few", "none", "part", "full", "crowd", "seednone", "full"]

        def plan(fb, slot, k=k, R=R, nl=nl, kinds=kinds, ps=ps):
            kind = kinds[(slot + n) % len(kinds)]
            errs = ERRS[["mix", "tiny", "neg", "rms", "pos", "max"][(slot + n) % 6]]
            if kind == "full":
                fill_frame(fb, k, min(R - nl + 1, 24 + 2 * slot), errs, full=[slot % nl])
            elif kind == "seeded":
                fill_frame(fb, k, min(R - nl, 20), errs, seeds={l: (0.5 - 2.0 ** -12) / float(ps) for l in range(0, nl, 2)})
            elif kind == "few":
                fill_frame(fb, k, k - 1, errs)
            elif kind == "part":                  # no full list, far candidates the cut may leave behind
                fill_frame(fb, k, min(R - nl - 3, 18), errs, extra=[(0.25 - j * 2.0 ** -10, 0.0) for j in range(3)])
            elif kind == "crowd":                 # as many entries as fit, up to 70 + k: more than 64 take the ranking walk
                fill_frame(fb, k, min(R - nl, 70 + k), ERRS["small"])
            elif kind == "seednone":
                fb.seed(nl - 1, 0.3 / float(ps))
            # "none": nothing
        base = 0 if n % 2 == 0 else 1_000_000
        kw = dict(idx_base=base, flag_cnt0=0 if n % 3 else 5)
        if L == 8:
            kw.update(thr=True, slack=SLACK if n % 2 else F32(0.0))
        c = board_case(f"shape_R{R}_L{L}_k{k}_T{Tt}", P, kp, L, k, Tt, ps, prior, plan, 100 + n, **kw)
        if L == 16 and n % 2 == 0:
            c.force_fail = np.array([(f + n) % 4 != 0 for f in range(Tt)], np.uint8)
        for slot in range(Tt):
            pin(c, slot, WHERE[(slot + n) % 3])
        out.append(c)
    return out


TRIPLE_FORMS = ["tiny", "rms", "max", "neg", "pos"]


def triple_cases():
    """for every form of the bound three frames that differ in the k-th exact score alone: at the bound, one ulp above, one below"""
    out = []
    specs = [("triples_tiny_rms_max", ["tiny", "rms", "max"], 4, 16, 8, 4, PS1, SD8, None),
             ("triples_neg_pos_tiny", ["neg", "pos", "tiny"], 9, 32, 16, 2, PS8, SD6, None),
             ("triples_rms_max_neg_R1024", ["rms", "max", "neg"], 32, 32, 16, 8, PS6, SD8R, None),
             ("triples_det", ["small"], 5, 16, 8, 4, PS1, SD16, (F32(3.0e-4), F32(2.5e-4))),
             ("triples_det_R208", ["tiny"], 13, 16, 8, 1, PS1, SD16, (F32(1.0e-4), F32(6.0e-4)))]
    for sn, (name, forms, P, kp, L, k, ps, prior, det) in enumerate(specs):
        Tt = 3 * len(forms)

        def plan(fb, slot, forms=forms, k=k):
            fb.b.rng = np.random.default_rng(7000 + 10 * sn + slot // 3)          # the three frames of a triple get identical lists
            fb.pool_rows = list(fb.b.rng.permutation(fb.b.M))
            # 16 candidates: all of them are rescored wherever the k-th stands, so the three frames share statistics and bound
            fill_frame(fb, k, 16, ERRS[forms[slot // 3]], full=[1])
        kw = dict(thr=(L == 8))
        if det:
            kw.update(det_q=np.full(Tt, det[0], F32), det_lib=np.array([det[1]], F32))
        c = board_case(name, P, kp, L, k, Tt, ps, prior, plan, 200 + sn, **kw)
        c.forms = forms
        for slot in range(Tt):
            assert pin(c, slot, WHERE[slot % 3]), (name, slot)
        out.append(c)
    return out


def selection_cases():
    """a candidate with the best exact score exactly AT the cut and one ulp below it, with 15 / 16 / 17 / 20 candidates within the
    prune of the k-th (tight prune: sd_prior 8e-5); c.sel[slot] = (index of that candidate, 'at' | 'below', candidates within the prune)"""
    out = []
    for P, kp, L, k in [(4, 16, 8, 4), (13, 16, 8, 2)]:
        variants = [(n_above, x) for n_above in (15, 16, 17, 20) for x in ("at", "below")]
        Tt, ps, prior, sel = len(variants), PS1, SD16, {}
        prune = ((F32(2.0) * ZSIG) * prior) / ps
        sk = F32(0.75)
        cut = F32(sk - prune)

        def plan(fb, slot, k=k):
            n_above, x = variants[slot]
            es = [e for e in fb.free() if e % fb.L != 0]          # no list is full: no floor above the cut
            for i in range(n_above):          # k-th largest stage score 0.75; the others within 20 * 2^-16 below it
                stage = 0.75 + (k - 1 - i) * 2.0 ** -12 if i < k else 0.75 - (i - k + 1) * 2.0 ** -16
                err = ERRS["mix"](i)
                fb.put(es.pop(), stage - err, err)
            xs = cut if x == "at" else np.nextafter(cut, NINF)
            score = F32(np.float64(xs) + 2.0 ** -5)             # e = -2^-5 exactly wherever it is rescored
            assert np.float64(score) == np.float64(xs) + 2.0 ** -5
            sel[slot] = (fb.put_stage(es.pop(), xs, score), x, n_above)
            for j in range(6):
                fb.put(es.pop(), 0.5 - j * 2.0 ** -10, ERRS["tiny"](j))
        c = board_case(f"selection_R{P * kp}_k{k}", P, kp, L, k, Tt, ps, prior, plan, 300 + P, thr=True)
        c.sel = sel
        out.append(c)
    return out


def ranking_cases():
    """64 and 65 entries reaching the cut (the switch to the ranking walk), pinned at and above the bound, and a plateau: 15 candidates
    within the prune and 60 tied ones below it, of which the walk takes the one with the lowest index and stops"""
    out = []
    for P, kp, L, k, ps, prior in [(5, 16, 8, 2, PS1, SD16), (9, 32, 16, 4, PS8, SD8), (17, 32, 16, 8, PS6, SD6)]:
        R = P * kp
        variants = [(64, "at"), (64, "above"), (65, "at"), (65, "above"), (65, "below"), ("plateau", None)]
        Tt = len(variants)

        def plan(fb, slot, k=k, prior=prior, R=R):
            n, _ = variants[slot]
            if n == "plateau":
                es = [e for e in fb.free() if e % fb.L != 0]
                lanes, tied = set(), []
                for e in es:                  # tied entries in 52 different lanes
                    if e % 64 not in lanes and len(tied) < 52:
                        lanes.add(e % 64)
                        tied.append(e)
                rest = [e for e in es if e not in tied]
                for i in range(15):
                    fb.put(rest.pop(), 0.75 - i * 2.0 ** -16, ERRS["tiny"](i))
                for j, e in enumerate(tied):
                    fb.put(e, 0.625, 0.0)
                return
            # a cluster of distinct stage scores within 4e-4 of one another, far candidates well below: exactly n entries reach the
            # cut wherever the pin puts the k-th.  64: a full list gives the floor; 65: no list is full, so c_cut is the stage score
            # of the one entry the walk leaves behind
            far = [(0.25 - j * 2.0 ** -10, 0.0) for j in range(5)]
            fill_frame(fb, k, n, ERRS["small"], full=[0] if n == 64 else (), extra=far)
        c = board_case(f"ranking_R{R}_k{k}", P, kp, L, k, Tt, ps, prior, plan, 400 + P, thr=(L == 8), M=1024)
        c.variants = variants
        for slot, (n, where) in enumerate(variants):
            if where:
                assert pin(c, slot, where), (c.name, slot)
        out.append(c)
    return out


def collect_cases():
    """collect mode: -2 markers, the join of the current top-k on exactly enough / one too few free lanes, 64 / 65 collected rows"""
    out = []
    # (name, P, kp, k, idx_base, thr, [per slot: (valid entries, marker, rows of the current top-k already present, new rows, -1 entries)])
    specs = [
        ("collect_R64_cap64", 1, 64, 4, 0, False,
         [(30, False, 2, 1, 1), (30, True, 0, 2, 2), (64, False, 4, 0, 0), (63, False, 0, 1, 3), (62, False, 1, 2, 1), (61, False, 0, 3, 1),
          (60, False, 0, 4, 0), (64, False, 3, 1, 0), (63, False, 0, 2, 2)]),
        ("collect_R12_cap4", 3, 4, 8, 1_000_000, True, [(12, False, 3, 5, 0), (5, True, 0, 0, 8), (0, False, 0, 3, 5)]),
        ("collect_R64_k8", 2, 32, 8, 0, False, [(56, False, 0, 8, 0), (57, False, 0, 8, 0), (57, False, 1, 7, 0), (64, False, 8, 0, 0)]),
        ("collect_R80_cap40", 2, 40, 4, 7, False, [(64, False, 4, 0, 0), (65, False, 4, 0, 0), (62, False, 1, 2, 1), (62, False, 0, 3, 1), (70, True, 0, 0, 4)]),
        ("collect_R320_cap64", 5, 64, 2, 0, True, [(64, False, 2, 0, 0), (65, False, 0, 0, 2), (63, False, 0, 1, 1), (63, False, 0, 2, 0), (10, False, 1, 1, 0)]),
        ("collect_R1024_cap64", 16, 64, 4, 0, False, [(64, False, 0, 0, 4), (65, False, 0, 0, 4), (100, False, 2, 2, 0)]),
    ]
    for sn, (name, P, kp, k, base, thr, slots) in enumerate(specs):
        Tt, R = len(slots), P * kp
        cur = np.full((Tt, k), -1, np.int32)

        def plan(fb, slot, k=k, base=base, R=R):
            n, marker, present, new, _ = slots[slot]
            es = fb.free()
            if marker:
                es.remove(R - 1)
            vals = (1229 + fb.b.rng.permutation(2400)[:n]) * 2.0 ** -12         # distinct scores (= stage scores)
            ids = [fb.put(es.pop(), float(v), 0.0) for v in vals]
            if marker:
                fb.ci[R - 1] = -2
            rows = [ids[j] for j in range(present)]
            for _ in range(new):                              # rows that beat most candidates, so the join shows in the output
                idx = fb.row()
                fb.b.S[fb.ft, idx] = F32(grid(fb.b.rng.uniform(0.85, 0.95)))
                rows.append(idx)
            order = fb.b.rng.permutation(k)
            for j, idx in enumerate(rows):
                cur[fb.ft, int(order[j])] = base + idx
        c = board_case(name, P, kp, 8, k, Tt, PS1, SD16, plan, 500 + sn, collect=1, idx_base=base, thr=thr, slack=SLACK if thr else F32(0.0),
                       out_idx0=cur, M=1024)
        c.slots = slots
        out.append(c)
    return out


def gate_cases():
    """the three gate forms at their edges, frame lists (a permutation of a subset, fewer listed than slots), no certificate at all"""
    out = []

    def plan(fb, slot):
        fill_frame(fb, 4, 14, ERRS["mix"], full=[slot % 2])
    perm = np.array([6, 2, 7, 0, 4], np.int32)
    gates = [("count_closed_at_lo", ("count", 2, 2, 5), None), ("count_open_above_lo", ("count", 3, 2, 5), None),
             ("count_open_at_hi", ("count", 5, 2, 5), None), ("count_closed_above_hi", ("count", 6, 2, 5), None),
             ("bool_closed", ("bool", 0, GATE_BOOL, 0), None), ("bool_open", ("bool", 1, GATE_BOOL, 0), None),
             ("bool_open_negative", ("bool", -7, GATE_BOOL, 0), perm),
             ("list_count_3_of_5", ("count", 3, 0, 5), perm), ("list_count_closed_at_lo", ("count", 3, 3, 5), perm),
             ("list_count_open_at_hi", ("count", 5, 3, 5), perm), ("list_count_closed_above_hi", ("count", 6, 3, 5), perm),
             ("zero_count_mode_gate", ("count", 0, -1, 0), None), ("one_count_mode_gate", ("count", 1, -1, 0), None)]
    for gn, (name, gate, fl) in enumerate(gates):
        c = board_case("gate_" + name, 1, 16, 8, 4, 5, PS1, SD16, plan, 600, frames=8 if fl is not None else 5, gate=gate,
                       frame_list=fl, thr=True, flag_cnt0=2)
        for slot in range(5):
            pin(c, slot, WHERE[slot % 3])
        out.append(c)
    c = board_case("no_certificate", 5, 16, 8, 4, 3, PS1, SD16, lambda fb, slot: fill_frame(fb, 4, 30, ERRS["mix"], full=[0]), 601, certify=False)
    out.append(c)
    return out


def tie_cases():
    """equal exact scores across the k-th place: five rows tied for places k - 1 .. k + 3 (their stage scores all differ), the lower
    library indices must take the places; c.tied[slot] = the tied rows"""
    out = []
    for P, kp, L, k, base in [(4, 16, 8, 4, 0), (13, 16, 8, 2, 77), (9, 32, 16, 8, 0)]:
        tied = {}

        def plan(fb, slot, k=k):
            es = [e for e in fb.free() if e % fb.L != 0]
            for i in range(k - 2):
                fb.put(es.pop(), 0.9375 - i * 2.0 ** -8, ERRS["mix"](i))
            rows = [fb.put(es.pop(), 0.75, (j - 2) * 2.0 ** -10) for j in range(5)]
            if slot % 2:                      # the same rows the other way round: list order must not decide
                for e, idx in zip(sorted(e for e in range(fb.R) if fb.ci[e] in rows), sorted(rows, reverse=slot % 4 == 1)):
                    fb.ci[e] = idx
            tied[slot] = sorted(rows)
            for j in range(12):
                fb.put(es.pop(), 0.5 + j * 2.0 ** -12, ERRS["tiny"](j))
        c = board_case(f"ties_R{P * kp}_k{k}", P, kp, L, k, 4, PS1 if L == 8 else PS8, SD16 if L == 8 else SD8, plan, 900 + P, idx_base=base,
                       thr=(L == 8))
        c.tied = tied
        out.append(c)
    return out


def pool_cases():
    """the pool form: two groups (k 2 and 8, stride 8) with padding slots between them, per-voice library bounds, deterministic
    certificate; every frame of group 0 fails (pinned at / below its bound), none of group 1 does (pinned above)"""
    out = []
    for P in (4, 13):
        fl = np.array([3, 0, 5, 1, 4, -1, -1, -1, 7, 2, 6, -1], np.int32)
        sg = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1], np.int32)
        groups = [dict(voice=1, blk0=1, k=2), dict(voice=0, blk0=0, k=8)]

        def plan(fb, slot):
            fill_frame(fb, groups[sg[slot]]["k"], 16 if slot % 2 else 26, ERRS["small"], full=[slot % 3])
        c = board_case(f"pool_R{P * 16}", P, 16, 8, 8, 12, PS1, SD16, plan, 700 + P, frames=8, frame_list=fl,
                       det_q=(F32(2.0e-4) + F32(1.0e-5) * np.arange(8)).astype(F32), det_lib=np.array([F32(3.0e-4), F32(7.0e-4)], F32),
                       pool=dict(slot_grp=sg, groups=groups, fb_blocks=2))
        for slot in range(12):
            if fl[slot] >= 0:
                g = groups[sg[slot]]
                assert pin(c, slot, ("at", "below")[slot % 2] if sg[slot] == 0 else "above", k=g["k"], voice=g["voice"]), (c.name, slot)
        out.append(c)
    return out


def ramp_cases():
    """rows whose 768 elements all differ (permutations of the ramp -384 .. 383) against frames of the integers -96 .. 95 (four times
    each, permuted); norm 2^23 or 2^24, so scores are multiples of 2^-24 below 1 and stage scores score + e, e a multiple of 2^-12"""
    out = []
    for P, kp, L, k, Tt, ps, prior in [(4, 16, 8, 4, 5, PS1, SD16), (9, 32, 16, 8, 4, PS8, SD8)]:
        rng = np.random.default_rng(800 + P)
        R, M = P * kp, 512
        s = np.stack([rng.permutation(np.repeat(np.arange(-96, 96), 4)) for _ in range(Tt)]).astype(F32)
        rows = np.stack([rng.permutation(np.arange(-384, 384)) for _ in range(M)]).astype(F32)
        norms = np.where(np.arange(M) % 2 == 0, 2.0 ** 23, 2.0 ** 24).astype(F32)
        sc = (s.astype(np.float64) @ rows.astype(np.float64).T) / norms.astype(np.float64)[None, :]
        cv, ci = np.full((Tt, R), -np.inf, F32), np.full((Tt, R), -1, np.int32)
        for t in range(Tt):
            n_valid = min(R - R // L, 40)
            ids = np.argsort(-sc[t])[:n_valid]                 # the best rows, as a stage would list them
            pos = [e for e in rng.permutation(R) if e % L != L - 1][:n_valid]
            for j, (e, m) in enumerate(zip(pos, ids)):
                stage = (sc[t, m] + ERRS["mix"](j)) / np.float64(ps)
                assert np.float64(F32(stage)) == stage
                cv[t, e], ci[t, e] = F32(stage), m
            for e in range(0, L):                              # list 0 full: a floor
                if ci[t, e] < 0:
                    m = int(np.argsort(-sc[t])[n_valid + e])
                    cv[t, e], ci[t, e] = F32((sc[t, m]) / np.float64(ps)), m
        out.append(Case(f"ramp_R{R}_k{k}", P=P, kp=kp, list_len=L, k=k, Tt=Tt, frames=Tt, M=M, pre_scale=ps, sd_prior=prior, s=s, rows=rows,
                        norms=norms, cand_val=cv, cand_idx=ci, out_idx0=np.full((Tt, k), SENT, np.int32), thr=(L == 8), idx_base=12345))
    return out


def realistic(seed=REAL_SEED):
    """64 Gaussian unit frames against 2048 Gaussian rows; the candidate lists are the 16 best rows of each half of the library by a
    CPU fp8 score (operands x 2^8 rounded to e4m3, float64 dot product, pre_scale 1 / 256^2): one split of two 16-entry lists, k = 8 --
    the eighth best of 2048 cosines lies about as far above the sixteenth best of 1024 as the bound's slack, so both verdicts occur"""
    from knn_codes import e4m3_decode, e4m3_encode
    rng = np.random.default_rng(seed)
    T, M, P, kp, L, k = 64, 2048, 1, 32, 16, 8
    s = rng.standard_normal((T, D))
    s = (s / np.linalg.norm(s, axis=1, keepdims=True)).astype(F32)
    rows = rng.standard_normal((M, D)).astype(F32)
    norms = np.sqrt(np.sum(rows.astype(np.float64) ** 2, axis=1)).astype(F32)
    q = lambda x: e4m3_decode(e4m3_encode(x * 256.0))
    stage = (q(s.astype(np.float64)) @ q(rows.astype(np.float64) / norms.astype(np.float64)[:, None]).T).astype(F32)
    cv, ci = np.zeros((T, P * kp), F32), np.zeros((T, P * kp), np.int32)
    for t in range(T):
        for l in range(2):
            sub = np.arange(l * 1024, (l + 1) * 1024)
            best = sub[np.argsort(-stage[t, sub], kind="stable")[:L]]
            cv[t, l * L:(l + 1) * L], ci[t, l * L:(l + 1) * L] = stage[t, best], best
    return Case("realistic", P=P, kp=kp, list_len=L, k=k, Tt=T, frames=T, M=M, pre_scale=PS8, sd_prior=SD8, s=s, rows=rows, norms=norms,
                cand_val=cv, cand_idx=ci, out_idx0=np.full((T, k), SENT, np.int32), exact=False)


def real_margin(r, ps):
    """the realistic case's verdict margin for one model_frame result (module docstring)"""
    slack = max(float(ZSIG) * float(r["err_sd"]), 2.0 * float(r["err_max"]))
    return 2.0 ** -17 * (abs(float(r["c_cut"]) * float(ps)) + abs(float(r["err_mu"])) + slack)


_CACHE = {}


def all_cases():
    """every exact case, built once (list of Case); check_indices has passed on each"""
    if "all" not in _CACHE:
        cs = shape_cases() + triple_cases() + selection_cases() + ranking_cases() + collect_cases() + gate_cases() + tie_cases() + pool_cases() + ramp_cases()
        for c in cs:
            check_indices(c)
        assert len({c.name for c in cs}) == len(cs)
        _CACHE["all"] = cs
    return _CACHE["all"]


def expected(c):
    """model_launch(c), computed once per case and never changed"""
    if c.name not in _CACHE:
        _CACHE[c.name] = model_launch(c)
    return _CACHE[c.name]
