"""Multi-session streaming at its limits, against fp64 references.

1. The grouped exact search (alive_knn_search_grouped) at every k in 1..8 and in every regime of its plan -- slab-limited,
   4096 lists per frame, over-subscribed (more items than waves: the scan's wave-stride loop), chunks that straddle batch rows,
   N * T = 2^20 -- against an fp64 brute force and the strict search of each segment packed alone.  A Python mirror of the
   plan's arithmetic asserts that every case lands in the regime it is named for.  The table's edges run on a pool embedded
   between guard rows that would be every frame's best match: a broken bounds check shows up as a wrong answer.
2. Graph replay with changing tables, a workspace left behind by a different table, guard bands around the buffers.
3. The per-row edges (merge-gather, pitch transform, resample) against fp64 at their own edges.
4. MultiStreamConverter at its slot limit (1024 slots).
"""
import math
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
from module import audio_io, synthetic                               # noqa: E402
from module import multistream as MS                                 # noqa: E402
from module.common import PackedLibrary                              # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = list(range(1, 9))
GR_ITEMS = 4096          # csrc/knn.hip: items the plan aims for, waves the scan launches, lists a frame merges at most
VAL_TOL = 2e-6           # |val - fp64 cosine at the returned row| (test_gpu_knn_audit.py's bar)
SEP = 1e-5               # the top-k SET must be the fp64 one where the k-th and (k+1)-th cosines are further apart


# ---------------------------------------------------------------------------------------------------- plan mirror
def plan(lo, ln, P, T, k):
    """knn_grouped_plan_kernel's arithmetic on the host: groups (first-appearance order of the distinct active (lo, len)),
    chunks of F = 64 // k frames, per = GR_ITEMS // chunks_total, nslab = max(1, min(len // 4, per)), items"""
    F = 64 // k
    size = {}
    for a, b in zip(lo, ln):
        if b > 0 and b >= k and a >= 0 and a + b <= P:
            size[(a, b)] = size.get((a, b), 0) + 1
    groups = list(size)
    chunks = [-(-size[g] * T // F) for g in groups]
    total = sum(chunks)
    per = GR_ITEMS // total if total > 0 else 0
    nslab = [max(1, min(g[1] // 4, per)) for g in groups]
    return dict(F=F, groups=groups, sizes=[size[g] for g in groups], chunks=chunks, chunks_total=total, per=per, nslab=nslab,
                items=sum(a * b for a, b in zip(nslab, chunks)))


def assert_regime(regime, p, N, T):
    if regime == "slab_limited":                 # every segment cut into len // 4 slabs, fewer than the plan would allow
        assert p["per"] > 0 and p["items"] <= GR_ITEMS and all(g[1] // 4 < p["per"] for g in p["groups"]), p
    elif regime == "lists4096":                  # one chunk, one segment cut into the most lists a frame merges
        assert p["chunks_total"] == 1 and p["nslab"] == [GR_ITEMS], p
    elif regime == "oversubscribed":             # per = 0: one slab per segment, more items than launched waves
        assert p["per"] == 0 and p["items"] > GR_ITEMS and p["nslab"] == [1] * len(p["groups"]), p
    elif regime == "straddle":                   # some chunk holds the frames of two batch rows
        F = p["F"]
        assert T % F != 0 or T == 1
        assert any((c * F) // T != (min(c * F + F, s * T) - 1) // T for s, ch in zip(p["sizes"], p["chunks"]) for c in range(ch)), p
    elif regime == "upper":
        assert N * T == 1 << 20 and p["per"] == 0, p
    else:
        raise AssertionError(regime)


def over_T(k):
    """T with N * ceil(T / F) > 4096 at N = 1024 and T % F != 0 (also for one segment shared by all rows)"""
    return 4 * (64 // k) + 1


# ---------------------------------------------------------------------------------------------------- pools, checks
def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def make_pool(sizes, seed, edit=None):
    """VoicePool of random voices v<i> of the given sizes (edit(i, tokens) may change a voice before packing)"""
    g = torch.Generator().manual_seed(seed)
    voices = {}
    for i, m in enumerate(sizes):
        t = torch.randn(768, m, generator=g)
        if edit is not None:
            edit(i, t)
        voices[f"v{i}"] = t
    return MS.VoicePool({n: t.to(DEV) for n, t in voices.items()})


def unit64(rows):
    r = rows.double()
    return r / r.norm(dim=1, keepdim=True)


def grouped(src, rows, norms, lo, ln, k):
    """the search on host tables; rows / norms may be a view of a larger pool (P = rows.shape[0])"""
    lo_t = torch.tensor(lo, dtype=torch.int32, device=DEV)
    ln_t = torch.tensor(ln, dtype=torch.int32, device=DEV)
    val, idx = MS.knn_search_grouped(src, rows, norms, lo_t, ln_t, k)
    N, _, T = src.shape
    return val.view(N, T, k), idx.view(N, T, k)


def active(a, b, P, k):
    return b > 0 and b >= k and a >= 0 and a + b <= P


def check_fp64(src, rows, val, idx, lo, ln, k, frames_per_block=1 << 16, cells=1 << 26):
    """every row of the batch against the fp64 brute force of its segment: values, order, sets; inactive rows -inf / -1"""
    N, _, T = src.shape
    P = rows.shape[0]
    u64 = unit64(rows)
    act = [n for n in range(N) if active(lo[n], ln[n], P, k)]
    inact = sorted(set(range(N)) - set(act))
    if inact:
        ii = torch.tensor(inact, device=DEV)
        assert bool((val[ii] == -math.inf).all()) and bool((idx[ii] == -1).all()), "an inactive row got a result"
    n_sep = 0
    i = 0
    while i < len(act):
        blk = [act[i]]
        r0, r1 = lo[act[i]], lo[act[i]] + ln[act[i]]
        while i + len(blk) < len(act) and (len(blk) + 1) * T <= frames_per_block:
            n = act[i + len(blk)]
            a, b = min(r0, lo[n]), max(r1, lo[n] + ln[n])
            if (len(blk) + 1) * T * (b - a) > cells:
                break
            blk.append(n)
            r0, r1 = a, b
        i += len(blk)
        bt = torch.tensor(blk, device=DEV)
        q = src[bt].double()                                              # [B, 768, T]
        q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-300)             # zero frames: cosine 0 against every row
        cos = torch.einsum("rd,bdt->btr", u64[r0:r1], q)                  # [B, T, R]
        pos = torch.arange(r0, r1, device=DEV)
        lo_b = torch.tensor([lo[n] for n in blk], device=DEV)[:, None, None]
        hi_b = torch.tensor([lo[n] + ln[n] for n in blk], device=DEV)[:, None, None]
        cos = cos.masked_fill((pos < lo_b) | (pos >= hi_b), -math.inf)
        v, ix = val[bt], idx[bt].long()                                    # [B, T, k]
        assert bool(((ix >= lo_b) & (ix < hi_b)).all()), "an index outside its row's segment"
        at = torch.gather(cos, 2, ix - r0)
        err = (v.double() - at).abs().max().item()
        assert err <= VAL_TOL, f"val differs from the fp64 cosine at its row by {err:.3g}"
        if k > 1:
            d, e = v[..., :-1], v[..., 1:]
            ok = (d > e) | ((d == e) & (ix[..., :-1] < ix[..., 1:]))
            assert bool(ok.all()), "val not descending with ties by ascending row"
        kk = min(k + 1, r1 - r0)
        top = torch.topk(cos, kk, dim=2)
        if kk == k + 1:
            sep = (top.values[..., k - 1] - top.values[..., k]) > SEP
        else:
            sep = torch.ones(top.values.shape[:2], dtype=torch.bool, device=DEV)
        want = torch.sort(top.indices[..., :k] + r0, dim=2).values
        got = torch.sort(ix, dim=2).values
        bad = sep & ~(want == got).all(dim=2)
        assert not bool(bad.any()), f"top-{k} set differs from fp64 at {torch.nonzero(bad)[:4].tolist()} (block rows {blk[:4]}...)"
        n_sep += int(sep.sum())
        del cos, q
    return n_sep


def sample_rows(N, n=64):
    s = sorted(set(np.linspace(0, N - 1, n).round().astype(int).tolist()) | {0, N - 1})
    return s


def check_strict(src, rows, val, idx, lo, ln, k, rows_to_check, cache=None):
    """val and idx - lo bitwise those of PackedLibrary(segment, strict=True).search on the segment alone"""
    cache = {} if cache is None else cache
    P = rows.shape[0]
    for n in rows_to_check:
        if not active(lo[n], ln[n], P, k):
            continue
        key = (lo[n], ln[n])
        if key not in cache:
            cache[key] = PackedLibrary(rows[lo[n]:lo[n] + ln[n]].t().contiguous(), strict=True)
        rv, ri = cache[key].search(src[n:n + 1].contiguous(), k)
        T = src.shape[2]
        assert torch.equal(val[n], rv.view(T, k)), (n, key)
        assert torch.equal(idx[n] - lo[n], ri.view(T, k)), (n, key)


def check_all(src, pool_rows, val, idx, lo, ln, k, sample=None):
    nsep = check_fp64(src, pool_rows, val, idx, lo, ln, k)
    N, _, T = src.shape
    n_act = sum(active(a, b, pool_rows.shape[0], k) for a, b in zip(lo, ln)) * T
    assert nsep >= n_act // 2, (nsep, n_act)                            # the set check was not vacuous
    check_strict(src, pool_rows, val, idx, lo, ln, k, range(N) if sample is None or N <= 64 else sample)
    return nsep


# ---------------------------------------------------------------------------------------------------- 1. regimes
DUP_ROW, DUP_EVERY, DUP_AT = 1000, 97, 3         # the long voice: row DUP_ROW copied at every position p % 97 == 3


def _dup_long(i, t):
    if i == 0:
        t[:, DUP_AT::DUP_EVERY] = t[:, DUP_ROW:DUP_ROW + 1]


@pytest.fixture(scope="module")
def pool():
    """v0: 100 003 rows (with the copies), v1..v6 short voices, v7: 4000 rows for overlapping sub-segments, v8: 1201 rows"""
    return make_pool((100_003, 37, 100, 250, 613, 1500, 9, 4000, 1201, 200), 41, edit=_dup_long)


def _seg(pool, i):
    return pool.segment(f"v{i}")


def _table(pool, regime, k, N=None):
    """(N, T, lo, ln) of a regime"""
    if regime == "slab_limited":
        segs = [_seg(pool, i) for i in (1, 2, 3, 6, 3, 2, 1)]
        N, T = len(segs) + 1, 24
        lo = [s[0] for s in segs] + [0]
        ln = [s[1] for s in segs] + [0]                                  # and an inactive row
        return N, T, lo, ln
    if regime == "lists4096":
        a, m = _seg(pool, 0)
        return 3, 64 // k, [-1, a, a], [10, m, 0]                        # one active row between two inactive ones
    if regime == "oversubscribed_shared":
        a, m = _seg(pool, 8)
        return 1024, over_T(k), [a] * 1024, [m] * 1024
    if regime == "oversubscribed_distinct":
        a, _ = _seg(pool, 7)                                             # 1024 distinct, overlapping sub-segments of v7
        lo = [a + 3 * n for n in range(1024)]
        ln = [300 + 5 * (n % 97) for n in range(1024)]
        return 1024, over_T(k), lo, ln
    if regime in ("straddle", "straddle_T1"):
        rng = np.random.default_rng(k)
        member = rng.permutation(sum(([g] * s for g, s in enumerate((3, 4, 5, 6, 7))), []))
        segs = [_seg(pool, i) for i in (2, 3, 4, 5, 8)]
        F = 64 // k
        T = 1 if regime == "straddle_T1" else F + F // 2 + 1
        return len(member), T, [segs[g][0] for g in member], [segs[g][1] for g in member]
    if regime == "upper":
        a, m = _seg(pool, 9)
        lo = [a + (5 * n) % 150 for n in range(1024)]
        ln = [12 + n % 37 for n in range(1024)]
        return 1024, 1024, lo, ln
    raise AssertionError(regime)


REGIMES = {"slab_limited": "slab_limited", "lists4096": "lists4096", "oversubscribed_shared": "oversubscribed",
           "oversubscribed_distinct": "oversubscribed", "straddle": "straddle", "straddle_T1": "straddle", "upper": "upper"}


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("regime", list(REGIMES))
def test_grouped_search_matches_fp64_and_strict_in_every_plan_regime(pool, regime, k):
    pool_ = pool
    N, T, lo, ln = _table(pool, regime, k)
    assert_regime(REGIMES[regime], plan(lo, ln, pool_.P, T, k), N, T)
    src = torch.randn(N, 768, T, device=DEV, generator=_gen(1000 * k + len(regime)))
    zero = [(n, t) for n, t in ((0, 0), (N - 1, T - 1), (N // 2, T // 2)) if active(lo[n], ln[n], pool_.P, k)]
    for n, t in zero:
        src[n, :, t] = 0.0
    if regime == "lists4096":
        dup = pool_.rows[lo[1] + DUP_ROW]
        src[1, :, T - 1] = dup                                          # equal to the copied row: ties across slab cuts
        if T > 2:
            src[1, :, 1] = dup * 3.0
    val, idx = grouped(src, pool_.rows, pool_.norms, lo, ln, k)
    for n, t in zero:                                                   # zero-norm frames: val 0, the k lowest rows
        assert torch.equal(val[n, t], torch.zeros(k, device=DEV))
        assert idx[n, t].tolist() == list(range(lo[n], lo[n] + k))
    if regime == "lists4096":
        copies = [lo[1] + DUP_AT + DUP_EVERY * j for j in range(k)]
        for t in {T - 1, 1} if T > 2 else {T - 1}:
            assert idx[1, t].tolist() == copies, (t, idx[1, t].tolist())
            assert len(set(val[1, t].tolist())) == 1
    check_all(src, pool_.rows, val, idx, lo, ln, k, sample=sample_rows(N))


# ---------------------------------------------------------------------------------------------------- 1b. table edges
G_ROWS = 64          # guard rows on either side of the pool the search is given


def _edge_setup(k, seed):
    """a pool of P = 512 rows (voices a: 300, b: 212) between 64 guard rows on each side; guard rows and decoys are the
    direction u every frame leans to, so a row read outside its segment would win"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(768, generator=g)
    a, b = torch.randn(768, 300, generator=g), torch.randn(768, 212, generator=g)
    P = 512
    body = torch.cat([a, b], 1)
    decoys = [59, 60 + k, P - 26, 149, 170, 190, 279, 320]
    for d in decoys:
        body[:, d] = u
    guard = u[:, None].expand(768, G_ROWS).clone()
    vp = MS.VoicePool({"g0": guard.to(DEV), "a": body[:, :300].to(DEV), "b": body[:, 300:].to(DEV), "g1": guard.to(DEV)})
    rows, norms = vp.rows[G_ROWS:G_ROWS + P], vp.norms[G_ROWS:G_ROWS + P]
    assert vp.segment("a")[0] == G_ROWS and vp.P == P + 2 * G_ROWS
    return u, rows, norms, P


@pytest.mark.parametrize("k", KS)
def test_grouped_search_table_edges_inside_guard_rows(k):
    u, rows, norms, P = _edge_setup(k, 90 + k)
    N, T = 1024, 5
    rng = np.random.default_rng(k)
    lo, ln = [], []
    for n in range(N):                                                  # random valid segments, some inactive rows
        m = int(rng.integers(k, 100))
        lo.append(int(rng.integers(0, P - m + 1)))
        ln.append(m if n % 11 else 0)
    edges = {0: (10, 37), 1: (60, k), 2: (80, k - 1), 3: (90, 0), 4: (-1, 10), 5: (P - 25, 25), 6: (P - 24, 25),
             7: (150, 20), 8: (150, 40), 9: (280, 40), N - 1: (10, 37)}
    for n, (a, b) in edges.items():
        lo[n], ln[n] = a, b
    src = 40.0 * u.to(DEV)[None, :, None] + torch.randn(N, 768, T, device=DEV, generator=_gen(7 + k))
    src[N - 1] = src[0]
    src[1, :, 0] = 0.0
    src[5, :, T - 1] = 0.0
    val, idx = grouped(src, rows, norms, lo, ln, k)
    # the edges one by one
    assert torch.equal(val[0], val[N - 1]) and torch.equal(idx[0], idx[N - 1])             # one segment, rows 0 and 1023
    assert torch.equal(torch.sort(idx[1], dim=1).values, torch.arange(60, 60 + k, device=DEV).expand(T, k).int())  # len = k
    assert idx[1, 0].tolist() == list(range(60, 60 + k))                 # (the zero frame: the k lowest rows)
    for n in (2, 3, 4, 6):                                              # len = k - 1, len = 0, lo = -1, lo + len = P + 1
        assert bool((val[n] == -math.inf).all()) and bool((idx[n] == -1).all()), n
    assert bool(((idx[5] >= P - 25) & (idx[5] < P)).all())              # lo + len = P: active, never the guard row at P
    assert idx[5, T - 1].tolist() == list(range(P - 25, P - 25 + k))
    assert bool((idx[7] < 170).all()) and bool((idx[7] >= 150).all())   # same lo, len 20: never the decoy at 170
    assert bool((idx[8, :, 0] == 170).all())                            # same lo, len 40: the decoy at 170 first
    assert bool(((idx[9] >= 280) & (idx[9] < 320)).all())               # across the voices' boundary at 300
    check_all(src, rows, val, idx, lo, ln, k, sample=sample_rows(N) + sorted(edges))
    # a table where every row is inactive (G = 0): the outputs are written all the same
    bad = [(0, 0), (80, k - 1), (-1, 10), (P - 24, 25), (2 ** 31 - 1, 5), (10, -5), (-(2 ** 31), 100), (P, 1)]
    lo2, ln2 = [a for a, _ in bad], [b for _, b in bad]
    assert plan(lo2, ln2, P, T, k)["groups"] == []
    lo_t = torch.tensor(lo2, dtype=torch.int32, device=DEV)
    ln_t = torch.tensor(ln2, dtype=torch.int32, device=DEV)
    s2 = src[:len(bad)].contiguous()
    v2 = torch.full((len(bad) * T, k), 7.0, device=DEV)
    i2 = torch.full((len(bad) * T, k), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(nat.lib().alive_knn_grouped_workspace_bytes(len(bad), T, k), dtype=torch.uint8, device=DEV)
    _direct(s2, rows, norms, P, lo_t, ln_t, k, ws, v2, i2)
    assert bool((v2 == -math.inf).all()) and bool((i2 == -1).all())


def _direct(src, rows, norms, P, lo_t, ln_t, k, ws, v, i):
    N, _, T = src.shape
    nat.check(nat.lib().alive_knn_search_grouped(nat.ptr(src), N, T, rows.data_ptr(), norms.data_ptr(), P, nat.ptr(lo_t),
                                                  nat.ptr(ln_t), k, v.data_ptr(), i.data_ptr(), ws.data_ptr(), nat.stream()),
              "alive_knn_search_grouped")


# ---------------------------------------------------------------------------------------------------- 2. replay, workspace
@pytest.mark.parametrize("k", [3, 8])
def test_grouped_search_graph_replay_with_changing_tables(pool, k):
    p = pool
    N, T = 1024, over_T(k)
    tables = []
    for regime in ("slab_limited", "oversubscribed_distinct", None, "slab_limited"):
        if regime is None:
            lo, ln = [0] * N, [0] * N
        else:
            _, _, a, b = _table(p, regime, k)
            lo, ln = a + [0] * (N - len(a)), b + [0] * (N - len(b))
            assert_regime(REGIMES[regime], plan(lo, ln, p.P, T, k), N, T)
        tables.append((lo, ln))
    src = torch.randn(N, 768, T, device=DEV, generator=_gen(300 + k))
    lo_t = torch.zeros(N, dtype=torch.int32, device=DEV)
    ln_t = torch.zeros(N, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # the workspace of the capture stream exists first
        for _ in range(2):
            MS.knn_search_grouped(src, p.rows, p.norms, lo_t, ln_t, k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gv, gi = MS.knn_search_grouped(src, p.rows, p.norms, lo_t, ln_t, k)
    for lo, ln in tables:
        lo_t.copy_(torch.tensor(lo, dtype=torch.int32))
        ln_t.copy_(torch.tensor(ln, dtype=torch.int32))
        graph.replay()
        ev, ei = grouped(src, p.rows, p.norms, lo, ln, k)
        assert torch.equal(gv.view(N, T, k), ev) and torch.equal(gi.view(N, T, k), ei)
    del graph


@pytest.mark.parametrize("k", [2, 5])
def test_grouped_search_ignores_the_previous_calls_plan(pool, k):
    """1024 groups, then 1 group in the same workspace == that call on a zeroed workspace (stale but valid contents)"""
    p = pool
    N, T, lo_a, ln_a = _table(p, "oversubscribed_distinct", k)
    _, _, lo_b, ln_b = _table(p, "oversubscribed_shared", k)
    assert len(plan(lo_a, ln_a, p.P, T, k)["groups"]) == 1024 and len(plan(lo_b, ln_b, p.P, T, k)["groups"]) == 1
    src = torch.randn(N, 768, T, device=DEV, generator=_gen(500 + k))
    nb = nat.lib().alive_knn_grouped_workspace_bytes(N, T, k)
    t = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    out = lambda: (torch.empty(N * T, k, device=DEV), torch.empty(N * T, k, dtype=torch.int32, device=DEV))
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    va, ia = out()
    _direct(src, p.rows, p.norms, p.P, t(lo_a), t(ln_a), k, ws, va, ia)
    vb, ib = out()
    _direct(src, p.rows, p.norms, p.P, t(lo_b), t(ln_b), k, ws, vb, ib)
    ws.zero_()
    vz, iz = out()
    _direct(src, p.rows, p.norms, p.P, t(lo_b), t(ln_b), k, ws, vz, iz)
    assert torch.equal(vb, vz) and torch.equal(ib, iz)
    _direct(src, p.rows, p.norms, p.P, t(lo_a), t(ln_a), k, ws, vz, iz)           # and back: 1 group, then 1024
    assert torch.equal(va, vz) and torch.equal(ia, iz)


@pytest.mark.parametrize("k", [1, 6])
def test_grouped_search_stays_inside_its_workspace_and_outputs(pool, k):
    p = pool
    N, T, lo, ln = _table(p, "oversubscribed_distinct", k)
    assert plan(lo, ln, p.P, T, k)["items"] > GR_ITEMS
    src = torch.randn(N, 768, T, device=DEV, generator=_gen(700 + k))
    need = nat.lib().alive_knn_grouped_workspace_bytes(N, T, k)
    guard = 8 << 20
    ws = torch.zeros(need + guard, dtype=torch.uint8, device=DEV)
    ws[need:] = 0xAB
    tt = N * T
    outv = torch.full((tt * k + 2048,), 12345.0, device=DEV)
    outi = torch.full((tt * k + 2048,), 54321, dtype=torch.int32, device=DEV)
    v, i = outv[1024:1024 + tt * k], outi[1024:1024 + tt * k]
    _direct(src, p.rows, p.norms, p.P, torch.tensor(lo, dtype=torch.int32, device=DEV),
            torch.tensor(ln, dtype=torch.int32, device=DEV), k, ws, v, i)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all()), "the grouped search wrote behind its workspace"
    assert bool((outv[:1024] == 12345.0).all() and (outv[1024 + tt * k:] == 12345.0).all())
    assert bool((outi[:1024] == 54321).all() and (outi[1024 + tt * k:] == 54321).all())
    rv, ri = grouped(src, p.rows, p.norms, lo, ln, k)
    assert torch.equal(v.view(N, T, k), rv) and torch.equal(i.view(N, T, k), ri)


# ---------------------------------------------------------------------------------------------------- 3. per-row edges
U32 = 2.0 ** -24


@pytest.mark.parametrize("k", KS)
def test_merge_gather_rows_against_fp64(k):
    """out = (1 - a) * mean(rows[idx]) + a * src per window.  Bound: (k + 4) fp32 unit roundoffs of mean|rows[idx]| +
    |a * src| (k - 1 sums and the division, 1 - a and a rounded to fp32, two products, the sum); out == src bitwise at
    a = 1 and inactive rows (idx -1); out == the fp32 mean (sum in order, / k) at a = 0"""
    M = 3000
    rows = torch.randn(M, 768, device=DEV, generator=_gen(40 + k))
    rows64 = rows.double()
    for N, T in ((3, 40), (21, 33), (31, 65), (1024, 37)):              # N * ceil(T/32) < 64: the 12-way feature split
        g = torch.Generator(device=DEV).manual_seed(N * 100 + T + k)
        src = torch.randn(N, 768, T, device=DEV, generator=g)
        idx = torch.randint(0, M, (N * T, k), device=DEV, generator=g, dtype=torch.int32)
        val = torch.sort(torch.rand(N * T, k, device=DEV, generator=g), dim=1, descending=True).values
        base = [0.0, 1.0, 1e-8, 1.0 - 1e-8, 0.5, 0.3]
        alpha = torch.rand(N, generator=g, device=DEV, dtype=torch.float64)
        alpha[:len(base)] = torch.tensor(base[:N], dtype=torch.float64)
        inactive = [n for n in range(N) if n % 7 == 6]
        ix = idx.view(N, T, k)
        ix[inactive] = -1
        out = MS.merge_gather_rows(val, idx, k, alpha, rows, src)
        mean64 = sum(rows64[idx[:, j].clamp_min(0).long()] for j in range(k)) / k              # [N*T, 768]
        abs64 = sum(rows64[idx[:, j].clamp_min(0).long()].abs() for j in range(k)) / k
        s = src.permute(0, 2, 1).reshape(N * T, 768).double()
        a = alpha.repeat_interleave(T)[:, None]
        ref = (1 - a) * mean64 + a * s
        bound = (k + 4) * U32 * (abs64 + (a * s).abs())
        act = torch.ones(N, T, dtype=torch.bool, device=DEV)
        act[inactive] = False
        act = act.reshape(-1)
        got = out.permute(0, 2, 1).reshape(N * T, 768)
        over = ((got.double() - ref).abs() > bound) & act[:, None]
        assert not bool(over.any()), (N, T, int(over.sum()))
        for n in inactive + [1]:                                        # passed through; a = 1
            assert torch.equal(out[n], src[n]), n
        rows_c, idx_c = rows.cpu(), idx.view(N, T, k)[0].clamp_min(0).long().cpu()   # (IEEE fp32 division on the host)
        m32 = rows_c[idx_c[:, 0]]
        for j in range(1, k):
            m32 = m32 + rows_c[idx_c[:, j]]
        m32 = (m32 / float(k)).t()
        assert torch.equal(out[0].cpu(), m32)                           # a = 0


def _f0_rows(N, T, seed):
    g = torch.Generator().manual_seed(seed)
    f0 = torch.rand(N, 1, T, generator=g) * 440 + 60
    f0[torch.rand(N, 1, T, generator=g) < 0.2] = 0.0                    # unvoiced frames
    rate = 0.5 + 1.5 * torch.rand(N, generator=g)
    shift = torch.randint(-24, 25, (N,), generator=g).float() + 0.25 * torch.randint(0, 4, (N,), generator=g).float()
    inton = 1.5 * torch.rand(N, generator=g)
    f0[0] = 0.0                                                         # all unvoiced
    if T > 1:
        f0[1] = 0.0
        f0[1, 0, T // 2] = 180.0                                        # a single voiced frame
    inton[2] = 0.0
    shift[3], shift[4] = 24.0, -24.0
    shift[5], inton[5], rate[5] = 0.0, 1.0, 1.0
    return f0, rate, shift, inton


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N,T", [(1024, 37), (1024, 1), (9, 700)])
def test_pitch_transform_rows_against_fp64(mode, N, T):
    f0, rate, shift, inton = _f0_rows(N, T, 11 * N + T + mode)
    got = MS.pitch_transform_rows_(f0.to(DEV), mode, rate.to(DEV), shift.to(DEV), inton.to(DEV)).cpu()
    ref = torch.empty(N, 1, T, dtype=torch.float64)
    for n in range(N):
        x = f0[n].double()
        if mode == 0:
            ref[n] = O.pitch_transform_offline(x, float(shift[n]), float(inton[n]), float(rate[n]))
        else:
            ref[n] = O.pitch_transform_realtime(x * float(rate[n]), float(shift[n]))
    assert bool((got[0] == 0).all())                                    # all unvoiced -> zeros
    zero = ref == 0
    assert torch.equal(got == 0, zero), "zeros differ"
    rel = ((got.double() - ref).abs() / ref.abs().clamp_min(1e-300))[~zero]
    assert rel.numel() > 0 and rel.max().item() <= 2e-6, rel.max().item()


def _filt64(orig, new):
    """oracle/alive_oracle.py:resample_filter's windowed sinc, in fp64 without the final rounding"""
    base = min(orig, new) * 0.99
    width = math.ceil(6 * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx[None]
    t = np.clip(t * base, -6, 6)
    window = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0, 1.0, np.sin(t) / t)
    return s * window * (base / orig), width


def _resample64(x, orig, new, pre, post):
    """y[b][m * new + p] = post_b * sum_j h[p][j] * pre_b * x[b][m * orig + j - width], zero outside the input"""
    h, width = _filt64(orig, new)
    B, L = x.shape
    taps = h.shape[1]
    lout = -(-new * L // orig)
    xp = np.pad(x * pre[:, None], ((0, 0), (width, width + orig)))
    nm = -(-lout // new)
    win = np.lib.stride_tricks.sliding_window_view(xp, taps, axis=1)[:, ::orig][:, :nm]
    y = np.tensordot(win, h, axes=([2], [1])).reshape(B, nm * new)[:, :lout]
    return y * post[:, None]


@pytest.mark.parametrize("rates", [(24000, 16000), (44100, 16000), (16000, 48000)])
@pytest.mark.parametrize("B,L", [(1, 4801), (1024, 1601), (5, 13), (3, 300), (4, 441 * 7 + 5)])
def test_resample_rows_against_fp64(rates, B, L):
    orig, new = audio_io._reduced(*rates)
    taps = int(nat.lib().alive_resample_taps(orig, new))
    g = torch.Generator().manual_seed(B * 7 + L)
    x = torch.randn(B, L, generator=g) * 0.3
    pre_db = [0.0 if b % 3 == 0 else float(v) for b, v in enumerate(torch.rand(B, generator=g) * 12 - 6)]
    post_db = [0.0 if b % 2 == 0 else float(v) for b, v in enumerate(torch.rand(B, generator=g) * 12 - 6)]
    assert MS.db_scale(0.0) == 1.0
    pre = torch.tensor([MS.db_scale(v) for v in pre_db], dtype=torch.float32)
    post = torch.tensor([MS.db_scale(v) for v in post_db], dtype=torch.float32)
    got = MS.resample_rows(x.to(DEV), *rates, pre.to(DEV), post.to(DEV)).cpu()
    ref = _resample64(x.double().numpy(), orig, new, pre.double().numpy(), post.double().numpy())
    assert got.shape == ref.shape
    err = np.abs(got.double().numpy() - ref).max(axis=1)
    bar = 2e-6 * np.maximum(1.0, np.abs(ref).max(axis=1))
    assert (err <= bar).all(), (int(np.argmax(err / bar)), float(err.max()))
    if L < taps:
        assert ref.shape[1] == -(-new * L // orig)                      # (an input shorter than the filter)
    b0 = 0                                                              # 0 dB in and out: the plain resampler bitwise
    assert torch.equal(got[b0:b0 + 1], audio_io.resample(x[b0:b0 + 1].to(DEV), *rates).cpu())
    # equal rates: the gains alone, (x * pre) * post in fp32
    same = MS.resample_rows(x.to(DEV), rates[0], rates[0], pre.to(DEV), post.to(DEV)).cpu()
    assert torch.equal(same, (x * pre[:, None]) * post[:, None])


# ---------------------------------------------------------------------------------------------------- 4. 1024 slots
def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _sds():
    from module import schema
    return tuple(synthetic.make_state_dict(s, 2, p) for s, p in ((schema.content_encoder_schema(), "ce."),
                                                                (schema.f0_estimator_schema(), "pe."),
                                                                (schema.decoder_schema(), "dec.")))


def test_converter_at_1024_slots():
    chunk, bs, B = 160, 16, 1024
    ticks = bs + 3
    names = [f"v{i}" for i in range(8)]
    voices = {n: synthetic.make_library(m, 60 + i) for i, (n, m) in enumerate(zip(names, (50_000, 300, 700, 1000, 1500, 2000,
                                                                                          3000, 5000)))}
    conv = MS.MultiStreamConverter(*_nets(), MS.VoicePool(voices), B, chunk=chunk, buffersize=bs, k=4).enable_graph()
    trio = (0, 511, 1023)
    base = [(synthetic.make_waveform(chunk * ticks + 2000, 900 + i)[0].numpy() * 12000).astype(np.int16) for i in range(16)]
    pcm = [np.ascontiguousarray(base[s % 16][(37 * s) % 2000:][:chunk * ticks]) for s in range(B)]
    sess = [dict(voice=names[s % 8], pitch=float(s % 7 - 3), f0_rate=0.5 + 0.1 * (s % 4), alpha=0.1 * (s % 3)) for s in range(B)]
    for s in trio:
        pcm[s] = pcm[0]
        sess[s] = dict(voice="v0", pitch=1.5, f0_rate=0.75, alpha=0.2)
    closed = [s for s in range(B) if s % 2 == 1 and s not in trio]      # half the slots close on tick bs + 1 ...
    switched = {s: names[(s + 3) % 8] for s in range(B) if s % 4 == 2}   # ... and a quarter switch voices
    outs = [[] for _ in range(B)]
    live = set(range(B))
    for tick in range(ticks):
        if tick == 0:
            for s in range(B):
                conv.open(s, **sess[s])
        if tick == bs + 1:
            for s in closed:
                conv.close(s)
                live.discard(s)
            for s, v in switched.items():
                conv.set(s, voice=v)
        res = conv.step({s: pcm[s][tick * chunk:(tick + 1) * chunk] for s in live})
        assert set(res) == live
        for s, o in res.items():
            if o is not None:
                outs[s].append(o)
    assert conv.captures == 1
    assert all(len(outs[s]) == 3 for s in live) and all(len(outs[s]) == 1 for s in closed)
    for s in trio[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[s])), s
    # sampled sessions against the oracle's realtime step (one of them switches voice)
    ce, pe, dec = _sds()
    begin, end = O.realtime_geometry(chunk, bs, 16000)
    c = bs * chunk // 2
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    worst = 0.0
    for s in (0, 300, 514, 1020):
        p, phi, want = sess[s], 0, []
        for j in range(bs, ticks):
            voice = switched[s] if (s in switched and j >= bs + 1) else p["voice"]
            ring = torch.from_numpy(pcm[s][(j - bs + 1) * chunk:(j + 1) * chunk].astype(np.float32) / 32768)[None]
            wave, phi = O.realtime_step(ce, pe, dec, ring, voices[voice], phi, begin, end, k=4, alpha=p["alpha"],
                                        pitch_shift=p["pitch"], f0_rate=p["f0_rate"])
            want.append((wave[0].numpy() * 32768).astype(np.int16)[c - chunk // 2: c + chunk // 2])
        got = np.concatenate(outs[s]).astype(np.float64)
        want = np.concatenate(want).astype(np.float64)
        assert got.shape == want.shape, s
        worst = max(worst, float(np.sqrt(np.mean((got - want) ** 2)) / 32768))
    assert worst < 1e-3, worst
