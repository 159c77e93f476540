"""Half-precision voice pool on the device: every kernel that reads a pool's row table, on an fp16 table H against its fp32 twin on
H.float() with the same norms.  fp16 -> fp32 is exact and the half kernels widen in registers before the twin's arithmetic in the
twin's order, so every comparison here is BITWISE; the one exception is test 6, whose bound is derived in its docstring.

1. alive_pool_append_f16: the stored halves against the CPU's round-to-nearest-even (tok.cpu().half()), the norms against
   alive_pool_append on tok.half().float(), guard rows, the two-word report.
2. alive_pool_move_rows_f16 against a host copy of the bytes.
3. alive_knn_search_grouped(_k)_f16, eager and replayed from a captured graph.
4. alive_knn_merge_gather_rows(_k)_f16 and alive_knn_blend_gather_rows(_k)_f16.
5. alive_knn_path_rows_f16.
6. a half pool against an fp32 pool of the UNROUNDED tokens: the derived bound.
7. MultiStreamConverter over a half pool against one over an fp32 pool of tokens.half().float(): byte-identical PCM.
8. multistream_inference.py --pool-dtype fp16.

The tables are the guard-row tables of test_gpu_voice_enrol.py: every row outside the range a call may touch is the direction all
frames lean to, so a row read or written out of place is every frame's best match."""
import json
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

from module import _native as nat                                    # noqa: E402
from module import audio_io, ops, schema, synthetic                  # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64                   # guard rows on either side of the rows a call may write
F16, F32, I32, F64 = torch.float16, torch.float32, torch.int32, torch.float64


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


def _bits(t):
    """the bytes of a tensor as integers: equality of bits, so that -0.0 != +0.0 and a NaN equals itself"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _t(v, dtype=I32):
    return torch.tensor(v, dtype=dtype, device=DEV)


def _guarded_half_table(cap, seed=3):
    """rows fp16 [cap, 768] / norms[cap] where EVERY row is the (rounded) direction u that every frame of the tests leans to"""
    u = _randn(768, seed=seed).half()
    return u[None, :].expand(cap, 768).contiguous(), torch.full((cap,), float(u.float().norm()), device=DEV), u


# ---------------------------------------------------------------------------------------------------- 1. alive_pool_append_f16
# exact ties (the even neighbour wins), fp16's subnormal range (spacing 2^-24; 2^-25 is the tie between 0 and the least subnormal),
# the least normal, signed zeros, and the top of the range (65520 is the tie that would round to inf: stay just under it)
SPECIALS = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11), 2048.0 + 1.0, 2048.0 + 3.0,
            2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 3e-6, -4.7e-7, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -26,
            1e-9, -1e-9, 0.0, -0.0, 65504.0, 65503.9, 65519.0, -65519.9, 65488.0, 65496.0, 0.1, 1.0 / 3.0]


def _append16(tok, rows, norms, at, report, cap=None):
    return nat.lib().alive_pool_append_f16(tok.data_ptr(), tok.stride(0), tok.stride(1), tok.shape[1], tok.shape[0], nat.ptr(rows),
                                           nat.ptr(norms), rows.shape[0] if cap is None else cap, at, nat.ptr(report), nat.stream())


def _append32(tok, rows, norms, at, report):
    return nat.lib().alive_pool_append(tok.data_ptr(), tok.stride(0), tok.stride(1), tok.shape[1], tok.shape[0], nat.ptr(rows),
                                       nat.ptr(norms), rows.shape[0], at, nat.ptr(report), nat.stream())


def _views(m, seed):
    """the same [768, m] tokens, the SPECIALS among them, three ways: contiguous, a column slice of a wider matrix (row-strided) and
    the every-4th-frame view of an encoder-output-like [768, 4 m - 3] (column-strided)"""
    base = _randn(768, m, seed=seed)
    sp = torch.tensor(SPECIALS, dtype=F32, device=DEV)
    for rep in range(3):                                     # three places each, spread over the features and the tokens
        d = torch.arange(len(SPECIALS), device=DEV) * 7 + 250 * rep
        base[d, (torch.arange(len(SPECIALS), device=DEV) + 11 * rep) % m] = sp
    wide = _randn(768, m + 37, seed=seed + 1)
    wide[:, 11:11 + m] = base
    frames = _randn(768, 4 * m - 3, seed=seed + 2)
    frames[:, ::4] = base
    return base, {"contiguous": base, "row-strided": wide[:, 11:11 + m], "column-strided": frames[:, ::4]}


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_pool_append_f16_rounds_as_the_cpu_and_takes_the_norms_of_the_rounded_rows(m):
    base, views = _views(m, 100 + m)
    want_rows = base.cpu().half().t().contiguous().to(DEV)                  # the CPU's round to nearest even
    assert _same(want_rows, base.half().t().contiguous())                   # (and the device's conversion agrees with it)
    rounded = base.half().float()
    want_norms = torch.empty(m, device=DEV)
    report = torch.full((2,), 7, dtype=I32, device=DEV)
    assert _append32(rounded, torch.empty(m, 768, device=DEV), want_norms, 0, report) == 0
    assert report.tolist() == [0, 2 ** 31 - 1]
    cap = m + 2 * G
    for how, tok in views.items():
        assert m == 1 or tok.stride() == {"contiguous": (m, 1), "row-strided": (m + 37, 1), "column-strided": (4 * m - 3, 4)}[how]
        for at in (0, 1, G, cap - m):
            rows, norms, u = _guarded_half_table(cap)
            report.fill_(7)
            assert _append16(tok, rows, norms, at, report) == 0, nat.lib().alive_last_error()
            assert _same(rows[at:at + m], want_rows), (how, at)
            assert _same(norms[at:at + m], want_norms), (how, at)
            outside = torch.ones(cap, dtype=torch.bool, device=DEV)
            outside[at:at + m] = False
            assert bool((_bits(rows[outside]) == _bits(u)).all()) and bool((norms[outside] == float(u.float().norm())).all()), (how, at)
            assert report.tolist() == [0, 2 ** 31 - 1]


def test_pool_append_f16_reports_rows_beyond_the_range_and_rows_that_round_to_zero():
    m, at = 200, 17
    rows, norms, _ = _guarded_half_table(m + 2 * G)
    report = torch.zeros(2, dtype=I32, device=DEV)
    tok = _randn(768, m, seed=5)
    assert _append16(tok, rows, norms, at, report) == 0 and report.tolist() == [0, 2 ** 31 - 1]
    big = tok.clone()
    big[300, 70] = 70000.0                                  # finite in fp32, inf in fp16
    assert _append16(big, rows, norms, at, report) == 0
    assert report.tolist() == [1, at + 70] and math.isinf(float(norms[at + 70])) and math.isinf(float(rows[at + 70, 300]))
    tiny = tok.clone()
    tiny[:, 131] = 1e-9                                     # a norm of 2.8e-8 in fp32, all zeros in fp16
    assert _append16(tiny, rows, norms, at, report) == 0
    assert report.tolist() == [1, at + 131] and float(norms[at + 131]) == 0.0
    both = big.clone()
    both[:, 131] = 1e-9
    both[5, 199] = float("nan")
    assert _append16(both, rows, norms, at, report) == 0
    assert report.tolist() == [3, at + 70]                   # the lowest of them
    # the fp32 append takes the same rows without a word: the report is about what the half table holds
    assert _append32(both[:, :199].contiguous(), torch.empty(m + 2 * G, 768, device=DEV), norms.clone(), at, report) == 0
    assert report.tolist() == [0, 2 ** 31 - 1]
    # through the pool: the voice is refused and the pool is as it was
    pool = MS.VoicePool({"a": _randn(768, 10, seed=6)}, capacity=500, dtype=F16)
    for bad in (big, tiny):
        with pytest.raises(ValueError, match=r"row \d+ has zero or non-finite norm \(1 such.*fp16"):
            pool.add("bad", bad)
        assert pool.segments == {"a": (0, 10)} and pool.free_rows == 490
    with pytest.raises(ValueError, match="row 80 has zero or non-finite norm"):
        MS.VoicePool({"a": _randn(768, 10, seed=6), "bad": big}, dtype=F16)         # a default half pool: the same append


def test_pool_append_f16_refuses_rows_past_the_capacity_and_writes_nothing():
    m = 100
    tok = _randn(768, m, seed=8)
    rows, norms, u = _guarded_half_table(m + 2 * G)
    report = torch.full((2,), 7, dtype=I32, device=DEV)
    for cap, at in ((m + G, G + 1), (m - 1, 0), (m + G, m + G)):
        assert _append16(tok, rows, norms, at, report, cap=cap) == -1
        assert b"outside the table" in nat.lib().alive_last_error()
    torch.cuda.synchronize()
    assert bool((_bits(rows) == _bits(u)).all()) and report.tolist() == [7, 7]


# ---------------------------------------------------------------------------------------------------- 2. alive_pool_move_rows_f16
@pytest.mark.parametrize("n", [1, 5, 64, 1000])
def test_pool_move_rows_f16_is_bitwise_a_host_copy_for_overlapping_ranges(n):
    cap = 2 * n + 3 + 2 * G
    table, tnorms = _randn(cap, 768, seed=n).half(), _randn(cap, seed=n + 1)
    moves = [(G, G + n + 3), (G + n + 3, G),                                 # disjoint, up and down
             (G + 1, G), (G, G + 1),                                         # by one row
             (G + n - 1, G), (G, G + n - 1), (G + n, G), (G, G + n),         # by n - 1 and n rows
             (G + n // 3 + 1, G), (G, G + n // 3 + 1)]                       # by about a third of the range
    for src, dst in moves:
        rows, norms = table.clone(), tnorms.clone()
        want_rows, want_norms = table.cpu(), tnorms.cpu()
        want_rows[dst:dst + n] = table.cpu()[src:src + n]
        want_norms[dst:dst + n] = tnorms.cpu()[src:src + n]
        nat.check(nat.lib().alive_pool_move_rows_f16(nat.ptr(rows), nat.ptr(norms), cap, src, dst, n, nat.stream()))
        assert _same(rows.cpu(), want_rows), (n, src, dst)                   # bytes: guards included
        assert _same(norms.cpu(), want_norms), (n, src, dst)
    rows = table.clone()
    assert nat.lib().alive_pool_move_rows_f16(nat.ptr(rows), nat.ptr(tnorms), cap, cap - n + 1, 0, n, nat.stream()) == -1
    assert nat.lib().alive_pool_move_rows_f16(nat.ptr(rows), nat.ptr(tnorms), cap, 0, cap - n + 1, n, nat.stream()) == -1
    assert _same(rows, table)


# ---------------------------------------------------------------------------------------------------- 3. grouped search
SEGS = {"one": 1, "eight": 8, "dup63": 63, "s300": 300, "s5000": 5000, "s20011": 20011, "tail": 40}


@pytest.fixture(scope="module")
def table():
    """one half table H with its norms, its widened fp32 copy, and the segments: guard rows before, between and behind them; `tail`
    ends at the table's last row (lo + len = P); dup63 holds three distinct rows 21 times each (ties go to the lower row)"""
    u = _randn(768, seed=3)
    seg, at = {}, G
    for name, m in SEGS.items():
        seg[name] = (at, m)
        at += m + (G if name != "tail" else 0)
    P = at
    tok = u[None, :].expand(P, 768).clone()                                                      # every row the guard ...
    for i, (name, (lo, m)) in enumerate(seg.items()):                                           # ... but the segments
        tok[lo:lo + m] = _randn(m, 768, seed=20 + i) + (0.5 * u[None, :] if name != "dup63" else 0.0)
    lo, m = seg["dup63"]
    tok[lo:lo + m] = (_randn(3, 768, seed=30) + 0.5 * u[None, :])[torch.arange(m, device=DEV) % 3]
    H = torch.empty(P, 768, dtype=F16, device=DEV)
    norms = torch.empty(P, device=DEV)
    report = torch.zeros(2, dtype=I32, device=DEV)
    assert _append16(tok.t(), H, norms, 0, report) == 0 and report.tolist() == [0, 2 ** 31 - 1]
    return dict(H=H, W=H.float(), norms=norms, seg=seg, P=P, u=u)


def _frames(tb, n, t, seed):
    return (40.0 * tb["u"][None, :, None] + _randn(n, 768, t, seed=seed)).contiguous()


def _both(fn, tb, *before, after=()):
    """fn(..., rows, ...) on the half table and on its widened copy"""
    return fn(*before, tb["H"], *after), fn(*before, tb["W"], *after)


def _segments(tb, names):
    lo = [tb["seg"][n][0] if isinstance(n, str) else n[0] for n in names]
    ln = [tb["seg"][n][1] if isinstance(n, str) else n[1] for n in names]
    return _t(lo), _t(ln)


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("T", [1, 24])
@pytest.mark.parametrize("N", [1, 3, 16])
def test_grouped_search_f16_is_bitwise_the_fp32_search_of_the_widened_table(table, k, T, N):
    tb = table
    lo8, P = tb["seg"]["s300"][0], tb["P"]
    mix = ["s300", "one", "eight", "dup63", "s5000", "tail", "s20011", "dup63",
           (lo8, k), (lo8, k - 1), (lo8, 0), (P - k, k), "s300", (P - 7, 8), "s5000", "eight"]     # len = k, k - 1, 0, lo + len = P, past P
    names = {1: ["s20011"], 3: ["dup63", "s300", "tail"], 16: mix}[N]
    lo, ln = _segments(tb, names)
    src = _frames(tb, N, T, seed=1000 + 100 * k + 10 * T + N)
    (hv, hi), (wv, wi) = _both(lambda rows: MS.knn_search_grouped(src, rows, tb["norms"], lo, ln, k), tb)
    assert _same(hv, wv) and torch.equal(hi, wi)
    for r, nm in enumerate(names):                           # active exactly where the segment lies in the table and has k rows
        a, m = (tb["seg"][nm] if isinstance(nm, str) else nm)
        active = m >= k and m > 0 and a + m <= P
        got = hi[r * T:(r + 1) * T]
        assert bool((got >= 0).all()) == active and (active or bool((got == -1).all())), (r, nm)
        if active:
            assert bool(((got >= a) & (got < a + m)).all()), (r, nm)         # never a guard row
    if N == 3:                                               # dup63: equal scores, the lower row first
        v, i = hv[:T], hi[:T]
        a = tb["seg"]["dup63"][0]
        if k > 1:
            tied = v[:, 1:] == v[:, :-1]
            assert bool(tied.any()) and bool((i[:, 1:][tied] > i[:, :-1][tied]).all())
        assert bool((i[:, 0] < a + 3).all())                 # the best match is one of the first three: every later copy ties with it
    # every row inactive: the outputs are written all the same
    zero = torch.zeros(N, dtype=I32, device=DEV)
    (hv, hi), (wv, wi) = _both(lambda rows: MS.knn_search_grouped(src, rows, tb["norms"], lo, zero, k), tb)
    assert bool((hv == -math.inf).all()) and bool((hi == -1).all()) and _same(hv, wv) and torch.equal(hi, wi)


@pytest.mark.parametrize("T", [1, 24])
def test_grouped_search_k_f16_with_a_k_per_row(table, T):
    tb = table
    names = ["s300", "s300", "dup63", "one", "eight", "s5000", "tail", "s20011", "eight", "s300", "dup63"]
    k_row = [1, 8, 3, 1, 8, 5, 2, 4, 9, 0, 7]                # (9 and 0: outside [1, k_max], the rows are inactive)
    lo, ln = _segments(tb, names)
    src = _frames(tb, len(names), T, seed=77 + T)
    kr = _t(k_row)
    (hv, hi), (wv, wi) = _both(lambda rows: MS.knn_search_grouped_k(src, rows, tb["norms"], lo, ln, kr, 8), tb)
    assert _same(hv, wv) and torch.equal(hi, wi)
    for r, kk in enumerate(k_row):
        got = hi[r * T:(r + 1) * T]
        if 1 <= kk <= 8:
            assert bool((got[:, :kk] >= 0).all()) and bool((got[:, kk:] == -1).all()), r
            uv, ui = MS.knn_search_grouped(src[r:r + 1].contiguous(), tb["H"], tb["norms"], lo[r:r + 1], ln[r:r + 1], kk)
            assert _same(hv[r * T:(r + 1) * T, :kk].contiguous(), uv) and torch.equal(got[:, :kk], ui), r
        else:
            assert bool((got == -1).all()), r


@pytest.mark.parametrize("k", [4])
def test_grouped_search_f16_replays_from_a_captured_graph_over_changing_tables(table, k):
    tb = table
    N, T = 16, 24
    tables = [["s300", "dup63", "s5000", "tail"] * 4, ["s20011", "one", (0, 0), "eight"] * 4]
    src = _frames(tb, N, T, seed=5)
    lo_t, ln_t = torch.zeros(N, dtype=I32, device=DEV), torch.zeros(N, dtype=I32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # the workspace of the capture stream exists first
        for _ in range(2):
            MS.knn_search_grouped(src, tb["H"], tb["norms"], lo_t, ln_t, k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gv, gi = MS.knn_search_grouped(src, tb["H"], tb["norms"], lo_t, ln_t, k)
    for names in tables + tables[:1]:
        lo, ln = _segments(tb, names)
        lo_t.copy_(lo)
        ln_t.copy_(ln)
        graph.replay()
        torch.cuda.synchronize()
        wv, wi = MS.knn_search_grouped(src, tb["W"], tb["norms"], lo, ln, k)
        assert _same(gv, wv) and torch.equal(gi, wi)
        assert bool((gi.view(N, T, k)[0] >= 0).all())
    del graph


# ---------------------------------------------------------------------------------------------------- 4. gathers
def _lists(tb, rows_n, T, k, seed, dead=()):
    """top-k lists [rows_n * T, k] as a search returns them, over the whole table (guard rows included: a gather reads what it is
    told to); the list rows in `dead` are inactive (-inf / -1)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.randint(0, tb["P"], (rows_n * T, k), device=DEV, generator=g, dtype=torch.int64).to(I32)
    val = torch.rand(rows_n * T, k, device=DEV, generator=g).sort(dim=1, descending=True).values
    for r in dead:
        idx[r * T:(r + 1) * T] = -1
        val[r * T:(r + 1) * T] = -math.inf
    return val.contiguous(), idx.contiguous()


@pytest.mark.parametrize("N,T", [(3, 5), (4, 520)], ids=["few-frames", "many-frames"])       # 12 feature slabs per block / one block walks all
def test_merge_gather_rows_f16_is_bitwise_the_fp32_gather_of_the_widened_table(table, N, T):
    tb = table
    assert ((T + 31) // 32 * N < 64) == (T == 5)
    src = _randn(N, 768, T, seed=40 + T)
    alpha = _t([0.0, 1e-8, 1.0, 0.3][:N], F64)
    for k in range(1, 9):
        val, idx = _lists(tb, N, T, k, seed=50 + k, dead=(1,))
        idx[2 * T + 1, k - 1] = -1                           # a list that ends early: the kernel's NaN row, on both sides
        got, want = _both(lambda rows: MS.merge_gather_rows(val, idx, k, alpha, rows, src), tb)
        assert _same(got, want), k
        assert _same(got[1], src[1])                         # the frame without a match passes its source through
        assert bool(torch.isfinite(got[0]).all()) and not _same(got[0], src[0])
        # per-row k at k_max = 8: lists at stride 8, row n's mean over its own k
        val8, idx8 = _lists(tb, N, T, 8, seed=60 + k, dead=(1,))
        kr = _t([k, 8, (k % 8) + 1, 9][:N])                  # (9: out of range, the row passes through)
        got, want = _both(lambda rows: MS.merge_gather_rows_k(val8, idx8, kr, 8, alpha, rows, src), tb)
        assert _same(got, want), k
        one = MS.merge_gather_rows(val8[:T, :k].contiguous(), idx8[:T, :k].contiguous(), k, alpha[:1], tb["H"], src[:1].contiguous())
        assert _same(got[:1], one), k                        # row 0 at its own k


@pytest.mark.parametrize("N,T", [(3, 5), (4, 520)], ids=["few-frames", "many-frames"])
def test_blend_gather_rows_f16_is_bitwise_the_fp32_gather_of_the_widened_table(table, N, T):
    tb = table
    sizes = [1, 2, 4, 2][:N]                                 # 1-, 2- and 4-voice blends
    first = _t(np.concatenate([[0], np.cumsum(sizes)]).tolist())
    R = sum(sizes)
    w = torch.rand(R, dtype=F64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    for n in range(N):
        a, b = int(first[n]), int(first[n + 1])
        w[a:b] /= w[a:b].sum()
    src = _randn(N, 768, T, seed=70 + T)
    alpha = _t([0.0, 1e-8, 1.0, 0.3][:N], F64)
    dead = (1, 4) if N == 3 else (1, 4, 7, 8)                # one list of blend 1, one of blend 2, and (N = 4) all of blend 3
    for k in range(1, 9):
        val, idx = _lists(tb, R, T, k, seed=80 + k, dead=dead)
        got, want = _both(lambda rows: MS.blend_gather_rows(val, idx, k, first, w, alpha, rows, src), tb)
        assert _same(got, want), k
        if N == 4:
            assert _same(got[3], src[3])                     # no active list: the source
        val8, idx8 = _lists(tb, R, T, 8, seed=90 + k, dead=dead)
        kr = _t([k, 8, (k % 8) + 1, 3][:N])
        got, want = _both(lambda rows: MS.blend_gather_rows_k(val8, idx8, kr, 8, first, w, alpha, rows, src), tb)
        assert _same(got, want), k
    # one list at weight 1: the merge gather
    val, idx = _lists(tb, N, T, 4, seed=99)
    ones = torch.ones(N, dtype=F64, device=DEV)
    got = MS.blend_gather_rows(val, idx, 4, _t(list(range(N + 1))), ones, alpha, tb["H"], src)
    assert _same(got, MS.merge_gather_rows(val, idx, 4, alpha, tb["H"], src))


# ---------------------------------------------------------------------------------------------------- 5. match path
@pytest.mark.parametrize("k_max", [4, 8])
def test_path_rows_f16_is_bitwise_the_fp32_path_on_the_widened_table(table, k_max):
    tb = table
    R, T = 4, 33
    lo, m = tb["seg"]["s300"]
    g = torch.Generator(device=DEV).manual_seed(k_max)
    # candidates from a narrow range, so that consecutive frames share rows and the join cost decides
    idx = (lo + torch.randint(0, 40, (R * T, k_max), device=DEV, generator=g, dtype=torch.int64)).to(I32)
    val = (0.9 + 0.02 * torch.rand(R * T, k_max, device=DEV, generator=g)).sort(dim=1, descending=True).values.contiguous()
    idx[5] = -1                                              # an inactive frame cuts row 0's path in two
    val[5] = -math.inf
    k_row = _t([k_max, 2, k_max - 1, 3])
    on = _t([1, 1, 1, 0])
    moved_any = False
    for weight in ([0.0] * R, [1.0] * R, [0.0, 1.0, 0.25, 1.0]):
        wt = _t(weight, F64)
        (hv, hi, hm), (wv, wi, wm) = _both(lambda rows: ops.knn_path_rows(val, idx, k_row, k_max, on, wt, rows, tb["norms"]), tb)
        assert _same(hv, wv) and torch.equal(hi, wi) and torch.equal(hm, wm), weight
        assert bool((hi[:, 1:][:3 * T] == -1).all()) and int(hm[3]) == 0
        assert _same(hv[3 * T:], val[3 * T:]) and torch.equal(hi[3 * T:], idx[3 * T:])          # the row that is off: copied
        if not any(weight):
            assert hm.tolist() == [0] * R and torch.equal(hi[:3 * T, 0], idx[:3 * T, 0])
        moved_any = moved_any or int(hm.sum()) > 0
    assert moved_any                                         # the join cost moved some frame off its best candidate


# ---------------------------------------------------------------------------------------------------- 6. the derived bound
def test_half_pool_against_the_unrounded_pool_stays_within_the_rounding_bound():
    """The one comparison that is not bitwise: a half pool against an fp32 pool of the UNROUNDED tokens (randn rows, 5000 x 768,
    k = 4, 96 frames 0.5 row + randn).  Rounding x to fp16 moves it by at most b(x) = 2^-11 |x| for |x| >= 2^-14 (half an ulp of an
    11-bit significand) and by at most 2^-25 below (half the subnormal spacing 2^-24).  On a frame whose top-k index SETS agree the
    gathered feature (alpha = 0) is the mean of the same k rows on both sides, so the two means differ by at most mean_j b(row_j[d])
    in exact arithmetic; each side then rounds its mean to fp32 once more, which the slack 2^-24 (|mean_half| + |mean_full|) covers.
    At most 2 % of the frames may be left out for differing sets (the construction leaves out 0 of 96 in fp64 on the CPU).
    On the MI355X: 0 of 96 frames left out, and the largest |half - full| / bound over 96 x 768 features is 0.84."""
    M, k, N, T = 5000, 4, 4, 24
    rows = _randn(M, 768, seed=123)
    pick = torch.randint(0, M, (N * T,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    frames = 0.5 * rows[pick] + _randn(N * T, 768, seed=124)                  # [N T, 768]
    src = frames.view(N, T, 768).permute(0, 2, 1).contiguous()
    tok = rows.t().contiguous()
    half, full = MS.VoicePool({"v": tok}, dtype=F16), MS.VoicePool({"v": tok})
    assert _same(half.rows, rows.half()) and _same(full.rows, rows)
    lo, ln = _t([0] * N), _t([M] * N)
    alpha = torch.zeros(N, dtype=F64, device=DEV)
    out, sets = [], []
    for pool in (half, full):
        val, idx = MS.knn_search_grouped(src, pool.rows, pool.norms, lo, ln, k)
        sets.append(idx.sort(dim=1).values)
        out.append(MS.merge_gather_rows(val, idx, k, alpha, pool.rows, src).permute(0, 2, 1).reshape(N * T, 768).double().cpu())
    agree = (sets[0] == sets[1]).all(dim=1).cpu()
    left_out = int((~agree).sum())
    print(f"frames left out for differing top-{k} sets: {left_out} of {N * T}")
    assert left_out <= 0.02 * N * T
    r = rows.double().cpu()[sets[1].long().cpu()]                             # [N T, k, 768]: the unrounded rows of each frame's set
    b = torch.where(r.abs() >= 2.0 ** -14, r.abs() * 2.0 ** -11, torch.full_like(r, 2.0 ** -25))
    bound = b.mean(dim=1) + 2.0 ** -24 * (out[0].abs() + out[1].abs())
    diff = (out[0] - out[1]).abs()
    worst = float((diff / bound)[agree].max())
    print(f"largest |half - full| / bound over {int(agree.sum())} frames x 768 features: {worst:.4f}")
    assert bool((diff <= bound)[agree].all()), worst
    assert float(diff[agree].max()) > 0.0                                     # (the two pools do hold different rows)


# ---------------------------------------------------------------------------------------------------- 7. converter
def _voices():
    return {n: synthetic.make_library(m, s)[0].to(DEV) for n, m, s in (("a", 600, 31), ("b", 400, 32), ("c", 500, 33), ("d", 350, 34))}


OPEN = {0: dict(voice="a", pitch=1.0, k=2), 1: dict(voice={"a": 2.0, "b": 1.0}, pitch=-2.0, alpha=0.2, k=4),
        2: dict(voice="b", match_path=True, path_weight=1.0, k=8)}
CONV = dict(chunk=160, buffersize=16, k=4, blend=2, k_max=8, match_path=True)
TICKS = 16 + 12                                              # the ring fills for 16 ticks, then 12 ticks emit


def _run(convs, ticks, between=None):
    """step the converters side by side on the same chunks; -> the number of ticks that emitted PCM, identical on all"""
    pcm = [_pcm(CONV["chunk"] * ticks, 500 + s) for s in range(3)]
    emitted = 0
    for tick in range(ticks):
        if between is not None:
            between(tick)
        feed = {s: pcm[s][tick * CONV["chunk"]:(tick + 1) * CONV["chunk"]] for s in OPEN}
        outs = [c.step(feed) for c in convs]
        for s in OPEN:
            assert len({o[s] is None for o in outs}) == 1, (tick, s)
            if outs[0][s] is not None:
                for o in outs[1:]:
                    assert o[s].dtype == np.int16 and o[s].tobytes() == outs[0][s].tobytes(), (tick, s)
                emitted += s == 0
    return emitted


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_converter_over_a_half_pool_emits_the_pcm_of_an_fp32_pool_of_the_rounded_tokens(graph):
    tok = _voices()
    first = {n: tok[n] for n in "ab"}
    half = MS.VoicePool(first, dtype=F16)
    full = MS.VoicePool({n: t.half().float() for n, t in first.items()})
    assert half.rows.dtype == F16 and half.row_bytes == 1536 and full.row_bytes == 3072 and half.P == full.P == 1000
    assert 2 * half.rows.numel() * half.rows.element_size() == full.rows.numel() * full.rows.element_size()
    assert _same(half.rows, full.rows.half()) and _same(half.rows.float(), full.rows) and _same(half.norms, full.norms)
    assert _same(half.tokens("a"), tok["a"].half().float()) and half.tokens("a").dtype == F32
    convs = [MS.MultiStreamConverter(*_nets(), p, 3, **CONV) for p in (half, full)]
    for c in convs:
        if graph:
            c.enable_graph()
        for s, p in OPEN.items():
            c.open(s, **p)
    assert _run(convs, TICKS) == 12
    assert [c.captures for c in convs] == [1 if graph else 0] * 2


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_reserved_half_pool_serves_through_add_extend_remove_and_compact_on_one_capture(graph):
    tok = _voices()
    pools = [MS.VoicePool(capacity=3000, dtype=F16), MS.VoicePool(capacity=3000)]
    rnd = [lambda t: t, lambda t: t.half().float()]          # the fp32 side is given the rounded tokens
    for p, f in zip(pools, rnd):
        p.add("c", f(tok["c"][:, :100]))                     # rows 0..99: removed later, so that compact has a hole to close
        p.add("b", f(tok["b"]))
        p.add("a", f(tok["a"][:, :400]))
    half, full = pools
    assert half.rows.dtype == F16 and half.rows.shape == (3000, 768) and half.row_bytes == 1536
    assert 2 * half.rows.numel() * half.rows.element_size() == full.rows.numel() * full.rows.element_size()
    ptr = half.rows.data_ptr()
    convs = [MS.MultiStreamConverter(*_nets(), p, 3, **CONV) for p in pools]
    for c in convs:
        if graph:
            c.enable_graph()
        for s, p in OPEN.items():
            c.open(s, **p)

    def between(tick):
        for p, f in zip(pools, rnd):
            if tick == 18:
                p.add("d", f(tok["d"]))                      # a voice is enrolled mid-stream
            if tick == 20:
                p.extend("a", f(tok["a"][:, 400:]))          # a voice grows under two sessions: d lies behind it, so it moves
            if tick == 22:
                p.remove("c")
            if tick == 24:
                p.compact()                                  # b moves down by 100 rows < its 400, a by 500 < its 600: both overlap
    assert _run(convs, TICKS, between) == 12
    assert half.segments == full.segments == dict(b=(0, 400), d=(400, 350), a=(750, 600))
    assert [c.captures for c in convs] == [1 if graph else 0] * 2
    assert half.rows.data_ptr() == ptr and half.version == 0 and half.layout == full.layout
    for n in "abd":
        lo, m = half.segment(n)
        assert _same(half.rows[lo:lo + m], tok[n].t().half().contiguous()) and _same(half.rows[lo:lo + m].float(), full.rows[lo:lo + m])
        assert _same(half.norms[lo:lo + m], full.norms[lo:lo + m]) and _same(half.tokens(n), full.tokens(n))


def _voice_files(d):
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    audio_io.save(str(d / "spk.wav"), synthetic.make_waveform(24000 * 3, 60).repeat(2, 1) * torch.tensor([[0.5], [0.25]]), 24000)
    return str(d / "spk.wav"), str(d / "voice_library.pt")


def test_enrol_voice_with_a_codebook_into_a_half_pool_is_add_of_the_rounded_centroids(tmp_path):
    spk, libf = _voice_files(tmp_path)
    CE = _nets()[0].to(DEV)
    wav, sr = audio_io.load(spk)
    (centroids,) = MS.voice_parts(CE, wav, sr, libf, codebook=64)
    assert centroids.shape == (768, 64)
    pool = MS.VoicePool({"other": _randn(768, 29, seed=2)}, capacity=200, dtype=F16)
    assert MS.enrol_voice(pool, "v", CE, wav, sr, lib=libf, codebook=64) == 64 and pool.segment("v") == (29, 64)
    want = MS.VoicePool({"other": _randn(768, 29, seed=2)}, capacity=200, dtype=F16).add("v", centroids.half().float())
    assert _same(pool.rows[:93], want.rows[:93]) and _same(pool.norms[:93], want.norms[:93])
    assert _same(pool.rows[29:93].cpu(), centroids.cpu().half().t().contiguous())
    full = MS.VoicePool(capacity=200).add("v", centroids.half().float())
    assert _same(pool.norms[29:93], full.norms[:64]) and _same(pool.tokens("v"), full.tokens("v"))


# ---------------------------------------------------------------------------------------------------- 8. the CLI
def test_multistream_cli_with_pool_dtype_fp16_writes_the_files_of_the_rounded_fp32_pool(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    for name, sd in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _sds()):
        torch.save(sd, d / name)
    _voice_files(d)
    for i in range(3):
        audio_io.save(str(d / f"in{i}.wav"), synthetic.make_waveform(9600 + 1600 * i, 50 + i) * 0.5, 16000)
    sessions = [dict(input="in0.wav", lib="voice_library.pt", pitch=2.0),
                dict(input="in1.wav", target="spk.wav", alpha=0.2, start=3),
                dict(input="in2.wav", blend=[dict(lib="voice_library.pt", weight=3), dict(target="spk.wav", weight=1)], start=5)]
    json.dump(sessions, open(d / "sessions.json", "w"))
    common = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt"),
              "-c", "320", "-b", "8", str(d / "sessions.json")]
    names = ["0_in0.wav", "1_in1.wav", "2_in2.wav"]

    def run(out, extra):
        outs = msi.main(["-o", str(d / out)] + extra + common)
        return outs, [open(d / out / n, "rb").read() for n in names]
    plain_outs, plain = run("half", ["--pool-dtype", "fp16"])
    assert all(len(w) > 44 + 2 * 320 for w in plain)
    _, reserved = run("half_reserved", ["--pool-dtype", "fp16", "--pool-rows", "2000"])
    assert reserved == plain
    _, no_graph = run("half_no_graph", ["--pool-dtype", "fp16", "--no-graph"])
    assert no_graph == plain
    # the Python API on an fp32 pool of the rounded tokens, built as the CLI builds its run
    dev = torch.device(DEV)
    PE, CE, Dec = (n.to(dev) for n in (_nets()[1], _nets()[0], _nets()[2]))
    for net, sd in zip((CE, PE, Dec), _sds()):
        net.load_state_dict(sd)
    ss = msi.load_sessions(str(d / "sessions.json"))
    pool = MS.VoicePool(device=dev)
    for s in ss:
        for target, lib in msi.session_sources(s):
            if msi.voice_name(target, lib) not in pool.segments:
                pool.add(msi.voice_name(target, lib), msi.voice_tokens(CE, target, lib, dev).half().float())
    conv = MS.MultiStreamConverter(CE, PE, Dec, pool, len(ss), chunk=320, buffersize=8, input_sr=16000, output_sr=16000, k=4, device=dev,
                                   rates=[16000], world_pitch=False, blend=msi.blend_size(ss), k_max=None, auto_pitch=False)
    conv.enable_graph()
    params = [dict(voice=msi.session_voice(s), pitch=s["pitch"], f0_rate=s["f0_rate"], alpha=s["alpha"], gain=s["gain"],
                   input_gain=s["input_gain"], rate=16000, world_pitch=s["world_pitch"], k=s["k"], auto_pitch=s["auto_pitch"]) for s in ss]
    want = msi.run(conv, [msi.input_pcm(s["input"], 16000, dev) for s in ss], [s["start"] for s in ss], 320, params)
    for i, (g, w) in enumerate(zip(plain_outs, want)):
        assert g.dtype == w.dtype == np.int16 and g.tobytes() == w.tobytes(), i
    # and an fp32 run of the unrounded tokens is another run: the flag did something
    fp32_outs, _ = run("full", [])
    assert any(g.tobytes() != w.tobytes() for g, w in zip(fp32_outs, plain_outs))
