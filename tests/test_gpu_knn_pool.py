"""The pool search (alive_knn_search_pool): every batch row against its own voice of a VoicePool in one call.

Contract: val and idx - seg_lo[voice[n]] are bitwise alive_knn_search_grouped on the same segments (within the grouped search's
limits: N <= 1024, N * T <= 2^20) and bitwise alive_knn_search_strict on the voice packed alone (beyond them, on a sample of rows).
Rows with voice -1, or on a voice shorter than k, get val -inf / idx -1.
"""
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
from module import multistream as MS                                 # noqa: E402
from module.common import PackedLibrary                              # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
VAL_TOL = 2e-6
SEP = 1e-5


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def make_voice(m, seed, dup=0):
    """tokens [768, m]; dup > 0: clusters of near-copies (and exact duplicates) of a few rows"""
    g = _gen(seed)
    t = torch.randn(768, m, device=DEV, generator=g) + 0.3
    if dup and m > 8:
        base = t[:, :4].clone()
        for j in range(4, m):
            if j % 3 == 0:
                t[:, j] = base[:, j % 4]                                           # exact duplicates
            elif j % 3 == 1:
                t[:, j] = base[:, j % 4] * (1 + 1e-4 * torch.randn(768, device=DEV, generator=g))   # near-copies
    return t


def make_source(pool, names, T, seed, noise=0.3):
    """[N, 768, T]: each frame a noisy copy of a row of its row's voice (rows without a voice: noise)"""
    g = _gen(seed)
    N = len(names)
    src = torch.randn(N, 768, T, device=DEV, generator=g)
    for n, name in enumerate(names):
        if name is None:
            continue
        lo, m = pool.segment(name)
        pick = torch.randint(0, m, (T,), device=DEV, generator=g) + lo
        src[n] = pool.rows[pick].T + noise * src[n] * pool.rows[pick].T.abs().mean()
    return src.contiguous()


def seg_tables(pool, names):
    lo = [pool.segment(n)[0] if n is not None else 0 for n in names]
    ln = [pool.segment(n)[1] if n is not None else 0 for n in names]
    return (torch.tensor(lo, dtype=torch.int32, device=DEV), torch.tensor(ln, dtype=torch.int32, device=DEV))


def grouped(pool, src, names, k):
    lo, ln = seg_tables(pool, names)
    return MS.knn_search_grouped(src, pool.rows, pool.norms, lo, ln, k)


def strict_rows(pool, voices, src, names, k, rows):
    """alive_knn_search_strict of each sampled row on its voice packed alone -> (val, idx + seg_lo) per row"""
    out = {}
    for n in rows:
        name = names[n]
        lo, m = pool.segment(name)
        lib = PackedLibrary(voices[name], strict=True)
        v, i = lib.search(src[n:n + 1], k)
        out[n] = (v, i + lo)
    return out


def assert_rows_equal(val, idx, ref, T):
    for n, (rv, ri) in ref.items():
        assert torch.equal(val[n * T:(n + 1) * T], rv), f"row {n}: values differ"
        assert torch.equal(idx[n * T:(n + 1) * T], ri), f"row {n}: indices differ"


def fp64_check(pool, src, names, val, idx, k, rows):
    rws = pool.rows.double()
    nr = rws / rws.norm(dim=1, keepdim=True)
    T = src.shape[2]
    for n in rows:
        lo, m = pool.segment(names[n])
        q = src[n].double().T
        q = q / q.norm(dim=1, keepdim=True)
        cos = q @ nr[lo:lo + m].T
        top = torch.topk(cos, min(k + 1, m), dim=1)
        for t in range(T):
            got = idx[n * T + t].long() - lo
            ref_at = cos[t, got]
            assert torch.all((val[n * T + t].double() - ref_at).abs() < VAL_TOL)
            if m > k and top.values[t, k - 1] - top.values[t, k] > SEP:
                assert set(got.tolist()) == set(top.indices[t, :k].tolist())


def pool_of(sizes, seed, dup=()):
    voices = {f"v{j}": make_voice(m, seed + j, dup=(j in dup)) for j, m in enumerate(sizes)}
    return MS.VoicePool(voices), voices


# ------------------------------------------------------------------------------------------------ bitwise vs grouped
@pytest.mark.parametrize("k", list(range(1, 9)))
def test_pool_matches_grouped_every_k_mixed_sizes(k):
    sizes = [k, k + 1, 127, 128, 129, 512, 4097]
    pool, voices = pool_of(sizes, 100 * k)
    names = [f"v{j % len(sizes)}" for j in range(29)]
    for T in (1, 37, 300):
        src = make_source(pool, names, T, 7 * k + T)
        val, idx = MS.knn_search_pool(src, pool, pool.voice_ids(names), k)
        gv, gi = grouped(pool, src, names, k)
        assert torch.equal(val, gv) and torch.equal(idx, gi), (k, T)


def test_pool_one_voice_shared_by_all_rows_is_strict():
    m, k, N, T = 50_000, 4, 64, 450
    pool, voices = pool_of([m], 5)
    names = ["v0"] * N
    src = make_source(pool, names, T, 11)
    val, idx = MS.knn_search_pool(src, pool, pool.voice_ids(names), k)
    lib = PackedLibrary(voices["v0"], strict=True)
    sv, si = lib.search(src, k)
    assert torch.equal(val, sv) and torch.equal(idx, si)
    gv, gi = grouped(pool, src, names, k)
    assert torch.equal(val, gv) and torch.equal(idx, gi)
    fp64_check(pool, src, names, val, idx, k, rows=[0, 31, 63])


def test_pool_every_row_its_own_voice():
    k = 5
    rng = np.random.default_rng(3)
    sizes = [int(s) for s in rng.integers(5, 700, 256)]
    pool, voices = pool_of(sizes, 900)
    names = [f"v{j}" for j in range(256)]
    for T in (1, 450):
        src = make_source(pool, names, T, 13 + T)
        val, idx = MS.knn_search_pool(src, pool, pool.voice_ids(names), k)
        gv, gi = grouped(pool, src, names, k)
        assert torch.equal(val, gv) and torch.equal(idx, gi), T


def test_pool_256_small_voices_and_two_large_beyond_grouped_limits():
    k = 4
    rng = np.random.default_rng(4)
    sizes = [int(s) for s in rng.integers(8, 600, 256)] + [50_000, 200_000]
    pool, voices = pool_of(sizes, 2000)
    N, T = 4096, 256                                          # N * T = 2^20, N beyond the grouped search's 1024 rows
    names = [f"v{(j * 37) % len(sizes)}" if j % 5 else ("v256" if j % 2 else "v257") for j in range(N)]
    src = make_source(pool, names, T, 21)
    val, idx, st = MS.knn_search_pool(src, pool, pool.voice_ids(names), k, stats=True)
    assert st["frame_blocks"] >= N * T // 256
    sample = [0, 1, 2, 5, 10, 1023, 2048, 4095]
    assert_rows_equal(val, idx, strict_rows(pool, voices, src, names, k, sample), T)
    fp64_check(pool, src, names, val, idx, k, rows=[5, 10])


def test_pool_grouped_regime_mixed_large():
    k = 8
    sizes = [200_000, 300] + [64] * 30
    pool, voices = pool_of(sizes, 77)
    names = [f"v{j % len(sizes)}" for j in range(1024)]
    src = make_source(pool, names, 3, 9)
    val, idx = MS.knn_search_pool(src, pool, pool.voice_ids(names), k)
    gv, gi = grouped(pool, src, names, k)
    assert torch.equal(val, gv) and torch.equal(idx, gi)


# ------------------------------------------------------------------------------------------------ the exact fallback
@pytest.mark.parametrize("k", [1, 4, 8])
def test_pool_duplicates_reach_the_exact_fallback(k):
    pool, voices = pool_of([3000, 512, 20_000], 300 + k, dup=(0, 1, 2))
    names = ["v0", "v1", "v2", "v0", "v2"] * 8
    src = make_source(pool, names, 200, 17, noise=0.0)        # frames ON the duplicated rows: ties and near-ties
    val, idx, st = MS.knn_search_pool(src, pool, pool.voice_ids(names), k, stats=True)
    assert st["frames_failed_certificate"] > 0 and st["frames_searched_exactly"] > 0, st
    gv, gi = grouped(pool, src, names, k)
    assert torch.equal(val, gv) and torch.equal(idx, gi)
    assert_rows_equal(val, idx, strict_rows(pool, voices, src, names, k, [0, 1, 2]), 200)


# ------------------------------------------------------------------------------------------------ edges
def test_pool_inactive_rows_and_short_voices():
    k = 4
    pool, voices = pool_of([k - 1, 600, k], 55)
    names = ["v1", None, "v0", "v2", "v1", None]
    src = make_source(pool, names, 40, 3)
    val, idx = MS.knn_search_pool(src, pool, pool.voice_ids(names), k)
    T = 40
    for n in (1, 2, 5):
        assert torch.all(idx[n * T:(n + 1) * T] == -1) and torch.all(val[n * T:(n + 1) * T] == -float("inf"))
    gv, gi = grouped(pool, src, names, k)
    assert torch.equal(val, gv) and torch.equal(idx, gi)


def test_pool_guard_voices_are_never_read():
    """the searched voice sits between guard voices whose rows ARE the frames: a read across a voice boundary wins"""
    k, T = 6, 300
    target = make_voice(5000, 1)
    g = _gen(2)
    src = torch.randn(8, 768, T, device=DEV, generator=g)
    guard = src.permute(1, 0, 2).reshape(768, -1).contiguous()
    pool = MS.VoicePool({"guard_lo": guard, "target": target, "guard_hi": guard.clone()})
    names = ["target"] * 8
    val, idx = MS.knn_search_pool(src, pool, pool.voice_ids(names), k)
    lo, m = pool.segment("target")
    assert int(idx.min()) >= lo and int(idx.max()) < lo + m
    sv, si = PackedLibrary(target, strict=True).search(src, k)
    assert torch.equal(val, sv) and torch.equal(idx - lo, si)


def test_pool_guard_bands_workspace_reuse_and_repeats():
    k = 4
    L = nat.lib()
    pool_a, _ = pool_of([700, 50_000, 90], 61)
    pool_b, _ = pool_of([20, 3000], 62)
    names_a = ["v0", "v1", "v2", "v1"] * 16
    names_b = ["v1", "v0"] * 300
    src_a = make_source(pool_a, names_a, 450, 1)
    src_b = make_source(pool_b, names_b, 7, 2)
    ref_a = MS.knn_search_pool(src_a, pool_a, pool_a.voice_ids(names_a), k)

    def raw(src, pool, names, ws):
        n, _, t = src.shape
        im = pool.search_images()
        G = 4096
        val = torch.full((n * t * k + 2 * G,), 12345.0, device=DEV)
        idx = torch.full((n * t * k + 2 * G,), 777, dtype=torch.int32, device=DEV)
        ids = pool.voice_ids(names)
        nat.check(L.alive_knn_search_pool(nat.ptr(src), n, t, nat.ptr(im["images"]), nat.ptr(im["img_off"]), nat.ptr(pool.rows),
                                          nat.ptr(pool.norms), nat.ptr(im["bounds"]), pool.P, nat.ptr(im["seg_lo"]),
                                          nat.ptr(im["seg_len"]), len(im["names"]), im["max_len"], nat.ptr(ids), k,
                                          val[G:].data_ptr(), idx[G:].data_ptr(), nat.ptr(ws), nat.stream()), "pool")
        torch.cuda.synchronize()
        assert torch.all(val[:G] == 12345.0) and torch.all(val[G + n * t * k:] == 12345.0)
        assert torch.all(idx[:G] == 777) and torch.all(idx[G + n * t * k:] == 777)
        return val[G:G + n * t * k].view(-1, k).clone(), idx[G:G + n * t * k].view(-1, k).clone()

    nb = max(MS.knn_pool_workspace_bytes(64, 450, k, pool_a), MS.knn_pool_workspace_bytes(600, 7, k, pool_b))
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV)
    raw(src_b, pool_b, names_b, ws)                                     # a different plan first
    runs = [raw(src_a, pool_a, names_a, ws) for _ in range(3)]
    for v, i in runs:
        assert torch.equal(v, ref_a[0]) and torch.equal(i, ref_a[1])
