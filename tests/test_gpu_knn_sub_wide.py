"""The wide form of the subspace fp6 candidate stage (csrc/knn.hip knn_sub6w_kernel: 128 stationary frames per wave, 512-frame blocks,
6-byte list entries) and its switch (alive_knn_sub_frames).

Frames lie in a subspace by construction: q = W h + b with a seeded 768 x 512 W of orthonormal columns (every coordinate of the unit
frame in the stage's basis then has standard deviation 1 / sqrt(513): 5.5 sigma below the e2m3 clip), and the library takes the form
with PackedLibrary.use_subspace(W, b).  No frame of the small cases is flagged; the tests assert it.

  stage     the kernel's candidate lists, read back from the search workspace under the 512-frame plan
            (alive_debug_knn_stage_view words 27 .. 31), against ONE float64 evaluation of the same e2m3 codes plus g rho -- per frame,
            library split and half-list as SETS (the lists are unordered): the reference of tests/test_gpu_knn_stage.py.
  search    (val, idx) under mode 512, mode 384 and a float64 brute force.
  index     the 16-bit tile offsets at their far end, and the hand-over to the 384-frame kernel beyond it, on the stage alone
            (alive_debug_knn_sub_stage cuts the library into ONE split, which no search does for a batch this small).
  seeded    153 600 frames: the rule takes the wide form by itself, seeded admission stays on, the results are mode 384's.

Tolerance of a stage score (as tests/test_gpu_knn_stage.py derives it): the MFMA sum of e2m3 products is exact in fp32, g 2^10 is exact,
the fold is one fma and the 4 index bits: 2^-18 (|integer part| + |2^10 g rho|).  Search values: the audit's 2e-6 against float64."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_codes as kc  # noqa: E402

from module import _native as nat  # noqa: E402
from module.common import PackedLibrary  # noqa: E402

pytestmark = pytest.mark.gpu

D, SUB = 768, 512
F6_SCALE = 32.0
H = 16                                    # entries per half-list


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True)
def _restore_switch():
    L = nat.lib()
    before = L.alive_knn_sub_frames(0)
    yield
    L.alive_knn_sub_frames(before if before else -1)


@functools.lru_cache(maxsize=None)
def _basis():
    g = torch.Generator().manual_seed(20261021)
    W = torch.linalg.qr(torch.randn(D, SUB, generator=g, dtype=torch.float64))[0].float().cuda().contiguous()
    b = (0.3 * torch.randn(D, generator=g, dtype=torch.float64)).float().cuda().contiguous()
    return W, b


def _frames(n, t):
    """[n, 768, t] frames q = W h + b"""
    W, b = _basis()
    g = torch.Generator(device="cuda").manual_seed(7 * n + t)
    h = torch.randn(n, SUB, t, device="cuda", generator=g)
    return (torch.einsum("dc,nct->ndt", W, h) + b[None, :, None]).contiguous()


@functools.lru_cache(maxsize=None)
def _library(m):
    tok = torch.randn(D, m, generator=torch.Generator().manual_seed(77 + m)).cuda()
    lib = PackedLibrary(tok, prefilter="fp6", strict=False)
    assert lib.prefilter == "fp6" and lib.rot is None and lib.M == m
    lib.use_subspace(*_basis())
    assert lib.sub is not None
    return lib


def _view(Tt, m, k):
    out = (ctypes.c_int64 * 32)()
    rc = nat.lib().alive_debug_knn_stage_view(Tt, m, k, 1, ctypes.cast(out, ctypes.c_void_p), 32)
    assert rc == 0
    o = list(out)
    v = dict(zip(("s_bf16", "s_f8", "clip6", "sub_f6", "sub_g", "cv", "ci", "bytes"), o[:8]))
    v["p6"] = dict(zip(("Tt_pad", "tiles_total", "tiles_per_split", "P"), o[16:20]))
    v["p6w"] = dict(zip(("Tt_pad", "tiles_total", "tiles_per_split", "P"), o[27:31]))
    v.update(KP8=o[21], FT6=o[23], LT=o[24], FT6W=o[31])
    return v


def _stage_lists(lib, src, k, mode):
    """one search under `mode`; -> (stats, view, plan, cv, ci) with the stage's lists [Tt, P, 32] as they stand in the workspace"""
    assert nat.lib().alive_knn_sub_frames(mode) == mode
    n, _, t = src.shape
    Tt = n * t
    assert Tt * k > 64 and Tt <= 16384                 # a candidate stage runs, no probe, no tier writes into cv / ci behind it
    val, idx = lib.search(src, k)
    st = lib.search_stats()
    assert st["stage_form"] == "subspace" and st["frames_left_subspace"] == 0 and st["frames_clipped"] == 0, st
    assert st["stage_frames"] == mode and st["fp8_blocks_seeded"] == 0, st
    ws = lib._last[3]
    v = _view(Tt, lib.M, k)
    assert ws.numel() >= v["bytes"] and v["KP8"] == 2 * H and (v["FT6"], v["FT6W"]) == (384, 512)
    plan = v["p6w" if mode == 512 else "p6"]
    P = plan["P"]
    cv = _np(ws[v["cv"]:v["cv"] + Tt * P * 2 * H * 4]).view(np.float32).reshape(Tt, P, 2 * H)
    ci = _np(ws[v["ci"]:v["ci"] + Tt * P * 2 * H * 4]).view(np.int32).reshape(Tt, P, 2 * H)
    return st, v, plan, cv, ci, ws, val, idx


def _reference(lib, ws, v, Tt):
    """float64 scores of the stage's own operands: decoded frame codes x decoded row codes + (g 2^10) rho, and the tolerance"""
    m = lib.M
    m_pad = nat.lib().alive_library_padded_rows(m)
    A = kc.fp6_image_decode(_np(ws[v["sub_f6"]:v["sub_f6"] + Tt * SUB]).reshape(Tt, SUB))
    B = kc.fp6_image_decode(_np(lib.sub["lib"]).reshape(m_pad, SUB)[:m])
    g = _np(ws[v["sub_g"]:v["sub_g"] + Tt * 4]).view(np.float32)
    rho = _np(lib.sub["rho"])[:m]
    whole = A @ B.T
    gr = (g * np.float32(F6_SCALE * F6_SCALE)).astype(np.float64)[:, None] * rho.astype(np.float64)[None, :]
    assert float(np.abs(whole).max()) < 2.0 ** 14 and float(np.abs(gr).max()) > 0.0
    return whole + gr, 2.0 ** -18 * (np.abs(whole) + np.abs(gr))


def _kth_best(x, k):
    if x.shape[1] < k:
        return np.full(x.shape[0], -np.inf)
    return np.partition(x, x.shape[1] - k, axis=1)[:, x.shape[1] - k]


def _check_lists(cv, ci, ref, tol, M, LT, plan):
    """every list is the set of the 16 best rows of its own rows (split s, half h = ((row % 8) >= 4)), up to 2 tol at the boundary;
    entries are fillers or distinct rows < M; a stored value is the row's score, its 4 low bits the row's register"""
    Tt, P = cv.shape[0], plan["P"]
    tps = plan["tiles_per_split"]
    assert P * tps >= plan["tiles_total"]
    real = ci >= 0
    assert np.all(ci[~real] == -1) and np.all(np.isneginf(cv[~real]))
    assert np.all(ci[real] < M) and np.all(np.isfinite(cv[real]))
    flat = np.sort(ci.reshape(Tt, -1), axis=1)
    assert not ((flat[:, 1:] == flat[:, :-1]) & (flat[:, 1:] >= 0)).any()
    f, s, e = np.nonzero(real)
    idx, val = ci[f, s, e], cv[f, s, e]
    assert np.all(np.abs(val.astype(np.float64) - ref[f, idx]) <= tol[f, idx])
    r32, bits = idx % 32, val.view(np.uint32) & 15
    assert np.array_equal(r32 & 3, bits & 3) and np.array_equal(r32 >> 3, (bits >> 2) & 3) and np.array_equal((r32 >> 2) & 1, e // H)
    rows = np.arange(M)
    row_split, row_half = (rows // LT) // tps, (rows % 8 >= 4).astype(np.int64)
    assert np.array_equal(row_split[idx], s)
    here = np.zeros((Tt, M), dtype=bool)
    here[f, idx] = True
    counts = real.reshape(Tt, P, 2, H).sum(-1)
    for sp in range(P):
        for h in range(2):
            R = rows[(row_split == sp) & (row_half == h)]
            assert np.all(counts[:, sp, h] == min(H, len(R))), (sp, h, len(R))
            if len(R) == 0:
                continue
            sub, t2, inside = ref[:, R], 2.0 * tol[:, R], here[:, R]
            kth = _kth_best(sub, H)[:, None]
            assert not ((sub > kth + t2) & ~inside).any(), (sp, h, "a clearly better row is missing")
            assert not ((sub < kth - t2) & inside).any(), (sp, h, "a clearly worse row is listed")


# (1, 512, 517): one block, ragged last tile; (1, 513, 2048): two blocks, 511 padded frames; (2, 300, 4097): 600 frames across two
# windows, ragged library
STAGE_SHAPES = [(1, 512, 517), (1, 513, 2048), (2, 300, 4097)]


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-M{s[2]}")
def test_wide_stage_lists_are_the_best_rows_of_the_same_codes(shape, k):
    n, t, m = shape
    lib = _library(m)
    st, v, plan, cv, ci, ws, _, _ = _stage_lists(lib, _frames(n, t), k, 512)
    Tt = n * t
    assert plan["Tt_pad"] == (Tt + 511) // 512 * 512
    ref, tol = _reference(lib, ws, v, Tt)
    _check_lists(cv, ci, ref, tol, m, v["LT"], plan)


def test_switch_returns_the_mode_and_384_is_the_old_path():
    L = nat.lib()
    assert L.alive_knn_sub_frames(384) == 384 and L.alive_knn_sub_frames(0) == 384
    assert L.alive_knn_sub_frames(512) == 512 and L.alive_knn_sub_frames(0) == 512
    assert L.alive_knn_sub_frames(7) == 512                       # not a mode: nothing changes
    assert L.alive_knn_sub_frames(-1) == 0 and L.alive_knn_sub_frames(0) == 0
    n, t, m = STAGE_SHAPES[2]
    lib, src = _library(m), _frames(n, t)
    # mode 384: knn_sub6_kernel on the 384-frame plan, its lists where and what they were
    st, v, plan, cv, ci, ws, val4, idx4 = _stage_lists(lib, src, 4, 384)
    assert plan["Tt_pad"] == 768
    ref, tol = _reference(lib, ws, v, n * t)
    _check_lists(cv, ci, ref, tol, m, v["LT"], plan)
    val4, idx4 = val4.clone(), idx4.clone()
    # the rule, at 600 frames: far below 300 blocks of 512 frames -> the 384-frame kernel, and the same bits
    L.alive_knn_sub_frames(-1)
    val0, idx0 = lib.search(src, 4)
    assert lib.search_stats()["stage_frames"] == 384
    assert torch.equal(val0, val4) and torch.equal(idx0, idx4)


def _brute(src, lib, k):
    q = _np(src).astype(np.float64).transpose(0, 2, 1).reshape(-1, D)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r = _np(lib.rows).astype(np.float64)
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    sc = q @ r.T
    order = np.argsort(-sc, axis=1, kind="stable")[:, :k]          # ties to the lower index
    return np.take_along_axis(sc, order, axis=1), order


def test_search_is_exact_in_both_modes():
    n, t, m, k = 3, 400, 20011, 4
    lib, src = _library(m), _frames(n, t)
    L = nat.lib()
    out = {}
    for mode in (512, 384):
        assert L.alive_knn_sub_frames(mode) == mode
        val, idx = lib.search(src, k)
        st = lib.search_stats()
        assert st["stage_form"] == "subspace" and st["stage_frames"] == mode, st
        out[mode] = (val.clone(), idx.clone())
    assert torch.equal(out[512][0], out[384][0]) and torch.equal(out[512][1], out[384][1])
    bv, bi = _brute(src, lib, k + 1)
    # a frame is unambiguous when no two of its k + 1 best float64 scores lie within 1e-5 (the audit's rule): its list is the brute
    # force's, index for index; the values are the k best scores for every frame
    safe = np.min(bv[:, :-1] - bv[:, 1:], axis=1) >= 1e-5
    assert safe.mean() > 0.9
    assert np.array_equal(_np(out[512][1]).astype(np.int64)[safe], bi[safe, :k] + lib.idx_base)
    assert float(np.abs(_np(out[512][0]).astype(np.float64) - bv[:, :k]).max()) <= 2e-6


def test_seeded_batch_takes_the_wide_form_by_the_rule():
    n, t, m, k = 300, 512, 65536, 4
    lib, src = _library(m), _frames(n, t)
    L = nat.lib()
    assert L.alive_knn_sub_frames(-1) == 0
    val, idx = lib.search(src, k)
    st = lib.search_stats()
    assert st["stage_form"] == "subspace" and st["stage_frames"] == 512 and st["fp8_blocks_seeded"] > 0, st
    val, idx = val.clone(), idx.clone()
    assert L.alive_knn_sub_frames(384) == 384
    val4, idx4 = lib.search(src, k)
    st4 = lib.search_stats()
    assert st4["stage_form"] == "subspace" and st4["stage_frames"] == 384, st4
    assert torch.equal(val, val4) and torch.equal(idx, idx4)


# ---- 16-bit tile offsets ------------------------------------------------------------------------------------------------------------

def _positive_codes(rows, seed):
    """[rows, 512] byte image of positive e2m3 codes and their decoded values"""
    rng = np.random.default_rng(seed)
    img = kc.fp6_image(np.minimum(np.abs(rng.standard_normal((rows, SUB))) * 1.5, 7.5))
    return img, kc.fp6_image_decode(img)


def test_tile_offsets_up_to_16_bits_and_the_hand_over_beyond():
    """A library of zero codes (score 0 for every frame) with planted rows of positive codes, frames of positive codes: every plant
    beats every other row of its half-list, so each frame's lists must hold every plant the launch can see, under its own index.
    M1: 65 532 tiles in one split, the most the 16-bit offsets hold (tiles come in fours) -> the 512-frame kernel, plants in its last
    two tiles, a ragged end.  M2 = 32 x 70 000 in one split -> the 384-frame kernel takes over (plants at 32 x 65 536, where a 16-bit
    offset would wrap to 0, at 32 x 65 535, whose offset is the seed mark, and in the last tile); in two splits the wide kernel again,
    with a tile_begin to add."""
    L = nat.lib()
    M2 = 32 * 70000
    M1 = 128 * 16383 - 5
    assert L.alive_library_padded_rows(M2) == M2 and L.alive_library_padded_rows(M1) // 32 == 65532
    Tt, Tp = 512, 1536
    plants = [5, 32 * 1000 + 12, M1 - 40, M1 - 1, M1 + 1, 32 * 65535 + 3, 32 * 65536, 32 * 65536 + 20, 32 * 69999 + 7, M2 - 1]
    fimg, fval = _positive_codes(Tt, 1)
    pimg, pval = _positive_codes(len(plants), 2)
    rng = np.random.default_rng(3)
    g = rng.uniform(-1.0, 1.0, Tt).astype(np.float32) * np.float32(2.0 ** -6)
    prho = rng.standard_normal(len(plants)).astype(np.float32)
    whole = fval @ pval.T
    gr = (g * np.float32(1024.0)).astype(np.float64)[:, None] * prho.astype(np.float64)[None, :]
    ref, tol = whole + gr, 2.0 ** -18 * (np.abs(whole) + np.abs(gr))
    assert 100.0 < float(ref.min()) and float(np.abs(whole).max()) < 2.0 ** 14

    s_sub = torch.zeros(Tp, SUB, dtype=torch.uint8, device="cuda")
    s_sub[:Tt] = torch.from_numpy(fimg).cuda()
    gq = torch.zeros(Tp, dtype=torch.float32, device="cuda")
    gq[:Tt] = torch.from_numpy(g).cuda()
    lib_sub = torch.zeros(M2, SUB, dtype=torch.uint8, device="cuda")
    rho = torch.zeros(M2, dtype=torch.float32, device="cuda")
    at = torch.tensor(plants, device="cuda")
    lib_sub[at] = torch.from_numpy(pimg).cuda()
    rho[at] = torch.from_numpy(prho).cuda()

    def run(mode, M, split):
        assert L.alive_knn_sub_frames(mode) == max(mode, 0)
        cv = torch.full((Tp, split, 2 * H), float("nan"), device="cuda")
        ci = torch.full((Tp, split, 2 * H), -7, dtype=torch.int32, device="cuda")
        frames = ctypes.c_int(0)
        nat.check(L.alive_debug_knn_sub_stage(nat.ptr(s_sub), nat.ptr(gq), Tp, nat.ptr(lib_sub), nat.ptr(rho), M, split, nat.ptr(cv), nat.ptr(ci),
                                              ctypes.cast(ctypes.byref(frames), ctypes.c_void_p), nat.stream()), "alive_debug_knn_sub_stage")
        torch.cuda.synchronize()
        return frames.value, _np(cv)[:Tt], _np(ci)[:Tt]

    def check(cv, ci, M, split):
        tiles = L.alive_library_padded_rows(M) // 32
        tps = (tiles + split - 1) // split
        assert np.all(ci >= 0) and np.all(ci < M)                          # every half-list is full, of rows below M
        flat = np.sort(ci.reshape(Tt, -1), axis=1)
        assert not (flat[:, 1:] == flat[:, :-1]).any()
        e = np.broadcast_to(np.arange(2 * H), ci.shape)
        s = np.broadcast_to(np.arange(split)[None, :, None], ci.shape)
        r32, bits = ci % 32, cv.view(np.uint32) & 15
        assert np.array_equal(r32 & 3, bits & 3) and np.array_equal(r32 >> 3, (bits >> 2) & 3) and np.array_equal((r32 >> 2) & 1, e // H)
        assert np.array_equal((ci // 32) // tps, s)
        planted = np.zeros(ci.shape, dtype=bool)
        for j, p in enumerate(plants):
            hit = ci == p
            if p >= M:
                assert not hit.any(), p
                continue
            assert np.all(hit.reshape(Tt, -1).sum(1) == 1), p             # in every frame's lists, once
            got = cv[hit].astype(np.float64)                              # (frame order: one hit per frame)
            assert np.all(np.abs(got - ref[:, j]) <= tol[:, j]), p
            planted |= hit
        assert np.all((cv.view(np.uint32)[~planted] & ~np.uint32(15)) == 0)   # every other entry is a row of zero codes: score 0

    f512, cv_w, ci_w = run(-1, M1, 1)
    assert f512 == 512
    check(cv_w, ci_w, M1, 1)
    f384, cv_n, ci_n = run(384, M1, 1)
    assert f384 == 384
    check(cv_n, ci_n, M1, 1)
    assert np.array_equal(np.sort(ci_w.reshape(Tt, -1), axis=1), np.sort(ci_n.reshape(Tt, -1), axis=1))
    fb, cv_f, ci_f = run(512, M2, 1)                                      # 70 000 tiles in one split: beyond 16 bits
    assert fb == 384
    check(cv_f, ci_f, M2, 1)
    f2, cv_2, ci_2 = run(512, M2, 2)                                      # 35 000 tiles per split
    assert f2 == 512
    check(cv_2, ci_2, M2, 2)
