"""The search's work outside the scoring kernels (csrc/knn.hip): the library's unit rows packed once (alive_library_pack_unit_rows,
read by knn_rescore_kernel instead of a division per gathered element), every tiered search behind alive_knn_search_unit, and the
subspace form's plain fp6 image of the frames, built only when it is read.

The brute force here is the reference's arithmetic (divide the row by its norm in fp32, then dot: rows / norms by torch) in the
summation order of the exact tiers, emulated bit for bit: a lane's twelve fp32 fmaf's over d = 4 lane + e, 256 + 4 lane + e,
512 + 4 lane + e, then the xor tree 32 .. 1 over the 64 lanes.  The frames' unit vectors are the search's own (src_prep's s_f32, read
from the workspace).  Lists compare with torch.equal, values included."""
import ctypes

import pytest
import torch

from module import _native as nat
from module.common import PackedLibrary
from module.content_encoder import ContentEncoder

pytestmark = pytest.mark.gpu

N, T = 3, 131                       # 393 frames: ragged against 64, 256 and 384
LIBS = (5037, 4096)                 # ragged against the 128-row padding / exact
KS = (1, 4, 8)
STAGES = ("fp6_sub", "fp6", "fp8", "bf16", "strict")


# ---------------------------------------------------------------------------------------------------- exact arithmetic
def _fma32(a, b, c):
    """fmaf of fp32 values held in float64: the product is exact, the sum is rounded to 53 bits and then to 24.  The one case in
    which that differs from a single rounding -- the 53-bit sum exactly on a 24-bit midpoint while the true sum is not -- is undone
    with the sum's exact error (TwoSum) before the second rounding"""
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    mid = (s.view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)
    if bool(mid.any()):
        inf = torch.full_like(s, float("inf"))
        s = torch.where(mid & (err > 0), torch.nextafter(s, inf), torch.where(mid & (err < 0), torch.nextafter(s, -inf), s))
    return s.float().double()


def exact_scores(s_hat, r_hat, chunk=32):
    """[F, 768] unit frames x [M, 768] unit rows -> [F, M] fp32 cosines, bitwise those of knn_rescore_kernel / knn_exact_kernel"""
    F, M = s_hat.shape[0], r_hat.shape[0]
    r = r_hat.double().view(M, 3, 64, 4)
    out = torch.empty(F, M, device=s_hat.device)
    for f0 in range(0, F, chunk):
        q = s_hat[f0:f0 + chunk].double().view(-1, 3, 64, 4)
        p = torch.zeros(q.shape[0], M, 64, dtype=torch.float64, device=s_hat.device)
        for b in range(3):
            for e in range(4):
                p = _fma32(q[:, None, b, :, e], r[None, :, b, :, e], p)
        v = p.float()
        for half in (32, 16, 8, 4, 2, 1):
            v = v[..., :half] + v[..., half:2 * half]
        out[f0:f0 + chunk] = v[..., 0]
    return out


def brute_topk(scores, k, idx_base=0):
    """descending, ties to the lower row"""
    neg, order = torch.sort(-scores, dim=1, stable=True)
    return (-neg[:, :k]).contiguous(), (order[:, :k] + idx_base).to(torch.int32).contiguous()


def unit_frames(lib, frames):
    """s_f32 of the last search on lib's workspace: [Tt][768] behind the counters (knn.hip ws_layout)"""
    ws = lib._last[3]
    view = (ctypes.c_int64 * 25)()
    nat.check(nat.lib().alive_debug_knn_stage_view(frames, lib.M, 4, 0, view, 25))
    assert view[0] == (256 + frames * 3072 + 255) // 256 * 256          # s_bf16 follows s_f32, which follows the 128 B of counters
    torch.cuda.synchronize()
    return ws[256:256 + frames * 3072].view(torch.float32).view(frames, 768).clone()


# ---------------------------------------------------------------------------------------------------- operands
def _encoder(seed=2):
    ce = ContentEncoder(seed=seed).to("cuda")
    return ce, ce._sd["output_layer.weight"], ce._sd["output_layer.bias"]


def _frames(ce, n, t, seed=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ce(torch.rand(n, 641, t, device="cuda", generator=g)).contiguous()


def _tokens(M, seed=11):
    return torch.randn(768, M, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.ce, e.w, e.b = _encoder()
    e.feat = _frames(e.ce, N, T)
    assert e.feat.shape == (N, 768, T)
    e.rnd = torch.randn(N, 768, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    e.libs, e.ref, e.ref_rnd = {}, {}, {}
    for M in LIBS:
        plain = PackedLibrary(_tokens(M), prefilter="fp6", strict=False)
        assert plain.prefilter == "fp6" and plain.rot is None
        sub = plain.with_prefilter("fp6").set_subspace(e.w, e.b)
        assert sub.sub is not None
        e.libs[M] = {"fp6": plain, "fp6_sub": sub, "fp8": plain.with_prefilter("fp8"), "bf16": plain.with_prefilter("bf16"),
                     "strict": plain.with_strict()}
        assert e.libs[M]["fp8"].prefilter == "fp8" and e.libs[M]["strict"].lib_lo is not None
        r_hat = plain.rows / plain.norms[:, None]
        plain.search(e.feat, 4)
        e.ref[M] = brute_topk(exact_scores(unit_frames(plain, N * T), r_hat), 8)
        plain.search(e.rnd, 4)
        e.ref_rnd[M] = brute_topk(exact_scores(unit_frames(plain, N * T), r_hat), 8)
    yield e
    torch.cuda.empty_cache()


def old_search(lib, source, k, ws_holder):
    """the entry point PackedLibrary.search called for this library before alive_knn_search_unit, on a workspace of its own"""
    L = nat.lib()
    n, d, t = source.shape
    val = torch.empty(n * t, k, dtype=torch.float32, device=source.device)
    idx = torch.empty(n * t, k, dtype=torch.int32, device=source.device)
    split = lib.strict and lib.lib_lo is not None
    sub = lib.sub is not None and lib.prefilter == "fp6" and not lib.strict
    wsb = L.alive_knn_workspace_bytes_strict if split else (L.alive_knn_workspace_bytes_sub if sub else L.alive_knn_workspace_bytes_fast)
    ws = ws_holder.get(wsb(n * t, lib.M), source.device)
    p, s = nat.ptr, nat.stream()
    tail = (lib.M, lib.idx_base, k, p(val), p(idx), p(ws), s, None, None)
    if lib.strict:
        rc = L.alive_knn_search_strict(p(source), n, t, p(lib.lib_bf16), p(lib.lib_lo), p(lib.rows), p(lib.norms), p(lib.bound), *tail)
    elif sub:
        y = lib._rotate_frames(source, lib.sub)
        rc = L.alive_knn_search_fp6_sub_timed(p(source), p(y), n, t, p(lib.sub["lib"]), p(lib.sub["rho"]), p(lib.lib_f8), p(lib.lib_bf16),
                                              p(lib.rows), p(lib.norms), *tail)
    elif lib.lib_f8 is not None:
        fn = L.alive_knn_search_fp6_timed if lib.prefilter == "fp6" else L.alive_knn_search_fp8_timed
        rc = fn(p(source), n, t, p(lib.lib_f8), p(lib.lib_bf16), p(lib.rows), p(lib.norms), *tail)
    else:
        rc = L.alive_knn_search_timed(p(source), n, t, p(lib.lib_bf16), p(lib.rows), p(lib.norms), *tail)
    nat.check(rc, "old entry point")
    return val, idx


# ---------------------------------------------------------------------------------------------------- 1. unit rows
@pytest.mark.parametrize("M", LIBS)
def test_unit_rows_are_the_ieee_quotients(env, M):
    lib = env.libs[M]["fp6"]
    assert lib.rows_hat.shape == lib.rows.shape and torch.equal(lib.rows_hat, lib.rows / lib.norms[:, None])
    for other in env.libs[M].values():                                   # the copies share the tensor
        assert other.rows_hat.data_ptr() == lib.rows_hat.data_ptr()


def test_unit_rows_over_forty_octaves_of_norms():
    M = 5037
    g = torch.Generator(device="cuda").manual_seed(21)
    scale = torch.exp2(torch.rand(M, device="cuda", generator=g) * 40.0 - 20.0)
    scale[:3] = torch.tensor([2.0 ** -20, 1.0, 2.0 ** 20], device="cuda")
    lib = PackedLibrary(_tokens(M, seed=22) * scale[None, :], prefilter="bf16", strict=False)
    lo, hi = float(lib.norms.min()), float(lib.norms.max())
    assert lo < 2.0 ** -14 and hi > 2.0 ** 24, (lo, hi)                 # |row| = 27.7 x scale
    assert torch.equal(lib.rows_hat, lib.rows / lib.norms[:, None])
    # and the kernel's own sequence (norm_div / div_by) gives the same lists on such rows: old entry = new entry
    feat = torch.randn(N, 768, T, device="cuda", generator=g)
    v1, i1 = lib.search(feat, 4)
    v0, i0 = old_search(lib, feat, 4, nat.Workspace())
    assert torch.equal(i1, i0) and torch.equal(v1, v0)


# ---------------------------------------------------------------------------------------------------- 2. every stage, old = new = brute force
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("M", LIBS)
def test_new_entry_equals_old_entry_equals_brute_force(env, M, stage, k):
    lib = env.libs[M][stage]
    v1, i1 = lib.search(env.feat, k)
    st = lib.search_stats()
    v0, i0 = old_search(lib, env.feat, k, nat.Workspace())
    bv, bi = env.ref[M]
    torch.cuda.synchronize()
    if stage == "fp6_sub":
        assert st["stage_form"] == "subspace", st
    assert torch.equal(i1, i0) and torch.equal(v1, v0), st
    assert torch.equal(i1, bi[:, :k].contiguous()) and torch.equal(v1, bv[:, :k].contiguous()), st


# ---------------------------------------------------------------------------------------------------- 3. the change of basis
@pytest.mark.parametrize("M", LIBS)
def test_basis_change_against_float64(env, M):
    """y = [U | u]^T x on two bf16 planes per operand, three MFMAs per product (hi hi + hi lo + lo hi), fp32 accumulation:
    per product the dropped lo lo term (2^-16 relative) and the two operands' plane residuals (2^-16 each), plus 768 fp32 additions
    (768 x 2^-24), all relative to sum_k |W_k| |x_k| -- derived, not measured"""
    lib = env.libs[M]["fp6_sub"]
    lib.search(env.feat, 4)
    ws = lib._last[3]
    torch.cuda.synchronize()
    view = (ctypes.c_int64 * 27)()
    nat.check(nat.lib().alive_debug_knn_stage_view(N * T, lib.M, 4, 1, view, 27))
    co = nat.lib().alive_knn_sub_coordinates()
    cols = N * T
    cols_pad = (cols + 127) // 128 * 128
    assert nat.lib().alive_planes_bytes(cols, 768, 2) == 2 * cols_pad * 768 * 2
    y = ws[view[26]:view[26] + cols * co * 4].view(torch.float32).view(N, co, T)
    planes = ws[view[25]:view[25] + 2 * cols_pad * 768 * 2].view(torch.bfloat16).view(2, 24, cols_pad, 32)
    # the planes: hi = bf16(x), lo = bf16(x - hi) of frame n T + t, zero rows beyond the frames (768 has no padded coordinate)
    x = env.feat.permute(0, 2, 1).reshape(cols, 24, 32).permute(1, 0, 2)                       # [k-block][frame][32]
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    assert torch.equal(planes[0, :, :cols], hi) and torch.equal(planes[1, :, :cols], lo)
    assert not bool(planes[:, :, cols:].view(torch.int16).any())
    # the weights: rows 0 .. 575 of the form's two planes; rows 513 .. 575 (padded coordinates) are zero
    Wp = lib.sub["W"].float()                                                                   # [2][24][576][32]
    assert Wp.shape == (2, 24, co, 32) and not bool(Wp[:, :, 513:].any())
    W64 = lib.sub["basis"].t().double()                                                         # [576][768]: the fp32 [U | u]^T
    held = (Wp[0].double() + Wp[1].double()).permute(1, 0, 2).reshape(co, 768)                  # what the planes hold of it
    assert bool(((held - W64).abs() <= 2.0 ** -16 * W64.abs()).all())
    x64 = env.feat.double()
    y64 = torch.einsum("ck,nkt->nct", W64, x64)
    mag = torch.einsum("ck,nkt->nct", W64.abs(), x64.abs())
    err = (y.double() - y64).abs()
    bound = (3 * 2.0 ** -16 + 768 * 2.0 ** -24) * mag
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    assert not bool(y[:, 513:].any())                                                           # padded coordinates


# ---------------------------------------------------------------------------------------------------- 4. the lazy plain image
def _plain_image_region(lib, frames, k):
    view = (ctypes.c_int64 * 25)()
    nat.check(nat.lib().alive_debug_knn_stage_view(frames, lib.M, k, 1, view, 25))
    rows = max(view[8], view[16])                                       # frames padded for the bf16 / for the fp6 stage
    return view[1], view[1] + rows * 768, view[1] + view[16] * 768      # the region; the end of what the fp6 stage reads


@pytest.mark.parametrize("M", LIBS)
def test_subspace_frames_leave_the_plain_image_unbuilt(env, M):
    lib = env.libs[M]["fp6_sub"]
    lib.search(env.feat, 4)                                             # (the workspace exists from here on)
    ws = lib._last[3]
    lo, hi, used = _plain_image_region(lib, N * T, 4)
    ws[lo:hi] = 0xA5
    v, i = lib.search(env.feat, 4)
    st = lib.search_stats()
    assert lib._last[3] is ws
    assert st["stage_form"] == "subspace" and st["frames_left_subspace"] == 0, st
    off = nat.lib().alive_knn_search_stats(N, T, lib.M, nat.ptr(ws)) - ws.data_ptr()
    assert ws[off:off + 128].view(torch.int32)[21].item() == 1          # ST_SUB_GATE: the subspace kernel scored
    assert bool((ws[lo:hi] == 0xA5).all())
    bv, bi = env.ref[M]
    assert torch.equal(i, bi[:, :4].contiguous()) and torch.equal(v, bv[:, :4].contiguous())


@pytest.mark.parametrize("M", LIBS)
def test_gaussian_frames_take_the_plain_stage_on_a_fresh_image(env, M):
    lib = env.libs[M]["fp6_sub"]
    lib.search(env.rnd, 4)
    ws = lib._last[3]
    lo, hi, used = _plain_image_region(lib, N * T, 4)
    ws[lo:hi] = 0xA5                                                    # a stale image would score garbage: 0xA5 codes are not these frames'
    v, i = lib.search(env.rnd, 4)
    st = lib.search_stats()
    assert st["stage_form"] == "plain" and st["frames_left_subspace"] == N * T, st
    off = nat.lib().alive_knn_search_stats(N, T, lib.M, nat.ptr(ws)) - ws.data_ptr()
    assert ws[off:off + 128].view(torch.int32)[21].item() == 2
    assert not bool((ws[lo:lo + N * T * 768] == 0xA5).all())
    # the image is the one the old entry builds
    ws0 = nat.Workspace()
    v0, i0 = old_search(lib, env.rnd, 4, ws0)
    torch.cuda.synchronize()
    old = next(iter(ws0.bufs.values()))
    assert torch.equal(ws[lo:used], old[lo:used])
    bv, bi = env.ref_rnd[M]
    assert torch.equal(i, i0) and torch.equal(v, v0)
    assert torch.equal(i, bi[:, :4].contiguous()) and torch.equal(v, bv[:, :4].contiguous()), st


@pytest.mark.parametrize("M", LIBS)
def test_eighteen_searches_on_one_workspace(env, M):
    lib = env.libs[M]["fp6_sub"].with_prefilter("fp6")                  # a workspace (and history) of its own
    assert lib.sub is not None
    first = lib.search(env.feat, 4)
    for _ in range(17):
        v, i = lib.search(env.feat, 4)
        assert torch.equal(i, first[1]) and torch.equal(v, first[0])
    bv, bi = env.ref[M]
    assert torch.equal(first[1], bi[:, :4].contiguous()) and torch.equal(first[0], bv[:, :4].contiguous())


def test_eighteen_searches_across_a_due_probe(env):
    """393 frames never probe (the probe starts at 16 384 frames): the same eighteen searches on a batch that does, so that the image is
    built for the first two searches' probes, skipped on history, and built again for the probe of the 17th"""
    n, t, M = 48, 350, 4096
    feat = _frames(env.ce, n, t, seed=3)
    lib = env.libs[M]["fp6_sub"].with_prefilter("fp6")
    first = lib.search(feat, 4)
    st = lib.search_stats()
    assert st["stage_form"] == "subspace" and st["probe_sample"] == 1024 and not st["probe_skipped_on_history"], st
    v0, i0 = old_search(lib, feat, 4, nat.Workspace())
    assert torch.equal(first[1], i0) and torch.equal(first[0], v0)
    ws = lib._last[3]
    lo, hi, used = _plain_image_region(lib, n * t, 4)
    skipped = []
    for call in range(1, 18):
        ws[lo:hi] = 0xA5
        v, i = lib.search(feat, 4)
        st = lib.search_stats()
        assert lib._last[3] is ws and st["stage_form"] == "subspace", st
        assert torch.equal(i, first[1]) and torch.equal(v, first[0]), (call, st)
        skipped.append(st["probe_skipped_on_history"])
        assert bool((ws[lo:hi] == 0xA5).all()) == st["probe_skipped_on_history"], (call, st)
    assert skipped[0] is False and all(skipped[1:15]) and skipped[15] is False and skipped[16] is True, skipped
