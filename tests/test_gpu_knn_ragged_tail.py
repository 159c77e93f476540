"""Pad rows never enter a candidate list: every search form on libraries whose true cosines are ALL negative.

The tile bodies of the scoring kernels built from knn_score8_body (csrc/knn.hip) fold the previous tile without masking the rows beyond M;
only fold_rare (before it picks) and the fold of a split's last tile mask them.  A pad row scores 0 (zero codes), so on a library in
which every real row scores below 0 a pad row that got past the mask would beat every real row and show up as an index >= M -- or push
a true neighbour out of a list.  Rows come padded to 128 = four 32-row tiles: M = 5, 33, 70 and 100 leave the ragged tile FIRST, second,
third and last of the four (three, two, one and no all-pad tiles behind it, all but the last of them folded inside a tile body);
M = 4 097 is a search of several splits whose last split alone is ragged, with three all-pad tiles at its end.

Construction: d = W h0 for the seeded orthonormal W of the subspace form, rows r = -a d + sqrt(1 - a^2) n with n a random unit vector
orthogonal to d and a in [0.90, 0.95] for the crowd; frames q = W (100 h0 + 0.3 z) + b, so that every form, the subspace stage included,
scores the same frames (cos(q, d) ~ 0.994, no coordinate near the e2m3 clip: the test asserts that no frame is clipped or flagged).  The
true top-k are planted in the highest rows, M - 1 downwards -- the valid rows of the ragged tile first -- with a = 0.30, 0.35, ...: gaps
of 0.05 in cosine against a spread of ~0.004 (one sigma) over the frames, so the order is the same in every stage's arithmetic.

Reference: float64 brute force.  Values within 2e-6 (the audit's bound on the exact fp32 rescoring that every form ends in); indices
equal wherever the k + 1 best float64 scores of the frame lie at least 1e-5 apart (the audit's rule), which is every frame but for the
near-equal pairs of the last test."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from module import _native as nat  # noqa: E402
from module.common import PackedLibrary  # noqa: E402

pytestmark = pytest.mark.gpu

D, SUB = 768, 512
T = 96                                    # frames: above 64 / k for every k, so that a candidate stage runs and not the small exact scan
SIZES = [5, 33, 70, 100, 4097]
FORMS = ["fp8", "fp6", "sub384", "sub512", "bf16", "strict"]


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
    W = torch.linalg.qr(torch.randn(D, SUB, generator=g, dtype=torch.float64))[0]
    b = 0.3 * torch.randn(D, generator=g, dtype=torch.float64)
    h0 = (torch.randint(0, 2, (SUB,), generator=g).double() * 2.0 - 1.0) / SUB ** 0.5      # unit, every coordinate 0.044
    return W, b, h0


@functools.lru_cache(maxsize=None)
def _frames():
    W, b, h0 = _basis()
    g = torch.Generator().manual_seed(5)
    h = 100.0 * h0[:, None] + 0.3 * torch.randn(SUB, T, generator=g, dtype=torch.float64)
    return (W @ h + b[:, None]).float()[None].cuda().contiguous()                           # [1, 768, T]


def _rows(m, a, seed):
    """[768, m] float64: column j = -a[j] d + sqrt(1 - a[j]^2) n_j, n_j a unit vector orthogonal to d"""
    W, _, h0 = _basis()
    d = W @ h0
    d = d / d.norm()
    n = torch.randn(D, m, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    n = n - d[:, None] * (d @ n)[None, :]
    n = n / n.norm(dim=0, keepdim=True)
    return -d[:, None] * a[None, :] + n * torch.sqrt(1.0 - a * a)[None, :]


@functools.lru_cache(maxsize=None)
def _tokens(m):
    g = torch.Generator().manual_seed(100 + m)
    a = 0.90 + 0.05 * torch.rand(m, generator=g, dtype=torch.float64)
    planted = min(m, 8)
    a[m - planted:] = torch.tensor([0.30 + 0.05 * j for j in range(planted)], dtype=torch.float64).flip(0)     # best: row m - 1
    return _rows(m, a, 200 + m).float()


@functools.lru_cache(maxsize=None)
def _paired_tokens():
    """M = 200 (six whole tiles and 8 rows): two pairs of near-equal best rows in the ragged tile, (192, 193) in the lower half of the
    accumulator rows (row % 8 < 4: one lane per frame holds both) and (198, 199) in the upper half"""
    m = 200
    g = torch.Generator().manual_seed(300)
    a = 0.90 + 0.05 * torch.rand(m, generator=g, dtype=torch.float64)
    a[192], a[193], a[198], a[199] = 0.300, 0.301, 0.350, 0.351
    return _rows(m, a, 301).float()


def _form(base, form):
    if form == "bf16":
        return base
    if form == "strict":
        lib = base.with_strict()
        assert lib.strict and lib.prefilter == "bf16"
        return lib
    if form == "fp8":
        lib = base.with_prefilter("fp8")
        assert lib.prefilter == "fp8" and lib.rot is None
        return lib
    lib = base.with_prefilter("fp6")
    assert lib.prefilter == "fp6" and lib.rot is None and not lib.fp6_declined
    if form.startswith("sub"):
        W, b, _ = _basis()
        lib.set_subspace(W.float().cuda().contiguous(), b.float().cuda().contiguous())
        assert lib.sub is not None
    return lib


@functools.lru_cache(maxsize=None)
def _library(key, form):
    tok = _paired_tokens() if key == "pairs" else _tokens(key)
    base = _library(key, "bf16") if form != "bf16" else PackedLibrary(tok.cuda(), prefilter="bf16", strict=False)
    return _form(base, form)


@functools.lru_cache(maxsize=None)
def _brute(key):
    """float64 cosines [T, M] of the frames against the library `key`, once per library"""
    tok = _paired_tokens() if key == "pairs" else _tokens(key)
    q = _np(_frames())[0].astype(np.float64).T
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r = _np(tok).astype(np.float64).T
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    sc = q @ r.T
    assert sc.max() < -0.1                      # every true cosine is negative: a pad row's 0 would win
    sc.setflags(write=False)
    return sc


def _search_and_check(key, form, k):
    lib = _library(key, form)
    m = lib.M
    L = nat.lib()
    if form.startswith("sub"):
        mode = int(form[3:])
        assert L.alive_knn_sub_frames(mode) == mode
    val, idx = lib.search(_frames(), k)
    st = lib.search_stats()
    assert "tier" not in st, st                                  # a candidate stage ran
    if form.startswith("sub"):
        assert st["stage_form"] == "subspace" and st["stage_frames"] == int(form[3:]), st
        assert st["frames_left_subspace"] == 0 and st["frames_clipped"] == 0, st
    else:
        assert st["prefilter"] == ("bf16" if form == "strict" else form), st
    val, idx = _np(val).astype(np.float64), _np(idx).astype(np.int64) - lib.idx_base
    sc = _brute(key)
    order = np.argsort(-sc, axis=1, kind="stable")[:, :min(k + 1, m)]
    best = np.take_along_axis(sc, order, axis=1)
    err = float(np.abs(val - best[:, :k]).max())
    print(f"{key} {form} k={k}: max |val - float64| {err:.3e}, idx range [{idx.min()}, {idx.max()}]")
    assert idx.min() >= 0 and idx.max() < m, (idx.min(), idx.max(), m)
    assert err <= 2e-6, err
    safe = np.min(best[:, :-1] - best[:, 1:], axis=1) >= 1e-5 if best.shape[1] > 1 else np.ones(len(best), dtype=bool)
    assert np.array_equal(idx[safe], order[safe, :k])
    return idx, order, safe


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", SIZES)
def test_no_pad_row_enters_a_list(m, form):
    for k in (1, 4, 8):
        if k > m:                              # the search refuses k > M (check_search_args): M = 5 runs k = 1 and 4
            continue
        idx, order, safe = _search_and_check(m, form, k)
        assert safe.all()
        assert np.array_equal(idx, np.broadcast_to(np.arange(m - 1, m - 1 - k, -1), idx.shape))     # the planted rows, best first


@pytest.mark.parametrize("form", FORMS)
def test_two_admissions_per_lane_in_the_ragged_tile(form):
    """both rows of a near-equal pair beat a full half-list's floor in the same tile and the same lane: the out-of-line block goes
    through fold_loop as well (M = 200 pads to eight tiles: the ragged tile is the seventh, folded inside the last tile's body)"""
    idx, order, safe = _search_and_check("pairs", form, 4)
    assert np.array_equal(np.sort(idx, axis=1), np.broadcast_to(np.array([192, 193, 198, 199]), idx.shape))
